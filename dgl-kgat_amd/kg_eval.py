"""Link prediction with the TransR embedding of the KG phase (reference ``models.py:114-133``), and with a translation
model that has no projection (``kge_models.CFKG``: no ``W_R``, ``u_x = normalize(e_x)``).

The score of a triple is the reference's ``|u_h + u_r - u_t|^2`` (``models.py:120-126``) with
``u_x = normalize(e_x W_r)`` and ``u_r = normalize(rel_r)``.  ``kg_rank`` gives the *filtered* rank of the true tail
(or head) of each triple among all entities (or a contiguous id range of them): every other entity that is known to
complete the triple is left out.  ``kg_metrics`` turns ranks into MR / MRR / Hits@k, ``kg_complete`` returns the K
entities closest to ``(h, r, ?)``.

On a HIP device in fp32 with d, k in {16, 32, 64, 128} the work is two kernels per relation
(``csrc/kgat_transr_rank.hip``): ``kgat_transr_project_f32`` projects and normalises the candidates and the queries on
the fp32 MFMA, ``kgat_transr_rank_f32`` streams the candidates past the queries and counts, per query, the candidates
that score below (``lt``) and equal to (``eq``) the true answer - no (entities x k) temporary per batch and no
(queries x entities) score matrix.  Other widths, dtypes and CPU modules take a restatement in torch operators, as
``transR`` does for the loss.

Everything here is evaluation: it runs under ``torch.no_grad()`` semantics.  Parameters and inputs that require a
gradient are read, never differentiated - no result carries a graph.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

KGRanks = namedtuple("KGRanks", ["lt", "eq", "rank"])

SIDES = ("tail", "head")
MAX_COMPLETE_K = 128


def _ids(x, device, name):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).reshape(-1)
    if t.numel() and t.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
        raise TypeError("%s must hold integer ids, got %s" % (name, t.dtype))
    return t.to(device=device, dtype=torch.int64)


class KnownTriples:
    """Every triple that counts as true (train, validation and test together), as two CSR structures on the device:
    keyed by ``(h, r)`` with the sorted unique tails - the filter of tail prediction - and keyed by ``(t, r)`` with the
    sorted unique heads for head prediction.  Only keys that occur are stored (sorted, looked up by binary search), so
    the size is that of the triple set, not ``n_entities x n_relations``.  Duplicated triples are stored once."""

    def __init__(self, h, r, t, n_entities, n_relations, device=None):
        if device is None:
            device = h.device if isinstance(h, torch.Tensor) else torch.device("cpu")
        self.device = torch.device(device)
        self.n_entities, self.n_relations = int(n_entities), int(n_relations)
        h, r, t = (_ids(x, self.device, n) for x, n in ((h, "h"), (r, "r"), (t, "t")))
        if not (h.numel() == r.numel() == t.numel()):
            raise ValueError("KnownTriples: h, r, t must have one length")
        if h.numel() and (int(torch.min(torch.stack([h.min(), r.min(), t.min()]))) < 0 or
                          int(torch.stack([h.max(), t.max()]).max()) >= self.n_entities or
                          int(r.max()) >= self.n_relations):
            raise IndexError("KnownTriples: an id outside [0, n_entities) / [0, n_relations)")
        if self.n_entities * self.n_relations * self.n_entities >= 2 ** 62:
            raise ValueError("KnownTriples: n_entities^2 x n_relations beyond 2^62")
        self._tables = {"tail": self._table(h, r, t), "head": self._table(t, r, h)}
        self.n_triples = int(self._tables["tail"][2].numel())

    def _table(self, a, r, b):
        # one sort orders keys and, within a key, the answers; unique drops repeated triples
        flat = torch.unique((a * self.n_relations + r) * self.n_entities + b)
        key = torch.div(flat, self.n_entities, rounding_mode="floor")
        ukeys, counts = torch.unique_consecutive(key, return_counts=True)
        ptr = torch.zeros(ukeys.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(counts, 0, out=ptr[1:])
        return ukeys, ptr, (flat - key * self.n_entities).to(torch.int32)

    def lists(self, keys, side, id_range=None):
        """``(ptr, ids)`` - int32 CSR over the batch - of the known answers of every query of ``keys = (e, r)``: the
        tails of ``(e, r, .)`` for ``side="tail"``, the heads of ``(., r, e)`` for ``side="head"``; ascending and
        unique per query.  ``id_range=(lo, hi)`` keeps only the ids inside it."""
        if side not in SIDES:
            raise ValueError("side must be 'tail' or 'head', got %r" % (side,))
        e, r = (_ids(x, self.device, n) for x, n in zip(keys, ("e", "r")))
        if e.numel() != r.numel():
            raise ValueError("KnownTriples.lists: the key arrays must have one length")
        ukeys, tptr, tids = self._tables[side]
        n = e.numel()
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        if n == 0 or ukeys.numel() == 0:
            return ptr.to(torch.int32), torch.zeros(0, dtype=torch.int32, device=self.device)
        key = e * self.n_relations + r
        pos = torch.searchsorted(ukeys, key).clamp(max=ukeys.numel() - 1)
        found = ukeys[pos] == key
        start = tptr[pos]
        length = torch.where(found, tptr[pos + 1] - start, torch.zeros_like(start))
        torch.cumsum(length, 0, out=ptr[1:])
        total = int(ptr[-1])
        owner = torch.repeat_interleave(torch.arange(n, device=self.device), length, output_size=total)
        ids = tids[start[owner] + (torch.arange(total, device=self.device) - ptr[owner])]
        if id_range is not None:
            keep = (ids >= int(id_range[0])) & (ids < int(id_range[1]))
            ids, owner = ids[keep], owner[keep]
            ptr = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(torch.bincount(owner, minlength=n), 0, out=ptr[1:])
        if int(ptr[-1]) >= 2 ** 31:
            raise ValueError("KnownTriples.lists: more than 2^31 filter entries in one batch")
        return ptr.to(torch.int32), ids.contiguous()


# ---------------------------------------------------------------------------------------------- the two formulations
def _params(model):
    """ent, W_R, rel; W_R is None for a translation model without a projection (kge_models.CFKG): u_x = normalize(e_x)."""
    W_R = getattr(model, "W_R", None)
    return model.entity_embed.weight.detach(), None if W_R is None else W_R.detach(), model.relation_embed.weight.detach()


def _use_kernels(ent, W_R):
    from . import ops
    if W_R is None:   # no projection to run: the counting kernel alone decides
        return bool(ent.is_cuda and ent.dtype == torch.float32 and ops.transr_rank_supported(ent.shape[1]))
    return bool(ent.is_cuda and ent.dtype == torch.float32 and W_R.dtype == torch.float32 and
                ops.transr_project_supported(W_R.shape[1], W_R.shape[2]))


def _unit_table(ent, lo, hi):
    """Without a projection the candidates do not depend on the relation: normalize(ent[lo:hi]) and its squared norms,
    formed once per call."""
    U = F.normalize(ent[lo:hi], p=2, dim=1).contiguous()
    return U, (U * U).sum(1)


def _unit_queries(ent, rel_row, sign, ids):
    return (F.normalize(ent.index_select(0, ids), p=2, dim=1) + sign * F.normalize(rel_row.unsqueeze(0), p=2, dim=1)).contiguous()


def _project_torch(ent, W_r, rel_row, sign, ids=None, rows=None):
    x = ent.index_select(0, ids) if ids is not None else (ent if rows is None else ent[rows[0]:rows[1]])
    u = F.normalize(x @ W_r, p=2, dim=1)
    n2 = (u * u).sum(1)
    if rel_row is not None:
        u = u + sign * F.normalize(rel_row.unsqueeze(0), p=2, dim=1)
    return u, n2


def _rank_torch(Q, t, P, n2, c0, fptr, fids, chunk=2048):
    """lt / eq of ops.transr_rank in torch operators (one (chunk x n_c) score matrix at a time)."""
    n_q, n_c = Q.shape[0], P.shape[0]
    lt = torch.empty(n_q, dtype=torch.int32, device=Q.device)
    eq = torch.empty(n_q, dtype=torch.int32, device=Q.device)
    owner = torch.repeat_interleave(torch.arange(n_q, device=Q.device), (fptr[1:] - fptr[:-1]).long())
    fpos = fids.long() - c0
    inside = (fpos >= 0) & (fpos < n_c)
    owner, fpos = owner[inside], fpos[inside]
    for lo in range(0, n_q, chunk):
        hi = min(lo + chunk, n_q)
        S = n2.unsqueeze(0) - 2.0 * (Q[lo:hi] @ P.t())
        rows = torch.arange(hi - lo, device=Q.device)
        tp = t[lo:hi].long() - c0
        st = S[rows, tp].unsqueeze(1)
        out = torch.zeros_like(S, dtype=torch.bool)
        sel = (owner >= lo) & (owner < hi)
        out[owner[sel] - lo, fpos[sel]] = True
        out[rows, tp] = True
        lt[lo:hi] = ((S < st) & ~out).sum(1).to(torch.int32)
        eq[lo:hi] = ((S == st) & ~out).sum(1).to(torch.int32)
    return lt, eq


def _check_triples(model, h, r, t, what):
    ent, W_R, _ = _params(model)
    dev = ent.device
    h, r, t = _ids(h, dev, "h"), _ids(r, dev, "r"), _ids(t, dev, "t")
    if not (h.numel() == r.numel() == t.numel()):
        raise ValueError("%s: h, r, t must have one length" % what)
    return h, r, t


def _candidate_range(candidates, n_ent, what):
    if candidates is None:
        return 0, n_ent
    lo, hi = int(candidates[0]), int(candidates[1])
    if not 0 <= lo < hi <= n_ent:
        raise ValueError("%s: candidates must be a non-empty id range (lo, hi) inside [0, %d], got %r"
                         % (what, n_ent, (candidates,)))
    return lo, hi


def _by_relation(r, n_rel, fptr):
    """For queries sorted by relation: the per-relation [begin, end) and the filter offsets at those boundaries -
    ONE host read."""
    bounds = torch.zeros(n_rel + 1, dtype=torch.int64, device=r.device)
    torch.cumsum(torch.bincount(r, minlength=n_rel), 0, out=bounds[1:])
    host = torch.stack([bounds, fptr.long()[bounds]]).tolist()
    return host[0], host[1]


def kg_rank(model, h, r, t, known=None, side="tail", candidates=None):
    """Filtered ranks of the triples ``(h, r, t)`` under the model's TransR score.  Returns
    ``KGRanks(lt, eq, rank)``: per triple the candidates that score strictly better than the true answer, those that
    tie with it, and ``rank = 1 + lt + eq / 2`` (float64) - the "realistic" rank, the mean of the optimistic and the
    pessimistic one.

    ``side="tail"`` ranks ``t`` for ``(h, r, ?)`` with the query ``u_h + u_r``; ``side="head"`` ranks ``h`` for
    ``(?, r, t)`` with ``u_t - u_r``.  ``known`` (a ``KnownTriples``) lists the other true answers, which are left
    out; the true answer itself never counts.  ``candidates`` is None (all entities) or a contiguous id range
    ``(lo, hi)`` that holds every true answer - the CKG's ids run users | items | attribute entities, so "items only"
    is a range.  Results come back in the caller's order.

    Queries are grouped by relation on the device (one host read of the group sizes); a relation with queries costs
    one projection of the candidates (into a buffer shared by all relations), one of the queries and one rank launch.
    Runs under ``torch.no_grad()`` semantics: parameters and inputs that require a gradient are read, not
    differentiated."""
    if side not in SIDES:
        raise ValueError("side must be 'tail' or 'head', got %r" % (side,))
    with torch.no_grad():
        ent, W_R, rel = _params(model)
        h, r, t = _check_triples(model, h, r, t, "kg_rank")
        n_ent, n_rel = ent.shape[0], rel.shape[0]
        lo, hi = _candidate_range(candidates, n_ent, "kg_rank")
        anchor, answer, sign = (h, t, 1.0) if side == "tail" else (t, h, -1.0)
        n = h.numel()
        dev = ent.device
        lt = torch.zeros(n, dtype=torch.int32, device=dev)
        eq = torch.zeros(n, dtype=torch.int32, device=dev)
        if n == 0:
            return KGRanks(lt, eq, torch.zeros(0, dtype=torch.float64, device=dev))
        if int(r.min()) < 0 or int(r.max()) >= n_rel or int(anchor.min()) < 0 or int(anchor.max()) >= n_ent:
            raise IndexError("kg_rank: an id outside [0, n_entities) / [0, n_relations)")
        if int(answer.min()) < lo or int(answer.max()) >= hi:
            raise IndexError("kg_rank: a true answer lies outside the candidate range [%d, %d)" % (lo, hi))
        order = torch.argsort(r, stable=True)
        a_s, r_s, ans_s = anchor[order], r[order], answer[order].to(torch.int32)
        if known is not None:
            fptr, fids = known.lists((a_s, r_s), side)
        else:
            fptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            fids = torch.zeros(0, dtype=torch.int32, device=dev)
        qb, fb = _by_relation(r, n_rel, fptr)
        kernels = _use_kernels(ent, W_R)
        lt_s, eq_s = torch.empty_like(lt), torch.empty_like(eq)
        if kernels:
            from . import ops
        if W_R is None:
            P, n2 = _unit_table(ent, lo, hi)
        elif kernels:
            ent_c, a32 = ent.contiguous(), a_s.to(torch.int32)
            P = torch.empty((hi - lo, W_R.shape[2]), dtype=torch.float32, device=dev)
            n2 = torch.empty(hi - lo, dtype=torch.float32, device=dev)
        for x in range(n_rel):
            b, e = qb[x], qb[x + 1]
            if b == e:
                continue
            fp = (fptr[b:e + 1] - fb[x]).contiguous()
            fi = fids[fb[x]:fb[x + 1]]
            if W_R is None:
                Q = _unit_queries(ent, rel[x], sign, a_s[b:e])
                if kernels:
                    lt_s[b:e], eq_s[b:e] = ops.transr_rank(Q, ans_s[b:e].contiguous(), P, n2, lo, fp, fi.contiguous())
                else:
                    lt_s[b:e], eq_s[b:e] = _rank_torch(Q, ans_s[b:e], P, n2, lo, fp, fi)
            elif kernels:
                W_r = W_R[x].contiguous()
                ops.transr_project(ent_c, W_r, rows=(lo, hi), out=P, n2_out=n2)
                Q, _ = ops.transr_project(ent_c, W_r, rel_row=rel[x].contiguous(), sign=sign, ids=a32[b:e].contiguous(),
                                          want_n2=False)
                lt_s[b:e], eq_s[b:e] = ops.transr_rank(Q, ans_s[b:e].contiguous(), P, n2, lo, fp, fi.contiguous())
            else:
                Pt, n2t = _project_torch(ent, W_R[x], None, 1.0, rows=(lo, hi))
                Q, _ = _project_torch(ent, W_R[x], rel[x], sign, ids=a_s[b:e])
                lt_s[b:e], eq_s[b:e] = _rank_torch(Q, ans_s[b:e], Pt, n2t, lo, fp, fi)
        lt[order], eq[order] = lt_s, eq_s
        return KGRanks(lt, eq, 1.0 + lt.double() + eq.double() / 2.0)


def metrics_from_ranks(rank, hits=(1, 3, 10)):
    """``{"mr", "mrr", "hits@k"..., "n"}`` of a tensor / array of (possibly fractional) ranks: mean rank, mean
    reciprocal rank, the share of ranks <= k."""
    rank = torch.as_tensor(rank, dtype=torch.float64).reshape(-1)
    n = rank.numel()
    if n == 0:
        raise ZeroDivisionError("no ranks")
    out = {"mr": float(rank.mean()), "mrr": float((1.0 / rank).mean())}
    for k in hits:
        out["hits@%d" % int(k)] = float((rank <= float(k)).double().mean())
    out["n"] = n
    return out


def metrics_from_counts(lt, eq, hits=(1, 3, 10)):
    """The same from the counts of ``kg_rank``: ``rank = 1 + lt + eq / 2``."""
    lt = torch.as_tensor(lt).double().reshape(-1)
    eq = torch.as_tensor(eq).double().reshape(-1)
    return metrics_from_ranks(1.0 + lt + eq / 2.0, hits)


def kg_metrics(model, h, r, t, known=None, side="both", hits=(1, 3, 10), batch=2048):
    """MR, MRR and Hits@k of the filtered ranks of ``(h, r, t)``: ``{"mr", "mrr", "hits@1", ..., "n"}``.
    ``side`` is "tail", "head" or "both" - the ranks of the two sides averaged together, as is usual; ``"n"`` is the
    number of ranks behind the means.  The triples are ranked ``batch`` at a time."""
    if side not in SIDES + ("both",):
        raise ValueError("side must be 'tail', 'head' or 'both', got %r" % (side,))
    h, r, t = _check_triples(model, h, r, t, "kg_metrics")
    batch = int(batch)
    if batch < 1:
        raise ValueError("kg_metrics: batch must be >= 1")
    ranks = []
    for s in (SIDES if side == "both" else (side,)):
        for lo in range(0, h.numel(), batch):
            ranks.append(kg_rank(model, h[lo:lo + batch], r[lo:lo + batch], t[lo:lo + batch], known=known, side=s).rank)
    return metrics_from_ranks(torch.cat(ranks).cpu() if ranks else torch.zeros(0), hits)


def kg_complete(model, h, r, K, known=None, candidates=None):
    """The K entities closest to ``(h, r, ?)``: ``(ids, distances)``, each ``(len(h), K)``, closest first - int64
    entity ids and the float32 squared distance ``|u_h + u_r - u_t|^2``.  ``known`` tails of ``(h, r)`` are dropped as
    ``metrics.recommend`` drops a user's ``seen`` items; a query with fewer than K candidates left gets ``-1`` /
    ``+inf`` at the end.  ``candidates`` as in ``kg_rank``.  With ``r`` the interaction relation, ``h`` users and the
    item range as candidates this is the KGE-only recommender (the KGAT paper's CKE-style baseline).

    The ranking is the existing top-K sweep (``kgat_eval_topk_f32``, 1 <= K <= 128) by ``q . p`` over the projected
    candidates: every non-zero projected row is a unit vector, so descending ``q . p`` is ascending distance, and the
    distance returned is ``|q|^2 + 1 - 2 q . p``.  RESTRICTION: an entity whose projection ``e W_r`` is exactly zero has
    norm 0, not 1 - the shortcut places it (and reports its distance) one unit too far.  HIP tensors only.  Widths: with
    d, k outside the projection kernel's {16, 32, 64, 128} the table is projected in torch operators; the sweep itself
    takes any relation width ``ops.eval_topk_supported(k, K)`` accepts (every k up to 352, wider ones while a
    wavefront's rows fit the LDS) and raises ``KGATLibraryError`` beyond."""
    from . import ops
    K = int(K)
    if not 1 <= K <= MAX_COMPLETE_K:
        raise ops.KGATLibraryError("kg_complete: K = %d outside 1..%d (the top-K sweep's range)" % (K, MAX_COMPLETE_K))
    with torch.no_grad():
        ent, W_R, rel = _params(model)
        dev = ent.device
        h, r = _ids(h, dev, "h"), _ids(r, dev, "r")
        if h.numel() != r.numel():
            raise ValueError("kg_complete: h and r must have one length")
        if not ent.is_cuda:
            raise ops.KGATLibraryError("kg_complete: the model is on %s: the top-K sweep only runs on a HIP device" % dev)
        n_ent, n_rel = ent.shape[0], rel.shape[0]
        lo, hi = _candidate_range(candidates, n_ent, "kg_complete")
        n = h.numel()
        ids = torch.full((n, K), -1, dtype=torch.int64, device=dev)
        dist = torch.full((n, K), float("inf"), dtype=torch.float32, device=dev)
        if n == 0:
            return ids, dist
        if int(r.min()) < 0 or int(r.max()) >= n_rel or int(h.min()) < 0 or int(h.max()) >= n_ent:
            raise IndexError("kg_complete: an id outside [0, n_entities) / [0, n_relations)")
        order = torch.argsort(r, stable=True)
        h_s, r_s = h[order], r[order]
        if known is not None:
            fptr, fids = known.lists((h_s, r_s), "tail", id_range=(lo, hi))
        else:
            fptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            fids = torch.zeros(0, dtype=torch.int32, device=dev)
        qb, fb = _by_relation(r, n_rel, fptr)
        kernels = _use_kernels(ent, W_R)
        ent_c = ent.contiguous().float()
        n_c, k = hi - lo, ent.shape[1] if W_R is None else W_R.shape[2]
        unit = _unit_table(ent_c, lo, hi)[0] if W_R is None else None
        item_ids = torch.arange(n_c, dtype=torch.int32, device=dev)
        ids_s, dist_s = torch.empty_like(ids), torch.empty_like(dist)
        for x in range(n_rel):
            b, e = qb[x], qb[x + 1]
            if b == e:
                continue
            table = torch.empty((n_c + e - b, k), dtype=torch.float32, device=dev)   # candidates, then the queries
            W_r = None if W_R is None else W_R[x].float().contiguous()
            if W_R is None:
                table[:n_c] = unit
                table[n_c:] = _unit_queries(ent_c, rel[x].float(), 1.0, h_s[b:e])
            elif kernels:
                ops.transr_project(ent_c, W_r, rows=(lo, hi), want_n2=False, out=table[:n_c])
                ops.transr_project(ent_c, W_r, rel_row=rel[x].contiguous(), ids=h_s[b:e].to(torch.int32).contiguous(),
                                   want_n2=False, out=table[n_c:])
            else:
                table[:n_c] = _project_torch(ent_c, W_r, None, 1.0, rows=(lo, hi))[0]
                table[n_c:] = _project_torch(ent_c, W_r, rel[x].float(), 1.0, ids=h_s[b:e])[0]
            fp = (fptr[b:e + 1] - fb[x]).contiguous()
            fi = (fids[fb[x]:fb[x + 1]] - lo).contiguous()      # positions in the candidate range
            users = torch.arange(n_c, n_c + e - b, dtype=torch.int32, device=dev)
            top, score = ops.eval_topk(table, users, item_ids, fp, fi, K, drop_train=True)
            q2 = (table[n_c:] * table[n_c:]).sum(1, keepdim=True)
            pos = top.long()
            ids_s[b:e] = torch.where(pos >= 0, pos + lo, pos)
            dist_s[b:e] = torch.where(pos >= 0, q2 + 1.0 - 2.0 * score, torch.full_like(score, float("inf")))
        ids[order], dist[order] = ids_s, dist_s
        return ids, dist


class LinkPrediction:
    """The three functions above as methods of a model that holds ``entity_embed``, ``relation_embed`` and, for a
    projected score, ``W_R`` (``_params``): inherited by ``KGATPropagation``, ``kge_models.CFKG`` and ``kge_models.CKE``."""

    def kg_rank(self, h, r, t, known=None, side="tail", candidates=None):
        """Filtered ranks of the triples under the model's translation score (``kg_rank``): KGRanks(lt, eq, rank)."""
        return kg_rank(self, h, r, t, known=known, side=side, candidates=candidates)

    def kg_metrics(self, h, r, t, known=None, side="both", hits=(1, 3, 10), batch=2048):
        """MR / MRR / Hits@k of the filtered ranks (``kg_metrics``)."""
        return kg_metrics(self, h, r, t, known=known, side=side, hits=hits, batch=batch)

    def kg_complete(self, h, r, K, known=None, candidates=None):
        """The K entities closest to (h, r, ?) with their distances (``kg_complete``)."""
        return kg_complete(self, h, r, K, known=known, candidates=candidates)
