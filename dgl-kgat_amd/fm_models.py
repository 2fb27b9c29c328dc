"""The KGAT paper's "supervised learning" baselines, FM and NFM, on fused Bi-Interaction pooling.

Both take "IDs of a user, an item and its knowledge (entities connected to it) as input features": the feature
universe is every node of the collaborative KG, one table ``V (n_nodes x d)`` and one ``w_lin (n_nodes)`` serve the
model, and the features of the pair (u, i) are the set ``{u} + F(i)`` with ``F(i)`` the item's list in a
``FeatureSets``.  The operator is NFM's Bi-Interaction pooling

    f_BI(x) = sum_{f<g} v_f * v_g = ((sum_f v_f)^2 - sum_f v_f^2) / 2

(``autograd.bi_pool``: csrc/kgat_bi_pool.hip on a HIP device in fp32, ``bi_pool_torch`` elsewhere); FM is the same
operator with its d outputs summed.  NFM's evaluation has no dot-product form: ``NFM.scores`` evaluates the MLP per
(user, item) pair in torch operators over user blocks (the default route); for a one-hidden-layer NFM on a HIP device
``fused=True`` runs the all-pairs sweep of csrc/kgat_nfm_eval.hip instead (``ops.nfm_eval_topk``: MLP scores into the
top-K lists, nothing of size users x items written)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import metrics, ops
from .ckg_io import load_pretrained_rows


POOL_CHUNK = 8192   # the sets of one kernel call (ops.bi_pool_supported)


class FeatureSets:
    """A CSR over item positions: ``ids[indptr[j]:indptr[j + 1]]`` are the feature ids (rows of the embedding table, in
    [0, n_features)) of item position j.  Lists are multisets: a repeated id counts twice.  Holds device copies (int32)
    and the graph-static reversed CSR - ``rev_items[rev_indptr[f]:rev_indptr[f + 1]]``: the item positions whose list
    holds feature f, ascending, once per occurrence.  ``item_offset``: the node id of item position 0 (``from_kg`` sets
    it; the models subtract it from the item ids they are given)."""

    def __init__(self, indptr, ids, n_features, device="cpu", item_offset=0):
        indptr = np.ascontiguousarray(np.asarray(indptr, dtype=np.int64))
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
        if indptr.ndim != 1 or len(indptr) < 2 or indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != len(ids):
            raise ValueError("FeatureSets: indptr must be non-decreasing from 0 to len(ids), over at least one item")
        n_features = int(n_features)
        if len(ids) and (ids.min() < 0 or ids.max() >= n_features):
            raise ValueError("FeatureSets: feature ids must lie in [0, %d)" % n_features)
        if not (0 < n_features < 2 ** 31 - 1 and len(indptr) - 1 < 2 ** 31 - 1 and len(ids) < 2 ** 31 - 1):
            raise ValueError("FeatureSets: sizes must stay below 2^31")
        self.n_items, self.n_features, self.n_pairs = len(indptr) - 1, n_features, len(ids)
        self.item_offset = int(item_offset)
        item_of = np.repeat(np.arange(self.n_items, dtype=np.int64), np.diff(indptr))
        order = np.argsort(ids, kind="stable")   # by feature; equal features keep ascending item position
        rev_indptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n_features))])
        self._host = {"indptr": indptr.astype(np.int32), "ids": ids.astype(np.int32), "rev_indptr": rev_indptr.astype(np.int32),
                      "rev_items": item_of[order].astype(np.int32)}
        self._copies = {}
        self._place(torch.device(device))

    def _place(self, device):
        key = str(device)
        if key not in self._copies:
            self._copies[key] = {k: torch.as_tensor(v).to(device) for k, v in self._host.items()}
        self.device = device
        for k, v in self._copies[key].items():
            setattr(self, k, v)

    def to(self, device):
        """The same sets with their arrays on `device` (a view object: the host arrays and earlier copies are shared)."""
        device = torch.device(device)
        if device == self.device:
            return self
        other = object.__new__(FeatureSets)
        other.__dict__.update(self.__dict__)
        other._place(device)
        return other

    def lists(self):
        """The lists as host arrays, one per item position."""
        ip, ids = self._host["indptr"], self._host["ids"]
        return [ids[ip[j]:ip[j + 1]].astype(np.int64) for j in range(self.n_items)]

    @classmethod
    def from_kg(cls, triplets, item_range, n_nodes, include_self=True, device="cpu"):
        """Item i of ``item_range = (lo, hi)`` gets the list ``[i] + sorted(unique tails t of the triples (i, r, t))``.
        Triples whose tail is a user are excluded; in the collaborative KG's id layout (ckg_io) the users are the ids
        below ``lo``."""
        lo, hi = int(item_range[0]), int(item_range[1])
        if not 0 <= lo < hi <= n_nodes:
            raise ValueError("from_kg: item range %r outside [0, %d]" % ((lo, hi), n_nodes))
        trip = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
        keep = (trip[:, 0] >= lo) & (trip[:, 0] < hi) & (trip[:, 2] >= lo) & (trip[:, 2] < n_nodes)
        pairs = np.unique(trip[keep][:, [0, 2]], axis=0)   # sorted by head, then tail; duplicates gone
        if include_self:
            own = np.arange(lo, hi, dtype=np.int64)
            heads = np.concatenate([own, pairs[:, 0]])
            tails = np.concatenate([own, pairs[:, 1]])
            order = np.argsort(heads, kind="stable")       # the self entry stays in front of the item's sorted tails
            heads, tails = heads[order], tails[order]
        else:
            heads, tails = pairs[:, 0], pairs[:, 1]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(heads - lo, minlength=hi - lo))])
        return cls(indptr, tails, n_nodes, device=device, item_offset=lo)


def _long(t, device):
    return torch.as_tensor(t, device=device).long()


def bi_pool_torch(V, w_lin, feats, items, extra=None, want_S=False):
    """Bi-Interaction pooling in torch operators (index_select / index_add_), differentiable: what the kernels are
    compared with and what runs on the CPU, in float64 and outside ``ops.bi_pool_supported``.  Pooled set m is
    ``[extra[m]] + feats[items[m]]`` (``extra[m] = -1``: no extra).  Returns (bi, lin, sq), or (S, bi, lin, sq)."""
    dev = V.device
    feats = feats.to(dev)
    items = _long(items, dev)
    M = items.numel()
    indptr, ids = feats.indptr.long(), feats.ids.long()
    beg = indptr[items]
    cnt = indptr[items + 1] - beg
    set_of = torch.repeat_interleave(torch.arange(M, device=dev), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    f = ids[torch.arange(set_of.numel(), device=dev) - first[set_of] + beg[set_of]]
    if extra is not None:
        extra = _long(extra, dev)
        has = extra >= 0
        f = torch.cat([extra[has], f])
        set_of = torch.cat([torch.arange(M, device=dev)[has], set_of])
    rows = V.index_select(0, f)
    S = torch.zeros(M, V.shape[1], dtype=V.dtype, device=dev).index_add_(0, set_of, rows)
    Q = torch.zeros(M, V.shape[1], dtype=V.dtype, device=dev).index_add_(0, set_of, rows * rows)
    bi = 0.5 * (S * S - Q)
    lin = torch.zeros(M, dtype=V.dtype, device=dev)
    if w_lin is not None:
        lin = lin.index_add_(0, set_of, w_lin.index_select(0, f))
    sq = Q.sum(1)
    return (S, bi, lin, sq) if want_S else (bi, lin, sq)


def _kernels_apply(V, w_lin, n_sets):
    return (V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and V.data_ptr() % 16 == 0 and
            (w_lin is None or (w_lin.is_contiguous() and w_lin.dtype == torch.float32)) and
            ops.bi_pool_supported(V.shape[1], n_sets))


def pool_items(V, w_lin, feats, chunk=POOL_CHUNK):
    """(P, T, lin) of every item's own list without an extra - ``P = S``, ``T = bi`` - under no_grad, in calls of at most
    `chunk` sets: the item side of ``bi({u} + F(i)) = v_u * P_i + T_i``."""
    with torch.no_grad():
        feats = feats.to(V.device)
        out = []
        for lo in range(0, feats.n_items, chunk):
            items = torch.arange(lo, min(lo + chunk, feats.n_items), dtype=torch.int32, device=V.device)
            if _kernels_apply(V, w_lin, items.numel()):
                S, bi, lin, _ = ops.bi_pool_fwd(V.detach(), None if w_lin is None else w_lin.detach(), feats, items, want_sq=False)
                if lin is None:
                    lin = torch.zeros(items.numel(), dtype=V.dtype, device=V.device)
            else:
                S, bi, lin, _ = bi_pool_torch(V, w_lin, feats, items, want_S=True)
            out.append((S, bi, lin))
        return tuple(torch.cat(parts, 0) for parts in zip(*out))


class _Pooled(nn.Module):
    """What FM and NFM share: the table ``embed`` (n_nodes x dim), ``w_lin`` (n_nodes), ``w0`` and the pooled pass of a
    BPR batch.  Item arguments are node ids; ``feats.item_offset`` turns them into item positions."""

    def __init__(self, n_nodes, feats, dim, reg_lambda):
        super().__init__()
        if feats.n_features != int(n_nodes):
            raise ValueError("the feature universe (%d) must be all %d nodes" % (feats.n_features, n_nodes))
        self.feats = feats
        self.reg_lambda = float(reg_lambda)
        self.embed = nn.Embedding(n_nodes, dim)
        # Xavier rows, as CKE's tables: a set of n features sums n (n - 1) / 2 products per column, and with
        # nn.Embedding's N(0, 1) rows the scores start at hundreds instead of near 0
        nn.init.xavier_uniform_(self.embed.weight)
        self.w_lin = nn.Parameter(torch.zeros(n_nodes))
        self.w0 = nn.Parameter(torch.zeros(1))

    def _positions(self, items):
        return items.to(torch.int32) - self.feats.item_offset

    def pool(self, users, items):
        """(bi, lin, sq) of the sets ``{users[m]} + F(items[m])``: one ``bi_pool`` call (up to 8,192 sets)."""
        from .autograd import bi_pool
        V, w, pos, ex = self.embed.weight, self.w_lin, self._positions(items), users.to(torch.int32)
        n = pos.numel()
        if n <= POOL_CHUNK or not _kernels_apply(V, w, POOL_CHUNK):
            return bi_pool(V, w, self.feats, pos, ex)
        # beyond the kernels' sets per call: calls of POOL_CHUNK sets (autograd adds their dense gradients)
        parts = [bi_pool(V, w, self.feats, pos[lo:lo + POOL_CHUNK], ex[lo:lo + POOL_CHUNK]) for lo in range(0, n, POOL_CHUNK)]
        return tuple(torch.cat(t, 0) for t in zip(*parts))

    def _head(self, bi):
        raise NotImplementedError

    def score(self, users, items):
        bi, lin, _ = self.pool(users, items)
        return self.w0 + lin + self._head(bi)

    def get_loss(self, u, pos, neg):
        """``mean_b softplus(y_neg - y_pos) + reg_lambda * mean_b (sq_pos + sq_neg) / 2``; one pooled call over the 2 B
        sets, positives first."""
        b = u.numel()
        bi, lin, sq = self.pool(torch.cat([u, u]), torch.cat([pos, neg]))
        y = self.w0 + lin + self._head(bi)
        return F.softplus(y[b:] - y[:b]).mean() + self.reg_lambda * (0.5 * (sq[:b] + sq[b:])).mean()

    def load_pretrained(self, user_embed, item_embed, n_users):
        """BPR-MF embeddings into the user and item rows of ``embed``."""
        load_pretrained_rows(self.embed.weight, user_embed, item_embed, n_users)


class FM(_Pooled):
    """Factorisation machine over ``{u} + F(i)``: ``y(u, i) = w0 + lin + sum_c bi_c``."""

    def __init__(self, n_nodes, feats, dim=64, reg_lambda=1e-5):
        super().__init__(n_nodes, feats, dim, reg_lambda)

    def _head(self, bi):
        return bi.sum(1)

    @torch.no_grad()
    def readout(self, user_range, item_range):
        """An (n_nodes, d + 2) table whose dot products are y: user rows ``[v_u | 1 | w0 + w_u]``, item rows
        ``[P_i | lin_i + sum_c T_i,c | 1]`` with P = S and T = bi of the set F(i) without an extra, from
        ``bi({u} + F(i)) = v_u * P_i + T_i``; other rows zero.  The per-user constant stays: calc_recall_ndcg masks
        training items to 0.0, so absolute scores matter.  With it ``calc_recall_ndcg``, ``calc_metrics``,
        ``calc_rank_metrics`` and ``recommend`` evaluate FM unchanged.  Zero columns are appended where the evaluation
        kernels - the K <= 32 sweep, the top-K lists up to K = 128 and the rank sweep alike - refuse d + 2 columns.  Not
        differentiable."""
        V, w = self.embed.weight, self.w_lin
        (u0, u1), (i0, i1) = user_range, item_range
        if not (0 <= u0 <= u1 <= V.shape[0] and 0 <= i0 <= i1 <= V.shape[0]) or max(u0, i0) < min(u1, i1):
            raise ValueError("readout: user rows %r and item rows %r must be disjoint ranges inside [0, %d]"
                             % ((u0, u1), (i0, i1), V.shape[0]))
        if i0 != self.feats.item_offset or i1 - i0 != self.feats.n_items:
            raise ValueError("readout: item rows %r are not the feature sets' items [%d, %d)"
                             % ((i0, i1), self.feats.item_offset, self.feats.item_offset + self.feats.n_items))
        d = V.shape[1]
        width = d + 2
        if V.is_cuda:
            # a width every evaluation family takes at every cut-off it offers (the list families' buffers grow with K)
            def taken(f):
                return (ops.eval_supported(f, 20) and ops.eval_supported(f, 32) and ops.eval_rank_supported(f) and
                        all(ops.eval_topk_supported(f, k) for k in (20, 64, 128)))
            while not taken(width) and width < d + 66:
                width += 1
        P, T, lin = pool_items(V, w, self.feats)
        table = torch.zeros(V.shape[0], width, dtype=V.dtype, device=V.device)
        table[u0:u1, :d] = V[u0:u1]
        table[u0:u1, d] = 1.0
        table[u0:u1, d + 1] = self.w0 + w[u0:u1]
        table[i0:i1, :d] = P
        table[i0:i1, d] = lin + T.sum(1)
        table[i0:i1, d + 1] = 1.0
        return table


class NFM(_Pooled):
    """Neural factorisation machine: ``y = w0 + lin + h . MLP(dropout(bi))``, the MLP plain ``nn.Linear`` + ReLU."""

    def __init__(self, n_nodes, feats, dim=64, layers=(64,), dropout=0.0, reg_lambda=1e-5):
        super().__init__(n_nodes, feats, dim, reg_lambda)
        widths = [dim] + [int(x) for x in layers]
        mods = []
        for a, b in zip(widths[:-1], widths[1:]):
            mods += [nn.Linear(a, b), nn.ReLU()]
        self.mlp = nn.Sequential(*mods)
        self.drop = nn.Dropout(dropout)
        self.h = nn.Parameter(torch.empty(widths[-1]))
        # h = 1 / sqrt(width): the MLP's output enters the score at the scale of one hidden unit - with an empty `layers`
        # and h = 1 this is FM
        nn.init.constant_(self.h, 1.0 / float(widths[-1]) ** 0.5 if len(widths) > 1 else 1.0)

    def _head(self, bi):
        return self.mlp(self.drop(bi)) @ self.h

    @torch.no_grad()
    def scores(self, users, max_bytes=1 << 28):
        """The (len(users), n_items) score matrix in torch operators, from ``bi({u} + F(i)) = v_u * P_i + T_i``, in user
        blocks sized so that a block's (users x items x widest layer) tensor stays below `max_bytes`."""
        V, w = self.embed.weight, self.w_lin
        users = _long(users, V.device)
        P, T, lin = pool_items(V, w, self.feats)
        widest = max([V.shape[1]] + [m.out_features for m in self.mlp if isinstance(m, nn.Linear)])
        block = max(1, int(max_bytes // (max(1, self.feats.n_items) * widest * V.element_size() * 2)))
        out = []
        was_training = self.training
        self.eval()
        try:
            for lo in range(0, users.numel(), block):
                u = users[lo:lo + block]
                bi = V[u].unsqueeze(1) * P.unsqueeze(0) + T.unsqueeze(0)
                out.append(self.w0 + (w[u].unsqueeze(1) + lin.unsqueeze(0)) + self._head(bi))
        finally:
            self.train(was_training)
        return torch.cat(out, 0) if out else torch.zeros(0, self.feats.n_items, dtype=V.dtype, device=V.device)

    def _fused_refusal(self, K):
        """Why the fused sweep cannot evaluate this model at depth K (None: it can)."""
        linear = [m for m in self.mlp if isinstance(m, nn.Linear)]
        V = self.embed.weight
        if len(linear) != 1:
            return "the fused sweep evaluates ONE hidden layer, the model has %d (layers=%r)" % (
                len(linear), tuple(m.out_features for m in linear))
        if not V.is_cuda:
            return "the parameters are on %s: the fused sweep only runs on a HIP device (CPU tensors)" % V.device
        if V.dtype != torch.float32:
            return "the parameters are %s, the fused sweep is float32" % V.dtype
        if not 1 <= int(K) <= ops.NFM_EVAL_MAX_K:
            return "K = %d is outside 1..%d" % (K, ops.NFM_EVAL_MAX_K)
        d, hidden = V.shape[1], linear[0].out_features
        if not ops.nfm_eval_supported(d, hidden, K):
            return "widths d = %d, hidden = %d: the fused sweep takes d in (16, 32, 64, 128), hidden in (16, 32, 64)" % (d, hidden)
        return None

    @torch.no_grad()
    def _fused_topk(self, what, user_ids, train_ptr, train_items, K, want_scores=True):
        """``ops.nfm_eval_topk`` for rows `user_ids` (int32 node ids) of the table: the item side pooled once, one addmm
        for ``C = T W1^T + b1``, the sweep.  No dropout, as ``scores``."""
        why = self._fused_refusal(K)
        if why is not None:
            raise ops.KGATLibraryError("%s(fused=True): %s" % (what, why))
        V, w = self.embed.weight.detach(), self.w_lin.detach()
        fc = self.mlp[0]
        P, T, lin = pool_items(V, w, self.feats)
        W1 = fc.weight.detach().contiguous()
        bias = fc.bias.detach() if fc.bias is not None else torch.zeros(W1.shape[0], dtype=V.dtype, device=V.device)
        C = torch.addmm(bias, T, W1.t())
        const = (self.w0.detach() + w[user_ids.long()]).contiguous()
        return ops.nfm_eval_topk(V, user_ids, W1, P.contiguous(), C, self.h.detach().contiguous(), lin.contiguous(), const,
                                 train_ptr, train_items, K, want_scores=want_scores)

    def _check_plan(self, plan):
        if plan.n_items != self.feats.n_items:
            raise ValueError("topk: the plan ranks %d items, the model scores %d" % (plan.n_items, self.feats.n_items))

    def topk(self, plan, K, max_bytes=1 << 28, fused=False):
        """The K best unseen items of every user of an ``EvalPlan`` as item positions, (n_users, K) int32.  Default:
        ``metrics.topk_unseen`` over ``scores`` (``torch.topk``).  ``fused=True``: the all-pairs sweep
        (``ops.nfm_eval_topk``) - score descending, equal scores by item position, ``-1`` where a user has fewer than K
        unseen items; ``KGATLibraryError`` naming the reason where the model or the device is outside its envelope."""
        if not fused:
            return metrics.topk_unseen(self.scores, self.feats.n_items, plan, K, max_bytes)
        self._check_plan(plan)
        return self._fused_topk("topk", plan.user_ids, plan.train_ptr, plan.train_items, K, want_scores=False)[0]

    def evaluate(self, plan, Ks=(20,), max_bytes=1 << 28, fused=False):
        """Mean recall / ndcg / precision / hit_ratio at the ascending cut-offs `Ks` for an ``EvalPlan``: the dict
        ``metrics.calc_metrics`` returns.  Default: ``metrics.calc_metrics_unseen`` over ``scores``.  ``fused=True``:
        ``topk(fused=True)`` at the largest cut-off, then ``ops.eval_metrics_at_ks``."""
        if not fused:
            return metrics.calc_metrics_unseen(self.scores, self.feats.n_items, plan, Ks, max_bytes)
        Ks = [int(k) for k in Ks]
        if plan.n_users == 0:
            raise ZeroDivisionError("no test users")
        self._check_plan(plan)
        top = self._fused_topk("evaluate", plan.user_ids, plan.train_ptr, plan.train_items, Ks[-1], want_scores=False)[0]
        out = ops.eval_metrics_at_ks(top, plan.test_ptr, plan.test_items, Ks)
        mean = (out.sum(0) / plan.n_users).cpu().numpy()
        return {name: mean[:, m].copy() for m, name in enumerate(metrics.METRIC_NAMES)}

    def recommend(self, user_ids, K, seen=None):
        """The K best items of every user of ``user_ids`` (node ids) that the user has not seen, on the fused sweep:
        ``(items, scores)`` - int64 item NODE ids ``(len(user_ids), K)`` in rank order (score descending, equal scores by
        item position) and their float32 scores ``y(u, i)``; ``-1`` / ``-inf`` at the end where fewer than K items are
        unseen.  ``seen`` maps a user id to the item positions to leave out (None: nothing).  The counterpart of
        ``metrics.recommend``; one hidden layer, HIP tensors, 1 <= K <= 128 (``KGATLibraryError`` otherwise)."""
        users = [int(u) for u in np.asarray(user_ids).reshape(-1)]
        why = self._fused_refusal(K)
        if why is not None:
            raise ops.KGATLibraryError("recommend: %s" % why)
        lo = self.feats.item_offset
        item_ids = np.arange(lo, lo + self.feats.n_items)
        plan = metrics.EvalPlan(seen if seen is not None else {}, dict.fromkeys(users, metrics._EMPTY), item_ids,
                                self.embed.weight.device)
        if len(plan.user_ids) != len(users):
            raise ValueError("recommend: a user is listed twice")
        if plan.n_users and plan.max_node_id >= self.embed.weight.shape[0]:
            raise IndexError("user / item node id %d outside the table's %d rows" % (plan.max_node_id, self.embed.weight.shape[0]))
        pos, scores = self._fused_topk("recommend", plan.user_ids, plan.train_ptr, plan.train_items, K)
        pos = pos.long()
        return torch.where(pos >= 0, pos + lo, pos), scores
