"""The KGAT paper's path-based baseline, RippleNet (Wang et al., CIKM 2018), on fused ripple-set attention.

A user's *ripple set* of hop k is a fixed-size sample of knowledge-graph triples (h, r, t) whose heads the user reached
in k - 1 steps from the items of the training interactions (``RippleSets``, graph-static, built on the host).  The
model scores a (user, item) pair by letting the item vector v attend over each hop's set,

    s_i = v^T R_{r_i} ent[h_i]      p = softmax(s)      o_k = sum_i p_i ent[t_i]

updating v between hops, and ``y = <v, sum_k o_k>``.  The attention is one operator, ``autograd.ripple_hop``
(csrc/kgat_ripple.hip on a HIP device in fp32, ``ripple_hop_torch`` elsewhere); the per-relation queries
``U[b, r] = v_b R_r`` are one matmul per hop.  The evaluation scores all (user, item) pairs using that a ripple set
depends on the user only: by default in torch operators over user blocks (``scores``), with ``fused=True`` on the
all-pairs sweep of csrc/kgat_ripple_eval.hip (``ops.ripple_eval_keys`` + ``ops.ripple_eval_topk``: per user the items
attend over the hops' memories on the fp32 MFMA and the K best unseen items are selected on chip)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import metrics
from .fm_models import _long

UPDATE_MODES = ("replace", "plus", "replace_transform", "plus_transform")


class RippleSets:
    """int32 arrays ``mem_h``, ``mem_r``, ``mem_t`` of shape [n_users, n_hop, n_memory]: the triples of every user's
    ripple set per hop, inside a (user, hop) sorted ascending by (r, h, t) - equal relations are consecutive, which the
    kernels rely on.  ``valid[user]`` is False where the user's items have no triple at all (the set is then a filler).
    Holds host arrays and per-device copies; ``to(device)`` gives a view object on another device."""

    def __init__(self, mem_h, mem_r, mem_t, n_nodes, n_rel, valid=None, device="cpu"):
        arrays = [np.ascontiguousarray(np.asarray(x, dtype=np.int64)) for x in (mem_h, mem_r, mem_t)]
        if arrays[0].ndim != 3 or any(x.shape != arrays[0].shape for x in arrays):
            raise ValueError("RippleSets: mem_h, mem_r, mem_t must share one shape [n_users, n_hop, n_memory]")
        n_users, n_hop, M = arrays[0].shape
        n_nodes, n_rel = int(n_nodes), int(n_rel)
        if not 1 <= n_hop <= 4:
            raise ValueError("RippleSets: n_hop must be in 1..4, got %d" % n_hop)
        if not 1 <= M <= 128:
            raise ValueError("RippleSets: n_memory must be in 1..128, got %d" % M)
        if not (0 < n_users and 0 < n_nodes < 2 ** 31 - 1 and 0 < n_rel < 2 ** 31 - 1 and n_users * n_hop * M < 2 ** 31 - 1):
            raise ValueError("RippleSets: sizes must be positive and stay below 2^31")
        h, r, t = arrays
        if min(h.min(), t.min()) < 0 or max(h.max(), t.max()) >= n_nodes or r.min() < 0 or r.max() >= n_rel:
            raise ValueError("RippleSets: node ids must lie in [0, %d) and relation ids in [0, %d)" % (n_nodes, n_rel))
        if (np.diff(r, axis=2) < 0).any():
            raise ValueError("RippleSets: the relations of a set must be ascending")
        self.n_users, self.n_hop, self.n_memory, self.n_nodes, self.n_rel = n_users, n_hop, M, n_nodes, n_rel
        self.valid = np.ones(n_users, bool) if valid is None else np.asarray(valid, bool).reshape(n_users).copy()
        self._host = {"mem_h": h.astype(np.int32), "mem_r": r.astype(np.int32), "mem_t": t.astype(np.int32)}
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
        other = object.__new__(RippleSets)
        other.__dict__.update(self.__dict__)
        other._place(device)
        return other

    @classmethod
    def build(cls, triplets, train_pairs, n_users, n_nodes, n_hop=2, n_memory=32, seed=0, add_inverse=False, device="cpu"):
        """Ripple sets from the collaborative KG's triples (h, r, t) and the training pairs (user, item node id).

        The adjacency holds the triples whose head and tail are both non-user nodes (ids >= n_users, the layout of
        ``ckg_io.CKGDataset``: the interaction relations drop out); ``add_inverse`` appends (t, r + n_kg_rel, h) for each,
        n_kg_rel = 1 + the largest kept relation id.  ``n_rel`` counts the relation ids after this step.  Hop 1 heads are
        the user's training items, hop k heads the distinct tails of hop k - 1.  A hop's candidates are all triples whose
        head is among the heads, in ascending (h, r, t) order; its set is the ``n_memory`` candidates
        ``np.random.default_rng([seed, user, k]).choice(n_cand, n_memory, replace=n_cand < n_memory)`` picks (k = 1 for
        the first hop), so a user's sets depend on no other user.  A hop without candidates copies the previous hop's
        set; an empty first hop is filled with (i0, 0, i0), i0 the user's first training item (the first non-user node
        for a user without any), and the user is marked ``valid[user] = False``."""
        n_users, n_nodes, n_hop, M = int(n_users), int(n_nodes), int(n_hop), int(n_memory)
        if not 1 <= n_hop <= 4:
            raise ValueError("RippleSets: n_hop must be in 1..4, got %d" % n_hop)
        if not 1 <= M <= 128:
            raise ValueError("RippleSets: n_memory must be in 1..128, got %d" % M)
        if not 0 < n_users < n_nodes < 2 ** 31 - 1:
            raise ValueError("RippleSets: needs 0 < n_users < n_nodes < 2^31")
        trip = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
        pairs = np.asarray(train_pairs, dtype=np.int64)
        pairs = pairs.reshape(-1, pairs.shape[-1] if pairs.ndim > 1 else 2)[:, :2]
        if len(trip) and (trip[:, [0, 2]].min() < 0 or trip[:, [0, 2]].max() >= n_nodes or trip[:, 1].min() < 0 or
                          trip[:, 1].max() >= 2 ** 30):
            raise ValueError("RippleSets: triple ids out of range")
        if len(pairs) and (pairs[:, 0].min() < 0 or pairs[:, 0].max() >= n_users or pairs[:, 1].min() < n_users or
                           pairs[:, 1].max() >= n_nodes):
            raise ValueError("RippleSets: training pairs need users in [0, %d) and item node ids in [%d, %d)"
                             % (n_users, n_users, n_nodes))
        kg = trip[(trip[:, 0] >= n_users) & (trip[:, 2] >= n_users)]
        n_rel = int(kg[:, 1].max()) + 1 if len(kg) else 1
        if add_inverse and len(kg):
            kg = np.vstack([kg, np.stack([kg[:, 2], kg[:, 1] + n_rel, kg[:, 0]], 1)])
            n_rel *= 2
        kg = np.unique(kg, axis=0) if len(kg) else kg      # ascending (h, r, t), a triple once
        kh, kr, kt = (np.ascontiguousarray(kg[:, c]) for c in range(3))
        start = np.zeros(n_nodes + 1, dtype=np.int64)
        np.cumsum(np.bincount(kh, minlength=n_nodes), out=start[1:])
        order = np.argsort(pairs[:, 0], kind="stable")
        p_user, p_item = pairs[order, 0], pairs[order, 1]
        u_ptr = np.zeros(n_users + 1, dtype=np.int64)
        np.cumsum(np.bincount(p_user, minlength=n_users), out=u_ptr[1:])
        mem = np.zeros((3, n_users, n_hop, M), dtype=np.int64)
        valid = np.ones(n_users, bool)
        for u in range(n_users):
            own = p_item[u_ptr[u]:u_ptr[u + 1]]
            heads = np.unique(own)
            for k in range(n_hop):
                deg = start[heads + 1] - start[heads]
                n_cand = int(deg.sum())
                if n_cand == 0:
                    if k == 0:
                        i0 = int(own[0]) if len(own) else n_users
                        mem[0, u, 0], mem[1, u, 0], mem[2, u, 0] = i0, 0, i0
                        valid[u] = False
                    else:
                        mem[:, u, k] = mem[:, u, k - 1]
                else:
                    pick = np.random.default_rng([int(seed), u, k + 1]).choice(n_cand, M, replace=n_cand < M)
                    ends = np.cumsum(deg)
                    which = np.searchsorted(ends, pick, side="right")
                    pos = start[heads[which]] + (pick - (ends[which] - deg[which]))
                    h, r, t = kh[pos], kr[pos], kt[pos]
                    o = np.lexsort((t, h, r))
                    mem[0, u, k], mem[1, u, k], mem[2, u, k] = h[o], r[o], t[o]
                heads = np.unique(mem[2, u, k])
        return cls(mem[0], mem[1], mem[2], n_nodes, n_rel, valid=valid, device=device)


def _L2_loss_mean(x):
    return torch.mean(torch.sum(torch.pow(x, 2), dim=1, keepdim=False) / 2.0)


class RippleNet(nn.Module):
    """RippleNet over the ripple sets `sets`; parameters under the release's names: ``entity_emb.weight`` (n_nodes, d),
    ``relation_emb.weight`` (n_rel, d * d) and ``transform_matrix.weight`` (d, d), no bias.  Item arguments are node
    ids.  ``item_range = (lo, hi)``: the node ids ``scores`` ranks (default: every non-user node)."""

    def __init__(self, n_nodes, sets, dim=16, kge_weight=0.01, reg_lambda=1e-7, item_update_mode="plus_transform",
                 using_all_hops=True, item_range=None):
        super().__init__()
        if sets.n_nodes != int(n_nodes):
            raise ValueError("the ripple sets index %d nodes, the model %d" % (sets.n_nodes, n_nodes))
        if item_update_mode not in UPDATE_MODES:
            raise ValueError("item_update_mode must be one of %s" % (UPDATE_MODES,))
        self.sets = sets
        self.dim, self.kge_weight, self.reg_lambda = int(dim), float(kge_weight), float(reg_lambda)
        self.item_update_mode, self.using_all_hops = item_update_mode, bool(using_all_hops)
        self.item_range = (sets.n_users, int(n_nodes)) if item_range is None else (int(item_range[0]), int(item_range[1]))
        if not 0 <= self.item_range[0] < self.item_range[1] <= n_nodes:
            raise ValueError("item_range %r outside [0, %d]" % (self.item_range, n_nodes))
        self.entity_emb = nn.Embedding(n_nodes, dim)
        self.relation_emb = nn.Embedding(sets.n_rel, dim * dim)
        self.transform_matrix = nn.Linear(dim, dim, bias=False)
        # Xavier tables, as the release's TensorFlow original and this package's other baselines: with nn.Embedding's
        # N(0, 1) entries a logit v^T R h is a sum of d^2 products of three unit normals and the softmax starts saturated
        nn.init.xavier_uniform_(self.entity_emb.weight)
        nn.init.uniform_(self.relation_emb.weight, -(3.0 / dim) ** 0.5, (3.0 / dim) ** 0.5)

    def queries(self, v):
        """U (n_samples, n_rel, d), ``U[b, r] = v_b R_r``: one matmul."""
        d, n_rel = self.dim, self.sets.n_rel
        R = self.relation_emb.weight.view(n_rel, d, d)
        return (v @ R.permute(1, 0, 2).reshape(d, n_rel * d)).view(-1, n_rel, d)

    def _update(self, v, o):
        mode = self.item_update_mode
        if mode == "replace":
            return o
        if mode == "plus":
            return v + o
        if mode == "replace_transform":
            return self.transform_matrix(o)
        return self.transform_matrix(v + o)

    def _predict(self, v, o_list):
        y = o_list[-1]
        if self.using_all_hops:
            for o in o_list[:-1]:
                y = y + o
        return (v * y).sum(-1)

    def hops(self, users, items):
        """(v_H, [o_1 .. o_H]) of the pairs: the item vector after every hop's update and the hops' responses."""
        from .autograd import ripple_hop
        ent = self.entity_emb.weight
        users = torch.as_tensor(users, device=ent.device)
        v = ent.index_select(0, _long(items, ent.device))
        o_list = []
        for k in range(self.sets.n_hop):
            o = ripple_hop(ent, self.queries(v), self.sets, users, k)
            o_list.append(o)
            v = self._update(v, o)
        return v, o_list

    def score(self, users, items):
        v, o_list = self.hops(users, items)
        return self._predict(v, o_list)

    def kge_term(self, users):
        """``-mean sigmoid(h^T R_r t)`` over the hop triples of the distinct users among `users`: torch operators,
        relation by relation on relation-sorted segments (the segment sizes are read on the host)."""
        ent, d = self.entity_emb.weight, self.dim
        sets = self.sets.to(ent.device)
        uu = torch.unique(_long(users, ent.device))
        h, r, t = (getattr(sets, name)[uu].reshape(-1).long() for name in ("mem_h", "mem_r", "mem_t"))
        r, order = torch.sort(r, stable=True)
        h, t = h[order], t[order]
        counts = torch.bincount(r, minlength=sets.n_rel).cpu().tolist()
        R = self.relation_emb.weight.view(sets.n_rel, d, d)
        parts, lo = [], 0
        for rel, n in enumerate(counts):
            if n:
                parts.append(((ent.index_select(0, h[lo:lo + n]) @ R[rel]) * ent.index_select(0, t[lo:lo + n])).sum(1))
                lo += n
        return -torch.sigmoid(torch.cat(parts)).mean()

    def get_loss(self, u, pos, neg):
        """``BCE-with-logits(y, [1 .. 1, 0 .. 0]) + kge_weight * kge_term + reg_lambda * L2``: one pass over the 2 B
        samples, positives first.  L2 is ``_L2_loss_mean`` of the item rows, of every o_k, of R and of W."""
        ent = self.entity_emb.weight
        b = u.numel()
        users, items = torch.cat([u, u]), _long(torch.cat([pos, neg]), ent.device)
        v, o_list = self.hops(users, items)
        y = self._predict(v, o_list)
        labels = torch.cat([torch.ones(b, dtype=y.dtype, device=y.device), torch.zeros(b, dtype=y.dtype, device=y.device)])
        loss = F.binary_cross_entropy_with_logits(y, labels)
        if self.kge_weight != 0:
            loss = loss + self.kge_weight * self.kge_term(u)
        l2 = _L2_loss_mean(ent.index_select(0, items)) + _L2_loss_mean(self.relation_emb.weight) + \
            _L2_loss_mean(self.transform_matrix.weight)
        for o in o_list:
            l2 = l2 + _L2_loss_mean(o)
        return loss + self.reg_lambda * l2

    @property
    def n_items(self):
        return self.item_range[1] - self.item_range[0]

    @torch.no_grad()
    def scores(self, users, max_bytes=1 << 28):
        """The (len(users), n_items) score matrix in torch operators over user blocks: with ``Rh = R_{r_i} ent[h_i]`` per
        user (a set depends on the user only), hop 1's logits are ``Rh @ V_items^T``, softmax over the slots,
        ``o = p^T T``; later hops through einsum on the updated item vectors.  A block's tensors stay below `max_bytes`."""
        ent, d = self.entity_emb.weight, self.dim
        sets = self.sets.to(ent.device)
        users = _long(users, ent.device)
        lo, hi = self.item_range
        n_items, M = hi - lo, sets.n_memory
        V = ent[lo:hi]
        R = self.relation_emb.weight.view(sets.n_rel, d, d)
        per_user = ent.element_size() * (n_items * (4 * d + 2 * M) + M * d * (d + 2))
        block = max(1, int(max_bytes // max(1, per_user)))
        out = []
        for b0 in range(0, users.numel(), block):
            us = users[b0:b0 + block]
            v = V.unsqueeze(0).expand(us.numel(), n_items, d)
            o_list = []
            for k in range(sets.n_hop):
                h, r, t = (getattr(sets, name)[us, k].long() for name in ("mem_h", "mem_r", "mem_t"))
                Rh = torch.bmm(R[r.reshape(-1)], ent[h.reshape(-1)].unsqueeze(2)).view(us.numel(), M, d)
                logits = Rh @ V.t() if k == 0 else torch.einsum("umd,uid->umi", Rh, v)
                p = torch.softmax(logits, 1)
                o = torch.einsum("umi,umd->uid", p, ent[t.reshape(-1)].view(us.numel(), M, d))
                o_list.append(o)
                v = self._update(v, o)
            out.append(self._predict(v, o_list))
        return torch.cat(out, 0) if out else torch.zeros(0, n_items, dtype=ent.dtype, device=ent.device)

    def _fused_refusal(self, K):
        """Why the fused sweep cannot evaluate this model at depth K (None: it can)."""
        from . import ops
        ent, sets = self.entity_emb.weight, self.sets
        if not ent.is_cuda:
            return "the parameters are on %s: the fused sweep only runs on a HIP device (CPU tensors)" % ent.device
        if ent.dtype != torch.float32:
            return "the parameters are %s, the fused sweep is float32" % ent.dtype
        if not 1 <= int(K) <= ops.RIPPLE_EVAL_MAX_K:
            return "K = %d is outside 1..%d" % (K, ops.RIPPLE_EVAL_MAX_K)
        if not ops.ripple_eval_supported(self.dim, sets.n_memory, sets.n_hop, UPDATE_MODES.index(self.item_update_mode), K):
            return "d = %d, n_memory = %d, n_hop = %d: the fused sweep takes d in (16, 32, 64), n_memory in 1..64, n_hop " \
                   "in (1, 2)" % (self.dim, sets.n_memory, sets.n_hop)
        return None

    @torch.no_grad()
    def _fused_topk(self, what, user_ids, train_ptr, train_items, K, max_bytes=1 << 28, want_scores=True):
        """``ops.ripple_eval_topk`` for the users `user_ids` (int32): the items laid out once, then per user block - sized
        so that its key table stays below `max_bytes` - the keys pass and the sweep."""
        from . import ops
        why = self._fused_refusal(K)
        if why is not None:
            raise ops.KGATLibraryError("%s(fused=True): %s" % (what, why))
        ent = self.entity_emb.weight.detach().contiguous()
        sets = self.sets.to(ent.device)
        rel = self.relation_emb.weight.detach().contiguous()
        mode = UPDATE_MODES.index(self.item_update_mode)
        W = self.transform_matrix.weight.detach().contiguous() if mode >= 2 else None
        lo, hi = self.item_range
        itemT = ops.ripple_eval_items(ent, lo, hi)
        n = user_ids.numel()
        block = max(1, int(max_bytes // (4 * sets.n_hop * sets.n_memory * self.dim)))
        ptr = train_ptr.cpu() if n > block else None
        tops, scs = [], []
        for b0 in range(0, n, block):
            b1 = min(b0 + block, n)
            us = user_ids[b0:b1].contiguous()
            if ptr is None:
                tp, ti = train_ptr, train_items
            else:
                first, last = int(ptr[b0]), int(ptr[b1])
                tp, ti = (train_ptr[b0:b1 + 1] - first).contiguous(), train_items[first:last].contiguous()
            keys = ops.ripple_eval_keys(ent, rel, sets, us)
            top, sc = ops.ripple_eval_topk(ent, sets, us, keys, itemT, hi - lo, W, mode, self.using_all_hops, tp, ti, K,
                                           want_scores=want_scores)
            tops.append(top)
            scs.append(sc)
        if not tops:
            return (torch.zeros(0, K, dtype=torch.int32, device=ent.device),
                    torch.zeros(0, K, dtype=torch.float32, device=ent.device) if want_scores else None)
        if len(tops) == 1:
            return tops[0], scs[0]
        return torch.cat(tops, 0), (torch.cat(scs, 0) if want_scores else None)

    def _check_plan(self, plan):
        if plan.n_items != self.n_items:
            raise ValueError("topk: the plan ranks %d items, the model scores %d" % (plan.n_items, self.n_items))

    def topk(self, plan, K, max_bytes=1 << 28, fused=False):
        """The K best unseen items of every user of an ``EvalPlan`` as item positions, (n_users, K) int32.  Default:
        ``metrics.topk_unseen`` over ``scores`` (``torch.topk``).  ``fused=True``: the all-pairs sweep
        (``ops.ripple_eval_topk``) - score descending, equal scores by item position, ``-1`` where a user has fewer than
        K unseen items; ``KGATLibraryError`` naming the reason where the model or the device is outside its envelope."""
        if not fused:
            return metrics.topk_unseen(self.scores, self.n_items, plan, K, max_bytes)
        self._check_plan(plan)
        return self._fused_topk("topk", plan.user_ids, plan.train_ptr, plan.train_items, K, max_bytes, want_scores=False)[0]

    def evaluate(self, plan, Ks=(20,), max_bytes=1 << 28, fused=False):
        """Mean recall / ndcg / precision / hit_ratio at the ascending cut-offs `Ks` for an ``EvalPlan``: the dict
        ``metrics.calc_metrics`` returns.  Default: ``metrics.calc_metrics_unseen`` over ``scores``.  ``fused=True``:
        ``topk(fused=True)`` at the largest cut-off, then ``ops.eval_metrics_at_ks``."""
        if not fused:
            return metrics.calc_metrics_unseen(self.scores, self.n_items, plan, Ks, max_bytes)
        from . import ops
        Ks = [int(k) for k in Ks]
        if plan.n_users == 0:
            raise ZeroDivisionError("no test users")
        self._check_plan(plan)
        top = self._fused_topk("evaluate", plan.user_ids, plan.train_ptr, plan.train_items, Ks[-1], max_bytes,
                               want_scores=False)[0].contiguous()
        out = ops.eval_metrics_at_ks(top, plan.test_ptr, plan.test_items, Ks)
        mean = (out.sum(0) / plan.n_users).cpu().numpy()
        return {name: mean[:, m].copy() for m, name in enumerate(metrics.METRIC_NAMES)}

    def recommend(self, user_ids, K, seen=None):
        """The K best items of every user of ``user_ids`` that the user has not seen, on the fused sweep: ``(items,
        scores)`` - int64 item NODE ids ``(len(user_ids), K)`` in rank order (score descending, equal scores by item
        position) and their float32 scores ``y(u, i)``; ``-1`` / ``-inf`` at the end where fewer than K items are unseen.
        ``seen`` maps a user id to the item positions to leave out (None: nothing).  HIP tensors, 1 <= K <= 128
        (``KGATLibraryError`` otherwise)."""
        from . import ops
        users = [int(u) for u in np.asarray(user_ids).reshape(-1)]
        why = self._fused_refusal(K)
        if why is not None:
            raise ops.KGATLibraryError("recommend: %s" % why)
        lo, hi = self.item_range
        plan = metrics.EvalPlan(seen if seen is not None else {}, dict.fromkeys(users, metrics._EMPTY), np.arange(lo, hi),
                                self.entity_emb.weight.device)
        if len(plan.user_ids) != len(users):
            raise ValueError("recommend: a user is listed twice")
        if users and not 0 <= min(users) <= max(users) < self.sets.n_users:
            raise IndexError("user id outside the ripple sets' %d users" % self.sets.n_users)
        pos, scores = self._fused_topk("recommend", plan.user_ids, plan.train_ptr, plan.train_items, K)
        pos = pos.long()
        return torch.where(pos >= 0, pos + lo, pos), scores
