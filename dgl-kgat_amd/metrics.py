"""recall@K / ndcg@K of the reference (``metric.py:36-68``) on the device.

Same definitions, including the reference's quirks: training items are masked by setting their
score to 0.0 (not -inf), and the ideal DCG of a user is the DCG of that user's *own* hit list
sorted (``one_ndcg_at_k``), not the DCG of min(|positives|, K) leading ones.

``calc_recall_ndcg`` runs ``kgat_eval_recall_ndcg_f32`` (csrc/kgat_eval.hip): the user x item
scores come out of the fp32 MFMA tile by tile and go straight into a running top-K per user -
no (users x items) score matrix, no sort of 24,915 scores per user.  Equal scores rank by item
position (what the reference's stable CPU ``th.sort`` gives: among the masked zeros the lower
index first).  ``calc_recall_ndcg_sorted`` is the batched matmul + full stable sort of rounds
1-4, kept as an independent check of the kernel (tests); nothing dispatches to it.

``calc_metrics`` gives the KGAT paper's table - recall, ndcg, precision and hit ratio at several
cut-offs up to 128 - from one sweep at the largest cut-off (``kgat_eval_topk_f32`` +
``kgat_eval_metrics_at_ks``, csrc/kgat_eval_topk.hip); ``recommend`` returns the K best unseen
items of a list of users with their scores.

``rank_items`` gives the exact rank of every held-out item at any depth and ``calc_rank_metrics`` the metrics that
follow from it - the four above at any cut-off up to the number of items, MRR, MAP, AUC and the mean rank - from one
counting sweep (``kgat_eval_rank_f32`` + ``kgat_eval_rank_metrics``, csrc/kgat_eval_rank.hip): no list, so no K.
"""
import numpy as np
import torch


_EMPTY = np.zeros(0, dtype=np.int64)


class EvalPlan:
    """The static part of an evaluation: test users, item node ids and the users' train / test item lists as CSR
    arrays on the device (positions ascending per user).  Build once per (train, test) split and pass it as
    ``plan=``; the dicts are read when the plan is built, never again.

    Train lists are de-duplicated (the reference masks ``score[train_items] = 0.0`` - an item listed twice is masked
    once, ``metric.py:50``); test lists keep their duplicates (``len(pos_item_l)`` counts them, ``metric.py:24``).
    Built with array operations over the concatenated lists: one dict lookup per user is the only per-user Python
    step (amazon-book: 650 k pairs, ~0.3 s; the per-user ``np.sort`` loops of round 5 took seconds)."""

    def __init__(self, train_user_dict, test_user_dict, all_item_id_range, device):
        users = list(test_user_dict.keys())
        self.n_users = len(users)
        items = np.asarray(all_item_id_range, dtype=np.int64).reshape(-1)
        self.n_items = len(items)
        n_items = max(self.n_items, 1)

        def csr(d, name, unique):
            lists = [d.get(u, _EMPTY) for u in users]
            lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
            total = int(lens.sum())
            if total >= 2 ** 31:
                raise ValueError("more than 2^31 (user, item) pairs")
            if total == 0:
                return (torch.zeros(len(users) + 1, dtype=torch.int32, device=device),
                        torch.zeros(0, dtype=torch.int32, device=device))
            flat = np.concatenate([np.asarray(x).reshape(-1) for x in lists if len(x)]).astype(np.int64, copy=False)
            owner = np.repeat(np.arange(len(users), dtype=np.int64), lens)
            bad = (flat < 0) | (flat >= self.n_items)
            if bad.any():
                # (the reference would index `score` out of range, metric.py:50)
                raise IndexError("%s items of user %r outside [0, %d)" % (name, users[int(owner[np.argmax(bad)])],
                                                                          self.n_items))
            key = owner * n_items + flat                  # one sort orders users and, within a user, positions
            key = np.unique(key) if unique else np.sort(key)
            owner = key // n_items
            ptr = np.zeros(len(users) + 1, dtype=np.int64)
            np.cumsum(np.bincount(owner, minlength=len(users)), out=ptr[1:])
            return (torch.as_tensor(ptr.astype(np.int32), device=device),
                    torch.as_tensor((key - owner * n_items).astype(np.int32), device=device))

        u = np.asarray(users, dtype=np.int64).reshape(-1)
        if u.size and (u.min() < 0 or u.max() >= 2 ** 31 or (items.size and (items.min() < 0 or items.max() >= 2 ** 31))):
            raise IndexError("user / item node ids must lie in [0, 2^31)")
        self.max_node_id = int(max(u.max() if u.size else -1, items.max() if items.size else -1))
        self.user_ids = torch.as_tensor(u.astype(np.int32), device=device)
        self.item_ids = torch.as_tensor(items.astype(np.int32), device=device)
        self.train_ptr, self.train_items = csr(train_user_dict, "train", True)
        self.test_ptr, self.test_items = csr(test_user_dict, "test", False)


def calc_recall_ndcg(embedding, train_user_dict, test_user_dict, all_item_id_range, K=20, plan=None,
                     return_per_user=False):
    """``embedding`` (N, F) node embeddings on the HIP device; the dicts map a user id to the array of its (raw,
    un-shifted) item ids; ``all_item_id_range`` the node ids of the items.  As the reference does
    (``metric.py:36-68``), the dicts are read on EVERY call - nothing is cached between calls; a caller that
    evaluates the same split repeatedly builds an ``EvalPlan`` once and passes it as ``plan=`` (the dicts are then
    ignored).

    Restrictions (no CPU / PyTorch fallback, by design): ``embedding`` must live on the HIP device
    (``KGATLibraryError`` otherwise), K <= 32; a float64 embedding is ranked in float32 - the kernel's
    arithmetic, and what the reference's fp32 model produces - so near-ties of a float64 input can rank
    differently than a float64 sort would rank them.  ``calc_recall_ndcg_sorted`` (torch operators) takes any K,
    dtype and device.  K up to 128, several cut-offs at once, precision and hit ratio: ``calc_metrics``."""
    from . import ops
    if plan is None:
        plan = EvalPlan(train_user_dict, test_user_dict, all_item_id_range, embedding.device)
    if plan.n_users == 0:
        raise ZeroDivisionError("no test users")   # (metric.py:65 divides by len(test_user_dict))
    if plan.max_node_id >= embedding.shape[0]:
        # (the reference's embedding[user_id] / embedding[all_item_id_range] raises IndexError, metric.py:44-46)
        raise IndexError("user / item node id %d outside the embedding's %d rows" % (plan.max_node_id,
                                                                                    embedding.shape[0]))
    emb = embedding.detach()
    if emb.dtype != torch.float32:
        emb = emb.float()
    if emb.stride(1) != 1:
        emb = emb.contiguous()
    with torch.no_grad():
        recall, ndcg = ops.eval_recall_ndcg(emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items,
                                            plan.test_ptr, plan.test_items, K)
    if return_per_user:
        return recall, ndcg
    return float(recall.sum()) / plan.n_users, float(ndcg.sum()) / plan.n_users


def _device_rows(embedding, what):
    from .ops import KGATLibraryError
    if not embedding.is_cuda:
        raise KGATLibraryError("%s: the embedding is on %s: the evaluation only runs on a HIP device (no CPU "
                               "implementation exists in this package)" % (what, embedding.device))
    emb = embedding.detach()
    if emb.dtype != torch.float32:
        emb = emb.float()
    if emb.stride(1) != 1:
        emb = emb.contiguous()
    return emb


METRIC_NAMES = ("recall", "ndcg", "precision", "hit_ratio")


def calc_metrics(embedding, train_user_dict, test_user_dict, all_item_id_range, Ks=(20, 40, 60, 80, 100), plan=None,
                 return_per_user=False):
    """recall, ndcg, precision and hit ratio at every cut-off of ``Ks`` (ascending, distinct, at most 8, each <= 128 -
    the KGAT paper's table is ``(20, 40, 60, 80, 100)``): one item layout pass, one sweep at ``max(Ks)`` and one
    metrics launch.  Inputs, masking rule (``metric.py:50``), checks and exceptions as ``calc_recall_ndcg``; recall and
    ndcg are the reference's (``metric.py:5-7, 23-34``) applied to the first k ranks, precision = hits / k, hit ratio =
    1 if any hit.  Returns a dict ``{"recall", "ndcg", "precision", "hit_ratio"}`` of float64 numpy arrays of
    ``len(Ks)`` - means over the test users - or, with ``return_per_user``, of ``(n_users, len(Ks))`` tensors."""
    from . import ops
    Ks = [int(k) for k in Ks]
    if not 1 <= len(Ks) <= 8:
        raise ValueError("calc_metrics: 1 to 8 cut-offs, got %d" % len(Ks))
    if Ks[0] < 1 or any(b <= a for a, b in zip(Ks, Ks[1:])):
        raise ValueError("calc_metrics: the cut-offs must be positive, ascending and distinct: %r" % (Ks,))
    if Ks[-1] > 128:
        raise ops.KGATLibraryError("calc_metrics: cut-off %d is beyond the kernel's 128" % Ks[-1])
    emb = _device_rows(embedding, "calc_metrics")
    if plan is None:
        plan = EvalPlan(train_user_dict, test_user_dict, all_item_id_range, embedding.device)
    if plan.n_users == 0:
        raise ZeroDivisionError("no test users")   # (metric.py:65 divides by len(test_user_dict))
    if plan.max_node_id >= embedding.shape[0]:
        raise IndexError("user / item node id %d outside the embedding's %d rows" % (plan.max_node_id,
                                                                                    embedding.shape[0]))
    with torch.no_grad():
        topk = ops.eval_topk(emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, Ks[-1],
                             want_scores=False)
        out = ops.eval_metrics_at_ks(topk, plan.test_ptr, plan.test_items, Ks)
    if return_per_user:
        return {name: out[:, :, m] for m, name in enumerate(METRIC_NAMES)}
    mean = (out.sum(0) / plan.n_users).cpu().numpy()
    return {name: mean[:, m].copy() for m, name in enumerate(METRIC_NAMES)}


@torch.no_grad()
def topk_unseen(scores, n_items, plan, K, max_bytes=1 << 28):
    """The K best unseen items of every user of an ``EvalPlan`` (its training items dropped), as item positions: an
    (n_users, K) int32 tensor, best first (``torch.topk``) - for a model whose scores are no dot product of table rows
    (``fm_models.NFM``, ``ripple_models.RippleNet``).  ``scores(users, max_bytes)`` returns the (len(users), n_items)
    score matrix of a block of user node ids (int64, on the plan's device); the blocks are sized so that a block's
    matrix, its mask indices and ``torch.topk``'s outputs stay below `max_bytes`."""
    if plan.n_items != n_items:
        raise ValueError("topk: the plan ranks %d items, the model scores %d" % (plan.n_items, n_items))
    if not 1 <= K <= n_items:
        raise ValueError("topk: K must be in [1, %d]" % n_items)
    users = plan.user_ids.long()
    tp = plan.train_ptr.long()
    out = []
    step = max(1, int(max_bytes // (max(1, n_items) * 4 * 4)))
    for lo in range(0, users.numel(), step):
        hi = min(lo + step, users.numel())
        sc = scores(users[lo:hi], max_bytes)
        seen = plan.train_items[int(tp[lo]):int(tp[hi])].long()
        row = torch.repeat_interleave(torch.arange(hi - lo, device=sc.device), tp[lo + 1:hi + 1] - tp[lo:hi])
        sc[row, seen] = float("-inf")
        out.append(torch.topk(sc, K, dim=1).indices.to(torch.int32))
    return torch.cat(out, 0) if out else torch.zeros(0, K, dtype=torch.int32, device=users.device)


def calc_metrics_unseen(scores, n_items, plan, Ks=(20,), max_bytes=1 << 28):
    """Mean recall / ndcg / precision / hit_ratio at the ascending cut-offs `Ks` for an ``EvalPlan`` and a block score
    function: ``topk_unseen`` at the largest cut-off, then the metric kernel of ``calc_metrics``
    (``ops.eval_metrics_at_ks``).  Returns the dict ``calc_metrics`` returns."""
    from . import ops
    Ks = [int(k) for k in Ks]
    if plan.n_users == 0:
        raise ZeroDivisionError("no test users")
    top = topk_unseen(scores, n_items, plan, Ks[-1], max_bytes).contiguous()
    out = ops.eval_metrics_at_ks(top, plan.test_ptr, plan.test_items, Ks)
    mean = (out.sum(0) / plan.n_users).cpu().numpy()
    return {name: mean[:, m].copy() for m, name in enumerate(METRIC_NAMES)}


RANK_SCALAR_NAMES = ("mrr", "map", "auc", "mean_rank")


def _rank_inputs(embedding, train_user_dict, test_user_dict, all_item_id_range, plan, mode, what):
    if mode not in ("mask", "drop"):
        raise ValueError("%s: mode must be 'mask' or 'drop', got %r" % (what, mode))
    emb = _device_rows(embedding, what)
    if plan is None:
        plan = EvalPlan(train_user_dict, test_user_dict, all_item_id_range, embedding.device)
    if plan.n_users == 0:
        raise ZeroDivisionError("no test users")   # (metric.py:65 divides by len(test_user_dict))
    if plan.max_node_id >= embedding.shape[0]:
        raise IndexError("user / item node id %d outside the embedding's %d rows" % (plan.max_node_id,
                                                                                    embedding.shape[0]))
    return emb, plan


def rank_items(embedding, train_user_dict, test_user_dict, all_item_id_range, plan=None, mode="mask"):
    """Where every held-out item landed: ``(ranks, ptr)`` - ``ranks`` an int64 device tensor with the 1-based rank of
    every test entry in the order of the plan's test CSR (per user the item positions ascending, duplicates kept), ``ptr``
    that CSR's pointer (user ``j`` of the plan owns ``ranks[ptr[j]:ptr[j + 1]]``).  The order is the evaluation's:
    score descending, equal scores by item position, so ``rank <= K`` exactly when ``kgat_eval_topk_f32`` lists the
    item at place ``rank - 1``.  ``mode="mask"`` is the reference's rule (``metric.py:50``: a training item competes at
    score 0.0); ``mode="drop"`` ranks among the items the user has not trained on, and a test entry that is itself a
    training item is not ranked: 0.  Inputs, checks and exceptions as ``calc_metrics``; no limit on a list's length."""
    from . import ops
    emb, plan = _rank_inputs(embedding, train_user_dict, test_user_dict, all_item_id_range, plan, mode, "rank_items")
    with torch.no_grad():
        above = ops.eval_rank(emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, plan.test_ptr,
                              plan.test_items, drop_train=mode == "drop")
    return above.long() + 1, plan.test_ptr


def calc_rank_metrics(embedding, train_user_dict, test_user_dict, all_item_id_range, Ks=(20, 100, 500), plan=None,
                      mode="mask", return_per_user=False):
    """recall, ndcg, precision and hit ratio at every cut-off of ``Ks`` (ascending, distinct, at most 64, each within
    1..n_items - no 128) and MRR, MAP, AUC and the mean rank, from the exact ranks of the held-out items
    (``rank_items``): one item layout pass, one counting sweep, one metrics launch.  The four metrics at a cut-off are
    ``calc_metrics``'s (a duplicated test item hits once and counts twice in recall's denominator, ``metric.py:24,61``);
    over a user's T distinct ranked test items with 0-based ranks a_0 < ... < a_{T-1} among C candidates,
    mrr = 1 / (a_0 + 1), map = mean_j (j + 1) / (a_j + 1), auc = 1 - sum_j (a_j - j) / (T (C - T)) - the share of
    (held-out, other) pairs ranked the right way round - and mean_rank = mean_j (a_j + 1); a user without a ranked
    item has 0 in all four.  ``mode`` as ``rank_items``.  Returns a dict: ``recall`` / ``ndcg`` / ``precision`` /
    ``hit_ratio`` float64 arrays of ``len(Ks)`` and ``mrr`` / ``map`` / ``auc`` / ``mean_rank`` floats - means over the
    test users, as ``calc_metrics`` - or, with ``return_per_user``, ``(n_users, len(Ks))`` and ``(n_users,)`` tensors.
    Checks and exceptions as ``calc_metrics``; a cut-off above the number of items or a list that does not ascend
    raises ``ValueError``."""
    from . import ops
    Ks = [int(k) for k in Ks]
    if not 1 <= len(Ks) <= ops.EVAL_RANK_MAX_KS:
        raise ValueError("calc_rank_metrics: 1 to %d cut-offs, got %d" % (ops.EVAL_RANK_MAX_KS, len(Ks)))
    if Ks[0] < 1 or any(b <= a for a, b in zip(Ks, Ks[1:])):
        raise ValueError("calc_rank_metrics: the cut-offs must be positive, ascending and distinct: %r" % (Ks,))
    n_items = plan.n_items if plan is not None else int(np.asarray(all_item_id_range).size)
    if Ks[-1] > n_items:
        raise ValueError("calc_rank_metrics: cut-off %d is beyond the %d items" % (Ks[-1], n_items))
    emb, plan = _rank_inputs(embedding, train_user_dict, test_user_dict, all_item_id_range, plan, mode,
                             "calc_rank_metrics")
    drop = mode == "drop"
    with torch.no_grad():
        above = ops.eval_rank(emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, plan.test_ptr,
                              plan.test_items, drop_train=drop)
        n_cand = (plan.n_items - (plan.train_ptr[1:] - plan.train_ptr[:-1])).contiguous() if drop else plan.n_items
        at_k, scalar = ops.eval_rank_metrics(above, plan.test_ptr, plan.test_items, n_cand, Ks, n_items=plan.n_items)
    if return_per_user:
        out = {name: at_k[:, :, m] for m, name in enumerate(METRIC_NAMES)}
        out.update({name: scalar[:, m] for m, name in enumerate(RANK_SCALAR_NAMES)})
        return out
    mean = (at_k.sum(0) / plan.n_users).cpu().numpy()
    smean = (scalar.sum(0) / plan.n_users).cpu().numpy()
    out = {name: mean[:, m].copy() for m, name in enumerate(METRIC_NAMES)}
    out.update({name: float(smean[m]) for m, name in enumerate(RANK_SCALAR_NAMES)})
    return out


def recommend(embedding, user_ids, all_item_id_range, K, seen=None):
    """The K best items of every user of ``user_ids`` (node ids) that the user has not seen: ``(items, scores)`` -
    int64 item NODE ids ``(len(user_ids), K)`` in rank order (score descending, equal scores in the order of
    ``all_item_id_range``) and their float32 scores; a user with fewer than K unseen items gets ``-1`` / ``-inf`` at
    the end.  ``seen`` maps a user id to the items to leave out, as positions in ``all_item_id_range`` (a dict like
    ``train_user_dict``; None: nothing is left out).  1 <= K <= 128; HIP tensors only."""
    from . import ops
    emb = _device_rows(embedding, "recommend")
    users = [int(u) for u in np.asarray(user_ids).reshape(-1)]
    plan = EvalPlan(seen if seen is not None else {}, dict.fromkeys(users, _EMPTY), all_item_id_range, embedding.device)
    if len(plan.user_ids) != len(users):
        raise ValueError("recommend: a user is listed twice")
    if plan.n_users and plan.max_node_id >= embedding.shape[0]:
        raise IndexError("user / item node id %d outside the embedding's %d rows" % (plan.max_node_id,
                                                                                    embedding.shape[0]))
    with torch.no_grad():
        topk, scores = ops.eval_topk(emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, K,
                                     drop_train=True)
        pos = topk.long()
        items = torch.where(pos >= 0, plan.item_ids.long()[pos.clamp(min=0)], pos) if plan.n_items else pos
    return items, scores


def calc_recall_ndcg_sorted(embedding, train_user_dict, test_user_dict, all_item_id_range, K=20, batch_users=2048):
    """The same metric by one matmul + one stable descending sort per user batch (torch operators; rounds 1-4)."""
    dev = embedding.device
    items = torch.as_tensor(np.asarray(all_item_id_range), device=dev, dtype=torch.long)
    item_emb = embedding.index_select(0, items).t().contiguous()
    users = list(test_user_dict.keys())
    n_items = items.numel()
    disc = 1.0 / torch.log2(torch.arange(2, K + 2, device=dev, dtype=torch.float64))
    recall_sum = ndcg_sum = 0.0
    with torch.no_grad():
        for lo in range(0, len(users), batch_users):
            ub = users[lo:lo + batch_users]
            u_idx = torch.as_tensor(np.asarray(ub), device=dev, dtype=torch.long)
            score = embedding.index_select(0, u_idx) @ item_emb  # (B, n_items)
            rows, cols, prow, pcol = [], [], [], []
            for b, u in enumerate(ub):
                tr = np.asarray(train_user_dict.get(u, ()), dtype=np.int64)
                rows.append(np.full(len(tr), b)); cols.append(tr)
                ps = np.asarray(test_user_dict[u], dtype=np.int64)
                prow.append(np.full(len(ps), b)); pcol.append(ps)
            score[torch.as_tensor(np.concatenate(rows), device=dev), torch.as_tensor(np.concatenate(cols), device=dev)] = 0.0
            pos = torch.zeros((len(ub), n_items), dtype=torch.bool, device=dev)
            pos[torch.as_tensor(np.concatenate(prow), device=dev), torch.as_tensor(np.concatenate(pcol), device=dev)] = True
            top = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :K]
            hits = pos.gather(1, top).to(torch.float64)  # (B, K) binary_rank_K
            n_pos = torch.as_tensor([len(test_user_dict[u]) for u in ub], device=dev, dtype=torch.float64)
            recall_sum += float((hits.sum(1) / n_pos.clamp(min=1)).where(n_pos > 0, torch.zeros_like(n_pos)).sum())
            dcg = (hits * disc).sum(1)
            ideal = (torch.sort(hits, dim=1, descending=True).values * disc).sum(1)
            ndcg_sum += float(torch.where(ideal > 0, dcg / ideal.clamp(min=1e-300), torch.zeros_like(dcg)).sum())
    return recall_sum / len(users), ndcg_sum / len(users)
