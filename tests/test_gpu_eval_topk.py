"""Ranked lists for K up to 128 (kgat_eval_topk_f32) and the metrics at several cut-offs (kgat_eval_metrics_at_ks;
metrics.calc_metrics / metrics.recommend) against fp64 stable sorts of exact integer scores, the oracle's per-user
restatement of the reference's loop (oracle.recall_ndcg_per_user) and the K <= 32 entry."""
import functools

import numpy as np
import pytest
import torch

from oracle import kgat_oracle as orc

pytestmark = pytest.mark.gpu

PAPER_KS = (20, 40, 60, 80, 100)

# (n_u, n_i, F, K)
TIE_SHAPES = [(33, 33, 8, 33),          # first K beyond the old limit, n_items == K, LDS form
              (70, 100, 13, 100),       # n_items == K
              (5, 128, 7, 128),         # the maximum K
              (60, 700, 257, 65),       # first K of the 256-entry buffer, LDS form at a wide F
              (97, 2300, 96, 40),       # KG 6, several segments
              (129, 2100, 176, 100),    # KG 11
              (77, 2500, 256, 64),      # KG 16
              (70, 1800, 352, 128),     # KG 22, one tile in flight
              (260, 1500, 24, 100),
              (40, 300, 520, 40),       # F > 512: the LDS form with one wavefront per workgroup, 128-entry buffer
              (40, 300, 520, 100)]      # the same with the 156-entry buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _tie_case(n_u, n_i, F):
    """Small-integer embeddings (every fp32 score exact): zero rows, duplicate item rows, "negative" users, one user
    with every item masked and one with none, a shuffled dict order; train lists of up to min(n_i, 160) items.
    Returns (emb fp64, train, test, item_range, scores) - scores (users in dict order) x items in fp64, masked."""
    rng = np.random.default_rng(100 * n_u + n_i + F)
    emb = rng.integers(-2, 3, (n_u + n_i, F)).astype(np.float64)
    emb[rng.random(n_u + n_i) < 0.1] = 0.0
    dup = rng.integers(n_u, n_u + n_i, 10)
    emb[dup] = emb[rng.integers(n_u, n_u + n_i, 10)]
    neg = rng.random(n_u) < 0.3
    item_range = np.arange(n_u, n_u + n_i)
    train, test = {}, {}
    users = list(range(n_u))
    rng.shuffle(users)                                          # the dict order is the evaluation order
    for u in users:
        if neg[u]:
            emb[u] = -np.sign(emb[item_range].sum(0))
        train[u] = rng.choice(n_i, int(rng.integers(0, min(n_i, 160))), replace=False)
        test[u] = rng.choice(n_i, int(rng.integers(0, 9)), replace=False)
    if n_u > 3:
        train[users[0]] = np.arange(n_i)                        # every item masked: the K lowest positions rank
        train[users[1]] = np.zeros(0, np.int64)
    score = emb[list(test.keys())] @ emb[item_range].T
    for r, u in enumerate(test.keys()):
        score[r, np.asarray(train[u], dtype=np.int64)] = 0.0
    score.setflags(write=False)
    return emb, train, test, item_range, score


def _ranking(score, K):
    """fp64 stable descending argsort, the first K."""
    return np.argsort(-score, axis=1, kind="stable")[:, :K]


def _topk(emb, train, test, item_range, K, dev, **kw):
    from dgl_kgat_amd import metrics, ops
    plan = metrics.EvalPlan(train, test, item_range, dev)
    e = torch.as_tensor(np.asarray(emb, np.float32), device=dev)
    return ops.eval_topk(e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, K, **kw), plan


@pytest.mark.parametrize("n_u,n_i,F,K", TIE_SHAPES)
def test_topk_ties_and_masked_zeros_exact(dev, n_u, n_i, F, K):
    """Exact scores, so the rule alone decides: the ranked positions equal an fp64 stable descending argsort with the
    training scores set to 0.0 (users with more masked items than K included), the scores equal the fp64 scores, and
    a second call gives the same bits."""
    emb, train, test, item_range, score = _tie_case(n_u, n_i, F)
    (topk, scores), _ = _topk(emb, train, test, item_range, K, dev)
    exp = _ranking(score, K)
    got = topk.cpu().numpy().astype(np.int64)
    assert got.shape == (n_u, K) and np.array_equal(got, exp), np.argwhere(got != exp)[:5]
    assert np.array_equal(scores.cpu().numpy().astype(np.float64), np.take_along_axis(score, exp, 1))
    (topk2, scores2), _ = _topk(emb, train, test, item_range, K, dev)
    assert torch.equal(topk, topk2) and torch.equal(scores, scores2)


def _metrics_from_ranking(rank, test, Ks):
    """precision and hit ratio (means over the users) of a ranking, straight from their definitions."""
    prec, hr = np.zeros(len(Ks)), np.zeros(len(Ks))
    for r, pos in enumerate(test.values()):
        hit = np.isin(rank[r], np.asarray(pos, dtype=np.int64))
        for j, k in enumerate(Ks):
            prec[j] += hit[:k].sum() / k
            hr[j] += float(hit[:k].any())
    return prec / len(test), hr / len(test)


@pytest.mark.parametrize("n_u,n_i,F,K", TIE_SHAPES)
def test_metrics_at_paper_cutoffs(dev, n_u, n_i, F, K):
    from dgl_kgat_amd import metrics
    emb, train, test, item_range, score = _tie_case(n_u, n_i, F)
    Ks = tuple(k for k in PAPER_KS if k <= n_i)
    got = metrics.calc_metrics(torch.as_tensor(emb, device=dev), train, test, item_range, Ks=Ks)
    assert set(got) == {"recall", "ndcg", "precision", "hit_ratio"}
    assert all(v.dtype == np.float64 and v.shape == (len(Ks),) for v in got.values())
    prec, hr = _metrics_from_ranking(_ranking(score, Ks[-1]), test, Ks)
    for j, k in enumerate(Ks):
        ref = orc.recall_ndcg_per_user(emb, train, test, item_range, k)
        assert abs(got["recall"][j] - ref[0]) < 1e-12 and abs(got["ndcg"][j] - ref[1]) < 1e-12, (k, got, ref)
        assert abs(got["precision"][j] - prec[j]) < 1e-12 and abs(got["hit_ratio"][j] - hr[j]) < 1e-12, (k, got)
    per_user = metrics.calc_metrics(torch.as_tensor(emb, device=dev), train, test, item_range, Ks=Ks,
                                    return_per_user=True)
    for name, v in per_user.items():
        assert v.shape == (n_u, len(Ks)) and v.dtype == torch.float64
        assert np.allclose(v.mean(0).cpu().numpy(), got[name], rtol=0, atol=1e-12)


def test_metrics_vs_oracle_distinct_scores_and_empty_lists(dev):
    """300 users x 500 items, fp64 scores all distinct: the best raw scores are training items (masked to 0.0), some
    users have no test item (recall 0), hits that are not a prefix of the ranking (own-hit-list ideal DCG)."""
    from dgl_kgat_amd import metrics
    rng = np.random.default_rng(11)
    n_u, n_i = 300, 500
    e = rng.standard_normal((n_u + n_i, 12))
    item_range = np.arange(n_u, n_u + n_i)
    train, test = {}, {}
    score = e[:n_u] @ e[item_range].T
    for u in range(n_u):
        top = np.argsort(-score[u])
        train[u] = top[:rng.integers(0, 8)]
        n_pos = 0 if u % 37 == 0 else int(rng.integers(1, 12))
        cand = np.concatenate([top[8:140], rng.integers(0, n_i, 20)])
        test[u] = np.unique(rng.choice(cand, n_pos, replace=False)) if n_pos else np.zeros(0, np.int64)
        score[u, train[u]] = 0.0
    got = metrics.calc_metrics(torch.as_tensor(e, device=dev), train, test, item_range, Ks=PAPER_KS)
    prec, hr = _metrics_from_ranking(_ranking(score, 100), test, PAPER_KS)
    for j, k in enumerate(PAPER_KS):
        ref = orc.recall_ndcg_per_user(e, train, test, item_range, k)
        assert 0.05 < ref[0] < 0.95 and abs(got["recall"][j] - ref[0]) < 1e-12 and abs(got["ndcg"][j] - ref[1]) < 1e-12
        assert abs(got["precision"][j] - prec[j]) < 1e-12 and abs(got["hit_ratio"][j] - hr[j]) < 1e-12


@pytest.mark.parametrize("n_u,n_i,F", [(129, 2100, 176), (70, 45, 13), (64, 40, 200)])
def test_old_and_new_entries_agree(dev, n_u, n_i, F):
    """The list at K = 20, and the first 20 ranks of the list at K = 100, are the K <= 32 entry's list; recall of the
    first 20 ranks is its recall, ndcg within 1e-15."""
    from dgl_kgat_amd import metrics, ops
    emb, train, test, item_range, _ = _tie_case(n_u, n_i, F)
    plan = metrics.EvalPlan(train, test, item_range, dev)
    e = torch.as_tensor(emb.astype(np.float32), device=dev)
    rec, ndcg, old = ops.eval_recall_ndcg(e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items,
                                          plan.test_ptr, plan.test_items, 20, want_topk=True)
    rec, ndcg, old = rec.cpu().numpy(), ndcg.cpu().numpy(), old.cpu().numpy()
    for K in (20, 100):
        if n_i < K:
            continue
        new = ops.eval_topk(e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, K, want_scores=False)
        assert np.array_equal(new.cpu().numpy()[:, :20], old)
        m = ops.eval_metrics_at_ks(new, plan.test_ptr, plan.test_items, [20]).cpu().numpy()
        assert np.array_equal(m[:, 0, 0], rec)
        assert np.all(np.abs(m[:, 0, 1] - ndcg) <= 1e-15)


@pytest.mark.parametrize("n_u,n_i,F,K", [(300, 5000, 176, 100), (200, 3000, 64, 64), (150, 4000, 352, 128),
                                         (260, 2100, 96, 40)])
def test_topk_real_valued_scores_and_racing_thresholds(dev, n_u, n_i, F, K):
    """Real-valued embeddings at sizes with several item segments per user block: the same bits from four calls (the
    segments race through the shared K-th best, which may change the work, never the result), and against an fp64
    ranking of the same fp32 inputs every user rank-for-rank equal or different only within the fp32 rounding of the
    dot product - at least 0.99 of the users equal (a numpy fp32 matmul gives 1.0, 1.0, 1.0 and 0.996 on these seeds:
    one user of 260, off by 4.4e-6; the kernel's fmaf order is not numpy's, hence the margin)."""
    from dgl_kgat_amd import metrics, ops
    rng = np.random.default_rng(7 * n_u + n_i)
    emb = rng.standard_normal((n_u + n_i, F)).astype(np.float32)
    item_range = np.arange(n_u, n_u + n_i)
    train = {u: np.unique(rng.integers(0, n_i, int(rng.integers(0, 60)))) for u in range(n_u)}
    test = {u: np.unique(rng.integers(0, n_i, 1 + u % 7)) for u in range(n_u)}
    e64 = emb.astype(np.float64)
    score = e64[:n_u] @ e64[item_range].T
    for u in range(0, n_u, 97):   # users whose best 45 + K items are all training items
        train[u] = np.unique(np.argsort(-score[u])[:45 + K])
    for u in range(n_u):
        score[u, train[u]] = 0.0
    plan = metrics.EvalPlan(train, test, item_range, dev)
    e = torch.as_tensor(emb, device=dev)
    runs = [ops.eval_topk(e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, K) for _ in range(4)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1])
    topk = runs[0][0].cpu().numpy()
    order = _ranking(score, K)
    tol = 2e-4
    n_exact = 0
    for u in range(n_u):
        if np.array_equal(topk[u], order[u]):
            n_exact += 1
            continue
        got = score[u, topk[u]]
        assert np.all(got >= score[u, order[u, K - 1]] - tol), (u, got, score[u, order[u]])
        assert np.all(np.diff(got) <= tol), (u, got)
        assert len(set(topk[u].tolist())) == K
    print("[eval_topk] %d x %d x %d, K = %d: %d of %d users rank-for-rank equal" % (n_u, n_i, F, K, n_exact, n_u))
    assert n_exact >= 0.99 * n_u, (n_exact, n_u)


@pytest.mark.parametrize("n_u,n_i,F,K", [(40, 300, 24, 50), (20, 60, 8, 50)])
def test_drop_mode_and_recommend(dev, n_u, n_i, F, K):
    """`drop`: no seen item is listed, the order is a stable argsort over the unseen items, a short list ends in
    -1 / -inf; recommend returns node ids."""
    from dgl_kgat_amd import metrics
    rng = np.random.default_rng(31 * n_u + n_i)
    emb = rng.integers(-2, 3, (n_u + n_i, F)).astype(np.float64)
    item_range = np.arange(n_u, n_u + n_i)
    users = list(range(n_u))
    rng.shuffle(users)
    seen = {u: rng.choice(n_i, int(rng.integers(0, 56)), replace=False) for u in users if u % 5}   # (some users: no entry)
    seen[users[0]] = rng.choice(n_i, 55, replace=False)
    (topk, scores), _ = _topk(emb, seen, dict.fromkeys(users, np.zeros(0, np.int64)), item_range, K, dev, drop_train=True)
    topk, scores = topk.cpu().numpy(), scores.cpu().numpy()
    items, rscores = metrics.recommend(torch.as_tensor(emb, device=dev), users, item_range, K, seen=seen)
    assert items.dtype == torch.int64 and rscores.dtype == torch.float32 and items.shape == rscores.shape == (n_u, K)
    items, rscores = items.cpu().numpy(), rscores.cpu().numpy()
    short = 0
    for r, u in enumerate(users):
        s = emb[item_range] @ emb[u]
        unseen = np.setdiff1d(np.arange(n_i), seen.get(u, ()))
        exp = unseen[np.argsort(-s[unseen], kind="stable")][:K]
        n = len(exp)
        short += n < K
        assert np.array_equal(topk[r, :n], exp) and np.array_equal(scores[r, :n].astype(np.float64), s[exp])
        assert not np.isin(topk[r, :n], seen.get(u, ())).any()
        assert np.all(topk[r, n:] == -1) and np.all(np.isneginf(scores[r, n:]))
        assert np.array_equal(items[r, :n], item_range[exp]) and np.all(items[r, n:] == -1)
        assert np.array_equal(rscores[r], scores[r])
    assert (short > 0) == (n_i - 55 < K)
    # nothing seen: the plain ranking
    plain, _ = metrics.recommend(torch.as_tensor(emb, device=dev), users[:3], item_range, min(K, n_i))
    for r, u in enumerate(users[:3]):
        assert np.array_equal(plain[r].cpu().numpy(), item_range[np.argsort(-(emb[item_range] @ emb[u]), kind="stable")[:min(K, n_i)]])


def test_topk_rejections(dev):
    from dgl_kgat_amd import metrics, ops
    from dgl_kgat_amd.ops import KGATLibraryError
    emb = torch.zeros((80, 8), device=dev)
    train, test = {0: np.array([1])}, {0: np.array([2])}
    plan = metrics.EvalPlan(train, test, np.arange(4, 64), dev)   # 60 items
    args = (emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items)
    for K in (129, 0):
        with pytest.raises(KGATLibraryError):
            ops.eval_topk(*args, K)
    with pytest.raises(KGATLibraryError):     # mask mode: fewer items than K (the reference reads rank K - 1)
        ops.eval_topk(*args, 61)
    with pytest.raises(KGATLibraryError):
        metrics.calc_metrics(emb, train, test, np.arange(4, 64), Ks=(20, 61))
    topk, scores = ops.eval_topk(*args, 61, drop_train=True)   # drop mode pads
    assert topk.shape == (1, 61) and (topk[0, :59] >= 0).all() and (topk[0, 59:] == -1).all()
    assert not (topk[0] == 1).any() and torch.isneginf(scores[0, 59:]).all()
    with pytest.raises(KGATLibraryError):     # CPU tensors: no CPU implementation
        ops.eval_topk(emb.cpu(), *args[1:], 20)
    with pytest.raises(KGATLibraryError):
        metrics.calc_metrics(emb.cpu(), train, test, np.arange(4, 64), Ks=(20,))
    with pytest.raises(KGATLibraryError):
        metrics.recommend(emb.cpu(), [0], np.arange(4, 64), 20)
    with pytest.raises(IndexError):           # an item id outside the item range, as calc_recall_ndcg
        metrics.calc_metrics(emb, {0: np.array([99])}, test, np.arange(4, 64), Ks=(20,))


@pytest.mark.parametrize("Ks,exc", [((40, 20), ValueError), ((20, 20), ValueError), (tuple(range(1, 10)), ValueError),
                                    ((20, 129), None)])
def test_bad_cutoffs_raise(dev, Ks, exc):
    from dgl_kgat_amd import metrics, ops
    emb = torch.zeros((200, 8), device=dev)
    train, test = {0: np.array([1])}, {0: np.array([2])}
    with pytest.raises(exc or ops.KGATLibraryError):
        metrics.calc_metrics(emb, train, test, np.arange(4, 200), Ks=Ks)
    if exc is ValueError:
        with pytest.raises(ValueError):
            ops.eval_metrics_at_ks(torch.zeros((1, 128), dtype=torch.int32, device=dev),
                                   torch.zeros(2, dtype=torch.int32, device=dev),
                                   torch.zeros(0, dtype=torch.int32, device=dev), Ks)
