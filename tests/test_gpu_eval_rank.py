"""Exact ranks of the held-out items (kgat_eval_rank_f32, kgat_eval_rank_metrics; metrics.rank_items /
calc_rank_metrics) against the numpy restatement on exact integer scores, against the top-K sweep's lists on
real-valued scores (the arithmetic's oracle: the same total order, bit for bit), inside the fp64 band of the dot
product's rounding, and end to end through the training example."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _rank_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("mask", "drop")

# (n_u, n_i, F)
EXACT_SHAPES = [(33, 33, 8),            # a user block of 32 plus 1, items 32 plus 1, LDS form
                (5, 20, 7),             # fewer items than a tile
                (60, 700, 257),         # LDS form at a wide F
                (97, 2300, 96),         # KG 6, several item segments where the plan makes them
                (129, 2100, 176),       # KG 11
                (77, 2500, 256),        # KG 16
                (70, 1800, 352),        # KG 22, one tile in flight
                (260, 1500, 24),
                (40, 300, 520)]         # F > 512: the LDS form with one wavefront per workgroup
REAL_SHAPES = [(300, 5000, 176), (150, 4000, 352), (200, 3000, 64), (260, 2100, 96), (100, 1000, 24)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _tie_case(n_u, n_i, F):
    """The recipe of test_gpu_eval_topk.py - small-integer embeddings (every fp32 score exact): zero rows, duplicate item
    rows, "negative" users, one user with every item in train and one with none (and no test item), a shuffled dict
    order - plus one user with 300 test entries (the threshold groups wrap; repeats where there are fewer items), one
    with a duplicated entry and one whose test items are training items.  Returns (emb fp64, train, test, item_range,
    raw scores) - scores of the users in dict order x items, fp64, NOT masked."""
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
    train[users[0]] = np.arange(n_i)                            # every item a training item
    train[users[1]] = np.zeros(0, np.int64)
    test[users[1]] = np.zeros(0, np.int64)                      # (and nothing held out)
    test[users[2]] = rng.choice(n_i, 300, replace=False) if n_i >= 300 else rng.integers(0, n_i, 300)
    test[users[3]] = np.array([n_i - 1, 0, n_i - 1, n_i // 2])   # a duplicated entry
    train[users[4]] = rng.choice(n_i, min(n_i, 12), replace=False)
    test[users[4]] = np.concatenate([train[users[4]][:2], rng.integers(0, n_i, 2)])   # test items that are training items
    score = emb[list(test.keys())] @ emb[item_range].T
    score.setflags(write=False)
    return emb, train, test, item_range, score


@functools.lru_cache(maxsize=None)
def _exact_ref(n_u, n_i, F, mode):
    _, train, test, _, score = _tie_case(n_u, n_i, F)
    users = list(test.keys())
    return R.rank_items(score, [train[u] for u in users], [test[u] for u in users], mode)


def _n_candidates(train, test, n_i, mode):
    return [n_i - (len(np.unique(train[u])) if mode == "drop" else 0) for u in test]


def _rank(emb, train, test, item_range, dev, mode, **kw):
    from dgl_kgat_amd import metrics, ops
    plan = metrics.EvalPlan(train, test, item_range, dev)
    e = torch.as_tensor(np.asarray(emb, np.float32), device=dev)
    return ops.eval_rank(e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, plan.test_ptr,
                         plan.test_items, drop_train=mode == "drop", **kw), plan


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_u,n_i,F", EXACT_SHAPES)
def test_rank_exact_cases(dev, n_u, n_i, F, mode):
    """Exact scores, so the rule alone decides: every count equals the restatement's, the target scores are s'(u, t),
    and a second call gives the same bits."""
    emb, train, test, item_range, score = _tie_case(n_u, n_i, F)
    ref = _exact_ref(n_u, n_i, F, mode)
    (above, scores), plan = _rank(emb, train, test, item_range, dev, mode, want_scores=True)
    exp = np.concatenate(ref)
    got = above.cpu().numpy().astype(np.int64)
    assert got.shape == exp.shape and np.array_equal(got, exp), (np.argwhere(got != exp)[:5], got[got != exp][:5],
                                                                 exp[got != exp][:5])
    users = list(test.keys())
    s_exp = R.masked_scores(score, [train[u] for u in users], mode)
    s_exp = np.concatenate([s_exp[r, np.sort(np.asarray(test[u], dtype=np.int64))] for r, u in enumerate(users)])
    assert np.array_equal(scores.cpu().numpy().astype(np.float64), s_exp)
    if mode == "drop":
        assert (got == -1).sum() >= 2 and (ref[0] == -1).all()      # the user with every item in train
    (above2, scores2), _ = _rank(emb, train, test, item_range, dev, mode, want_scores=True)
    assert torch.equal(above, above2) and torch.equal(scores, scores2)
    above3, _ = _rank(emb, train, test, item_range, dev, mode)           # (the scores in the workspace: the same counts)
    assert torch.equal(above, above3)


@functools.lru_cache(maxsize=None)
def _real_case(n_u, n_i, F):
    """Real-valued embeddings; users whose best 45 + K items are all training items (masked zeros near the cut), some
    of them held out too."""
    K = min(128, n_i)
    rng = np.random.default_rng(7 * n_u + n_i)
    emb = rng.standard_normal((n_u + n_i, F)).astype(np.float32)
    item_range = np.arange(n_u, n_u + n_i)
    train = {u: np.unique(rng.integers(0, n_i, int(rng.integers(0, 60)))) for u in range(n_u)}
    test = {u: np.unique(rng.integers(0, n_i, 1 + u % 7)) for u in range(n_u)}
    e64 = emb.astype(np.float64)
    score = e64[:n_u] @ e64[item_range].T
    for u in range(0, n_u, 97):
        best = np.argsort(-score[u])
        train[u] = np.unique(best[:45 + K])
        test[u] = np.unique(np.concatenate([test[u], best[40:44], best[45 + K:48 + K]]))
    test[1] = np.unique(rng.integers(0, n_i, 300))               # several threshold groups
    score.setflags(write=False)
    return emb, train, test, item_range, score, K


@functools.lru_cache(maxsize=None)
def _real_run(n_u, n_i, F, mode):
    """(above, topk at K, plan arrays on the host): one device run per (shape, mode), shared by the tests below."""
    from dgl_kgat_amd import ops
    emb, train, test, item_range, _, K = _real_case(n_u, n_i, F)
    dev = torch.device("cuda:0")
    above, plan = _rank(emb, train, test, item_range, dev, mode)
    e = torch.as_tensor(emb, device=dev)
    topk = ops.eval_topk(e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, K,
                         drop_train=mode == "drop", want_scores=False)
    return (above.cpu().numpy().astype(np.int64), topk.cpu().numpy().astype(np.int64),
            plan.test_ptr.cpu().numpy().astype(np.int64), plan.test_items.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_u,n_i,F", REAL_SHAPES)
def test_rank_consistent_with_the_topk_sweep(dev, n_u, n_i, F, mode):
    """The counts describe the order of kgat_eval_topk_f32: for EVERY test entry, above < K puts the item at place
    `above` of the user's list, above >= K (or -1: never ranked) keeps it off the list."""
    K = min(128, n_i)
    above, topk, ptr, items = _real_run(n_u, n_i, F, mode)
    owner = np.repeat(np.arange(n_u), np.diff(ptr))
    assert above.shape == items.shape and len(above) == ptr[-1] > n_u
    inside = (above >= 0) & (above < K)
    assert inside.sum() > 10 and (~inside).sum() > 10
    at = topk[owner[inside], above[inside]]
    assert np.array_equal(at, items[inside]), np.argwhere(at != items[inside])[:5]
    listed = (topk[owner[~inside]] == items[~inside][:, None]).any(1)
    assert not listed.any(), np.argwhere(listed)[:5]
    assert (above >= -1).all() and ((above == -1).sum() > 0) == (mode == "drop")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_u,n_i,F", REAL_SHAPES)
def test_rank_inside_the_fp64_band(dev, n_u, n_i, F, mode):
    """Against fp64 scores of the same fp32 inputs: with delta(u,i) = gamma_F sum_k |e_u[k] e_i[k]|, gamma_F =
    F 2^-24 / (1 - F 2^-24) - the bound of an F-term fused-multiply-add chain in any order - every count lies between
    the candidates that beat the target beyond both roundings and those that may.  Masked entries are exactly 0."""
    emb, train, test, item_range, score, _ = _real_case(n_u, n_i, F)
    above, _, ptr, items = _real_run(n_u, n_i, F, mode)
    gamma = F * 2.0 ** -24 / (1.0 - F * 2.0 ** -24)
    a = np.abs(emb.astype(np.float64))
    delta_all = gamma * (a[:n_u] @ a[item_range].T)
    for r, u in enumerate(test.keys()):
        s, d = score[r].copy(), delta_all[r].copy()
        cand = np.ones(n_i, dtype=bool)
        if mode == "mask":
            s[train[u]] = 0.0
            d[train[u]] = 0.0
        else:
            cand[train[u]] = False
        t = items[ptr[r]:ptr[r + 1]]
        got = above[ptr[r]:ptr[r + 1]]
        ranked = cand[t]
        assert np.array_equal(got[~ranked], np.full((~ranked).sum(), -1))
        t, got = t[ranked], got[ranked]
        diff = s[None, :] - s[t][:, None]
        tol = d[None, :] + d[t][:, None]
        m = np.broadcast_to(cand, diff.shape).copy()
        m[np.arange(len(t)), t] = False                              # the target itself
        lo, hi = ((diff > tol) & m).sum(1), ((diff >= -tol) & m).sum(1)
        assert np.all(lo <= got) and np.all(got <= hi), (u, t, lo, got, hi)


def _cutoffs(n_i):
    return sorted({min(k, n_i) for k in (1, 20, 128, 129, 500, n_i)})


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_u,n_i,F", EXACT_SHAPES)
def test_rank_metrics_exact_cases(dev, n_u, n_i, F, mode):
    from dgl_kgat_amd import ops
    emb, train, test, item_range, _ = _tie_case(n_u, n_i, F)
    ks = _cutoffs(n_i)
    above, plan = _rank(emb, train, test, item_range, dev, mode)
    n_cand = _n_candidates(train, test, n_i, mode)
    at_k, scalar = ops.eval_rank_metrics(above, plan.test_ptr, plan.test_items,
                                         torch.as_tensor(n_cand, dtype=torch.int32, device=dev), ks, n_items=n_i)
    ref_at_k, ref_scalar = R.rank_metrics(_exact_ref(n_u, n_i, F, mode), list(test.values()), n_cand, ks)
    assert at_k.shape == (n_u, len(ks), 4) and scalar.shape == (n_u, 4) and at_k.dtype == scalar.dtype == torch.float64
    e_at_k = np.abs(at_k.cpu().numpy() - ref_at_k).max((0, 1))
    e_scalar = np.abs(scalar.cpu().numpy() - ref_scalar).max(0)
    print("[eval_rank_metrics] %s %s: max |error| recall %.1e ndcg %.1e precision %.1e hit %.1e | mrr %.1e ap %.1e auc "
          "%.1e mean_rank %.1e" % ((n_u, n_i, F), mode, *e_at_k, *e_scalar))
    assert np.all(e_at_k <= 1e-12) and np.all(e_scalar <= 1e-12)
    assert ref_scalar[:, 2].max() > 0.5 and ref_at_k[:, -1, 0].max() > 0.0   # (the cases are not degenerate)
    at_k2, scalar2 = ops.eval_rank_metrics(above, plan.test_ptr, plan.test_items,
                                           torch.as_tensor(n_cand, dtype=torch.int32, device=dev), ks, n_items=n_i)
    assert torch.equal(at_k, at_k2) and torch.equal(scalar, scalar2)


@pytest.mark.parametrize("n_u,n_i,F", EXACT_SHAPES)
def test_calc_rank_metrics_agrees_with_calc_metrics(dev, n_u, n_i, F):
    """At the cut-offs within 128, per user: recall, precision and hit ratio bit for bit those of the list-based
    calc_metrics, ndcg within 1e-12 - the users with duplicated and empty test lists included; the means are the
    per-user values' means; rank_items is above + 1."""
    from dgl_kgat_amd import metrics
    emb, train, test, item_range, _ = _tie_case(n_u, n_i, F)
    e = torch.as_tensor(emb, device=dev)
    ks = [k for k in _cutoffs(n_i) if k <= 128]
    plan = metrics.EvalPlan(train, test, item_range, dev)
    new = metrics.calc_rank_metrics(e, train, test, item_range, Ks=ks, plan=plan, return_per_user=True)
    old = metrics.calc_metrics(e, train, test, item_range, Ks=ks, plan=plan, return_per_user=True)
    assert set(new) == {"recall", "ndcg", "precision", "hit_ratio", "mrr", "map", "auc", "mean_rank"}
    for name in ("recall", "precision", "hit_ratio"):
        assert new[name].shape == (n_u, len(ks)) and torch.equal(new[name], old[name]), name
    assert float((new["ndcg"] - old["ndcg"]).abs().max()) <= 1e-12
    lens = np.diff(plan.test_ptr.cpu().numpy())
    assert (lens == 0).any() and (lens >= 300).any()
    mean = metrics.calc_rank_metrics(e, train, test, item_range, Ks=ks, plan=plan)
    for name in ("recall", "ndcg", "precision", "hit_ratio"):
        assert mean[name].dtype == np.float64 and mean[name].shape == (len(ks),)
        assert np.allclose(new[name].mean(0).cpu().numpy(), mean[name], rtol=0, atol=1e-12)
    for name in ("mrr", "map", "auc", "mean_rank"):
        assert isinstance(mean[name], float) and abs(float(new[name].mean()) - mean[name]) <= 1e-9 * max(1.0, mean[name])
    for mode in MODES:
        ranks, ptr = metrics.rank_items(e, train, test, item_range, plan=plan, mode=mode)
        assert ranks.dtype == torch.int64 and ptr is plan.test_ptr
        assert np.array_equal(ranks.cpu().numpy(), np.concatenate(_exact_ref(n_u, n_i, F, mode)) + 1)


def test_rank_refusals(dev):
    """ops.eval_rank refuses what ops.eval_topk refuses, with the same exceptions; the raw entry refuses a short
    workspace before any device work."""
    from dgl_kgat_amd import _lib, metrics, ops
    from dgl_kgat_amd.ops import KGATLibraryError
    train, test, items = {0: np.array([1])}, {0: np.array([2, 5])}, np.arange(4, 64)
    plan = metrics.EvalPlan(train, test, items, dev)

    def both(emb, **over):
        a = dict(user_ids=plan.user_ids, item_ids=plan.item_ids, train_ptr=plan.train_ptr, train_items=plan.train_items)
        a.update(over)
        excs = []
        for call in (lambda: ops.eval_topk(emb, a["user_ids"], a["item_ids"], a["train_ptr"], a["train_items"], 20),
                     lambda: ops.eval_rank(emb, a["user_ids"], a["item_ids"], a["train_ptr"], a["train_items"],
                                           plan.test_ptr, plan.test_items)):
            with pytest.raises((KGATLibraryError, TypeError, ValueError)) as ei:
                call()
            excs.append(ei.type)
        assert excs[0] is excs[1], excs
        return excs[0]

    emb = torch.zeros((80, 8), device=dev)
    assert both(torch.zeros((80, 5000), device=dev)) is KGATLibraryError            # unsupported F
    assert both(emb.double()) is KGATLibraryError
    assert both(emb.cpu()) is KGATLibraryError
    assert both(torch.zeros((8, 80), device=dev).t()) is KGATLibraryError           # non-contiguous columns
    assert both(emb, user_ids=plan.user_ids.long()) is TypeError
    assert both(emb, train_items=plan.train_items.long()) is TypeError
    assert both(emb, train_ptr=plan.train_ptr[:1].contiguous()) is ValueError
    with pytest.raises(TypeError):
        ops.eval_rank(emb, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items, plan.test_ptr,
                      plan.test_items.long())
    with pytest.raises(IndexError):                                                # ids outside the embedding, as calc_metrics
        metrics.calc_rank_metrics(torch.zeros((10, 8), device=dev), train, test, items, Ks=(20,))
    with pytest.raises(ZeroDivisionError):
        metrics.calc_rank_metrics(emb, train, {}, items, Ks=(20,))
    with pytest.raises(ValueError):
        metrics.calc_rank_metrics(emb, train, test, items, Ks=(20, 61))
    # the raw entry: a workspace one byte short
    lib = _lib.load()
    need = lib.kgat_eval_rank_workspace_bytes(1, 60, 8, 1, 2)
    assert need > 256
    itemT = torch.zeros(int(lib.kgat_eval_items_elems(60, 8)), device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    above = torch.full((2,), 7, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                    # noqa: E731

    def raw(ws_bytes, F=8, stride=8, user_ids=p(plan.user_ids)):
        rc = lib.kgat_eval_rank_f32(1, user_ids, 60, F, p(emb), stride, p(itemT), p(plan.train_ptr), p(plan.train_items),
                                    1, p(plan.test_ptr), p(plan.test_items), 2, 0, p(ws), ws_bytes, p(above), None, None)
        torch.cuda.synchronize()
        return rc

    assert raw(need - 1) == -3 and b"workspace" in lib.kgat_last_error()           # KGAT_E_WORKSPACE
    assert raw(need, F=5000, stride=5000) == -2                                     # KGAT_E_UNSUPPORTED
    assert raw(need, user_ids=None) == -1 and raw(need, stride=4) == -1             # KGAT_E_BADARG
    assert (above == 7).all()                                                       # nothing was written
    assert raw(need) == 0 and (above >= 0).all() and (above < 60).all()


def test_planted_structure_auc_and_mrr_rise(dev, tmp_path, capsys):
    """End to end in a child process (the example's global switches stay there), the settings of
    test_planted_structure_recall_rises with --rank_metrics 1: one rank_metrics line per split and evaluation, and
    the test AUC and MRR after three short epochs above the untrained model's (no magnitude is asked; measured: AUC
    0.4904 -> 0.5794, 0.6749, 0.7501 and MRR 0.0185 -> 0.0285, 0.0590, 0.0883 by epoch)."""
    import json
    log = tmp_path / "train_rank.json"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_kgat.py"), "--planted", "--epochs", "3", "--lr", "0.03",
           "--batch_size", "512", "--batch_size_kg", "512", "--eval_before", "--seed", "1234", "--rank_metrics", "1",
           "--log_json", str(log)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert len(re.findall(r"rank_metrics test auc", r.stdout)) == 4 == len(re.findall(r"rank_metrics valid auc", r.stdout))
    with open(log) as f:
        hist = json.load(f)["epochs"]
    auc, mrr = [h["test_auc"] for h in hist], [h["test_mrr"] for h in hist]
    with capsys.disabled():
        print("\nplanted-structure run: test AUC by epoch %s, MRR %s, MAP %s, mean rank %s, recall@200 %s" % (
            ["%.4f" % x for x in auc], ["%.4f" % x for x in mrr], ["%.4f" % h["test_map"] for h in hist],
            ["%.1f" % h["test_mean_rank"] for h in hist], ["%.4f" % h["test_rank_recall@200"] for h in hist]))
    assert auc[3] > auc[0] and mrr[3] > mrr[0]
    assert all("test_rank_recall@20" in h and "valid_auc" in h for h in hist)
    assert abs(hist[3]["test_rank_recall@20"] - hist[3]["test_recall"]) <= 1e-12      # the K = 20 sweep's recall
