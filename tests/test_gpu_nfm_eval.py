"""The fused NFM evaluation sweep (csrc/kgat_nfm_eval.hip) on the device, through the C entry (ops.nfm_eval_topk is its
argument marshalling) and through fm_models.NFM: bit for bit against the numpy restatement on exact inputs, degenerate
users, real-valued inputs against float64 within the bound derived from the stated arithmetic, invariances, the memory
contract and the model-level routes."""
import os
import sys

import numpy as np
import pytest
import torch

import _arena
import _nfm_eval_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POISON = 0x7FC0DEAD        # a NaN word


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def run(inp, rows, train_lists, K, with_const=True, want_scores=True):
    """kgat_nfm_eval_topk_f32 for the rows `rows` of V: (items, scores) as numpy."""
    from dgl_kgat_amd import ops
    ptr, flat = R.csr(train_lists)
    rows = np.asarray(rows, dtype=np.int32)
    items, scores = ops.nfm_eval_topk(dev(inp["V"]), dev(rows), dev(inp["W1"]), dev(inp["P"]), dev(inp["C"]), dev(inp["h"]),
                                      dev(inp["lin"]), dev(inp["const"][rows]) if with_const else None, dev(ptr), dev(flat), K,
                                      want_scores=want_scores)
    torch.cuda.synchronize()
    return items.cpu().numpy(), None if scores is None else scores.cpu().numpy()


def want(inp, rows, train_lists, K, with_const=True):
    key, score, _, _ = R.keys_and_bounds(inp, np.asarray(rows), with_const)
    return R.ranked(key, score, train_lists, K)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_exact(inp, rows, train_lists, K, with_const=True):
    gi, gs = run(inp, rows, train_lists, K, with_const)
    wi, ws = want(inp, rows, train_lists, K, with_const)
    assert np.array_equal(gi, wi), (gi[:, :8], wi[:, :8])
    assert np.array_equal(gs, ws)            # (exact values: -0 and +0 compare equal, as the order treats them)
    return gi, gs


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("hidden", [16, 32, 64])
@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_exact_every_width(d, hidden):
    """Every d x hidden of the envelope (16 hidden units through the op layer's zero padding), 3 users x 95 items: lists
    and scores equal the restatement exactly - a stable descending sort, ties (frequent: small integers) by position."""
    inp = R.exact_inputs(100 * d + hidden, 9, 95, d, hidden)
    gi, _ = check_exact(inp, [4, 0, 7], R.random_train_lists(d + hidden, 3, 95), 20)
    key = R.keys_and_bounds(inp, np.array([4, 0, 7]))[0]
    assert any(len(np.unique(k)) < len(k) for k in key)          # ties exist


@pytest.mark.parametrize("n_items", [1, 31, 32, 33, 1500])
def test_exact_item_counts(n_items):
    """One item, a tile less one, a whole tile, a tile and one, many tiles (several segments): the padded end of the
    last tile never produces a candidate - every listed position is below n_items or -1."""
    inp = R.exact_inputs(n_items, 6, n_items, 64, 64)
    gi, _ = check_exact(inp, [1, 2, 5], R.random_train_lists(n_items, 3, n_items, most=min(n_items, 9) - 1), 20)
    assert gi.max() < n_items and (gi[:, min(n_items, 20):] == -1).all()


@pytest.mark.parametrize("K", [1, 20, 33, 64, 128])
def test_exact_every_depth(K):
    inp = R.exact_inputs(7, 6, 1500, 64, 64)
    check_exact(inp, [0, 3, 5], R.random_train_lists(K, 3, 1500), K)
    check_exact(inp, [0, 3, 5], R.random_train_lists(K, 3, 1500), K, with_const=False)


@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
@pytest.mark.parametrize("K", [20, 128])
def test_exact_score_orders_fill_and_prune_the_buffer(order, K):
    """1,500 items for 3 users.  The scratch size shows that the entry cuts them into at least two segments (it holds one
    list of K entries per user and segment behind C's layout).  With keys ascending in the item position every key of a
    tile reaches the user's K-th best so far, so every tile of 32 is appended whole and a segment of more than 256 items
    (here about 300) overflows the 256-entry buffer: at least one prune of a full buffer per segment.  Descending keys
    pass the threshold only until K are held; equal keys tie everywhere and are decided by position alone."""
    from dgl_kgat_amd import ops
    lib = ops._lib.load()
    n_items, d, hidden = 1500, 64, 64
    need = lib.kgat_nfm_eval_scratch_bytes(3, n_items, d, hidden, 128)
    clay = ((n_items + 31) // 32) * hidden * 32 * 4
    n_seg = (need - clay) // 2 // (3 * 128 * 4)
    assert n_seg >= 2 and n_items / n_seg > 256 + 32
    inp = R.exact_inputs(11, 5, n_items, d, hidden, order)
    key = R.keys_and_bounds(inp, np.array([0, 1, 2]))[0]
    if order == "ascending":
        assert (np.diff(key, axis=1) > 0).all()
    elif order == "descending":
        assert (np.diff(key, axis=1) < 0).all()
    else:
        assert (key == key[:, :1]).all()
    gi, _ = check_exact(inp, [0, 1, 2], R.random_train_lists(3, 3, n_items), K)
    if order == "equal":
        assert (np.diff(gi, axis=1) > 0).all()


# ------------------------------------------------------------------------------------------------ 2. degenerate users
@pytest.mark.parametrize("n_users", [1, 70])
def test_degenerate_users(n_users):
    """An empty train list, a list that leaves fewer than K unseen items (padding at the end, nothing listed twice),
    every item a training item, a user id repeated, and user counts that are no multiple of the four per workgroup."""
    n_items, K = 95, 20
    inp = R.exact_inputs(21, 40, n_items, 32, 64)
    rows = (np.arange(n_users) * 7) % 40                      # ids repeat beyond 40 users; 70 = 17 workgroups and a half
    lists = R.random_train_lists(5, n_users, n_items)
    lists[0] = np.zeros(0, dtype=np.int64)
    if n_users > 3:
        lists[1] = np.setdiff1d(np.arange(n_items), [3, 50, 94])          # three unseen items
        lists[2] = np.arange(n_items)                                      # none
        rows[5] = rows[0]                                                  # the same user twice, other lists
    else:
        lists[0] = np.setdiff1d(np.arange(n_items), [3, 50, 94])
    gi, gs = check_exact(inp, rows, lists, K)
    for r in range(n_users):
        listed = gi[r][gi[r] >= 0]
        assert len(set(listed)) == len(listed) == min(K, n_items - len(lists[r])) and not np.isin(listed, lists[r]).any()
        assert (gi[r, len(listed):] == -1).all() and np.isneginf(gs[r, len(listed):]).all()
    if n_users > 3:
        assert len(gi[2][gi[2] >= 0]) == 0 and sorted(gi[1][:3]) == [3, 50, 94]


# ------------------------------------------------------------------------------------------------ 3. real values
_real = {}


def real_case(d=64, hidden=64):
    """70 users x 1,500 items, Xavier-scale V, random W1 / b1 / h: inputs, train lists, the float64 keys, scores and
    bounds - computed once."""
    if (d, hidden) not in _real:
        rng = np.random.default_rng(1000 + d + hidden)
        n_rows, n_items = 90, 1500
        f = np.float32
        a = np.sqrt(6.0 / (n_rows + d))
        T = (rng.standard_normal((n_items, d)) * 0.3).astype(f)
        W1 = (rng.uniform(-1, 1, (hidden, d)) / np.sqrt(d)).astype(f)
        b1 = rng.uniform(-0.1, 0.1, hidden).astype(f)
        inp = dict(V=rng.uniform(-a, a, (n_rows, d)).astype(f), W1=W1, P=(rng.standard_normal((n_items, d)) * 0.7).astype(f),
                   C=(T.astype(np.float64) @ W1.astype(np.float64).T + b1).astype(f), h=(rng.standard_normal(hidden) / np.sqrt(hidden)).astype(f),
                   lin=(rng.standard_normal(n_items) * 0.05).astype(f), const=(rng.standard_normal(n_rows) * 0.1).astype(f))
        rows = rng.permutation(n_rows)[:70]
        lists = R.random_train_lists(9, 70, n_items, most=40)
        _real[(d, hidden)] = (inp, rows, lists) + R.keys_and_bounds(inp, rows)
    return _real[(d, hidden)]


@pytest.mark.parametrize("d, hidden", [(64, 64), (16, 32)])
def test_real_values_against_float64(d, hidden, capsys):
    """Every returned score within the per-element bound derived in _nfm_eval_ref.keys_and_bounds (roundings counted on
    the header's operation order, nothing tuned), and the lists inside the band around the float64 ranking: with tau
    the K-th best float64 key among a user's unseen items, no listed item has key* < tau - 2 bound and no unlisted
    unseen item has key* > tau + 2 bound.  The worst fraction of the bound is printed; measured on MI355X: 0.014 at
    d = hidden = 64, 0.058 at d = 16 / hidden = 32."""
    K = 100
    inp, rows, lists, key, score, e_key, e_score = real_case(d, hidden)
    gi, gs = run(inp, rows, lists, K)
    worst = 0.0
    for r in range(len(rows)):
        assert (gi[r] >= 0).all() and len(set(gi[r])) == K and not np.isin(gi[r], lists[r]).any()
        err = np.abs(gs[r].astype(np.float64) - score[r, gi[r]])
        worst = max(worst, float((err / e_score[r, gi[r]]).max()))
        unseen = np.ones(key.shape[1], dtype=bool)
        unseen[lists[r]] = False
        tau = np.sort(key[r, unseen])[-K]
        assert (key[r, gi[r]] >= tau - 2 * e_key[r, gi[r]]).all()
        unseen[gi[r]] = False
        assert (key[r, unseen] <= tau + 2 * e_key[r, unseen]).all()
        assert (np.diff(gs[r]) <= 0).all()                     # (the constant shifts a user's keys alike: rounding keeps the order weakly)
    with capsys.disabled():
        print("\nnfm_eval d=%d hidden=%d: worst fraction of the score bound %.3f" % (d, hidden, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. invariance
def test_invariance_bit_for_bit():
    """A user's list and scores are the same alone and among 70 users; the first 20 of the K = 128 list are the K = 20
    list; two runs agree; the lists do not depend on whether scores are asked for."""
    inp, rows, lists = real_case()[:3]
    all_i, all_s = run(inp, rows, lists, 128)
    again_i, again_s = run(inp, rows, lists, 128)
    assert np.array_equal(all_i, again_i) and same_bits(all_s, again_s)
    k20_i, k20_s = run(inp, rows, lists, 20)
    assert np.array_equal(all_i[:, :20], k20_i) and same_bits(np.ascontiguousarray(all_s[:, :20]), k20_s)
    for r in (0, 33, 69):
        one_i, one_s = run(inp, rows[r:r + 1], lists[r:r + 1], 128)
        assert np.array_equal(one_i[0], all_i[r]) and same_bits(one_s[0], all_s[r])
    without_i, _ = run(inp, rows, lists, 128, want_scores=False)
    assert np.array_equal(without_i, all_i)


# ------------------------------------------------------------------------------------------------ 5. memory contract
@pytest.mark.parametrize("n_users, n_items, K", [(70, 1500, 100), (3, 95, 20)])
def test_memory_contract(n_users, n_items, K):
    """Scratch of exactly kgat_nfm_eval_scratch_bytes between guard bands, scratch and outputs poisoned: the bands stay
    intact, no output word keeps the poison, the bits are the clean run's."""
    from dgl_kgat_amd import ops
    inp, rows, lists = real_case()[:3]
    inp = dict(inp, P=inp["P"][:n_items], C=inp["C"][:n_items], lin=inp["lin"][:n_items])
    rows = rows[:n_users]
    lists = [x[x < n_items] for x in lists[:n_users]]
    clean_i, clean_s = run(inp, rows, lists, K)
    for poison in (POISON, 0xC2280000):
        with _arena.patched(ops, poison) as ar:
            got_i, got_s = run(inp, rows, lists, K)
        assert "kgat_nfm_eval_topk_f32" in ar.calls and "kgat_eval_items_kmajor_f32" in ar.calls
        need = ops._lib.load().kgat_nfm_eval_scratch_bytes(n_users, n_items, 64, 64, K)
        assert any(g.nbytes == need and g.what.startswith("workspace") for g in ar.guards)
        assert not ar.broken_bands(), ar.broken_bands()
        assert np.array_equal(got_i, clean_i) and same_bits(got_s, clean_s), hex(poison)
        if poison == POISON:
            assert not _arena.poison_words(torch.as_tensor(got_i), poison).any()
            assert not _arena.poison_words(torch.as_tensor(got_s), poison).any()


# ------------------------------------------------------------------------------------------------ 6. model level
def _planted_model(layers=(64,), dim=64, exact=False):
    import dgl_kgat_amd as K
    from test_gpu_fm import planted_small
    ds, (train_dict, test_dict) = planted_small()
    items = (ds.n_users, ds.n_users + ds.n_items)
    feats = K.FeatureSets.from_kg(ds.train_KG_triplet, items, ds.n_KG_entity)
    torch.manual_seed(17)
    m = K.NFM(ds.n_KG_entity, feats, dim=dim, layers=layers, dropout=0.3).to(DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        if exact:
            # integers, and 1/256 of the item position in the item's own linear weight: every score is exact in fp32 on
            # both routes and a user's scores are distinct, so torch.topk has no tie to break its own way
            m.embed.weight.copy_(torch.randint(-1, 2, m.embed.weight.shape, generator=g).float())
            m.mlp[0].weight.copy_(torch.randint(-1, 2, m.mlp[0].weight.shape, generator=g).float())
            m.mlp[0].bias.copy_(torch.randint(-2, 3, m.mlp[0].bias.shape, generator=g).float())
            m.h.copy_(torch.randint(-1, 2, m.h.shape, generator=g).float())
            m.w_lin.zero_()
            m.w_lin[items[0]:items[1]] = torch.arange(ds.n_items, device=DEV) / 256.0
            m.w0.fill_(2.0)
        else:
            m.w_lin.normal_(0, 0.1, generator=None)
            m.w0.fill_(0.2)
            m.embed.weight.mul_(4.0)
    plan = K.metrics.EvalPlan(train_dict, test_dict, ds.item_id_range, DEV)
    return m, plan, ds


def test_model_routes():
    """NFM.evaluate(fused=True) returns calc_metrics' dict, its values are ops.eval_metrics_at_ks over
    NFM.topk(fused=True), the training mode and dropout do not enter, and recommend lists the same items as node ids."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    Ks = (20, 40, 100)
    m, plan, ds = _planted_model()
    m.train()
    out = m.evaluate(plan, Ks, fused=True)
    assert m.training and set(out) == {"recall", "ndcg", "precision", "hit_ratio"}
    assert all(v.shape == (3,) and v.dtype == np.float64 for v in out.values())
    top = m.topk(plan, 100, fused=True)
    assert top.shape == (plan.n_users, 100) and top.dtype == torch.int32
    per = ops.eval_metrics_at_ks(top, plan.test_ptr, plan.test_items, Ks)
    mean = (per.sum(0) / plan.n_users).cpu().numpy()
    for j, name in enumerate(("recall", "ndcg", "precision", "hit_ratio")):
        assert np.array_equal(out[name], mean[:, j]), name
    # recommend: node ids of the same lists
    users = plan.user_ids[:9].cpu().numpy()
    train = {int(u): plan.train_items[int(plan.train_ptr[j]):int(plan.train_ptr[j + 1])].cpu().numpy() for j, u in enumerate(users)}
    items, scores = m.recommend(users, 10, seen=train)
    assert items.shape == (9, 10) and items.dtype == torch.int64 and scores.dtype == torch.float32
    assert torch.equal(items - ds.n_users, top[:9, :10].long())
    assert torch.isfinite(scores).all() and (scores[:, 1:] <= scores[:, :-1]).all()
    with pytest.raises(ValueError):
        m.recommend([0, 0], 5)
    # the reasons stated on the device
    with pytest.raises(K.KGATLibraryError, match="outside 1..128"):
        m.topk(plan, 129, fused=True)
    wide, plan_w, _ = _planted_model(layers=(128,))
    with pytest.raises(K.KGATLibraryError, match="widths d = 64, hidden = 128"):
        wide.evaluate(plan_w, (20,), fused=True)
    with pytest.raises(K.KGATLibraryError, match="ONE hidden layer"):
        _planted_model(layers=(64, 32))[0].evaluate(plan, (20,), fused=True)


@pytest.mark.parametrize("hidden", [64, 16])
def test_exact_model_equals_the_torch_route(hidden):
    """On an integer-valued model whose scores are exact in fp32 and distinct per user the fused dict equals the torch
    route's exactly, and the fused lists are torch.topk's."""
    m, plan, ds = _planted_model(layers=(hidden,), exact=True)
    m.eval()
    sc = m.scores(plan.user_ids.long())
    assert torch.equal(sc * 256, (sc * 256).round()) and sc.abs().max() < 2 ** 15
    assert all(len(torch.unique(row)) == row.numel() for row in sc)
    Ks = (20, 60, 100)
    fused, ref = m.evaluate(plan, Ks, fused=True), m.evaluate(plan, Ks)
    for k in ref:
        assert np.array_equal(fused[k], ref[k]), (k, fused[k], ref[k])
    assert torch.equal(m.topk(plan, 100, fused=True), m.topk(plan, 100))
    # recommend's scores are y(u, i) itself: w0 + w_lin[u] + the key
    users = plan.user_ids[:9].cpu().numpy()
    items, scores = m.recommend(users, 10)
    assert torch.equal(sc[:9].gather(1, items - ds.n_users), scores)


def test_planted_structure_recall_rises_on_the_fused_route(capsys):
    """examples/train_kgat.py --model nfm --planted --nfm_eval fused with the arguments and under the criterion of
    test_gpu_fm.test_planted_structure_recall_rises."""
    from test_gpu_fm import PLANTED_ARGS
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--model", "nfm"] + PLANTED_ARGS + ["--nfm_eval", "fused"])
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\n--model nfm --nfm_eval fused planted-structure run: test recall@20 by epoch %s, CF loss %s" % (
            ["%.4f" % r for r in rec], ["%.4f" % h["cf_loss"] for h in hist[1:]]))
    assert len(hist) == 4 and 0.005 < rec[0] < 0.05                # untrained: a random ranking
    assert rec[3] > 3.0 * rec[0]
    assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
