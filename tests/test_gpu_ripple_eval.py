"""The fused RippleNet evaluation sweep (csrc/kgat_ripple_eval.hip) on the device, through the op layer (ops.ripple_eval_*
is the entries' argument marshalling) and through ripple_models.RippleNet: the keys pass bit for bit against its fp32
replay, exact inputs bit for bit against float64, degenerate users, real values against float64 under the bar of
tests/test_gpu_ripple.py, invariances, the memory contract and the model-level routes."""
import os
import sys

import numpy as np
import pytest
import torch

import _arena
import _ripple_eval_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POISON = 0x7FC0DEAD        # a NaN word
DIMS = (16, 32, 64)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def sets_of(inp):
    import dgl_kgat_amd as K
    if "_sets" not in inp:
        inp["_sets"] = K.RippleSets(inp["mem_h"], inp["mem_r"], inp["mem_t"], inp["ent"].shape[0], inp["rel"].shape[0], device=DEV)
    return inp["_sets"]


def run(inp, users, train_lists, K, want_scores=True):
    """kgat_eval_ripple_keys_f32 + kgat_eval_ripple_topk_f32 for the users `users`: (items, scores) as numpy."""
    from dgl_kgat_amd import ops
    ptr, flat = R.csr(train_lists)
    users = dev(np.asarray(users, dtype=np.int32))
    ent, sets = dev(inp["ent"]), sets_of(inp)
    keys = ops.ripple_eval_keys(ent, dev(inp["rel"]), sets, users)
    itemT = ops.ripple_eval_items(ent, inp["item_lo"], inp["item_lo"] + inp["n_items"])
    items, scores = ops.ripple_eval_topk(ent, sets, users, keys, itemT, inp["n_items"], dev(inp["W"]), inp["mode"],
                                         inp["all_hops"], dev(ptr), dev(flat), K, want_scores=want_scores)
    torch.cuda.synchronize()
    return items.cpu().numpy(), None if scores is None else scores.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_exact(inp, users, train_lists, K):
    """Lists AND scores equal the float64 contract's (whose values are fp32 numbers on these inputs)."""
    y = R.scores64(inp, users)
    y32 = y.astype(np.float32)
    assert np.abs(y - y32).max() < 1e-90                       # (the float64 softmax's residues of the saturated family)
    wi, ws = R.ranked(y32.astype(np.float64), train_lists, K)
    gi, gs = run(inp, users, train_lists, K)
    assert np.array_equal(gi, wi), (gi[:, :8], wi[:, :8])
    assert np.array_equal(gs, ws)            # (exact values: -0 and +0 compare equal, as the order treats them)
    return gi, gs


# ------------------------------------------------------------------------------------------------ 1. the keys pass
@pytest.mark.parametrize("M", [1, 5, 32, 33, 64])
@pytest.mark.parametrize("d", DIMS)
def test_keys_equal_the_fp32_replay(d, M):
    """One fmaf chain per element in ascending column order, bit for bit; 1, 5 and 41 relations rotating with the case;
    user 0's set is M copies of one triple, user 1's has one relation, user 2's another relation in every slot (a cycle
    where there are fewer relations than slots); user 2 is listed twice."""
    from dgl_kgat_amd import ops
    n_rel = (1, 5, 41)[(DIMS.index(d) + M) % 3]
    rng = np.random.default_rng(100 * d + M)
    n_nodes = 300
    h, t = (rng.integers(0, n_nodes, (R.N_USERS, 2, M)) for _ in range(2))
    r = np.sort(rng.integers(0, n_rel, (R.N_USERS, 2, M)), axis=2)
    for x in (h, r, t):
        x[0] = x[0, :, :1]
    r[1] = n_rel - 1
    r[2] = np.sort(np.arange(M) % n_rel)
    inp = dict(ent=rng.standard_normal((n_nodes, d)).astype(np.float32), rel=rng.standard_normal((n_rel, d * d)).astype(np.float32),
               mem_h=h, mem_r=r, mem_t=t)
    users = np.array([2, 0, 1, 7, 2, 39], dtype=np.int32)
    got = ops.ripple_eval_keys(dev(inp["ent"]), dev(inp["rel"]), sets_of(inp), dev(users)).cpu().numpy()
    want = R.keys32(inp, users)
    assert got.shape == want.shape == (6, 2, M, d) and same_bits(got, want)
    assert same_bits(got[0], got[4])


# ------------------------------------------------------------------------------------------------ 2. exact inputs
FORMS = [(d, mode, all_hops, H) for d in DIMS for mode in range(4) for all_hops in (True, False) for H in (1, 2)]


@pytest.mark.parametrize("d, mode, all_hops, H", FORMS)
def test_exact_every_form(d, mode, all_hops, H):
    """Every d x update mode x all_hops x hop count, 3 users x 95 items, on both exact families; the set sizes rotate with
    the case: uniform M in (1, 2, 32, 64), saturated M in (1, 5, 33, 64) - non-powers of two and padded slots."""
    j = FORMS.index((d, mode, all_hops, H))
    lists = R.random_train_lists(j, 3, 95)
    users = [(5 * j) % 40, 0, (j + 17) % 40]
    check_exact(R.uniform_inputs(j, 95, d, (1, 2, 32, 64)[j % 4], H, mode, all_hops), users, lists, 20)
    check_exact(R.saturated_inputs(j, 95, d, (1, 5, 33, 64)[(j // 4 + j) % 4], H, mode, all_hops), users, lists, 20)


@pytest.mark.parametrize("M", [1, 5, 33, 64])
def test_saturated_softmax_picks_a_slot_per_item(M):
    """d = 64, two hops, plus_transform: every saturated set size at the widest form, and the items of a user do not all
    choose one slot - the scores take many values."""
    inp = R.saturated_inputs(M, 95, 64, M, 2, 3, True)
    _, gs = check_exact(inp, [3, 11, 12], R.random_train_lists(M, 3, 95), 20)
    assert M == 1 or all(len(np.unique(row)) > 5 for row in gs)


@pytest.mark.parametrize("n_items", [1, 31, 32, 33, 95, 1500, 4000])
def test_exact_item_counts(n_items):
    """One item, a tile less one, a whole tile, a tile and one, many tiles (1,500: the four wavefronts' lists of one
    segment; 4,000: several segments): the padded end of the last tile never produces a candidate."""
    lists = R.random_train_lists(n_items, 3, n_items, most=min(n_items, 9) - 1)
    for inp in (R.uniform_inputs(n_items, n_items, 64, 32, 2, 3, True), R.saturated_inputs(n_items, n_items, 64, 33, 2, 3, True)):
        gi, _ = check_exact(inp, [1, 2, 5], lists, 20)
        assert gi.max() < n_items and (gi[:, min(n_items, 20):] == -1).all()


@pytest.mark.parametrize("K", [1, 20, 128])
def test_exact_every_depth(K):
    check_exact(R.uniform_inputs(7, 1500, 32, 64, 2, 3, True), [0, 3, 5], R.random_train_lists(K, 3, 1500), K)
    check_exact(R.saturated_inputs(7, 1500, 16, 5, 2, 1, False), [0, 3, 5], R.random_train_lists(K, 3, 1500), K)


@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
@pytest.mark.parametrize("K", [20, 128])
def test_exact_score_orders_fill_and_prune_the_buffer(order, K):
    """4,000 items for 3 users.  The scratch size shows that the entry cuts them into at least two segments (it holds one
    list of K entries per user, segment and wavefront).  With scores ascending in the item position every score of a
    tile reaches the wavefront's K-th best so far, so every tile of 32 is appended whole and a wavefront with more than
    eight tiles overflows its 256-entry buffer: at least one prune of a full buffer.  Descending scores pass the
    threshold only until K are held; equal scores tie everywhere and are decided by position alone."""
    from dgl_kgat_amd import ops
    n_items = 4000
    need = ops._lib.load().kgat_eval_ripple_scratch_bytes(3, n_items, 16, 32, 1, 128)
    n_seg = need // 2 // (3 * 4 * 128 * 4)
    assert n_seg >= 2 and n_items / (4 * n_seg) > 256 + 32
    inp = R.uniform_inputs(11, n_items, 16, 32, 1, 1, True, order)
    gi, gs = check_exact(inp, [0, 1, 2], R.random_train_lists(3, 3, n_items), K)
    if order == "equal":
        assert (np.diff(gi, axis=1) > 0).all() and (gs == 1).all()
    if order == "ascending":
        assert (np.diff(gi, axis=1) < 0).all()


# ------------------------------------------------------------------------------------------------ 3. degenerate users
def test_degenerate_users():
    """An empty train list, a list that leaves three unseen items (padding at the end, nothing listed twice), every item
    a training item, the same user twice with different lists, and a user id out of range: an empty list for it, the
    others as without it."""
    n_items, K = 95, 20
    inp = R.saturated_inputs(21, n_items, 32, 33, 2, 3, True)
    users = (np.arange(40) * 7) % 40
    users[5] = users[0]
    lists = R.random_train_lists(5, 40, n_items)
    lists[0] = np.zeros(0, dtype=np.int64)
    lists[1] = np.setdiff1d(np.arange(n_items), [3, 50, 94])
    lists[2] = np.arange(n_items)
    gi, gs = check_exact(inp, users, lists, K)
    for r in range(40):
        listed = gi[r][gi[r] >= 0]
        assert len(set(listed)) == len(listed) == min(K, n_items - len(lists[r])) and not np.isin(listed, lists[r]).any()
        assert (gi[r, len(listed):] == -1).all() and np.isneginf(gs[r, len(listed):]).all()
    assert len(gi[2][gi[2] >= 0]) == 0 and sorted(gi[1][:3]) == [3, 50, 94]
    for bad in (40, -1, 2 ** 31 - 1):
        with_bad = users.copy()
        with_bad[9] = bad
        bi, bs = run(inp, with_bad, lists, K)
        assert (bi[9] == -1).all() and np.isneginf(bs[9]).all()
        keep = np.arange(40) != 9
        assert np.array_equal(bi[keep], gi[keep]) and same_bits(bs[keep], gs[keep])


# ------------------------------------------------------------------------------------------------ 4. real values
_real = {}
REAL = [(64, 32, "plus_transform"), (16, 32, "plus_transform"), (64, 64, "plus_transform"), (32, 5, "replace")]


def real_case(d, M, mode, kind):
    """40 users x 1,500 items, two hops: the device model, the train lists, the float64 scores and the error of the CPU
    fp32 RippleNet.scores under err(x) = max|x - x64| / max|x64| - computed once."""
    import dgl_kgat_amd as K
    key = (d, M, mode, kind)
    if key not in _real:
        rng = np.random.default_rng(1000 + d + M + len(kind))
        n_items, n_rel = 1500, 7
        n_nodes = R.N_USERS + n_items + 100
        h, t = (rng.integers(0, n_nodes, (R.N_USERS, 2, M)) for _ in range(2))
        r = np.sort(rng.integers(0, n_rel, (R.N_USERS, 2, M)), axis=2)
        sets = K.RippleSets(h, r, t, n_nodes, n_rel)
        torch.manual_seed(d + M)
        m = K.RippleNet(n_nodes, sets, dim=d, item_update_mode=mode, item_range=(R.N_USERS, R.N_USERS + n_items))
        if kind == "sharp":
            with torch.no_grad():
                m.entity_emb.weight.normal_(0, 1)
        ref = K.RippleNet(n_nodes, sets, dim=d, item_update_mode=mode, item_range=m.item_range).double()
        ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        users = torch.arange(R.N_USERS)
        y64 = ref.scores(users).numpy()
        y32 = m.scores(users).numpy()
        scale = np.abs(y64).max()
        e_c = np.abs(y32.astype(np.float64) - y64).max() / scale
        lists = R.random_train_lists(9, R.N_USERS, n_items, most=40)
        _real[key] = (m.to(DEV), lists, y64, e_c)
    return _real[key]


def fused(model, lists, K, users=None, max_bytes=1 << 28):
    ptr, flat = R.csr(lists)
    users = np.arange(len(lists), dtype=np.int32) if users is None else np.asarray(users, dtype=np.int32)
    gi, gs = model._fused_topk("test", dev(users), dev(ptr), dev(flat), K, max_bytes)
    torch.cuda.synchronize()
    return gi.cpu().numpy(), gs.cpu().numpy()


@pytest.mark.parametrize("kind", ["init", "sharp"])
@pytest.mark.parametrize("d, M, mode", REAL)
def test_real_values_against_float64(d, M, mode, kind, capsys):
    """The bar of tests/test_gpu_ripple.py: bar = max(10 err(CPU fp32 RippleNet.scores), (d + M) 2^-24), measured in every
    run and never tuned against the kernel.  Every returned score lies within B = bar max|y64| of its float64 value and
    the lists lie inside the band: with tau the K-th best float64 score among a user's unseen items, no listed item
    has y64 < tau - 2 B and no unlisted unseen item has y64 > tau + 2 B.  The worst fraction of B is printed."""
    K = 100
    model, lists, y64, e_c = real_case(d, M, mode, kind)
    bar = max(10.0 * e_c, (d + M) * 2.0 ** -24)
    B = bar * np.abs(y64).max()
    gi, gs = fused(model, lists, K)
    worst = 0.0
    for u in range(len(lists)):
        assert (gi[u] >= 0).all() and len(set(gi[u])) == K and not np.isin(gi[u], lists[u]).any()
        assert np.isfinite(gs[u]).all() and (np.diff(gs[u]) <= 0).all()
        worst = max(worst, float(np.abs(gs[u].astype(np.float64) - y64[u, gi[u]]).max() / B))
    with capsys.disabled():
        print("\nripple_eval d=%d M=%d %s %s: cpu-fp32 err %.3e bar %.3e, worst fraction of the bar %.3f" % (
            d, M, mode, kind, e_c, bar, worst))
    assert worst <= 1.0
    for u in range(len(lists)):
        unseen = np.ones(y64.shape[1], dtype=bool)
        unseen[lists[u]] = False
        tau = np.sort(y64[u, unseen])[-K]
        assert (y64[u, gi[u]] >= tau - 2 * B).all()
        unseen[gi[u]] = False
        assert (y64[u, unseen] <= tau + 2 * B).all()


# ------------------------------------------------------------------------------------------------ 5. invariance
def test_invariance_bit_for_bit():
    """A user's list and scores are the same alone and among 40 users; the first 20 of the K = 128 list are the K = 20
    list; two max_bytes that block the users differently (all 40 at once, blocks of 6) agree; two runs agree."""
    model, lists, _, _ = real_case(64, 32, "plus_transform", "sharp")
    all_i, all_s = fused(model, lists, 128)
    again_i, again_s = fused(model, lists, 128)
    assert np.array_equal(all_i, again_i) and same_bits(all_s, again_s)
    k20_i, k20_s = fused(model, lists, 20)
    assert np.array_equal(all_i[:, :20], k20_i) and same_bits(np.ascontiguousarray(all_s[:, :20]), k20_s)
    for u in (0, 17, 39):
        one_i, one_s = fused(model, lists[u:u + 1], 128, users=[u])
        assert np.array_equal(one_i[0], all_i[u]) and same_bits(one_s[0], all_s[u])
    small = 6 * 4 * 2 * 32 * 64                                   # six users' key tables
    blk_i, blk_s = fused(model, lists, 128, max_bytes=small)
    assert np.array_equal(blk_i, all_i) and same_bits(blk_s, all_s)


# ------------------------------------------------------------------------------------------------ 6. memory contract
@pytest.mark.parametrize("n_call, n_items, K", [(40, 1500, 100), (3, 95, 20)])
def test_memory_contract(n_call, n_items, K):
    """Scratch of exactly kgat_eval_ripple_scratch_bytes between guard bands, scratch and outputs poisoned: the bands
    stay intact, no output word keeps the poison, the bits are the clean run's."""
    from dgl_kgat_amd import ops
    inp = R.saturated_inputs(3, n_items, 64, 33, 2, 3, True)
    users = (np.arange(n_call) * 3) % 40
    lists = R.random_train_lists(2, n_call, n_items)
    clean_i, clean_s = run(inp, users, lists, K)
    for poison in (POISON, 0xC2280000):
        with _arena.patched(ops, poison) as ar:
            got_i, got_s = run(inp, users, lists, K)
        for name in ("kgat_eval_ripple_keys_f32", "kgat_eval_ripple_topk_f32", "kgat_eval_items_kmajor_f32"):
            assert name in ar.calls
        need = ops._lib.load().kgat_eval_ripple_scratch_bytes(n_call, n_items, 64, 33, 2, K)
        assert any(g.nbytes == need and g.what.startswith("workspace") for g in ar.guards)
        assert not ar.broken_bands(), ar.broken_bands()
        assert np.array_equal(got_i, clean_i) and same_bits(got_s, clean_s), hex(poison)
        if poison == POISON:
            assert not _arena.poison_words(torch.as_tensor(got_i), poison).any()
            assert not _arena.poison_words(torch.as_tensor(got_s), poison).any()


# ------------------------------------------------------------------------------------------------ 7. model level
def test_exact_model_equals_the_torch_route():
    """A RippleNet whose scores are exact in fp32 on both routes and distinct per user (relation_emb = 0, 32 slots whose
    tails are one node with row e_0, `plus`, two hops: y = 2 (v_0[0] + 2), column 0 of the item rows a permutation of the
    positions over 256): the fused lists are torch.topk's, the evaluate dicts are equal, recommend returns node ids."""
    import dgl_kgat_amd as K
    rng = np.random.default_rng(5)
    n_items, d, M = 700, 32, 32
    n_nodes = R.N_USERS + n_items + 20
    h = rng.integers(0, n_nodes, (R.N_USERS, 2, M))
    r = np.sort(rng.integers(0, 3, (R.N_USERS, 2, M)), axis=2)
    sets = K.RippleSets(h, r, np.full_like(h, n_nodes - 1), n_nodes, 3, device=DEV)
    m = K.RippleNet(n_nodes, sets, dim=d, item_update_mode="plus", item_range=(R.N_USERS, R.N_USERS + n_items)).to(DEV)
    with torch.no_grad():
        ent = rng.integers(-1, 2, (n_nodes, d)).astype(np.float32)
        ent[R.N_USERS:R.N_USERS + n_items, 0] = rng.permutation(n_items) / 256.0
        ent[n_nodes - 1] = 0
        ent[n_nodes - 1, 0] = 1
        m.entity_emb.weight.copy_(dev(ent))
        m.relation_emb.weight.zero_()
    train = {u: rng.choice(n_items, 1 + u % 7, replace=False) for u in range(R.N_USERS)}
    test = {u: rng.choice(n_items, 3, replace=False) for u in range(R.N_USERS)}
    plan = K.metrics.EvalPlan(train, test, np.arange(R.N_USERS, R.N_USERS + n_items), DEV)
    sc = m.scores(plan.user_ids.long())
    assert torch.equal(sc, (2 * (dev(ent[R.N_USERS:R.N_USERS + n_items, 0]) + 2)).expand_as(sc))
    Ks = (20, 60, 100)
    got, ref = m.evaluate(plan, Ks, fused=True), m.evaluate(plan, Ks)
    assert set(got) == {"recall", "ndcg", "precision", "hit_ratio"}
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    top = m.topk(plan, 100, fused=True)
    assert top.dtype == torch.int32 and torch.equal(top, m.topk(plan, 100))
    assert torch.equal(m.topk(plan, 100, max_bytes=5 * 4 * 2 * M * d, fused=True), top)
    users = plan.user_ids[:9].cpu().numpy()
    items, scores = m.recommend(users, 10, seen={int(u): train[int(u)] for u in users})
    assert items.dtype == torch.int64 and torch.equal(items - R.N_USERS, top[:9, :10].long())
    assert torch.equal(sc[:9].gather(1, items - R.N_USERS), scores)
    with pytest.raises(ValueError):
        m.recommend([0, 0], 5)
    with pytest.raises(K.KGATLibraryError, match="outside 1..128"):
        m.topk(plan, 129, fused=True)


def test_refusals_stated_on_the_device():
    import dgl_kgat_amd as K
    rng = np.random.default_rng(1)
    for d, M, H, why in ((128, 8, 2, "d = 128"), (16, 65, 2, "n_memory = 65"), (16, 8, 3, "n_hop = 3")):
        n_nodes = 100
        h = rng.integers(0, n_nodes, (R.N_USERS, H, M))
        sets = K.RippleSets(h, np.zeros_like(h), h, n_nodes, 1, device=DEV)
        m = K.RippleNet(n_nodes, sets, dim=d).to(DEV)
        plan = K.metrics.EvalPlan({}, {0: np.array([1])}, np.arange(R.N_USERS, n_nodes), DEV)
        with pytest.raises(K.KGATLibraryError, match=why):
            m.evaluate(plan, (20,), fused=True)
        assert m.topk(plan, 5).shape == (1, 5)                  # the torch route serves them


def test_planted_structure_recall_rises_on_the_fused_route(capsys):
    """examples/train_kgat.py --model ripplenet --planted --ripple_inverse 1 --ripple_eval fused with the arguments and
    under the criterion of test_gpu_ripple.test_planted_structure_recall_rises."""
    from test_gpu_ripple import PLANTED_ARGS
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--model", "ripplenet", "--ripple_inverse", "1"] + PLANTED_ARGS + ["--ripple_eval", "fused"])
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\n--model ripplenet --ripple_eval fused planted-structure run: test recall@20 by epoch %s, CF loss %s" % (
            ["%.4f" % r for r in rec], ["%.4f" % h["cf_loss"] for h in hist[1:]]))
    assert len(hist) == 4 and 0.005 < rec[0] < 0.05                # untrained: a random ranking
    assert rec[3] > 3.0 * rec[0]
    assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
