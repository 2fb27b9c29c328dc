"""Bi-Interaction pooling / FM / NFM without a GPU: the feature sets, the float64 restatement against brute force, the
torch restatement and its autograd gradient, FM's dot-product readout, NFM's block scorer, the new entries' types and
refusals (made before any device work: they come back on a machine without a device) and the harness's arguments."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, fm_models  # noqa: E402

import _bi_pool_ref as R  # noqa: E402
from test_workspace_host import BADARG, OK, P, WORKSPACE, declarations  # noqa: E402

UNSUPPORTED = -2
GOLDEN = os.path.join(ROOT, "tests", "golden", "toy_dataset.npz")


# ------------------------------------------------------------------------------------------------ feature sets
def test_from_kg_on_the_toy_dataset():
    """Self first, tails unique and sorted, users excluded, and the reversed CSR is the transpose."""
    z = np.load(GOLDEN)
    n_users, n_items, n = int(z["n_users"]), int(z["n_items"]), int(z["n_KG_entity"])
    trip = z["train_KG_triplet"].astype(np.int64)
    lo, hi = n_users, n_users + n_items
    fs = K.FeatureSets.from_kg(trip, (lo, hi), n)
    assert (fs.n_items, fs.n_features, fs.item_offset) == (n_items, n, lo)
    lists = fs.lists()
    assert (trip[:, 2] < lo).any() and any(len(x) > 1 for x in lists)     # the fixture has user tails and item-KG tails
    for j, own in enumerate(lists):
        i = lo + j
        tails = sorted({int(t) for h, _, t in trip if h == i and t >= lo})
        assert own[0] == i and list(own[1:]) == tails, (i, own, tails)
    bare = K.FeatureSets.from_kg(trip, (lo, hi), n, include_self=False).lists()
    assert all(list(a) == list(b[1:]) for a, b in zip(bare, lists))
    # the reversed CSR: feature -> item positions holding it, ascending, once per occurrence
    rp, ri = fs.rev_indptr.numpy(), fs.rev_items.numpy()
    assert rp[0] == 0 and rp[-1] == fs.n_pairs == len(ri)
    for f in range(n):
        want = [j for j, own in enumerate(lists) for x in own if x == f]
        assert list(ri[rp[f]:rp[f + 1]]) == want, f
    with pytest.raises(ValueError):
        K.FeatureSets.from_kg(trip, (hi, lo), n)


def test_feature_sets_are_multisets_and_validate():
    fs = K.FeatureSets([0, 3, 3, 5], [2, 0, 2, 1, 1], 4)
    assert [list(x) for x in fs.lists()] == [[2, 0, 2], [], [1, 1]]
    assert list(fs.rev_indptr.numpy()) == [0, 1, 3, 5, 5] and list(fs.rev_items.numpy()) == [0, 2, 2, 0, 0]
    assert fs.indptr.dtype == torch.int32 and fs.to("cpu") is fs
    for bad in (([0, 2], [0, 4], 4), ([1, 2], [0, 1], 4), ([0, 2, 1], [0, 1], 4), ([0, 1], [0, 1], 4)):
        with pytest.raises(ValueError):
            K.FeatureSets(*bad)


# ------------------------------------------------------------------------------------------------ the restatements
def test_reference_against_brute_force():
    """The float64 restatement's bi against the literal sum over pairs, on small sets with duplicates and an empty one;
    its backward against central differences of sum(g_bi bi) + sum(g_lin lin) + sum(g_sq sq)."""
    rng = np.random.default_rng(0)
    indptr, ids = [0, 3, 3, 5, 9], [2, 0, 2, 1, 1, 5, 4, 3, 5]
    items, extra = np.array([0, 1, 2, 3, 0, 1]), np.array([-1, -1, 4, 5, 2, 3])
    V, w = rng.standard_normal((6, 5)), rng.standard_normal(6)
    f, ptr = R.set_lists(indptr, ids, items, extra)
    assert list(np.diff(ptr)) == [3, 0, 3, 5, 4, 1] and list(f[ptr[4]:ptr[5]]) == [2, 2, 0, 2]
    S, bi, lin, sq = R.forward(V, w, f, ptr)
    for m in range(len(items)):
        own = f[ptr[m]:ptr[m + 1]]
        assert np.allclose(bi[m], R.brute_bi(V, own), rtol=1e-12, atol=1e-12)
        assert np.allclose(S[m], V[own].sum(0)) and np.isclose(lin[m], w[own].sum()) and np.isclose(sq[m], (V[own] ** 2).sum())
    assert not bi[1].any() and not S[1].any() and lin[1] == 0 and sq[1] == 0
    g = (rng.standard_normal(bi.shape), rng.standard_normal(len(items)), rng.standard_normal(len(items)))
    gV, gw = R.backward(V, f, ptr, S, *g)

    def total(Vx, wx):
        _, b, l, q = R.forward(Vx, wx, f, ptr)
        return (g[0] * b).sum() + (g[1] * l).sum() + (g[2] * q).sum()
    eps = 1e-6
    for idx in [(0, 0), (2, 3), (5, 4), (1, 1), (3, 2)]:
        Vp, Vm = V.copy(), V.copy()
        Vp[idx] += eps
        Vm[idx] -= eps
        assert abs((total(Vp, w) - total(Vm, w)) / (2 * eps) - gV[idx]) <= 1e-6 * max(1.0, abs(gV[idx]))
    assert np.allclose(gw, np.bincount(f, weights=np.repeat(g[1], np.diff(ptr)), minlength=6))


@pytest.mark.parametrize("d", [16, 128])
def test_torch_restatement_and_its_gradient_in_float64(d):
    """bi_pool_torch (and autograd.bi_pool, which takes it on the CPU) against the reference in float64: outputs and
    autograd's gradients, multiset duplicates, empty sets and every list length of the GPU tests included."""
    rng = np.random.default_rng(d)
    n_sets = 257
    indptr, ids, _ = R.world(d)
    items, extra = R.batch(d, n_sets)
    fs = K.FeatureSets(indptr, ids, R.N_NODES)
    Vh, wh = rng.standard_normal((R.N_NODES, d)), rng.standard_normal(R.N_NODES)
    g = (rng.standard_normal((n_sets, d)), rng.standard_normal(n_sets), rng.standard_normal(n_sets))
    f, ptr = R.set_lists(indptr, ids, items, extra)
    assert set(R.list_lengths(d)) <= set(np.diff(ptr).tolist())
    S, bi, lin, sq = R.forward(Vh, wh, f, ptr)
    gV, gw = R.backward(Vh, f, ptr, S, *g)
    for fn in (fm_models.bi_pool_torch, K.bi_pool):
        V, w = torch.tensor(Vh, requires_grad=True), torch.tensor(wh, requires_grad=True)
        b, l, q = fn(V, w, fs, torch.as_tensor(items), torch.as_tensor(extra))
        for got, want in ((b, bi), (l, lin), (q, sq)):
            assert np.abs(got.detach().numpy() - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
        ((b * torch.tensor(g[0])).sum() + (l * torch.tensor(g[1])).sum() + (q * torch.tensor(g[2])).sum()).backward()
        assert np.abs(V.grad.numpy() - gV).max() <= 1e-11 * np.abs(gV).max()
        assert np.abs(w.grad.numpy() - gw).max() <= 1e-11 * np.abs(gw).max()
    # no extra at all, no linear term
    f0, ptr0 = R.set_lists(indptr, ids, items, None)
    b, l, q = K.bi_pool(torch.tensor(Vh), None, fs, torch.as_tensor(items))
    assert np.abs(b.numpy() - R.forward(Vh, None, f0, ptr0)[1]).max() <= 1e-9 and not l.any()


# ------------------------------------------------------------------------------------------------ the models
def _toy_model(kind, dim=8, **kw):
    z = np.load(GOLDEN)
    n_users, n_items, n = int(z["n_users"]), int(z["n_items"]), int(z["n_KG_entity"])
    fs = K.FeatureSets.from_kg(z["train_KG_triplet"], (n_users, n_users + n_items), n)
    torch.manual_seed(3)
    m = (K.FM if kind == "fm" else K.NFM)(n, fs, dim=dim, **kw).double()
    with torch.no_grad():
        m.w_lin.normal_()
        m.w0.fill_(0.3)
        m.embed.weight.normal_()
    return m, n_users, n_items, n


def test_fm_readout_dot_products_are_the_scores():
    """For every (user, item) pair the dot product of the two readout rows equals FM's own score to rounding."""
    m, n_users, n_items, n = _toy_model("fm")
    table = m.readout((0, n_users), (n_users, n_users + n_items))
    assert table.shape == (n, 8 + 2) and not table[n_users + n_items:].any()
    u, i = torch.meshgrid(torch.arange(n_users), torch.arange(n_users, n_users + n_items), indexing="ij")
    y = m.score(u.reshape(-1), i.reshape(-1)).detach().reshape(n_users, n_items)
    dots = table[:n_users] @ table[n_users:n_users + n_items].T
    assert (dots - y).abs().max() <= 1e-12 * y.abs().max()
    with pytest.raises(ValueError):
        m.readout((0, n_users), (n_users + 1, n_users + n_items))
    with pytest.raises(ValueError):
        m.readout((0, n_users + 1), (n_users, n_users + n_items))


def test_fm_loss_is_the_stated_objective_and_parameters():
    m, n_users, n_items, n = _toy_model("fm", reg_lambda=0.01)
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {"embed.weight": (n, 8), "w_lin": (n,), "w0": (1,)}
    g = torch.Generator().manual_seed(0)
    u = torch.randint(0, n_users, (13,), generator=g)
    p, q = (torch.randint(n_users, n_users + n_items, (13,), generator=g) for _ in range(2))
    loss = m.get_loss(u, p, q)
    yp, yn = m.score(u, p), m.score(u, q)
    _, _, sp = m.pool(u, p)
    _, _, sn = m.pool(u, q)
    want = torch.nn.functional.softplus(yn - yp).mean() + 0.01 * (0.5 * (sp + sn)).mean()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    loss.backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in m.parameters())
    # a score is w0 + the linear terms + the sum over all pairs of the set
    own = [int(u[0])] + list(m.feats.lists()[int(p[0]) - n_users])
    V, w = m.embed.weight.detach().numpy(), m.w_lin.detach().numpy()
    assert abs(float(yp[0].detach()) - (0.3 + w[own].sum() + R.brute_bi(V, own).sum())) <= 1e-12 * max(1.0, abs(float(yp[0].detach())))
    ue, ie = torch.randn(n_users, 8), torch.randn(n_items, 8)
    m.load_pretrained(ue, ie, n_users)
    assert torch.equal(m.embed.weight[:n_users].float(), ue) and torch.equal(m.embed.weight[n_users:n_users + n_items].float(), ie)
    with pytest.raises(ValueError):
        m.load_pretrained(ue[:, :4], ie, n_users)


def test_nfm_scores_equal_per_pair_evaluation():
    m, n_users, n_items, n = _toy_model("nfm", layers=(12, 6), dropout=0.5)
    assert "mlp.0.weight" in dict(m.named_parameters()) and m.h.shape == (6,)
    m.eval()
    users = torch.tensor([0, 3, 8, 3])
    sc = m.scores(users, max_bytes=4096)                 # several user blocks
    u, i = torch.meshgrid(users, torch.arange(n_users, n_users + n_items), indexing="ij")
    y = m.score(u.reshape(-1), i.reshape(-1)).detach().reshape(len(users), n_items)
    assert sc.shape == y.shape and (sc - y).abs().max() <= 1e-12 * y.abs().max()
    m.train()                                            # the block scorer evaluates without dropout, and restores the mode
    assert (m.scores(users) - y).abs().max() <= 1e-12 * y.abs().max() and m.training
    # without hidden layers and h = 1, NFM is FM
    m0, *_ = _toy_model("nfm", layers=())
    f0, *_ = _toy_model("fm")
    f0.load_state_dict({k: v for k, v in m0.state_dict().items() if k != "h"})
    assert m0.h.shape == (8,) and bool((m0.h == 1.0).all())
    assert torch.allclose(m0.score(u.reshape(-1), i.reshape(-1)), f0.score(u.reshape(-1), i.reshape(-1)), rtol=1e-13, atol=1e-13)
    loss = m.get_loss(users, torch.full((4,), n_users), torch.full((4,), n_users + 1))
    loss.backward()
    assert m.mlp[0].weight.grad is not None and m.embed.weight.grad.abs().sum() > 0


def test_exports():
    assert K.fm_models.FM is K.FM and K.fm_models.NFM is K.NFM and K.fm_models.FeatureSets is K.FeatureSets
    from dgl_kgat_amd import autograd
    assert K.bi_pool is autograd.bi_pool and all(n in K.__all__ for n in ("FM", "NFM", "FeatureSets", "bi_pool"))


# ------------------------------------------------------------------------------------------------ the entries
NEW = {"kgat_bi_pool_supported", "kgat_bi_pool_scratch_bytes", "kgat_bi_pool_fwd_f32", "kgat_bi_pool_bwd_f32"}
ENTRIES = {"kgat_bi_pool_fwd_f32": "bi_pool_fwd", "kgat_bi_pool_bwd_f32": "bi_pool_bwd"}
OPTIONAL = {"w_lin", "extra", "lin", "sq", "g_bi", "g_lin", "g_sq", "grad_w"}
_SIZES = dict(n_sets=2048, d=64, n_nodes=5000, n_items=900, n_pairs=40000)


def _call(entry, sizes=None, pointers=None, short=0):
    lib = _lib.load()
    s = dict(_SIZES, **(sizes or {}))
    args = []
    for ctype, pname in declarations()[entry][1]:
        if pname == "scratch_bytes":
            args.append(lib.kgat_bi_pool_scratch_bytes(s["n_sets"], s["n_items"], s["n_nodes"], s["n_pairs"]) - short)
        elif pname == "stream":
            args.append(None)
        elif pointers and pname in pointers:
            args.append(pointers[pname])
        elif "*" in ctype:
            args.append(P)
        else:
            args.append(s[pname])
    rc = getattr(lib, entry)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def test_new_symbols_are_declared_exported_and_bound():
    decl = declarations()
    assert {n for n in decl if n.startswith("kgat_bi_pool")} == NEW
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        ret, params = decl[name]
        # the closed tables of the workspace and memory-contract tests do not see these names
        assert not name.endswith("_workspace_bytes")
        assert not any(p == "workspace" or (t == "float *" and (p == "tmp" or p.startswith(("partials", "part_")))) for t, p in params)
    assert decl["kgat_bi_pool_bwd_f32"][1][-3:] == [("void *", "scratch"), ("size_t", "scratch_bytes"), ("kgat_stream_t", "stream")]
    assert "kgat_bi_pool.hip" in _lib.SOURCES and _lib.ABI_VERSION == 16
    text = open(os.path.join(ROOT, "dgl-kgat_amd", "ops.py")).read()
    body = text.split("# ---------------------------------------------------------------- Bi-Interaction pooling")[1].split("# ------------------")[0]
    assert ".new_" not in body and "kgat_bi_pool_bwd_f32" in body and "_workspace(" in body


def test_supported_is_the_envelope():
    lib = _lib.load()
    ok = lambda d, m: bool(lib.kgat_bi_pool_supported(d, m))   # noqa: E731
    assert all(ok(d, 2048) for d in (16, 32, 64, 128)) and ok(64, 1) and ok(64, 8192)
    assert not any(ok(d, 2048) for d in (0, 4, 8, 24, 48, 96, 256, -16))
    assert not ok(64, 0) and not ok(64, 8193) and not ok(64, -1)
    from dgl_kgat_amd import ops
    assert ops.bi_pool_supported(64, 2048) and not ops.bi_pool_supported(20, 2048) and not ops.bi_pool_supported(64, 10 ** 5)
    need = lib.kgat_bi_pool_scratch_bytes(2048, 900, 5000, 40000)
    assert need >= 4 * (900 + 5000 + 4 * 2048 + 40000 // 256) and need % 256 == 0


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_come_before_device_work(entry):
    word = ENTRIES[entry]
    params = declarations()[entry][1]
    if entry == "kgat_bi_pool_bwd_f32":
        rc, msg = _call(entry, short=1)                  # one byte short of the stated size
        assert rc == WORKSPACE and word in msg and "scratch" in msg, (rc, msg)
        rc, msg = _call(entry, pointers={"scratch": P + 4})
        assert rc == BADARG and word in msg
    for sizes in (dict(d=0), dict(d=20), dict(d=-64), dict(d=256), dict(n_sets=0), dict(n_sets=8193)):
        rc, msg = _call(entry, sizes)
        assert rc == UNSUPPORTED and word in msg, (sizes, rc, msg)
    for sizes in (dict(n_sets=-1), dict(n_nodes=0), dict(n_nodes=-3), dict(n_nodes=2 ** 31 - 1), dict(n_items=0), dict(n_items=-1),
                  dict(n_pairs=-1), dict(n_pairs=2 ** 31 - 1)):
        rc, msg = _call(entry, sizes)
        assert rc == BADARG and word in msg, (sizes, rc, msg)
    for ctype, pname in params:
        if "*" in ctype and pname not in OPTIONAL:
            rc, msg = _call(entry, pointers={pname: None})
            assert rc == BADARG and word in msg, (pname, rc, msg)
    rc, msg = _call(entry, pointers={"V": P + 4})
    assert rc == BADARG and word in msg
    assert OK == 0


def test_cpu_tensors_are_refused_by_the_raw_wrappers():
    from dgl_kgat_amd import ops
    fs = K.FeatureSets([0, 2], [0, 1], 2)
    with pytest.raises(K.KGATLibraryError):
        ops.bi_pool_fwd(torch.zeros(2, 16), None, fs, torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the harness
def test_cli_accepts_and_refuses():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    base = vars(train_kgat.parse_args([]))
    assert "model" not in base and "nfm_layers" not in base       # a run without the flags keeps its arguments
    assert train_kgat.parse_args(["--model", "fm", "--Ks", "20,40", "--rank_metrics", "1", "--grad_norm", "1.0"]).model == "fm"
    a = train_kgat.parse_args(["--model", "nfm", "--nfm_layers", "32,16", "--pretrain_load", "mf.npz"])
    assert a.model == "nfm" and a.nfm_layers == [32, 16]
    for model in ("fm", "nfm"):
        for flags in (["--gnn_model", "graphsage"], ["--gnn_model", "rgcn"], ["--res_type", "GCN"], ["--node_dropout", "0.1"],
                      ["--attention_grad", "1"], ["--explain", "3"], ["--use_attention", "0"], ["--gpus", "2"],
                      ["--num_bases", "2"], ["--pretrain_epochs", "1"], ["--pretrain_save", "mf.npz"], ["--kg_eval", "50"],
                      ["--kg_eval", "50", "--kg_holdout", "0.1"], ["--nfm_layers", "0"]):
            with pytest.raises(SystemExit) as e:
                train_kgat.parse_args(["--model", model] + flags)
            assert e.value.code == 2, (model, flags)
    for flags in (["--model", "fm", "--nfm_layers", "32"], ["--nfm_layers", "32"], ["--model", "nfm", "--rank_metrics", "1"],
                  ["--model", "transe"]):
        with pytest.raises(SystemExit) as e:
            train_kgat.parse_args(flags)
        assert e.value.code == 2, flags
