"""The relational graph convolution (kgat_rgcn_fwd_f32 / kgat_rgcn_bwd_x_f32 / kgat_rgcn_bwd_coef_f32,
autograd.rgcn_aggregate, RelGraphConv, gnn_model="rgcn") on the MI355X, against the fp64 restatement of
tests/_rgcn_ref.py on its adversarial graph.

* exact: dyadic inputs whose every sum of absolute terms stays below 2^24 granules - any fp32 summation order gives the
  same bits, so Z, g_x and g_a equal the restatement bit for bit; at every width and number of bases, with and without
  a normaliser, and at each run length the tile plan can select at D = 64;
* real-valued inputs: per element |x - ref64| <= (n + 4) 2^-24 S with n the number of terms and S the sum of their
  absolute values - Higham's bound for n fp32 terms in any order, with two product roundings; two calls give equal bits;
* autograd, the layer against a module-level fp64 restatement at 1e-5 of each tensor's scale (the project's bar for
  dense layers, tests/test_gpu_sage.py), dropout, degenerate graphs, the memory contract of the three entries (the
  helper of tests/test_gpu_memory_contract.py), and a planted-structure training run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _rgcn_ref  # noqa: E402
from _rgcn_ref import GRANULARITY, N_EDGES as E, N_NODES as N, N_REL as R  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 64, 128)
BASES = (1, 2, 3, 4, 8)
GRID = [(D, B) for D in WIDTHS for B in BASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _dgl_graph(n, src, dst, et, dev):
    import dgl_kgat_amd as K
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(src, dst)
    g.readonly()
    return dict(g=g, n=n, src=np.asarray(src), dst=np.asarray(dst), et=np.asarray(et),
                et_t=torch.as_tensor(np.asarray(et), device=dev))


@pytest.fixture(scope="module")
def graph(dev):
    from dgl_kgat_amd import _lib
    tiles = {D: _lib.load().kgat_spmm_tile_edges(E, D) for D in WIDTHS}
    src, dst, et = _rgcn_ref.adversarial_graph(set(tiles.values()))
    gr = _dgl_graph(N, src, dst, et, dev)
    csr = gr["g"]._st.csr(dev)
    assert not np.array_equal(csr.eid.cpu().numpy(), np.arange(E))      # edge id differs from CSR position
    return gr


def _run(gr, dev, x, a, norm, g_Z=None):
    """Z (and g_x, g_a when g_Z is given) of autograd.rgcn_aggregate, as numpy."""
    from dgl_kgat_amd import autograd
    xt = torch.as_tensor(x, device=dev).requires_grad_(g_Z is not None)
    at = torch.as_tensor(a, device=dev).requires_grad_(g_Z is not None)
    nt = None if norm is None else torch.as_tensor(norm, device=dev)
    Z = autograd.rgcn_aggregate(gr["g"], xt, at, gr["et_t"], nt)
    if g_Z is None:
        return {"Z": Z.detach().cpu().numpy()}
    Z.backward(torch.as_tensor(g_Z, device=dev))
    torch.cuda.synchronize()
    return {"Z": Z.detach().cpu().numpy(), "g_x": xt.grad.cpu().numpy(), "g_a": at.grad.cpu().numpy()}


def _assert_exactly_summable(ref):
    for name, r in ref.items():
        assert r.S.max() / GRANULARITY < 2 ** 24, (name, r.S.max())     # then every fp32 sum is exact in any order


@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("D,B", GRID)
def test_exact_on_the_adversarial_graph(dev, graph, D, B, with_norm):
    from dgl_kgat_amd import ops
    assert ops.rgcn_supported(D, B, R)
    x, g_Z, a, norm = _rgcn_ref.dyadic_inputs(N, E, D, B, R, 1000 + 10 * D + B, with_norm)
    ref = _rgcn_ref.restate(N, graph["src"], graph["dst"], graph["et"], norm, x, a, g_Z)
    _assert_exactly_summable(ref)
    got = _run(graph, dev, x, a, norm, g_Z)
    for name in ("Z", "g_x", "g_a"):
        want = ref[name].value.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref[name].value), name   # the reference itself is an fp32 value
        assert got[name].dtype == np.float32 and got[name].shape == want.shape, name
        assert np.array_equal(got[name], want), "%s: %d elements differ" % (name, (got[name] != want).sum())
    assert (got["Z"][290:] == 0).all() and (got["g_x"][290:] == 0).all()       # rows without edges
    assert (got["g_a"][3] == 0).all()                                            # the relation without an edge


def _run_length_cases():
    """(E, tile) per run length merge_plan can select at D = 64, each at the smallest E that selects it: short runs
    from one edge on, and past the short runs' tile limit the next length.  From the plan's own answers."""
    from dgl_kgat_amd import _lib
    lib = _lib.load()
    te_short = lib.kgat_spmm_tile_edges(1, 64)
    cases, e = [(1, te_short)], 1
    while True:                                                            # the first E whose tile differs, by bisection
        lo, hi = e, 1 << 30
        if lib.kgat_spmm_tile_edges(hi, 64) == cases[-1][1]:
            break
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if lib.kgat_spmm_tile_edges(mid, 64) == cases[-1][1] else (lo, mid)
        cases.append((hi, lib.kgat_spmm_tile_edges(hi, 64)))
        e = hi
    return cases


def test_exact_at_every_run_length(dev):
    from dgl_kgat_amd import autograd
    cases = _run_length_cases()
    assert len(cases) >= 2 and cases[1][0] == 4096 * cases[0][1] + 1      # kShortRunTileLimit tiles of short runs, plus one edge
    D, B, n = 64, 2, 3000
    for e, te in cases:
        rng = np.random.default_rng(e % 1000)
        src, dst = rng.integers(0, n - 50, e), rng.integers(0, n - 50, e)
        dst[: min(e, 12 * te)] = 7                                         # a row across twelve tiles: a long finish chain
        et = rng.integers(0, R, e)
        gr = _dgl_graph(n, src, dst, et, dev)
        x, g_Z, a, norm = _rgcn_ref.dyadic_inputs(n, e, D, B, R, 7 + te)
        xt = torch.as_tensor(x, device=dev).requires_grad_(e == 1)
        at = torch.as_tensor(a, device=dev).requires_grad_(e == 1)
        nt = torch.as_tensor(norm, device=dev)
        Z = autograd.rgcn_aggregate(gr["g"], xt, at, gr["et_t"], nt)
        # fp64 index_add on the device, one basis at a time
        s, d, t = (torch.as_tensor(v, device=dev) for v in (src, dst, et))
        c = nt.double().unsqueeze(1) * at.detach().double()[t]                                  # (E, B)
        xs = xt.detach().double()[s]
        for b in range(B):
            terms = c[:, b:b + 1] * xs
            want = torch.zeros((n, D), dtype=torch.float64, device=dev).index_add_(0, d, terms)
            S = torch.zeros((n, D), dtype=torch.float64, device=dev).index_add_(0, d, terms.abs())
            assert float(S.max()) / GRANULARITY < 2 ** 24
            assert torch.equal(Z.detach()[:, b].double(), want), (e, te, b)
        if e == 1:                                                         # forward only above the short class
            Z.backward(torch.as_tensor(g_Z, device=dev))
            ref = _rgcn_ref.restate(n, src, dst, et, norm, x, a, g_Z)
            assert np.array_equal(xt.grad.cpu().numpy().astype(np.float64), ref["g_x"].value)
            assert np.array_equal(at.grad.cpu().numpy().astype(np.float64), ref["g_a"].value)


_REAL = {}


def _real_case(graph, D, B, R_=R, et=None):
    """Real-valued inputs and their restatement, computed once per shape."""
    key = (D, B, R_)
    if key not in _REAL:
        rng = np.random.default_rng(500 + 10 * D + B + R_)
        x = rng.standard_normal((N, D)).astype(np.float32)
        g_Z = rng.standard_normal((N, B, D)).astype(np.float32)
        a = rng.standard_normal((R_, B)).astype(np.float32)
        indeg = np.bincount(graph["dst"], minlength=N)
        norm = (1.0 / indeg[graph["dst"]]).astype(np.float32)
        ref = _rgcn_ref.restate(N, graph["src"], graph["dst"], graph["et"] if et is None else et, norm, x, a, g_Z)
        _REAL[key] = (x, g_Z, a, norm, ref)
    return _REAL[key]


def _assert_within_bound(got, ref, tag):
    for name in ("Z", "g_x", "g_a"):
        r = ref[name]
        err = np.abs(got[name].astype(np.float64) - r.value)
        bound = np.broadcast_to(r.bound(), err.shape)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print("%s %s: max |x - ref64| / ((n + 4) 2^-24 S) = %.3f" % (tag, name, worst))
        assert (err <= bound).all(), "%s %s: %d elements beyond the bound, worst ratio %.3f" % (
            tag, name, int((err > bound).sum()), worst)


@pytest.mark.parametrize("D,B", GRID)
def test_real_inputs_within_the_summation_bound_and_reproducible(dev, graph, D, B):
    x, g_Z, a, norm, ref = _real_case(graph, D, B)
    got = _run(graph, dev, x, a, norm, g_Z)
    _assert_within_bound(got, ref, "D=%d B=%d" % (D, B))
    again = _run(graph, dev, x, a, norm, g_Z)
    for name in ("Z", "g_x", "g_a"):
        assert np.array_equal(got[name], again[name]), name


def test_largest_coefficient_table(dev, graph):
    """R B = 4096: the per-wavefront tables of the coefficient walk fill a launch's LDS."""
    from dgl_kgat_amd import ops
    D, B, R_ = 64, 8, 512
    assert ops.rgcn_supported(D, B, R_)
    et = np.random.default_rng(9).integers(0, R_, E)
    gr = dict(graph, et=et, et_t=torch.as_tensor(et, device=dev))
    x, g_Z, a, norm, ref = _real_case(graph, D, B, R_, et)
    _assert_within_bound(_run(gr, dev, x, a, norm, g_Z), ref, "D=64 B=8 R=512")


def test_autograd_against_torch_fp64(dev, graph):
    """rgcn_aggregate's two gradients against torch's autograd over an fp64 restatement (which the numpy helper's
    gradients must equal), within the per-element bound."""
    D, B = 32, 3
    x, g_Z, a, norm, ref = _real_case(graph, D, B)
    src, dst, et = (torch.as_tensor(graph[k]) for k in ("src", "dst", "et"))
    xt = torch.as_tensor(x).double().requires_grad_(True)
    at = torch.as_tensor(a).double().requires_grad_(True)
    c = torch.as_tensor(norm).double().unsqueeze(1) * at[et]
    Z = torch.zeros((N, B, D), dtype=torch.float64).index_add(0, dst, c.unsqueeze(2) * xt[src].unsqueeze(1))
    Z.backward(torch.as_tensor(g_Z).double())
    for name, t in (("Z", Z.detach()), ("g_x", xt.grad), ("g_a", at.grad)):
        assert np.abs(t.numpy() - ref[name].value).max() <= 1e-12 * np.abs(ref[name].value).max(), name
    # gradient only where asked for
    from dgl_kgat_amd import autograd
    xg = torch.as_tensor(x, device=dev).requires_grad_(True)
    Zg = autograd.rgcn_aggregate(graph["g"], xg, torch.as_tensor(a, device=dev), graph["et_t"], torch.as_tensor(norm, device=dev))
    Zg.backward(torch.as_tensor(g_Z, device=dev))
    err = np.abs(xg.grad.cpu().numpy().astype(np.float64) - ref["g_x"].value)
    assert (err <= ref["g_x"].bound()).all()
    with pytest.raises(TypeError):
        autograd.rgcn_aggregate(graph["g"], xg.half(), torch.as_tensor(a, device=dev), graph["et_t"])


def test_torch_route_beyond_eight_bases(dev, graph):
    """B = 9 is outside rgcn_supported: the fp64 restatement inside rgcn_aggregate, held to the same bound."""
    from dgl_kgat_amd import ops
    D, B, R_ = 32, 9, 10
    assert not ops.rgcn_supported(D, B, R_)
    et = np.random.default_rng(10).integers(0, R_, E)
    gr = dict(graph, et=et, et_t=torch.as_tensor(et, device=dev))
    x, g_Z, a, norm, ref = _real_case(graph, D, B, R_, et)
    _assert_within_bound(_run(gr, dev, x, a, norm, g_Z), ref, "D=32 B=9 (torch route)")
    # ... and an unsupported width
    x20 = np.random.default_rng(11).standard_normal((N, 20)).astype(np.float32)
    a2 = np.random.default_rng(12).standard_normal((R, 2)).astype(np.float32)
    ref20 = _rgcn_ref.restate(N, graph["src"], graph["dst"], graph["et"], None, x20, a2)
    got = _run(graph, dev, x20, a2, None)
    assert (np.abs(got["Z"].astype(np.float64) - ref20["Z"].value) <= ref20["Z"].bound()).all()


def _layer_ref64(gr, conv, x, norm):
    """DGL's own order - project by W_r per edge, then add - in fp64 on the CPU; (h, gradients by parameter name and x)."""
    src, dst, et = (torch.as_tensor(gr[k]) for k in ("src", "dst", "et"))
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    xt = torch.as_tensor(x).double().requires_grad_(True)
    W = torch.einsum("rb,bio->rio", p["w_comp"], p["weight"]) if "w_comp" in p else p["weight"]
    nm = torch.as_tensor(norm).double().reshape(-1, 1)
    h = torch.zeros((gr["n"], conv.out_feat), dtype=torch.float64)
    for r in range(W.shape[0]):                                            # one relation's edges at a time
        sel = torch.nonzero(et == r)[:, 0]
        h = h.index_add(0, dst[sel], (xt[src[sel]] @ W[r]) * nm[sel])
    if "h_bias" in p:
        h = h + p["h_bias"]
    if "loop_weight" in p:
        h = h + xt @ p["loop_weight"]
    if conv.activation is not None:
        h = conv.activation(h)
    return h, p, xt


@pytest.mark.parametrize("d_in, d_out, n_rel, bases", [(64, 32, R, 2), (32, 16, R, 4), (16, 64, 4, 4), (20, 12, R, 3)],
                         ids=["64-32-B2", "32-16-B4", "identity-B=R=4", "torch-route-d20"])
def test_relgraphconv_against_fp64(dev, graph, d_in, d_out, n_rel, bases):
    import dgl_kgat_amd as K
    torch.manual_seed(21)
    conv = K.RelGraphConv(d_in, d_out, n_rel, num_bases=bases, self_loop=True, activation=torch.relu, dropout=0.0).to(dev)
    assert hasattr(conv, "w_comp") == (bases < n_rel)
    with torch.no_grad():
        conv.h_bias.copy_(torch.randn(d_out) * 0.1)
    rng = np.random.default_rng(31)
    et = graph["et"] if n_rel == R else rng.integers(0, n_rel, E)
    gr = dict(graph, et=et, et_t=torch.as_tensor(et, device=dev))
    x = rng.standard_normal((N, d_in)).astype(np.float32)
    g_h = rng.standard_normal((N, d_out)).astype(np.float32)
    norm = (1.0 / np.bincount(graph["dst"], minlength=N)[graph["dst"]]).astype(np.float32).reshape(-1, 1)
    xt = torch.as_tensor(x, device=dev).requires_grad_(True)
    h = conv(gr["g"], xt, gr["et_t"], torch.as_tensor(norm, device=dev))
    h.backward(torch.as_tensor(g_h, device=dev))
    h64, p64, x64 = _layer_ref64(gr, conv, x, norm)
    h64.backward(torch.as_tensor(g_h).double())
    pairs = [("h", h.detach(), h64.detach()), ("x.grad", xt.grad, x64.grad)]
    pairs += [(k + ".grad", v.grad, p64[k].grad) for k, v in conv.named_parameters()]
    for name, got, want in pairs:
        want = want.numpy()
        err = np.abs(got.cpu().double().numpy() - want).max() / np.abs(want).max()
        print("RelGraphConv %d->%d B=%d %s: %.2e of the tensor's scale" % (d_in, d_out, bases, name, err))
        assert err <= 1e-5, (name, err)


def test_dropout_is_the_counter_hash_mask(dev, graph):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    torch.manual_seed(22)
    conv = K.RelGraphConv(32, 16, R, num_bases=2, self_loop=True, dropout=0.3).to(dev).train()
    x = torch.randn(N, 32, device=dev)
    norm = torch.rand(E, 1, device=dev)
    a = conv(graph["g"], x, graph["et_t"], norm, seed=99)
    b = conv(graph["g"], x, graph["et_t"], norm, seed=99)
    assert torch.equal(a, b)
    plain = conv.eval()(graph["g"], x, graph["et_t"], norm)
    keep = torch.as_tensor(ops.dropout_keep_mask(99, N, 16, 0.3), device=dev)
    assert 0.6 < float(keep.float().mean()) < 0.8
    assert bool((a[~keep] == 0).all())
    assert torch.allclose(a[keep], plain[keep] / 0.7, rtol=1e-6, atol=0)
    assert not torch.equal(conv.train()(graph["g"], x, graph["et_t"], norm, seed=100), a)


def test_degenerate_graphs(dev):
    D, B = 32, 2
    rng = np.random.default_rng(40)
    cases = {
        "no edges": (7, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)),
        "one node": (1, np.zeros(5, np.int64), np.zeros(5, np.int64), rng.integers(0, R, 5)),
        "one relation": (40, rng.integers(0, 40, 300), rng.integers(0, 40, 300), np.full(300, 2, np.int64)),
    }
    for tag, (n, src, dst, et) in cases.items():
        gr = _dgl_graph(n, src, dst, et, dev)
        x, g_Z, a, _ = _rgcn_ref.dyadic_inputs(n, len(src), D, B, R, 41)
        ref = _rgcn_ref.restate(n, src, dst, et, None, x, a, g_Z)
        _assert_exactly_summable(ref)
        got = _run(gr, dev, x, a, None, g_Z)                                  # norm=None: 1
        for name in ("Z", "g_x", "g_a"):
            assert np.array_equal(got[name].astype(np.float64), ref[name].value), (tag, name)
    assert (got["g_a"][[0, 1, 3, 4]] == 0).all()


CONTRACT_CASES = [("small", 64, 4, 256), ("small", 16, 3, 256), ("small", 128, 8, 128), ("big", 64, 2, 1024),
                  ("big", 32, 8, 512)]


@pytest.mark.parametrize("name, D, B, te", CONTRACT_CASES)
def test_memory_contract(dev, name, D, B, te):
    """The three promises of include/kgat_hip.h for the three entries: scratch of exactly kgat_rgcn_scratch_bytes between
    guard bands, outputs fully overwritten, nothing read before it is written (poisoned scratch and outputs give the
    clean pass's bits).  The graphs carry edge types outside [0, R): those edges contribute nothing."""
    import test_gpu_memory_contract as mc
    from dgl_kgat_amd import ops
    g = mc.graph(name, dev)
    assert mc._tile(g.e, D) == te
    rng = np.random.default_rng(50 + D + B)
    x = g.X(D)
    a = mc.tf(rng.standard_normal((mc.R, B)), dev)
    g_Z = mc.tf(rng.standard_normal((g.n, B, D)), dev)
    et_csr, et_rev = ops.gather(g.csr.eid, g.et), ops.gather(g.rev.eid, g.et)
    w_rev = ops.gather(g.rev.eid, ops.gather(ops.invert_permutation(g.csr.eid), g.w))   # g.w is in CSR order

    def run(alloc):
        Z = ops.rgcn_forward(g.csr, et_csr, g.w, x, a)
        g_x = ops.rgcn_backward_x(g.rev, et_rev, w_rev, g_Z, a)
        g_a = ops.rgcn_backward_coef(g.csr, et_csr, g.w, x, g_Z, mc.R, B)
        return dict(Z=Z, g_x=g_x, g_a=g_a)
    mc.check_contract("rgcn D=%d B=%d %s" % (D, B, name),
                      ["kgat_rgcn_fwd_f32", "kgat_rgcn_bwd_x_f32", "kgat_rgcn_bwd_coef_f32"], run, dev)


def test_propagation_stack_against_fp64(dev):
    """KGATPropagation(gnn_model="rgcn").gnn: the readout [h0 | normalize(h1) | ...] over the typed edges with the
    1 / in-degree normaliser, against the layers' fp64 restatement."""
    import torch.nn.functional as F
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth
    from conftest import blocks_rel_err_inf
    n, trip, n_rel = synth.amazon_book_ckg(scale=0.02)
    torch.manual_seed(23)
    m = K.KGATPropagation(n, n_rel, 64, 64, 3, 64, dropout=0.1, gnn_model="rgcn").to(dev).eval()
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        out = m.gnn(g)
    assert out.shape == (n, 64 + 64 + 32 + 16) and torch.equal(out[:, :64], m.entity_embed.weight)
    src, dst, et = trip[:, 2], trip[:, 0], trip[:, 1]
    norm = 1.0 / np.bincount(dst, minlength=n)[dst]
    gr = dict(n=n, src=src, dst=dst, et=et)
    h = m.entity_embed.weight.detach().cpu().double()
    cache = [h]
    for layer in m.layers:
        h = _layer_ref64(gr, layer, h.numpy(), norm)[0].detach()
        cache.append(F.normalize(h, dim=1))
    assert blocks_rel_err_inf(out.cpu().double().numpy(), torch.cat(cache, 1).numpy(), [64, 64, 32, 16]) <= 1e-5
    # training mode under autograd: every parameter of the stack receives a finite gradient
    m.train()
    out = m.gnn(g)
    (out[:100] * out[100:200]).sum().backward()
    for name, p_ in m.named_parameters():
        if name in ("W_R", "relation_embed.weight"):
            continue
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()) and float(p_.grad.abs().sum()) > 0, name


def test_planted_structure_recall_rises_rgcn(dev, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--planted", "--gnn_model", "rgcn", "--epochs", "3", "--lr", "0.03", "--batch_size",
                            "512", "--batch_size_kg", "512", "--eval_before", "--seed", "1234"])
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\nrgcn planted-structure run: test recall@20 by epoch %s, CF loss %s" % (
            ["%.4f" % r for r in rec], ["%.3f" % h["cf_loss"] for h in hist[1:]]))
    assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
    assert rec[3] > 3.0 * rec[0]
