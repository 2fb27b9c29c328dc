"""The fused graph attention (kgat_gat.hip) on the MI355X at every supported (heads, features) pair, at every tile class
merge_plan can pick, and on graphs whose rows are planted on the tile geometry - through the public path,
DGLGraph -> autograd.gat_aggregate -> backward.  tests/test_gpu_gat.py keeps the layer and the adversarial graph at four
shapes; this file is what it leaves unrun.

The metric is per element.  _gat_ref.term_scales gives, for every element of out, g_ft, g_el and g_er, the sum S of the
absolute values of the terms the element adds, and _gat_ref.scaled_error is max |x - ref64| / S over the elements with
S > 0, with x required to be exactly 0 where S == 0 (rows without edges, every edge dropped, slope 0 with every
z <= 0).  A low-degree row is judged at its own size, not at the hub's.

Bar, for each of the four tensors: scaled_error(kernel) <= max(10 x scaled_error(the restatement run in fp32), 2^-22) -
the project's bar for a kernel against fp32 arithmetic (DESIGN sections 4, 15 and 22), per element.  The fp32
restatement is the comparison, never the kernel.  Both restatements run on the CPU up to 1.3 M edges; the two cases
with 8.5 M edges run the same torch code on the device, where the order of torch's fp32 scatter adds is not fixed: the
fp32 error then varies a little from run to run, which the factor of 10 absorbs."""
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _gat_ref  # noqa: E402
from _gat_ref import NAMES  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = [(1, 16), (2, 8), (4, 4),
       (1, 32), (2, 16), (4, 8), (8, 4),
       (1, 64), (2, 32), (4, 16), (8, 8), (16, 4),
       (1, 128), (2, 64), (4, 32), (8, 16), (16, 8), (32, 4)]
FLOOR = 2.0 ** -22
SEED = 77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _tile_edges(e, hf):
    from dgl_kgat_amd import ops
    return ops._lib.load().kgat_spmm_tile_edges(e, hf)


def _make_graph(src, dst, n):
    import dgl_kgat_amd as K
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(src, dst)
    g.readonly()
    return g


def _run(g, dev, ft, el, er, slope=0.2, p=0.0, g_out=None):
    """out (and the three gradients when g_out is given) of autograd.gat_aggregate, as numpy."""
    from dgl_kgat_amd import autograd
    t = [torch.as_tensor(x, device=dev).requires_grad_(g_out is not None) for x in (ft, el, er)]
    out = autograd.gat_aggregate(g, t[0], t[1], t[2], slope, p, SEED)
    if g_out is None:
        return out.detach().cpu().numpy()
    out.backward(torch.as_tensor(g_out, device=dev))
    return [out.detach().cpu().numpy()] + [x.grad.cpu().numpy() for x in t]


def _forward_ml(g, dev, ft, el, er, slope=0.2):
    """(out, m, l) of ops.gat_forward, as numpy."""
    from dgl_kgat_amd import ops
    return [x.cpu().numpy() for x in ops.gat_forward(g._st.csr(dev), *(torch.as_tensor(x, device=dev) for x in (ft, el, er)), slope)]


def _gauss(n, H, F, seed, std=2.0):
    """ft, el, er, g_out: standard normal features and gradient, logits of standard deviation `std`."""
    rng = np.random.default_rng(seed)
    ft = rng.standard_normal((n, H, F)).astype(np.float32)
    el = (std * rng.standard_normal((n, H))).astype(np.float32)
    er = (std * rng.standard_normal((n, H))).astype(np.float32)
    g_out = rng.standard_normal((n, H, F)).astype(np.float32)
    return ft, el, er, g_out


def _keep(e, H, p):
    from dgl_kgat_amd import ops
    if p == 0:
        return None
    keep = ops.dropout_keep_mask(SEED, e, H, p)
    assert e * H < 100 or abs(keep.mean() - (1 - p)) < 0.05
    return keep


def _check(tag, got, ref, err32, S):
    """The bar of this file, for the four tensors; one printed line each."""
    bad = []
    for name, x, r, e32, s in zip(NAMES, got, ref, err32, S):
        assert x.dtype == np.float32 and x.shape == r.shape
        err, bar = _gat_ref.scaled_error(x, r, s), max(10 * e32, FLOOR)
        print("GATBAR %s %-4s err %.3e  fp32 %.3e  bar %.3e  ratio %.3f" % (tag, name, err, e32, bar, err / bar))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, bad


def _accuracy(tag, g, dev, src, dst, n, inputs, slope=0.2, p=0.0, device="cpu"):
    ft, el, er, g_out = inputs
    keep = _keep(len(src), ft.shape[1], p)
    ref, err32, S = _gat_ref.references(src, dst, n, ft, el, er, g_out, slope, keep, p, device)
    got = _run(g, dev, ft, el, er, slope, p, g_out)
    _check(tag, got, ref, err32, S)
    return got, S


def _bits(x):
    return np.asarray(x).view(np.int32)


def _same_bits(a, b):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(_bits(x), _bits(y)), name


# ---- every supported shape, on the adversarial graph

@pytest.fixture(scope="module")
def adv(dev):
    src, dst = _gat_ref.adversarial_graph()
    return dict(g=_make_graph(src, dst, _gat_ref.N), src=src, dst=dst, n=_gat_ref.N)


def test_the_shapes_are_the_supported_ones():
    from dgl_kgat_amd import ops
    assert len(set(ALL)) == 18
    assert sorted(ALL) == sorted((H, F) for H in range(1, 129) for F in range(1, 129) if ops.gat_supported(H, F))
    for H, F in ALL:
        assert ops.gat_supported(H, F) and F % 4 == 0 and H * F in (16, 32, 64, 128)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H,F", ALL)
def test_every_shape_against_fp64(dev, adv, H, F, p):
    _accuracy("adv H=%d F=%d p=%.1f" % (H, F, p), adv["g"], dev, adv["src"], adv["dst"], adv["n"],
              _gauss(adv["n"], H, F, 300 + H * F + H), 0.2, p)


@pytest.mark.parametrize("H,F", ALL)
def test_every_shape_exact_uniform_attention(dev, adv, H, F):
    ft, el, er, want = _gat_ref.uniform_attention_input(adv["src"], adv["dst"], adv["n"], H, F, 100 + H * F + H)
    got = _run(adv["g"], dev, ft, el, er)
    assert got.dtype == np.float32 and np.array_equal(got, want), "%d elements differ" % (got != want).sum()
    nz = np.bincount(adv["dst"], minlength=adv["n"]) > 0
    assert (got[~nz] == 0).all() and (~nz).sum() == adv["n"] // 20


@pytest.mark.parametrize("H,F", ALL)
def test_every_shape_exact_dominant_source(dev, adv, H, F):
    ft, el, er, want = _gat_ref.dominant_source_input(adv["src"], adv["dst"], adv["n"], H, F, 200 + H * F + H)
    got = _run(adv["g"], dev, ft, el, er)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want), "%d elements differ" % (got != want).sum()


@pytest.mark.parametrize("H,F", ALL)
def test_every_shape_reproducible(dev, adv, H, F):
    ft, el, er, g_out = _gauss(adv["n"], H, F, 300 + H * F + H)
    _same_bits(_run(adv["g"], dev, ft, el, er, 0.2, 0.5, g_out), _run(adv["g"], dev, ft, el, er, 0.2, 0.5, g_out))


# ---- planted tile geometry

PLANTED = [(4, 4), (8, 4), (4, 16), (8, 16), (1, 64), (1, 128)]
_PLANTED = {}


def _planted(H, F, transposed):
    """The planted graph of the width's tile size (tests/test_gat_host.py checks what it holds), or its transpose: the
    planted rows are then the reversed CSR's, which the source-side backward walks."""
    te = 128 if H * F == 128 else 256
    key = (te, transposed)
    if key not in _PLANTED:
        deg = _gat_ref.planted_degrees(te)
        src, dst = _gat_ref.graph_from_degrees(deg, 3)
        if transposed:
            src, dst = dst, src
        _PLANTED[key] = dict(g=_make_graph(src, dst, len(deg)), src=src, dst=dst, n=len(deg), deg=deg)
    gr = _PLANTED[key]
    assert _tile_edges(len(gr["src"]), H * F) == te          # the tile the call takes is the one the rows were planted on
    return gr


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("H,F", PLANTED)
def test_planted_rows_against_fp64(dev, H, F, transposed, p):
    gr = _planted(H, F, transposed)
    ft, el, er, g_out = inputs = _gauss(gr["n"], H, F, 400 + H * F + H)
    _accuracy("planted%s H=%d F=%d p=%.1f" % ("-T" if transposed else "", H, F, p), gr["g"], dev, gr["src"], gr["dst"], gr["n"],
              inputs, 0.2, p)
    if p == 0:
        _, m, _ = _forward_ml(gr["g"], dev, ft, el, er)
        nz = np.bincount(gr["dst"], minlength=gr["n"]) > 0
        want = _gat_ref.row_max_fp32(gr["src"], gr["dst"], gr["n"], el, er, 0.2)
        assert np.array_equal(m[nz], want[nz]), "%d row maxima differ" % (m[nz] != want[nz]).sum()


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("H,F", PLANTED)
def test_planted_rows_exact_uniform_attention(dev, H, F, transposed):
    gr = _planted(H, F, transposed)
    ft, el, er, want = _gat_ref.uniform_attention_input(gr["src"], gr["dst"], gr["n"], H, F, 500 + H * F + H)
    got = _run(gr["g"], dev, ft, el, er)
    assert np.array_equal(got, want), "%d elements differ" % (got != want).sum()
    out, m, l = _forward_ml(gr["g"], dev, ft, el, er)
    deg = np.bincount(gr["dst"], minlength=gr["n"])
    assert np.array_equal(out, want)
    assert np.array_equal(l, np.broadcast_to(deg.astype(np.float32)[:, None], l.shape))        # every p is exactly 1
    want_m = _gat_ref.row_max_fp32(gr["src"], gr["dst"], gr["n"], el, er, 0.2)
    assert np.array_equal(m[deg > 0], want_m[deg > 0])


def _degenerate(name):
    if name == "one-node-no-edge":
        return 1, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if name == "one-node-three-loops":
        return 1, np.zeros(3, np.int64), np.zeros(3, np.int64)
    if name == "five-nodes-no-edge":
        return 5, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if name == "three-edges-into-the-last-row":
        return 70, np.array([4, 69, 33], np.int64), np.full(3, 69, np.int64)
    assert name == "all-edges-one-pair"
    return 300, np.full(1000, 299, np.int64), np.zeros(1000, np.int64)


@pytest.mark.parametrize("name", ["one-node-no-edge", "one-node-three-loops", "five-nodes-no-edge",
                                  "three-edges-into-the-last-row", "all-edges-one-pair"])
@pytest.mark.parametrize("H,F", [(4, 4), (8, 16)])
def test_degenerate_graphs(dev, H, F, name):
    """Graphs of less than a run, less than a lane group, of nothing: against fp64 under the bar, the exact input bit for
    bit, and exact zeros wherever a node has no edge on the side in question."""
    n, src, dst = _degenerate(name)
    g = _make_graph(src, dst, n)
    inputs = _gauss(n, H, F, 600 + H * F)
    got, S = _accuracy("%s H=%d F=%d" % (name, H, F), g, dev, src, dst, n, inputs)
    ideg, odeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    assert (got[0][ideg == 0] == 0).all() and (got[3][ideg == 0] == 0).all()
    assert (got[1][odeg == 0] == 0).all() and (got[2][odeg == 0] == 0).all()
    assert all((s[d == 0] == 0).all() for s, d in zip(S, (ideg, odeg, odeg, ideg)))
    ft, el, er, want = _gat_ref.uniform_attention_input(src, dst, n, H, F, 700 + H * F)
    assert np.array_equal(_run(g, dev, ft, el, er), want)
    if name in ("one-node-three-loops", "all-edges-one-pair"):
        # k copies of one edge, any logits: every p = exp(0) = 1 and k x / k is exact for small integers
        assert np.array_equal(want[dst[0]], ft[src[0]])
        ft2 = np.rint(4 * inputs[0]).astype(np.float32)
        out = _run(g, dev, ft2, inputs[1], inputs[2])
        assert np.abs(ft2).max() * len(src) < 2 ** 24 and np.array_equal(out[dst[0]], ft2[src[0]])


# ---- production run lengths

PRODUCTION = [(8, 16, 600000, 512), (4, 16, 1200000, 1024), (8, 4, 1200000, 512), (4, 4, 1200000, 512),
              (8, 4, 8500000, 1024), (4, 4, 8500000, 1024)]
CPU_REFERENCE_EDGES = 1300000


@pytest.mark.parametrize("H,F,E,te", PRODUCTION)
def test_production_tiles(dev, H, F, E, te):
    """The half- and full-length runs merge_plan picks at amazon-book-size calls: several passes of the run loop per run,
    so cur_row and head_done are carried from pass to pass.  The exact input bit for bit, forward and backward against
    fp64 under the bar, the same bits from two calls.  Above 1.3 M edges the references run on the device (module
    docstring)."""
    t0 = time.time()
    assert _tile_edges(E, H * F) == te
    n = 20000
    src, dst = _gat_ref.production_graph(E)
    g = _make_graph(src, dst, n)
    where = "cpu" if E <= CPU_REFERENCE_EDGES else dev
    ft, el, er, want = _gat_ref.uniform_attention_input(src, dst, n, H, F, 800 + H * F, where)
    got = _run(g, dev, ft, el, er)
    assert np.array_equal(got, want), "%d elements differ" % (got != want).sum()
    assert (got[:n // 20] == 0).all()
    t1 = time.time()
    inputs = _gauss(n, H, F, 900 + H * F)
    a, _ = _accuracy("production H=%d F=%d E=%d" % (H, F, E), g, dev, src, dst, n, inputs, device=where)
    t2 = time.time()
    _same_bits(a, _run(g, dev, *inputs[:3], 0.2, 0.0, inputs[3]))
    del g
    torch.cuda.empty_cache()
    print("GATTIME production H=%d F=%d E=%d: exact %.1f s, fp64 %.1f s, all %.1f s" % (H, F, E, t1 - t0, t2 - t1, time.time() - t0))


# ---- slopes and zero logits

SLOPE_SHAPES = [(4, 16), (4, 4)]


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("H,F", SLOPE_SHAPES)
def test_slope_ends(dev, adv, H, F, slope):
    _accuracy("adv H=%d F=%d slope=%.1f" % (H, F, slope), adv["g"], dev, adv["src"], adv["dst"], adv["n"],
              _gauss(adv["n"], H, F, 1000 + H * F), slope, 0.0)


@pytest.mark.parametrize("H,F", SLOPE_SHAPES)
def test_exact_zero_logits(dev, adv, H, F):
    """el, er small integers: el[u] + er[v] == 0 exactly on a seventh of the edges, where leaky_relu's derivative is
    the slope (z > 0 ? 1 : slope) in the kernel as in torch."""
    n, src, dst = adv["n"], adv["src"], adv["dst"]
    ft, _, _, g_out = _gauss(n, H, F, 1100 + H * F)
    rng = np.random.default_rng(1200 + H * F)
    el = rng.integers(-3, 4, (n, H)).astype(np.float32)
    er = rng.integers(-3, 4, (n, H)).astype(np.float32)
    share = float((el[src] + er[dst] == 0).mean())
    assert share >= 0.01, share
    _accuracy("adv H=%d F=%d zero-logits" % (H, F), adv["g"], dev, src, dst, n, (ft, el, er, g_out), 0.2, 0.0)


@pytest.mark.parametrize("H,F", SLOPE_SHAPES)
def test_slope_zero_rows_without_a_positive_logit(dev, adv, H, F):
    """slope 0 and z <= 0 on every in-edge of a third of the rows (er = -64 there) and on every out-edge of a third of
    the sources (el = -64): there m = 0, the attention is uniform and no term reaches g_er, g_el - exact zeros, which
    scaled_error requires wherever the term scale is 0."""
    n, src, dst = adv["n"], adv["src"], adv["dst"]
    ft, el, er, g_out = _gauss(n, H, F, 1300 + H * F)
    rng = np.random.default_rng(1400 + H * F)
    rows, srcs = rng.random(n) < 1 / 3, rng.random(n) < 1 / 3
    er[rows], el[srcs] = -64.0, -64.0
    assert np.abs(el[~srcs]).max() < 32 and np.abs(er[~rows]).max() < 32
    got, S = _accuracy("adv H=%d F=%d slope=0 dead rows" % (H, F), adv["g"], dev, src, dst, n, (ft, el, er, g_out), 0.0, 0.0)
    ideg, odeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    assert (rows & (ideg > 0)).sum() > 100 and (srcs & (odeg > 0)).sum() > 100
    assert (S[3][rows] == 0).all() and (got[3][rows] == 0).all()
    assert (S[2][srcs] == 0).all() and (got[2][srcs] == 0).all()
    assert (S[3][~rows & (ideg > 0)] > 0).any() and (got[2] != 0).any() and (got[3] != 0).any()
    out, m, l = _forward_ml(adv["g"], dev, ft, el, er, 0.0)
    live = rows & (ideg > 0)
    assert (m[live] == 0).all()
    assert np.array_equal(l[live], np.broadcast_to(ideg[live].astype(np.float32)[:, None], l[live].shape))
