"""The sparse BACKWARD operators against float64 on adversarial graphs.

* ``u_mul_e_sum`` backward w.r.t. the features: the aggregation on the reversed graph's CSR with the weights
  re-permuted by ``rev_weights`` (every layer of ``_GNNTrain.backward`` runs it);
* the default ("Bi") training stack ``autograd.gnn_train`` against torch-fp64 autograd of a restatement;
* ``ops.edge_softmax_bwd`` (kgat_edge_softmax_bwd_f32) and ``ops.sddmm_dot`` (kgat_sddmm_dot_f32).

Every reference is float64 (oracle/kgat_oracle.py or torch-fp64 autograd) computed from the SAME fp32 inputs as
the device run, so only arithmetic error separates the two, and the bars are worst-case rounding bounds of the
kernels' documented summation structure, not measured tolerances: with u = 2^-24 and gamma_k = k u / (1 - k u),
a sum of L fma terms in any order is within gamma_L of its exact value relative to the sum of |terms|.  On top of
the bounds, inputs whose result is exact in fp32 (counts, a single non-zero term) are compared for equality:
a relative bar cannot see one dropped or doubled edge among 9,000, these can."""
import math

import numpy as np
import pytest
import torch

from conftest import sum_err
from oracle import kgat_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def tf(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def t32(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)


def _np64(t):
    return t.detach().cpu().double().numpy()


# ------------------------------------------------------------------------------------------------ graphs
HUB_SRC, HUB_DST, PAIR = 3, 7, (1, 4)  # planted hub source / hub destination / the pair repeated 10 x


def random_graph(seed, n, e, hub_src=0, hub_dst=0, no_out_tail=0, no_in_head=0):
    """Uniform random edges; `hub_src` of them leave node HUB_SRC and `hub_dst` OTHER ones enter node HUB_DST; the last
    `no_out_tail` nodes are never a source, the first `no_in_head` never a destination."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, max(n - no_out_tail, 1), e)
    dst = rng.integers(min(no_in_head, n - 1), n, e)
    if hub_src or hub_dst:
        idx = rng.choice(e, min(hub_src + hub_dst, e), replace=False)
        src[idx[:hub_src]] = min(HUB_SRC, n - 1)
        dst[idx[hub_src:]] = min(HUB_DST, n - 1)
    return src.astype(np.int32), dst.astype(np.int32)


def _self_loops_and_parallel():
    """7 nodes, 40 edges: a self-loop on every node, PAIR[0] -> PAIR[1] ten times, 23 random edges; shuffled ids."""
    rng = np.random.default_rng(21)
    n = 7
    src = np.concatenate([np.arange(n), np.full(10, PAIR[0]), rng.integers(0, n, 23)])
    dst = np.concatenate([np.arange(n), np.full(10, PAIR[1]), rng.integers(0, n, 23)])
    p = rng.permutation(len(src))
    return src[p].astype(np.int32), dst[p].astype(np.int32)


GRAPH_SPECS = {
    # name: (n, e, generator)
    "empty": (5, 0, lambda: random_graph(1, 5, 0)),
    "single_edge": (3, 1, lambda: (np.array([2], np.int32), np.array([0], np.int32))),
    "self_loops_and_parallel": (7, 40, _self_loops_and_parallel),
    "ragged": (300, 5000, lambda: random_graph(2, 300, 5000, no_out_tail=40, no_in_head=40)),
    "hub_source": (500, 20000, lambda: random_graph(3, 500, 20000, hub_src=9000, no_out_tail=100)),
    "all_from_one_source": (64, 7000, lambda: random_graph(4, 64, 7000, hub_src=7000)),
    "hub_both": (5000, 60000, lambda: random_graph(5, 5000, 60000, hub_src=3000, hub_dst=3000)),
}
GRAPH_NAMES = list(GRAPH_SPECS)


class _Graph:
    def __init__(self, name, dev):
        from dgl_kgat_amd import synth
        self.name = name
        self.n, self.e, make = GRAPH_SPECS[name]
        self.src, self.dst = make()
        assert len(self.src) == len(self.dst) == self.e
        trip = np.stack([self.dst, np.zeros(self.e, np.int32), self.src], 1).astype(np.int32)  # [h, r, t]: t -> h
        self.g = synth.build_graph(self.n, trip, dev)
        self.out_deg = np.bincount(self.src, minlength=self.n)
        self.in_deg = np.bincount(self.dst, minlength=self.n)


@pytest.fixture(scope="module")
def graphs(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Graph(name, dev)
        return cache[name]
    return get


def test_graph_set_is_what_it_claims(graphs):
    G = graphs("self_loops_and_parallel")
    assert all(np.any((G.src == v) & (G.dst == v)) for v in range(G.n))
    assert np.sum((G.src == PAIR[0]) & (G.dst == PAIR[1])) >= 10
    G = graphs("ragged")
    assert np.all(G.out_deg[-40:] == 0) and np.all(G.in_deg[:40] == 0) and np.all(G.out_deg[:260] > 0)
    G = graphs("hub_source")
    assert G.out_deg[HUB_SRC] >= 9000 and np.sum(G.out_deg == 0) == 100
    G = graphs("all_from_one_source")
    assert G.out_deg[HUB_SRC] == 7000
    G = graphs("hub_both")
    assert G.out_deg[HUB_SRC] >= 3000 and G.in_deg[HUB_DST] >= 3000
    assert np.sum((G.src == HUB_SRC) & (G.dst == HUB_DST)) < 10


# --------------------------------------------------------------- 1. u_mul_e_sum backward w.r.t. the features
def _features(rng, n, D, dev):
    """(host (n, D) array, device tensor): D == 1 is handed over 1-D (the squeeze path)."""
    x = rng.standard_normal((n, D)).astype(np.float32)
    return x, tf(x.reshape(-1) if D == 1 else x, dev)


def _grad_x(G, xd, wd, Gd, **kw):
    from dgl_kgat_amd.autograd import u_mul_e_sum
    xd = xd.detach().clone().requires_grad_(True)
    out = u_mul_e_sum(G.g, xd, wd)
    assert out.shape == xd.shape
    out.backward(Gd, **kw)
    assert xd.grad.shape == xd.shape
    return out, xd


def _check_gamma(got, ref, A, L, what):
    """|got - ref| <= gamma_{L+1} A per element (L per row), exact zeros where A == 0; returns the worst ratio."""
    got, ref, A = (np.asarray(t, np.float64).reshape(len(L), -1) for t in (got, ref, A))
    assert np.all(np.isfinite(got)), what
    assert np.all(got[A == 0] == 0), (what, "rows without terms must be exact zeros")
    bound = gamma(np.asarray(L) + 1)[:, None] * A
    err = np.abs(got - ref)
    nz = bound > 0
    ratio = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    print("[s1 gamma] %-44s worst |err| / bound = %.4f" % (what, ratio))
    assert np.all(err <= bound), (what, ratio)
    return ratio


@pytest.mark.parametrize("D", [1, 8, 20, 16, 32, 64, 128])
@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_umule_backward_x_fp64_bound(dev, graphs, name, D):
    """Any summation order of a row's L fma terms w_e * G[v] is within gamma_{L+1} of the exact sum relative to the sum
    of |terms| (L = the node's out-degree): no measured tolerance.  Nodes without out-edges get exact zeros.  Two
    backward passes give the same bits."""
    G = graphs(name)
    rng = np.random.default_rng(1000 + 7 * GRAPH_NAMES.index(name) + D)
    _, xd = _features(rng, G.n, D, dev)
    go, god = _features(rng, G.n, D, dev)
    w = rng.random(G.e).astype(np.float32)
    wd = tf(w, dev).reshape(-1, 1)
    out, xg = _grad_x(G, xd, wd, god, retain_graph=True)
    g1 = xg.grad.clone()
    xg.grad = None
    out.backward(god)
    assert torch.equal(g1, xg.grad), "two backward passes differ"
    ref = orc.spmm_backward_x(G.n, G.src, G.dst, go, w)
    A = orc.spmm_backward_x(G.n, G.src, G.dst, np.abs(go), w)
    _check_gamma(_np64(g1), ref, A, G.out_deg, "%s D=%d" % (name, D))
    assert sum_err(_np64(g1).reshape(G.n, -1), ref, A) < 1e-4


@pytest.mark.parametrize("D", [1, 16, 64, 128])
@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_umule_backward_x_counts_edges(dev, graphs, name, D):
    """w = 1, G = 1: every element of grad_x IS the node's out-degree (small integers add exactly in fp32 in any order),
    so one dropped or doubled edge in a 9,000-edge reversed row shows."""
    G = graphs(name)
    shape = (G.n,) if D == 1 else (G.n, D)
    xd = torch.zeros(shape, device=dev)
    _, xg = _grad_x(G, xd, torch.ones((G.e, 1), device=dev), torch.ones(shape, device=dev))
    got = xg.grad.cpu().numpy().reshape(G.n, -1)
    assert np.array_equal(got, np.broadcast_to(G.out_deg[:, None].astype(np.float32), got.shape))


NEEDLES = [
    ("hub_both", HUB_DST), ("hub_both", 4321), ("hub_source", 250), ("all_from_one_source", 40), ("ragged", 299),
    ("self_loops_and_parallel", 6), ("self_loops_and_parallel", PAIR[1]), ("single_edge", 0),
]


@pytest.mark.parametrize("D", [1, 64])
@pytest.mark.parametrize("name,v", NEEDLES)
def test_umule_backward_x_needle(dev, graphs, name, v, D):
    """Distinct weights, G zero except row v: grad_x[u] is the sum over the edges u -> v alone, so a weight read from
    the wrong position of a (long) reversed row cannot hide.  One edge u -> v: the bits of fp32(w_e) * G[v] (every
    other term of the row is an exact zero).  Several parallel edges u -> v (the planted pair, and the pairs a random
    graph repeats): an fma chain and a sum of rounded products are both correct and differ, so those rows are held to
    the float64 value under gamma_{L+1} with L the number of parallel edges.  No edge: exact zero."""
    G = graphs(name)
    rng = np.random.default_rng(50 + v + D)
    w = ((rng.permutation(G.e) + 1.0) / (G.e + 1.0)).astype(np.float32)
    assert len(np.unique(w)) == G.e
    go = np.zeros((G.n, D), np.float32)
    go[v] = rng.standard_normal(D).astype(np.float32)
    xd = torch.zeros((G.n,) if D == 1 else (G.n, D), device=dev)
    _, xg = _grad_x(G, xd, tf(w, dev).reshape(-1, 1), tf(go.reshape(-1) if D == 1 else go, dev))
    got = xg.grad.cpu().numpy().reshape(G.n, D)
    into_v = np.nonzero(G.dst == v)[0]
    assert len(into_v) > 0
    mult = np.bincount(G.src[into_v], minlength=G.n)   # edges u -> v per source u
    assert np.all(got[mult == 0] == 0)
    one = into_v[mult[G.src[into_v]] == 1]
    assert np.array_equal(got[G.src[one]], w[one][:, None] * go[v][None, :]), "single-edge rows must be exact"
    many = np.nonzero(mult > 1)[0]
    if (name, v) in (("self_loops_and_parallel", PAIR[1]), ("hub_both", HUB_DST)):
        assert len(many) > 0 and (name != "self_loops_and_parallel" or mult[PAIR[0]] >= 10)
    if len(many):
        ref = orc.spmm_backward_x(G.n, G.src, G.dst, go, w)
        A = orc.spmm_backward_x(G.n, G.src, G.dst, np.abs(go), w)
        _check_gamma(got[many], ref[many], A[many], mult[many], "needle %s v=%d D=%d" % (name, v, D))


@pytest.mark.parametrize("D", [1, 20, 64])
@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_umule_backward_x_stride0_gradient(dev, graphs, name, D):
    """out.sum().backward() hands the backward an expanded (stride-0) gradient: the same bits as a dense ones tensor."""
    from dgl_kgat_amd.autograd import u_mul_e_sum
    G = graphs(name)
    rng = np.random.default_rng(77 + D)
    _, xd = _features(rng, G.n, D, dev)
    wd = tf(rng.random(G.e), dev).reshape(-1, 1)
    xa = xd.clone().requires_grad_(True)
    u_mul_e_sum(G.g, xa, wd).sum().backward()
    _, xb = _grad_x(G, xd, wd, torch.ones_like(xd))
    assert torch.equal(xa.grad, xb.grad)


def test_umule_fused_epilogue_has_no_backward(dev, graphs):
    from dgl_kgat_amd.autograd import u_mul_e_sum
    G = graphs("ragged")
    x = torch.randn(G.n, 16, device=dev, requires_grad=True)
    out = u_mul_e_sum(G.g, x, torch.rand(G.e, 1, device=dev), mul_self=True)
    with pytest.raises(NotImplementedError):
        out.sum().backward()


def test_umule_backward_x_cancellation(dev, graphs):
    """Weights of mixed sign on the 9,000-edge reversed row: elements that nearly cancel are still within
    gamma_{L+1} of the sum of |terms| (the only assertion: a bar relative to the result itself would be meaningless)."""
    G = graphs("hub_source")
    rng = np.random.default_rng(99)
    _, xd = _features(rng, G.n, 64, dev)
    go, god = _features(rng, G.n, 64, dev)
    w = rng.standard_normal(G.e).astype(np.float32)
    _, xg = _grad_x(G, xd, tf(w, dev).reshape(-1, 1), god)
    ref = orc.spmm_backward_x(G.n, G.src, G.dst, go, w)
    A = orc.spmm_backward_x(G.n, G.src, G.dst, np.abs(go), np.abs(w))
    _check_gamma(_np64(xg.grad), ref, A, G.out_deg, "cancellation hub_source D=64")


# ------------------------------------------------------- 2. the default ("Bi") stack against torch-fp64 autograd
def _scale_err(x, y):
    """The sibling stack tests' metric: max |x - y| / max |y|."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y)) / max(np.abs(y).max(), 1e-30)) if y.size else 0.0


def _bi_stack_restated(h0, Ws, a, src, dst, masks, p, R, dtype):
    """[h0 | normalize(h1) | ...] with h_{l+1} = dropout(leaky_relu((h_l * h_N) W^T)) in plain torch on the host
    (index_add_, no project kernel), and the gradients of sum(readout * R) w.r.t. h0 and every W."""
    h = h0.to(dtype).clone().requires_grad_(True)
    Ws = [w.to(dtype).clone().requires_grad_(True) for w in Ws]
    a = a.to(dtype).reshape(-1, 1)
    x, cache = h, [h]
    for li, W in enumerate(Ws):
        hn = torch.zeros_like(x).index_add_(0, dst, a * x[src])
        z = torch.nn.functional.leaky_relu((x * hn) @ W.t(), 0.01)
        x = torch.where(masks[li], z / (1 - p), torch.zeros_like(z))
        cache.append(torch.nn.functional.normalize(x, p=2, dim=1))
    out = torch.cat(cache, 1)
    (out * R.to(dtype)).sum().backward()
    return [out.detach(), h.grad] + [W.grad for W in Ws]


@pytest.mark.parametrize("name,widths", [
    ("hub_both", (64, 64, 64, 64)),
    ("hub_source", (64, 64, 32, 16)),          # the paper's pyramid, which KGATPropagation never builds
    ("self_loops_and_parallel", (16, 64)),
    ("empty", (64, 64)),
    ("single_edge", (64, 64)),
])
def test_bi_stack_training_unit_vs_fp64_autograd(dev, graphs, name, widths):
    """autograd.gnn_train with the default aggregator (forms=None: "Bi", the form the benchmark trains) and hash
    dropout against torch-fp64 autograd of a restatement that shares NO kernel with it - neither the reversed-CSR
    aggregation nor rev_weights, which the fused-vs-unfused tests have on both sides.  Readout and the gradients
    w.r.t. h0 and every W2, max |x - y| / max |y| per tensor.  Bar: the project's 1e-5, or twice what a plain torch
    fp32 run of the same restatement shows against the same float64 result (another, equally valid fp32 summation
    order; the factor conftest.parity_8c uses)."""
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.autograd import gnn_train
    G = graphs(name)
    p, seed = 0.2, 99
    rng = np.random.default_rng(300 + len(widths) + G.n)
    # softmax-like weights: positive, summing to one over every destination's in-edges
    a = rng.random(G.e) + 0.05
    a = (a / np.maximum(np.bincount(G.dst, weights=a, minlength=G.n), 1e-30)[G.dst]).astype(np.float32)
    h0 = torch.as_tensor(rng.standard_normal((G.n, widths[0])).astype(np.float32))
    Ws = [torch.as_tensor((rng.standard_normal((do, di)) / math.sqrt(di)).astype(np.float32))
          for di, do in zip(widths[:-1], widths[1:])]
    R = torch.as_tensor(rng.standard_normal((G.n, sum(widths))).astype(np.float32))
    masks = [torch.as_tensor(ops.dropout_keep_mask(seed + li, G.n, w.shape[0], p)) for li, w in enumerate(Ws)]
    src, dst = torch.as_tensor(G.src.astype(np.int64)), torch.as_tensor(G.dst.astype(np.int64))
    a_t = torch.as_tensor(a)
    ref64 = _bi_stack_restated(h0, Ws, a_t, src, dst, masks, p, R, torch.float64)
    ref32 = _bi_stack_restated(h0, Ws, a_t, src, dst, masks, p, R, torch.float32)

    g = G.g.local_var()
    g.edata["w"] = a_t.to(dev).reshape(-1, 1)
    h0d = h0.to(dev).requires_grad_(True)
    Wd = [w.to(dev).requires_grad_(True) for w in Ws]
    out = gnn_train(g, h0d, Wd, 0.01, p, seed)
    assert type(out.grad_fn).__name__.startswith("_GNNTrain")
    (out * R.to(dev)).sum().backward()
    got = [out, h0d.grad] + [w.grad for w in Wd]
    names = ["readout", "grad h0"] + ["grad W2_%d" % i for i in range(len(Ws))]
    bad = []
    for nm, x, y32, y64 in zip(names, got, ref32, ref64):
        assert x is not None and tuple(x.shape) == tuple(y64.shape), nm
        e_dev, e_32 = _scale_err(_np64(x), y64.numpy()), _scale_err(y32.double().numpy(), y64.numpy())
        print("[s2 Bi stack] %-24s %-11s device %.3e   torch-fp32 %.3e   (max|x-y|/max|y| vs fp64; bar max(1e-5, 2 x fp32))"
              % (name, nm, e_dev, e_32))
        if not e_dev <= max(1e-5, 2 * e_32):
            bad.append((nm, e_dev, e_32))
    assert not bad, bad
    if G.e == 0:  # nothing is aggregated: the layers' outputs and every weight gradient are exact zeros
        assert torch.count_nonzero(out[:, widths[0]:]) == 0 and all(torch.count_nonzero(w.grad) == 0 for w in Wd)
        assert torch.equal(h0d.grad, R.to(dev)[:, :widths[0]])


# --------------------------------------------------------------------- 3. ops.edge_softmax_bwd
SM_DEGREES = [0, 1, 63, 64, 65, 0, 128, 129, 7000, 2]   # in-degrees of the rows, in row order


def _sm_case(n_rows, dev, seed=8):
    """The first `n_rows` rows of SM_DEGREES as a hand-built graph with shuffled edge ids, its device CSR, the device's
    own softmax of logits spread over +-10 (weights down to ~1e-9) and a standard-normal incoming gradient."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(seed)
    deg = np.asarray(SM_DEGREES[:n_rows])
    dst = np.repeat(np.arange(n_rows), deg)
    e = len(dst)
    dst = dst[rng.permutation(e)].astype(np.int32)
    src = rng.integers(0, n_rows, e).astype(np.int32)
    indptr, _, eid, row_of = ops.csr_from_coo(n_rows, t32(src, dev), t32(dst, dev))
    assert np.array_equal(np.diff(indptr.cpu().numpy()), deg)
    logits = rng.uniform(-10.0, 10.0, e).astype(np.float32)
    a = ops.edge_softmax(indptr, row_of, eid, tf(logits, dev))[0]
    g = rng.standard_normal(e).astype(np.float32)
    return dict(n=n_rows, e=e, deg=deg, dst=dst, indptr=indptr, eid=eid, a=a, g=tf(g, dev))


def _sm_bound_check(n, dst, a, g, gs, what):
    """|gs_e - ref_e| <= gamma_{m+3} (|a_e g_e| + a_e S) + 1e-37 and |sum_row gs| <= gamma_{m+3+L} 2 S, with S = the row's
    sum |a g| and m = ceil(L / 64) + 6: softmax_bwd_kernel gives a lane every 64th position of the row (ceil(L / 64)
    chained fmas), adds the 64 lanes' partials in six shuffle steps, and forms a g - a acc with three more roundings.
    The row sums are zero only as far as the given weights sum to one: sum gs = acc (1 - sum a), and a forward that
    adds L terms leaves |1 - sum a| within gamma_L.  `a`, `g`: the fp32 inputs the device read.  Returns the worst
    element ratio."""
    a64, g64 = np.asarray(a, np.float64).reshape(-1), np.asarray(g, np.float64).reshape(-1)
    gs = np.asarray(gs, np.float64).reshape(-1)
    dst = np.asarray(dst, np.int64)
    ref = orc.edge_softmax_backward(n, dst, a64, g64).reshape(-1) if len(dst) else np.zeros(0)
    L =np.bincount(dst, minlength=n)
    S = np.bincount(dst, weights=np.abs(a64 * g64), minlength=n)
    m = np.ceil(L / 64.0) + 6
    bound = gamma(m + 3)[dst] * (np.abs(a64 * g64) + a64 * S[dst]) + 1e-37
    err = np.abs(gs - ref)
    ratio = float(np.max(err / bound)) if len(err) else 0.0
    print("[s3 gamma] %-44s worst |err| / bound = %.4f" % (what, ratio))
    assert np.all(np.isfinite(gs)) and np.all(err <= bound), (what, ratio)
    rows = np.bincount(dst, weights=gs, minlength=n)
    assert np.all(np.abs(rows) <= gamma(m + 3 + L) * 2 * S + 1e-37), (what, "row sums")
    return ratio


@pytest.mark.parametrize("n_rows", [1, 4, 5, 10])
def test_edge_softmax_bwd_fp64_bound(dev, n_rows):
    """Row lengths 0, 1 and around one and two wavefront passes, a 7,000-edge row, row counts off the 4 rows a workgroup
    takes; both the edge-id-ordered (eid given, shuffled ids) and the CSR-ordered (eid = None) variant."""
    from dgl_kgat_amd import ops
    c = _sm_case(n_rows, dev)
    a, g = c["a"].cpu().numpy(), c["g"].cpu().numpy()
    gs = ops.edge_softmax_bwd(c["indptr"], c["eid"], c["a"], c["g"])
    assert gs.shape == c["a"].shape
    _sm_bound_check(c["n"], c["dst"], a, g, gs.cpu().numpy(), "eid, %d rows" % n_rows)
    assert torch.equal(gs, ops.edge_softmax_bwd(c["indptr"], c["eid"], c["a"], c["g"]))
    perm = c["eid"].cpu().numpy()   # CSR position -> edge id
    gs_csr = ops.edge_softmax_bwd(c["indptr"], None, tf(a[perm], dev), tf(g[perm], dev))
    _sm_bound_check(c["n"], c["dst"][perm], a[perm], g[perm], gs_csr.cpu().numpy(), "CSR order, %d rows" % n_rows)
    # the same row, the same lane-strided order: the two variants agree bit for bit
    assert np.array_equal(gs_csr.cpu().numpy(), gs.cpu().numpy()[perm])


@pytest.mark.parametrize("csr_order", [False, True])
@pytest.mark.parametrize("lo,cnt", [(0, 3), (3, 1), (4, 5), (8, 2), (10, 0)])
def test_edge_softmax_bwd_row_range(dev, lo, cnt, csr_order):
    """row_range=(first row, count): the rows in range get the full call's bits, every other position stays zero."""
    from dgl_kgat_amd import ops
    c = _sm_case(10, dev)
    a, g, eid, dst = c["a"], c["g"], c["eid"], c["dst"]
    if csr_order:
        perm = eid.cpu().numpy()
        a, g, eid, dst = tf(a.cpu().numpy()[perm], dev), tf(g.cpu().numpy()[perm], dev), None, dst[perm]
    full = ops.edge_softmax_bwd(c["indptr"], eid, a, g).cpu().numpy()
    part = ops.edge_softmax_bwd(c["indptr"], eid, a, g, row_range=(lo, cnt)).cpu().numpy()
    inside = (dst >= lo) & (dst < lo + cnt)
    assert inside.sum() == sum(SM_DEGREES[lo:lo + cnt])
    assert np.array_equal(part[inside], full[inside])
    assert np.all(part[~inside] == 0)


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("name", ["hub_both", "self_loops_and_parallel"])
def test_edge_softmax_autograd_fp64_bound(dev, graphs, name, flat):
    """Through autograd.edge_softmax with (E,1) and (E,) logits; the reference takes the device's own weights."""
    from dgl_kgat_amd.autograd import edge_softmax
    G = graphs(name)
    rng = np.random.default_rng(31 + flat)
    shape = (G.e,) if flat else (G.e, 1)
    s = tf(rng.uniform(-10.0, 10.0, G.e), dev).reshape(shape).requires_grad_(True)
    ga = rng.standard_normal(G.e).astype(np.float32)
    a = edge_softmax(G.g, s)
    assert a.shape == shape
    a.backward(tf(ga, dev).reshape(shape))
    assert s.grad.shape == shape
    _sm_bound_check(G.n, G.dst, a.detach().cpu().numpy(), ga, s.grad.cpu().numpy(),
                    "autograd %s %s" % (name, "(E,)" if flat else "(E,1)"))


# ----------------------------------------------------------------------------- 4. ops.sddmm_dot
def _sddmm_bound_check(src, dst, X, G, got, what):
    """|got - ref| <= gamma_k sum_d |x_d g_d| with k = ceil(D / 16) + 4: sddmm_dot_kernel gives each of an edge's 16
    lanes every 16th column (ceil(D / 16) chained fmas) and adds the lanes in four shuffle steps."""
    D = X.shape[1]
    ref = orc.sddmm_dot(src, dst, X, G)
    A = orc.sddmm_dot(src, dst, np.abs(X), np.abs(G))
    bound = gamma(math.ceil(D / 16) + 4) * A
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - ref)
    nz = bound > 0
    ratio = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    print("[s4 gamma] %-44s worst |err| / bound = %.4f" % (what, ratio))
    assert np.all(err <= bound), (what, ratio)
    return ratio


@pytest.mark.parametrize("E", [0, 1, 15, 16, 17, 5000])
@pytest.mark.parametrize("D", [1, 3, 8, 16, 20, 64, 100, 128, 176, 256])
def test_sddmm_dot_fp64_bound_and_exact_cases(dev, D, E):
    """Edge counts around the 16 edges a workgroup takes, widths off the 16-lane stride, self-loops and repeated pairs."""
    from dgl_kgat_amd import ops
    n = 300
    rng = np.random.default_rng(400 + D + E)
    src, dst = rng.integers(0, n, E).astype(np.int32), rng.integers(0, n, E).astype(np.int32)
    dst[:3] = src[:3]                                      # self-loops
    src[3:12:2], dst[3:12:2] = src[3:4], dst[3:4]          # one pair repeated
    X = rng.standard_normal((n, D)).astype(np.float32)
    Gm = rng.standard_normal((n, D)).astype(np.float32)
    if E:
        X[src[-1]] = 0.0                                   # an edge whose X row is zero
    sd, dd, Xd, Gd = t32(src, dev), t32(dst, dev), tf(X, dev), tf(Gm, dev)
    got = ops.sddmm_dot(sd, dd, Xd, Gd)
    assert got.shape == (E,)
    assert torch.equal(got, ops.sddmm_dot(sd, dd, Xd, Gd))
    got = got.cpu().numpy()
    _sddmm_bound_check(src, dst, X, Gm, got, "D=%d E=%d" % (D, E))
    if E:
        assert np.all(got[src == src[-1]] == 0)
    ones = torch.ones((n, D), device=dev)
    assert np.all(ops.sddmm_dot(sd, dd, ones, ones).cpu().numpy() == float(D))


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("D", [20, 64])
def test_sddmm_through_u_mul_e_sum_weight_gradient(dev, graphs, D, flat):
    """w requires grad, (E,1) and (E,): w.grad has w's shape and meets the SDDMM's bound."""
    from dgl_kgat_amd.autograd import u_mul_e_sum
    G = graphs("hub_both")
    rng = np.random.default_rng(500 + D + flat)
    X, xd = _features(rng, G.n, D, dev)
    go, god = _features(rng, G.n, D, dev)
    shape = (G.e,) if flat else (G.e, 1)
    w = tf(rng.random(G.e), dev).reshape(shape).requires_grad_(True)
    u_mul_e_sum(G.g, xd, w).backward(god)
    assert w.grad.shape == shape
    _sddmm_bound_check(G.src, G.dst, X, go, w.grad.cpu().numpy(), "u_mul_e_sum w.grad D=%d %s" % (D, shape))
