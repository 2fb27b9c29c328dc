"""Laplacian edge weights (use_attention=False, adj_type "si" / "bi") and node dropout on the MI355X: the two streaming
kernels (kgat_edge_norm_f32, kgat_edge_dropout_f32) at the sizes where an elementwise kernel goes wrong (tails, vector
alignment, zero-size launches, the choice of degree array), ``DGLGraph.laplacian_weights``, node dropout through the
fused training unit and the per-layer fallback, what must stay inert, the no-attention model, and two end-to-end
training runs.  References are numpy restatements inside this file:
    si   w[e] = 1 / indeg(dst[e])                       bi   w[e] = 1 / sqrt(outdeg(src[e]) * indeg(dst[e]))
    node dropout   w'[e] = keep[e] ? w[e] * (1.f / (1.f - p)) : 0,   keep = ops.edge_keep_mask(seed, E, p)
Draw order of a ``KGATPropagation.gnn`` call from torch's CPU generator (what test 4 repeats after the same
``torch.manual_seed``): the message-dropout seed first - one ``torch.empty((), dtype=torch.int64).random_()``, drawn
only by the fused training unit and only when the layers' dropout is > 0 - then the node-dropout seed, one more such
draw; with ``dropout=0`` the node-dropout seed is the first draw after ``manual_seed``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
SIZES = (0, 1, 3, 255, 256, 257, 1023, 1025, 4099)
NODES = (1, 7, 300)
RES_TYPES = ("Bi", "GCN", "GraphSage", "Bi2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _np(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().reshape(-1)


def _scale_err(x, y):
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y)) / max(np.abs(y).max(), 1e-30)) if y.size else 0.0


def _random_edges(n, e, rng):
    """Random endpoints; with n >= 7 node n - 1 has no in-edge and node n - 2 no out-edge."""
    if n < 7:
        return rng.integers(0, n, e), rng.integers(0, n, e)
    dst = rng.integers(0, n - 1, e)
    src = rng.integers(0, n - 1, e)
    src[src == n - 2] = n - 1
    return src, dst


def _hub_edges(rng):
    """N = 500: destination 7 with in-degree 3,000 and source 9 with out-degree 3,000 (both cross the aggregation's
    1,024-position tiles), 2,000 ordinary edges; node 499 has no in-edge, node 498 no out-edge."""
    n = 500
    src, dst = _random_edges(n, 8000, rng)
    dst[dst == 7] = 8
    src[src == 9] = 10
    dst[:3000] = 7
    src[3000:6000] = 9
    assert (dst == 7).sum() == 3000 and (src == 9).sum() == 3000
    return n, src, dst


def _loops_edges():
    """Self-loops and duplicate edges (each occurrence counts in the degrees); nodes 5, 6 isolated."""
    src = np.array([0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 0, 0])
    dst = np.array([0, 0, 1, 1, 1, 0, 0, 2, 3, 0, 3, 1, 1])
    return 7, src, dst


def _graph(n, src, dst):
    import dgl_kgat_amd as K
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    g.readonly()
    return g


def _cases():
    rng = np.random.default_rng(20240611)
    cases = [("N%d-E%d" % (n, e), n) + _random_edges(n, e, rng) for n in NODES for e in SIZES]
    cases.append(("hub",) + _hub_edges(rng))
    cases.append(("loops",) + _loops_edges())
    return cases


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _laplacian64(n, src, dst, mode):
    """The weights in edge-id order, fp64, degrees by np.bincount."""
    indeg = np.bincount(dst, minlength=n).astype(np.float64)
    outdeg = np.bincount(src, minlength=n).astype(np.float64)
    if mode == "si":
        return 1.0 / indeg[dst]
    return 1.0 / np.sqrt(outdeg[src] * indeg[dst])


# ---------------------------------------------------------------- 1. kgat_edge_norm_f32

@pytest.mark.parametrize("mode", ["si", "bi"])
def test_edge_norm_against_fp64(dev, cases, mode):
    from dgl_kgat_amd import ops
    for tag, n, src, dst in cases:
        g = _graph(n, src, dst)
        st = g._st
        csr, rev = st.csr(dev), st.csr_rev(dev)
        w_csr, w_eid = ops.edge_norm(csr, rev.indptr if mode == "bi" else None, mode)
        torch.cuda.synchronize()
        e = len(src)
        assert tuple(w_csr.shape) == tuple(w_eid.shape) == (e,), tag
        if e == 0:
            continue
        ref = _laplacian64(n, src, dst, mode)
        eid = csr.eid.cpu().numpy()
        got_eid, got_csr = _np(w_eid), _np(w_csr)
        assert np.all(np.isfinite(got_eid)) and np.all(got_eid > 0), tag
        rel_eid = float(np.max(np.abs(got_eid - ref) / ref))
        rel_csr = float(np.max(np.abs(got_csr - ref[eid]) / ref[eid]))
        assert rel_eid <= 8 * EPS24 and rel_csr <= 8 * EPS24, (tag, mode, rel_eid, rel_csr)
        assert np.array_equal(_bits(w_eid)[eid], _bits(w_csr)), (tag, mode)
        # without the edge-id-ordered output: the same CSR stream
        only_csr, none = ops.edge_norm(csr, rev.indptr if mode == "bi" else None, mode, want_eid=False)
        assert none is None and torch.equal(only_csr, w_csr), tag
        if mode == "si":
            indeg = np.bincount(dst, minlength=n)
            sums = np.bincount(dst, weights=got_eid, minlength=n)
            has = indeg > 0
            assert np.all(np.abs(sums[has] - 1.0) <= indeg[has] * 2.0 ** -23), tag


def test_edge_norm_wrong_degree_array_misses_the_bar(cases):
    """The bar separates the two degree arrays: in-degrees in the place of out-degrees miss it by orders of magnitude."""
    tag, n, src, dst = [c for c in cases if c[0] == "hub"][0]
    ref = _laplacian64(n, src, dst, "bi")
    indeg = np.bincount(dst, minlength=n).astype(np.float64)
    with np.errstate(divide="ignore"):
        wrong = 1.0 / np.sqrt(indeg[src] * indeg[dst])
    assert np.max(np.abs(wrong - ref) / ref) > 1e5 * 8 * EPS24


# ---------------------------------------------------------------- 2. kgat_edge_dropout_f32

def _dropped32(w, keep, p):
    """keep ? w * keep_scale : 0 in float32 as the kernel writes it: keep_scale = 1.f / (1.f - p), then one product."""
    keep_scale = np.float32(1) / (np.float32(1) - np.float32(p))
    return np.where(keep, np.asarray(w, np.float32) * keep_scale, np.float32(0)).astype(np.float32)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9])
def test_edge_dropout_bits(dev, p):
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(7)
    n = 300
    for e in SIZES:
        src, dst = _random_edges(n, e, rng)
        st = _graph(n, src, dst)._st
        csr, rev = st.csr(dev), st.csr_rev(dev)
        w_np = rng.uniform(0.25, 1.75, e).astype(np.float32)   # in edge-id order; no zero among them
        w_eid = torch.as_tensor(w_np, device=dev)
        eid_f, eid_r = csr.eid.cpu().numpy(), rev.eid.cpu().numpy()
        w_f, w_r = torch.as_tensor(w_np[eid_f], device=dev), torch.as_tensor(w_np[eid_r], device=dev)
        for seed in (0, 1234, 2 ** 63 + 977):
            tag = (e, p, seed)
            keep = ops.edge_keep_mask(seed, e, p)
            out_f = ops.edge_dropout(w_f, csr.eid, p, seed)
            out_r = ops.edge_dropout(w_r, rev.eid, p, seed)
            out_e = ops.edge_dropout(w_eid, None, p, seed)
            torch.cuda.synchronize()
            got = out_f.cpu().numpy()
            assert np.array_equal(got == 0, ~keep[eid_f]), tag
            want = _dropped32(w_np[eid_f], keep[eid_f], p)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), tag
            if p == 0.0:
                assert np.array_equal(_bits(out_f), _bits(w_f)), tag
            # the forward and the reversed stream describe the same surviving edges
            back_f, back_r = np.empty(e, np.int32), np.empty(e, np.int32)
            back_f[eid_f], back_r[eid_r] = _bits(out_f), _bits(out_r)
            assert np.array_equal(back_f, back_r) and np.array_equal(back_f, _bits(out_e)), tag
            # a 4-byte aligned, not 16-byte aligned w_in
            buf = torch.empty(e + 1, dtype=torch.float32, device=dev)
            buf[1:] = w_f
            if e:
                assert buf[1:].data_ptr() % 16 == 4
            assert torch.equal(ops.edge_dropout(buf[1:], csr.eid, p, seed), out_f), tag
            # ... and a key / w_out pair that is not 16-byte aligned either (the all-scalar path)
            kbuf = torch.empty(e + 1, dtype=torch.int32, device=dev)
            kbuf[1:] = csr.eid
            assert torch.equal(ops.edge_dropout(w_f, kbuf[1:], p, seed), out_f), tag
            if e == 4099:
                share = keep.mean()
                assert abs(share - (1 - np.float32(p))) <= 4 * np.sqrt(p * (1 - p) / e), (tag, share)
                assert abs((got != 0).mean() - (1 - np.float32(p))) <= 4 * np.sqrt(p * (1 - p) / e), tag
    # an (E,1) stream keeps its shape
    assert tuple(ops.edge_dropout(w_f.view(-1, 1), csr.eid, 0.5, 3).shape) == (4099, 1)


# ---------------------------------------------------------------- 3. DGLGraph.laplacian_weights

def _aggregate(g, x, w):
    import dgl_kgat_amd as K
    fn = K.function
    g = g.local_var()
    g.ndata["h"] = x
    g.edata["w"] = w
    g.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "h_neighbor"))
    return g.ndata["h_neighbor"]


@pytest.mark.parametrize("adj_type", ["si", "bi"])
def test_laplacian_weights_remembers_the_right_csr_copy(dev, cases, adj_type):
    tag, n, src, dst = [c for c in cases if c[0] == "hub"][0]
    g = _graph(n, src, dst)
    g.ndata["id"] = torch.arange(n, device=dev)
    a = g.laplacian_weights(adj_type)
    assert tuple(a.shape) == (len(src), 1) and a.dtype == torch.float32 and a.device == dev
    ref = _laplacian64(n, src, dst, adj_type)
    assert float(np.max(np.abs(_np(a).reshape(-1) - ref) / ref)) <= 8 * EPS24
    assert g.laplacian_weights(adj_type) is a          # cached per graph, device and adj_type
    plain = a.clone()
    for d in (64, 16):
        x = torch.randn(n, d, device=dev)
        fresh = _graph(n, src, dst)                    # the plain tensor goes through the permutation pass
        want = _aggregate(fresh, x, plain)
        csr_copy = g._st._cache(dev)["w_csr"][1]
        got = _aggregate(g, x, g.laplacian_weights(adj_type))
        assert g._st._cache(dev)["w_csr"][1] is csr_copy, "the remembered CSR copy was replaced by a permutation pass"
        assert torch.equal(got, want), (adj_type, d)
    with pytest.raises(ValueError):
        g.laplacian_weights("xx")


def test_laplacian_weights_after_the_host_edges_are_gone(dev, cases):
    tag, n, src, dst = [c for c in cases if c[0] == "N300-E4099"][0]
    g = _graph(n, src, dst)
    g.ndata["id"] = torch.arange(n, device=dev)
    g._st.csr(dev)                                     # first device use of a read-only graph: the host COO goes
    assert g._st._host is None
    for adj_type in ("si", "bi"):
        ref = _laplacian64(n, src, dst, adj_type)
        got = _np(g.laplacian_weights(adj_type)).reshape(-1)
        assert float(np.max(np.abs(got - ref) / ref)) <= 8 * EPS24, adj_type


def test_laplacian_weights_honours_the_lazy_opt_in(dev, cases):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import lazy
    tag, n, src, dst = [c for c in cases if c[0] == "N300-E4099"][0]
    eager = _graph(n, src, dst)
    want = eager.laplacian_weights("bi").clone()
    x = torch.randn(n, 16, device=dev)
    agg = _aggregate(eager, x, want)
    prev = K.enable_lazy_edge_weights(True)
    try:
        g = _graph(n, src, dst)
        a = g.laplacian_weights("bi")
        assert isinstance(a, lazy.LazyEdgeWeights) and a.pending
        assert torch.equal(_aggregate(g, x, a), agg) and a.pending     # streamed from the CSR copy, still unwritten
        assert g.laplacian_weights("bi") is a
        assert torch.equal(a + 0, want) and not a.pending              # the first look writes the values
        assert torch.equal(_aggregate(g, x, g.laplacian_weights("bi")), agg)
    finally:
        K.enable_lazy_edge_weights(prev)


# ---------------------------------------------------------------- 4. node dropout in the training step

def _model(dev, res_type, dims, seed=11, **kw):
    """dims = (input_node_dim, n_hidden): layer widths input -> n_hidden -> n_hidden / 2 -> n_hidden / 4."""
    import dgl_kgat_amd as K
    torch.manual_seed(seed)
    layers, dropout = kw.pop("layers", 3), kw.pop("dropout", 0.0)
    return K.KGATPropagation(300, 2, input_node_dim=dims[0], relation_dim=dims[0], num_gnn_layers=layers, n_hidden=dims[1],
                             dropout=dropout, res_type=res_type, **kw).to(dev)


@pytest.fixture(scope="module")
def train_case(dev, cases):
    tag, n, src, dst = [c for c in cases if c[0] == "N300-E4099"][0]
    rng = np.random.default_rng(5)
    w = rng.uniform(0.05, 1.0, (len(src), 1)).astype(np.float32)
    return n, src, dst, w


def _train_graph(dev, train_case, w=None):
    n, src, dst, w0 = train_case
    g = _graph(n, src, dst)
    g.ndata["id"] = torch.arange(n, device=dev)
    g.edata["w"] = torch.as_tensor(w0 if w is None else w, device=dev)
    return g


def _step(model, g, R):
    model.zero_grad()
    out = model.gnn(g, g.ndata["id"])
    (out * R).sum().backward()
    return out, [p.grad.clone() if p.grad is not None else None for p in model.parameters()]


def _ab(dev, train_case, res_type, dims, layers=3, p=0.3, s=77):
    """Model A drops edges itself; model B gets the dropped weights, formed here in edge-id order with the seed A drew."""
    from dgl_kgat_amd import ops
    n, src, dst, w = train_case
    A = _model(dev, res_type, dims, layers=layers, node_dropout=p)
    B = _model(dev, res_type, dims, layers=layers)
    B.load_state_dict(A.state_dict())
    A.train()
    B.train()
    widths = sum([dims[0]] + [dims[1] // 2 ** i for i in range(layers)])
    R = torch.randn(n, widths, device=dev)
    torch.manual_seed(s)
    seed = int(torch.empty((), dtype=torch.int64).random_())     # dropout=0: the node-dropout seed is the first draw
    gA = _train_graph(dev, train_case)
    gB = _train_graph(dev, train_case, _dropped32(w, ops.edge_keep_mask(seed, len(src), p).reshape(-1, 1), p))
    torch.manual_seed(s)
    out_a, grads_a = _step(A, gA, R)
    out_b, grads_b = _step(B, gB, R)
    return A, (out_a, grads_a), (out_b, grads_b)


@pytest.mark.parametrize("dims", [(16, 16), (16, 64)], ids=["16-16-8-4", "16-64-32-16"])
@pytest.mark.parametrize("res_type", RES_TYPES)
def test_node_dropout_training_unit_sees_one_edge_set(dev, train_case, res_type, dims):
    """Forward and backward streams of A hold the surviving edges of B's edge-id-ordered weights: the same kernels on
    the same weight bits, so the readout and every gradient are bitwise equal.  (Widths 16 -> 16 -> 8 -> 4 are inside
    the dense kernels for Bi only - the other aggregators take their per-layer path there, the same bits are asked
    of it; 16 -> 64 -> 32 -> 16 is inside them for every aggregator.)"""
    A, (out_a, grads_a), (out_b, grads_b) = _ab(dev, train_case, res_type, dims)
    if res_type == "Bi" or dims == (16, 64):
        assert type(out_a.grad_fn).__name__.startswith("_GNNTrain")
        assert type(out_b.grad_fn).__name__.startswith("_GNNTrain")
    assert torch.equal(out_a, out_b), res_type
    names = [k for k, _ in A.named_parameters()]
    reached = {"entity_embed.weight"} | {k for k in names if k.startswith("layers.")}
    for k, ga, gb in zip(names, grads_a, grads_b):
        assert (ga is None) == (gb is None), k
        assert (ga is not None) == (k in reached), k
        if ga is not None:
            assert torch.equal(ga, gb), (res_type, k)
    # and the edges were dropped at all: the undropped readout differs
    with torch.no_grad():
        A.eval()
        assert not torch.equal(A.gnn(_train_graph(dev, train_case)), out_a)


@pytest.mark.parametrize("res_type", RES_TYPES)
def test_node_dropout_per_layer_fallback(dev, train_case, res_type):
    """Widths 24 -> 24 are outside the dense kernels: the per-layer path puts the dropped edge-id-ordered weights on its
    local_var graph.  Readout bitwise; gradients within the 1e-5 of tensor scale the aggregator tests ask of that path."""
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.kgat_layer import _layer_dense
    A, (out_a, grads_a), (out_b, grads_b) = _ab(dev, train_case, res_type, (24, 24), layers=1)
    form, _, d_in, d_out = _layer_dense(A.layers[0])
    assert (d_in, d_out) == (24, 24) and not ops.aggregator_supported(form, d_in, d_out)
    assert not type(out_a.grad_fn).__name__.startswith("_GNNTrain")
    assert torch.equal(out_a, out_b), res_type
    for k, ga, gb in zip([k for k, _ in A.named_parameters()], grads_a, grads_b):
        assert (ga is None) == (gb is None), k
        if ga is not None:
            assert _scale_err(_np(ga), _np(gb)) <= 1e-5, (res_type, k)


# ---------------------------------------------------------------- 5. inert and reproducible

def test_node_dropout_is_inert_outside_training(dev, train_case):
    A = _model(dev, "Bi", (16, 64), node_dropout=0.3)
    B = _model(dev, "Bi", (16, 64))
    B.load_state_dict(A.state_dict())
    g = _train_graph(dev, train_case)
    A.eval()
    B.eval()
    with torch.no_grad():
        want = B.gnn(g)
        assert torch.equal(A.gnn(g), want)
    assert torch.equal(A.gnn(g).detach(), B.gnn(g).detach())        # eval() under autograd
    A.train()
    B.train()
    with torch.no_grad():
        assert torch.equal(A.gnn(g), B.gnn(g))                      # train() under no_grad


def test_node_dropout_redraws_and_reproduces(dev, train_case):
    A = _model(dev, "Bi", (16, 64), node_dropout=0.3)
    g = _train_graph(dev, train_case)
    A.train()
    torch.manual_seed(3)
    first = A.gnn(g).detach()
    second = A.gnn(g).detach()
    assert not torch.equal(first, second)
    torch.manual_seed(3)
    assert torch.equal(A.gnn(g).detach(), first)
    assert torch.equal(A.gnn(g).detach(), second)


@pytest.mark.parametrize("res_type", RES_TYPES)
def test_defaults_reproduce_the_model_without_the_keywords(dev, train_case, res_type):
    n = train_case[0]
    old = _model(dev, res_type, (16, 64), dropout=0.2)
    new = _model(dev, res_type, (16, 64), dropout=0.2, use_attention=True, adj_type="bi", node_dropout=0.0)
    new.load_state_dict(old.state_dict())
    R = torch.randn(n, 16 + 64 + 32 + 16, device=dev)
    outs = []
    for m in (old, new):
        m.train()
        torch.manual_seed(21)
        out, grads = _step(m, _train_graph(dev, train_case), R)
        draws_after = int(torch.empty((), dtype=torch.int64).random_())   # both drew the same number of seeds
        outs.append((out, grads, draws_after))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][2] == outs[1][2]
    for ga, gb in zip(outs[0][1], outs[1][1]):
        assert (ga is None) == (gb is None) and (ga is None or torch.equal(ga, gb))


@pytest.mark.parametrize("dims,layers", [((16, 64), 3), ((24, 24), 1)], ids=["unit", "per-layer"])
def test_training_step_keeps_the_cached_undropped_weights(dev, train_case, dims, layers):
    A = _model(dev, "Bi", dims, layers=layers, node_dropout=0.3)
    g = _train_graph(dev, train_case)
    n = train_case[0]
    R = torch.randn(n, sum([dims[0]] + [dims[1] // 2 ** i for i in range(layers)]), device=dev)
    A.eval()
    with torch.no_grad():
        before_eval = A.gnn(g)
    cache = g._st._cache(dev)
    w_csr = cache["w_csr"][1]
    A.train()
    _step(A, g, R)
    w_rev = cache["w_rev"][1]
    assert cache["w_csr"][1] is w_csr
    _step(A, g, R)
    assert cache["w_csr"][1] is w_csr and cache["w_rev"][1] is w_rev
    A.eval()
    with torch.no_grad():
        assert torch.equal(A.gnn(g), before_eval)      # the evaluation after the steps finds its cache warm
    assert cache["w_csr"][1] is w_csr


# ---------------------------------------------------------------- 6. the no-attention model

def _leaky(z):
    return np.where(z >= 0, z, 0.01 * z)


def _normalize(z):
    return z / np.maximum(np.sqrt((z * z).sum(1, keepdims=True)), 1e-12)


@pytest.mark.parametrize("adj_type", ["si", "bi"])
def test_no_attention_model(dev, train_case, adj_type):
    n, src, dst, _ = train_case
    model = _model(dev, "Bi", (16, 64), use_attention=False, adj_type=adj_type)
    g = _graph(n, src, dst)
    g.ndata["id"] = torch.arange(n, device=dev)
    g.edata["type"] = torch.as_tensor(np.arange(len(src)) % 2, device=dev)
    with torch.no_grad():
        a = model.compute_attention(g)
        assert torch.equal(a, g.laplacian_weights(adj_type))
        g.edata["w"] = a
        model.eval()
        assert model._can_fuse_readout()
        out = model.gnn(g)
        # compute_attention_surface is the attention still
        assert tuple(model.compute_attention_surface(g).shape) == (len(src), 1)
    # reference models.py:156-168 in fp64 with those weights
    w = _np(a).reshape(-1)
    h = _np(model.entity_embed.weight)
    blocks = [h]
    for layer in model.layers:
        hn = np.zeros_like(h)
        np.add.at(hn, dst, w[:, None] * h[src])
        h = _leaky((h * hn) @ _np(layer.res_fc_2.weight).T)
        blocks.append(_normalize(h))
    assert _scale_err(_np(out), np.concatenate(blocks, 1)) <= 1e-5, adj_type


def test_node_dropout_refuses_a_partitioned_graph(dev):
    from dgl_kgat_amd.graph import DGLError

    class Sharded:
        partition = object()

    model = _model(dev, "Bi", (16, 64), node_dropout=0.3)
    model.train()
    with pytest.raises(DGLError):
        model.gnn(Sharded())


# ---------------------------------------------------------------- 7. end to end

@pytest.mark.parametrize("flags", [("--use_attention", "0", "--adj_type", "si", "--node_dropout", "0.1"),
                                   ("--use_attention", "1", "--node_dropout", "0.1")], ids=["no-attention", "attention"])
def test_planted_structure_recall_rises_with_node_dropout(dev, flags, tmp_path, capsys):
    """End to end in a child process (the example's global switches stay there): recall@20 on the planted held-out
    interactions leaves a random ranking within three short epochs - the bar of test_planted_structure_recall_rises -
    with node dropout on, without and with the attention."""
    log = tmp_path / "train.json"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_kgat.py"), "--planted", "--epochs", "3", "--lr", "0.03",
           "--batch_size", "512", "--batch_size_kg", "512", "--eval_before", "--seed", "1234", *flags,
           "--log_json", str(log)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(log) as f:
        doc = json.load(f)
    hist = doc["epochs"]
    assert doc["args"]["use_attention"] == int(flags[1]) and doc["args"]["node_dropout"] == 0.1
    assert doc["args"]["adj_type"] == "si"
    rec = [h["test_recall"] for h in hist]
    val = [h["valid_recall"] for h in hist]
    with capsys.disabled():
        print("\n%s planted-structure run: test recall@20 by epoch %s, valid %s" % (
            " ".join(flags), ["%.4f" % x for x in rec], ["%.4f" % x for x in val]))
    assert rec[3] > 3.0 * rec[0] and rec[3] > rec[2] > rec[1]
    assert val[3] > 3.0 * val[0]
