"""The fused graph attention (kgat_gat_fwd_f32 / kgat_gat_bwd_f32, autograd.gat_aggregate, GATConv) on the MI355X,
against the torch restatement of tests/_gat_ref.py on the adversarial graph: two inputs whose result is exact (bit
equality), fp64 accuracy of the forward and of the three gradients, reproducibility, the forward's memory, the layer.

Bars of the accuracy tests: max|x - ref64| / max|ref64| <= max(10 x the same error of the restatement run in fp32 on the
CPU, 2^-22) - the project's bar for a kernel against CPU fp32 (DESIGN sections 4 and 15); 2^-22 is two ulps of the
tensor's scale, below which fp32 storage alone decides."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _gat_ref  # noqa: E402
from _gat_ref import E, HUB_DST, N, N_HUB_DST, N_HUB_SRC  # noqa: E402

pytestmark = pytest.mark.gpu

FAST = [(4, 16), (8, 4), (1, 64), (8, 16)]
SHAPES = FAST + [(3, 5)]          # (3, 5): the torch restatement inside gat_aggregate
FLOOR = 2.0 ** -22
SEED = 77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graph(dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    src, dst = _gat_ref.adversarial_graph()
    g = K.DGLGraph()
    g.add_nodes(N)
    g.add_edges(src, dst)
    g.readonly()
    csr = g._st.csr(dev)
    assert not np.array_equal(csr.eid.cpu().numpy(), np.arange(E))      # edge id differs from CSR position
    for H, F in FAST:
        te = ops._lib.load().kgat_spmm_tile_edges(E, H * F)
        assert te > 0 and N_HUB_DST >= 10 * te and N_HUB_SRC >= 10 * te    # both hubs span >= 10 tiles at every width
    return dict(g=g, src=src, dst=dst, deg=np.bincount(dst, minlength=N))


def _run(graph, dev, ft, el, er, p=0.0, g_out=None):
    """out (and the three gradients when g_out is given) of autograd.gat_aggregate, as numpy."""
    from dgl_kgat_amd import autograd
    t = [torch.as_tensor(x, device=dev).requires_grad_(g_out is not None) for x in (ft, el, er)]
    out = autograd.gat_aggregate(graph["g"], t[0], t[1], t[2], 0.2, p, SEED)
    if g_out is None:
        return out.detach().cpu().numpy()
    out.backward(torch.as_tensor(g_out, device=dev))
    return [out.detach().cpu().numpy()] + [x.grad.cpu().numpy() for x in t]


@pytest.mark.parametrize("H,F", SHAPES)
def test_exact_uniform_attention(dev, graph, H, F):
    """el constant per head: every p = exp(0) = 1, l = deg, integer sums: out = fp32(sum) / fp32(deg), bit for bit."""
    rng = np.random.default_rng(100 + H * F)
    ft = rng.integers(-8, 9, (N, H, F)).astype(np.float32)
    el = np.broadcast_to((0.75 * np.arange(H) - 1.0).astype(np.float32), (N, H)).copy()
    er = rng.standard_normal((N, H)).astype(np.float32)
    total = np.zeros((N, H, F), np.int64)
    np.add.at(total, graph["dst"], ft[graph["src"]].astype(np.int64))
    assert np.abs(total).max() < 2 ** 24
    deg = graph["deg"]
    want = np.zeros((N, H, F), np.float32)
    nz = deg > 0
    want[nz] = total[nz].astype(np.float32) / deg[nz].astype(np.float32)[:, None, None]
    got = _run(graph, dev, ft, el, er)
    assert got.dtype == np.float32 and np.array_equal(got, want), "%d elements differ" % (got != want).sum()
    assert (got[~nz] == 0).all() and (~nz).sum() == N // 20


@pytest.mark.parametrize("H,F", SHAPES)
def test_exact_dominant_source(dev, graph, H, F):
    """el = 600 x a permutation per head, er = 0: the competing logits lie >= 120 below the row's largest after the
    slope and fp32 exp of that is exactly 0, so out is ft of the row's largest-el source (k parallel edges: k x / k).
    Without the subtraction of the row maximum exp(600 ...) overflows."""
    rng = np.random.default_rng(200 + H * F)
    ft = rng.integers(-8, 9, (N, H, F)).astype(np.float32)
    rank = np.stack([rng.permutation(N) for _ in range(H)], 1)             # (N, H)
    el = (600.0 * rank).astype(np.float32)
    er = np.zeros((N, H), np.float32)
    assert np.exp(np.float32(-120.0)) == 0
    best = np.full((N, H), -1, np.int64)
    np.maximum.at(best, graph["dst"], rank[graph["src"]])
    inv = np.empty((N, H), np.int64)
    for h in range(H):
        inv[rank[:, h], h] = np.arange(N)
    want = np.zeros((N, H, F), np.float32)
    nz = graph["deg"] > 0
    for h in range(H):
        want[nz, h] = ft[inv[best[nz, h], h], h]
    got = _run(graph, dev, ft, el, er)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want), "%d elements differ" % (got != want).sum()


_REF = {}


def _reference(graph, H, F, p):
    """Inputs, the fp64 restatement's (out, g_ft, g_el, g_er) and the CPU-fp32 restatement's errors; computed once."""
    key = (H, F, p)
    if key not in _REF:
        from dgl_kgat_amd import ops
        rng = np.random.default_rng(300 + H * F)
        ft = rng.standard_normal((N, H, F)).astype(np.float32)
        el = (2.0 * rng.standard_normal((N, H))).astype(np.float32)
        er = (2.0 * rng.standard_normal((N, H))).astype(np.float32)
        g_out = rng.standard_normal((N, H, F)).astype(np.float32)
        keep = torch.as_tensor(ops.dropout_keep_mask(SEED, E, H, p)) if p > 0 else None
        src, dst = torch.as_tensor(graph["src"]), torch.as_tensor(graph["dst"])
        res = {}
        for dt in (torch.float64, torch.float32):
            t = [torch.as_tensor(x).to(dt).requires_grad_(True) for x in (ft, el, er)]
            out = _gat_ref.gat_aggregate(src, dst, N, t[0], t[1], t[2], 0.2, keep, p)
            out.backward(torch.as_tensor(g_out).to(dt))
            res[dt] = [out.detach().numpy()] + [x.grad.numpy() for x in t]
        err32 = [_gat_ref.scale_error(a, b) for a, b in zip(res[torch.float32], res[torch.float64])]
        _REF[key] = (ft, el, er, g_out, res[torch.float64], err32)
    return _REF[key]


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H,F", SHAPES)
def test_accuracy_against_fp64(dev, graph, H, F, p):
    ft, el, er, g_out, ref, err32 = _reference(graph, H, F, p)
    got = _run(graph, dev, ft, el, er, p, g_out)
    if p > 0:
        assert 0.4 < (ref[0] != _reference(graph, H, F, 0.0)[4][0]).mean()      # the mask does something
    bad = []
    for name, x, r, e32 in zip(("out", "g_ft", "g_el", "g_er"), got, ref, err32):
        err, bar = _gat_ref.scale_error(x, r), max(10 * e32, FLOOR)
        print("H=%d F=%d p=%.1f %-4s err %.3e  cpu-fp32 %.3e  bar %.3e  ratio %.3f" % (H, F, p, name, err, e32, bar, err / bar))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, bad


def _bits(x):
    return np.asarray(x).view(np.int32)


@pytest.mark.parametrize("H,F", FAST)
def test_reproducible(dev, graph, H, F):
    """The kernels (not the restatement of other shapes, whose torch scatter adds are unordered): forward and backward
    twice, then from inputs sub-allocated at an offset of 16 bytes - the same bits each time."""
    from dgl_kgat_amd import autograd
    ft, el, er, g_out, _, _ = _reference(graph, H, F, 0.5)
    a = _run(graph, dev, ft, el, er, 0.5, g_out)
    b = _run(graph, dev, ft, el, er, 0.5, g_out)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    t = []
    for x in (ft, el, er, g_out):
        buf = torch.empty(x.size + 8, dtype=torch.float32, device=dev)
        v = buf[4:4 + x.size].view(x.shape)
        v.copy_(torch.as_tensor(x))
        assert v.data_ptr() % 16 == 0 and v.data_ptr() % 256 != 0
        t.append(v)
    ins = [x.requires_grad_(True) for x in t[:3]]
    out = autograd.gat_aggregate(graph["g"], ins[0], ins[1], ins[2], 0.2, 0.5, SEED)
    out.backward(t[3])
    for x, y in zip(a, [out.detach()] + [i.grad for i in ins]):
        assert np.array_equal(_bits(x), _bits(y.cpu().numpy()))


def test_forward_allocates_nothing_edge_sized(dev, graph):
    from dgl_kgat_amd import autograd
    H, F = 8, 4
    ft, el, er, _, _, _ = _reference(graph, H, F, 0.0)
    t = [torch.as_tensor(x, device=dev).requires_grad_(True) for x in (ft, el, er)]
    autograd.gat_aggregate(graph["g"], t[0], t[1], t[2])                 # warm-up: the graph's caches exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = autograd.gat_aggregate(graph["g"], t[0], t[1], t[2])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("forward peak rise %d bytes; E*H*4 = %d" % (rise, E * H * 4))
    assert out.shape == (N, H, F) and rise < E * H * 4


def _layer_reference(conv, graph, feat, g_rst, dt):
    """GATConv restated: F.linear + the restatement, in dtype `dt` on the CPU; (rst, grads by name)."""
    import torch.nn.functional as Fn
    H, F = conv._num_heads, conv._out_feats
    params = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in conv.named_parameters()}
    x = torch.as_tensor(feat).to(dt).requires_grad_(True)
    ft = Fn.linear(x, params["fc.weight"]).view(-1, H, F)
    el, er = (ft * params["attn_l"]).sum(-1), (ft * params["attn_r"]).sum(-1)
    rst = _gat_ref.gat_aggregate(torch.as_tensor(graph["src"]), torch.as_tensor(graph["dst"]), N, ft, el, er, 0.2)
    if conv.res_fc is not None:
        rst = rst + (Fn.linear(x, params["res_fc.weight"]) if "res_fc.weight" in params else x).view(-1, H, F)
    rst = Fn.elu(rst)
    rst.backward(torch.as_tensor(g_rst).to(dt))
    grads = {k: v.grad.numpy() for k, v in params.items()}
    grads["feat"] = x.grad.numpy()
    return rst.detach().numpy(), grads


@pytest.mark.parametrize("residual,d_in", [(False, 24), (True, 24), (True, 64)])
def test_layer_against_fp64(dev, graph, residual, d_in):
    import torch.nn.functional as Fn
    import dgl_kgat_amd as K
    torch.manual_seed(5)
    H, F = 4, 16
    conv = K.GATConv(d_in, F, H, residual=residual, activation=Fn.elu).to(dev)
    assert ("res_fc.weight" in dict(conv.named_parameters())) == (residual and d_in != H * F)
    rng = np.random.default_rng(7)
    feat = rng.standard_normal((N, d_in)).astype(np.float32)
    g_rst = rng.standard_normal((N, H, F)).astype(np.float32)
    ref, ref_g = _layer_reference(conv, graph, feat, g_rst, torch.float64)
    r32, r32_g = _layer_reference(conv, graph, feat, g_rst, torch.float32)
    x = torch.as_tensor(feat, device=dev).requires_grad_(True)
    rst = conv(graph["g"], x)
    assert rst.shape == (N, H, F)
    rst.backward(torch.as_tensor(g_rst, device=dev))
    got_g = {k: v.grad.cpu().numpy() for k, v in conv.named_parameters()}
    got_g["feat"] = x.grad.cpu().numpy()
    assert set(got_g) == set(ref_g) and all(np.abs(v).max() > 0 for v in got_g.values())     # gradients reach every parameter
    bad = []
    for name, a, r, r3 in [("rst", rst.detach().cpu().numpy(), ref, r32)] + [(k, got_g[k], ref_g[k], r32_g[k]) for k in sorted(ref_g)]:
        err, e32 = _gat_ref.scale_error(a, r), _gat_ref.scale_error(r3, r)
        bar = max(10 * e32, FLOOR)
        print("residual=%s d_in=%d %-13s err %.3e  cpu-fp32 %.3e  bar %.3e  ratio %.3f" % (residual, d_in, name, err, e32, bar, err / bar))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, bad


def test_two_layer_stack_trains_and_eval_has_no_dropout(dev, graph):
    import torch.nn.functional as Fn
    import dgl_kgat_amd as K
    torch.manual_seed(9)
    g = graph["g"]
    l1 = K.GATConv(32, 16, 4, feat_drop=0.1, attn_drop=0.2, activation=Fn.elu).to(dev)
    l2 = K.GATConv(64, 8, 2, feat_drop=0.1, attn_drop=0.2, residual=True).to(dev)
    x = torch.randn(N, 32, device=dev)
    y = torch.randn(N, 16, device=dev)

    def model():
        return l2(g, l1(g, x).flatten(1)).flatten(1)

    opt = torch.optim.Adam(list(l1.parameters()) + list(l2.parameters()), lr=5e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ((model() - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    # training mode draws masks; eval mode applies none: the bits of a layer built without dropout
    a, b = l1(g, x, seed=1), l1(g, x, seed=2)
    assert not torch.equal(a, b) and torch.equal(a, l1(g, x, seed=1))
    l1.eval()
    plain = K.GATConv(32, 16, 4, activation=Fn.elu).to(dev)
    plain.load_state_dict(l1.state_dict())
    with torch.no_grad():
        e1, e2 = l1(g, x), l1(g, x, seed=3)
        assert torch.equal(e1, e2) and torch.equal(e1, plain(g, x))


def test_layer_refusals_on_device(dev, graph):
    import dgl_kgat_amd as K
    conv = K.GATConv(8, 4, 4).to(dev)
    x = torch.randn(N, 8, device=dev)
    with pytest.raises(NotImplementedError):
        conv(graph["g"], (x, x))
    g2 = K.DGLGraph()
    g2.add_nodes(N)
    g2.add_edges(graph["src"][:100], graph["dst"][:100])
    g2.partition = object()
    with pytest.raises(K.DGLError):
        conv(g2, x)
