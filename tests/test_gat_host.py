"""Host-side checks of the graph-attention layer (no GPU): the four ABI entries and their argument refusals, the
parameters and state_dict of GATConv, the dgl shim, the CPU refusals, and what the GPU tests' helpers claim: the
restatement, the per-element metric and the rows the planted graph holds."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, autograd, ops  # noqa: E402

import _gat_ref  # noqa: E402

NAMES = ("kgat_gat_supported", "kgat_gat_workspace_bytes", "kgat_gat_fwd_f32", "kgat_gat_bwd_f32")
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "kgat_gat.hip" in _lib.SOURCES
    assert lib.kgat_version() == 16 and _lib.ABI_VERSION == 16
    assert len(_lib.SIGNATURES["kgat_gat_fwd_f32"][1]) == 20 and len(_lib.SIGNATURES["kgat_gat_bwd_f32"][1]) == 28
    for name in ("gat_supported", "gat_forward", "gat_backward"):
        assert callable(getattr(ops, name))
    assert callable(autograd.gat_aggregate)


def test_supported_is_the_width_rule():
    lib = _lib.load()
    for H in range(0, 40):
        for F in range(0, 140):
            want = H > 0 and F > 0 and F % 4 == 0 and H * F in (16, 32, 64, 128)
            assert lib.kgat_gat_supported(H, F) == int(want), (H, F)
    for hf in ((4, 16), (8, 4), (1, 64), (8, 16), (2, 8), (1, 16), (32, 4)):
        assert ops.gat_supported(*hf)
    for hf in ((3, 5), (16, 2), (64, 1), (1, 8), (1, 256), (4, 64), (-4, -4)):
        assert not ops.gat_supported(*hf)


class _Host:
    """16-byte aligned host buffers standing in for device pointers: every refusal below comes before any device work."""

    def __init__(self, nbytes=4096):
        self.raw = (C.c_char * (nbytes + 16))()
        self.p = (C.addressof(self.raw) + 15) // 16 * 16


def _fwd(lib, n=10, e=20, H=4, F=16, slope=0.2, p=0.0, ptr=None, ws=None, ws_bytes=None, **over):
    b = ptr
    a = dict(indptr=b, col=b, row_of=b, eid=b, ft=b, el=b, er=b, out=b, m=b, l=b)
    a.update(over)
    if ws_bytes is None:
        ws_bytes = lib.kgat_gat_workspace_bytes(n, e, H, F, 0)
    return lib.kgat_gat_fwd_f32(n, e, H, F, a["indptr"], a["col"], a["row_of"], a["eid"], a["ft"], a["el"], a["er"], slope, p,
                                0, a["out"], a["m"], a["l"], ws, ws_bytes, None)


def _bwd(lib, n=10, e=20, H=4, F=16, slope=0.2, p=0.0, ptr=None, ws=None, ws_bytes=None, **over):
    b = ptr
    names = ("indptr col row_of eid rev_indptr rev_col rev_row_of rev_eid ft el er m l out g_out g_ft g_el g_er").split()
    a = {k: b for k in names}
    a.update(over)
    if ws_bytes is None:
        ws_bytes = lib.kgat_gat_workspace_bytes(n, e, H, F, 1)
    return lib.kgat_gat_bwd_f32(n, e, H, F, *[a[k] for k in names[:15]], slope, p, 0, a["g_ft"], a["g_el"], a["g_er"], ws,
                                ws_bytes, None)


@pytest.mark.parametrize("call, what", [(_fwd, b"gat_fwd"), (_bwd, b"gat_bwd")])
def test_entries_refuse_bad_arguments_without_gpu(call, what):
    lib = _lib.load()
    host = _Host()
    ok = dict(ptr=host.p, ws=host.p)

    def refused(code, **kw):
        args = dict(ok)
        args.update(kw)
        assert call(lib, **args) == code, kw
        assert what in lib.kgat_last_error(), lib.kgat_last_error()

    refused(BADARG, n=-1)
    refused(BADARG, e=-1)
    refused(BADARG, n=2 ** 31)
    refused(BADARG, H=0)
    refused(BADARG, F=-4)
    refused(UNSUPPORTED, H=3, F=5)
    refused(UNSUPPORTED, H=16, F=2)
    refused(UNSUPPORTED, H=4, F=64)
    refused(BADARG, slope=-0.1)
    refused(BADARG, slope=1.5)
    refused(BADARG, p=1.0)
    refused(BADARG, p=-0.5)
    refused(BADARG, p=0.5, eid=None)                 # the mask is keyed by edge id
    refused(BADARG, e=2 ** 31 - 2, H=4)              # e * H beyond the hash's 32-bit index
    refused(BADARG, ptr=None)                        # null pointers
    refused(BADARG, ft=None)
    refused(BADARG, col=None)
    refused(BADARG, ft=host.p + 4)                   # alignment
    refused(BADARG, ws=host.p + 4)
    refused(WORKSPACE, ws=None)
    refused(WORKSPACE, ws_bytes=lib.kgat_gat_workspace_bytes(10, 20, 4, 16, call is _bwd) - 1)
    if call is _bwd:
        refused(BADARG, g_out=None)
        refused(BADARG, rev_col=None)
        refused(BADARG, p=0.5, rev_eid=None)
        refused(BADARG, g_ft=host.p + 8)


def test_workspace_sizes():
    lib = _lib.load()
    n, e = 159251, 3663302
    for H, F in ((1, 64), (4, 16), (8, 16), (8, 4)):
        te = lib.kgat_spmm_tile_edges(e, H * F)
        tiles = -(-e // te)
        fwd, bwd = lib.kgat_gat_workspace_bytes(n, e, H, F, 0), lib.kgat_gat_workspace_bytes(n, e, H, F, 1)
        # two slots per tile of five floats per lane (the row partial and the head scalar), H F / 4 lanes
        assert fwd >= tiles * 2 * (H * F // 4) * 20 and bwd >= tiles * 2 * (H * F // 4) * 20 + n * H * 16
        assert fwd < e * 4                             # less than one fp32 per edge: tile partials only
    assert lib.kgat_gat_workspace_bytes(10, 20, 3, 5, 0) == 256 and lib.kgat_gat_workspace_bytes(-1, 20, 4, 16, 0) == 256


def test_gatconv_parameters_and_state_dict():
    torch.manual_seed(3)
    conv = K.GATConv(20, 16, 4, feat_drop=0.1, attn_drop=0.2)
    assert sorted(conv.state_dict()) == ["attn_l", "attn_r", "fc.weight"]
    assert conv.fc.weight.shape == (64, 20) and conv.attn_l.shape == (1, 4, 16) and conv.attn_r.shape == (1, 4, 16)
    assert conv.fc.bias is None and conv.res_fc is None
    assert conv.feat_drop.p == 0.1 and conv.attn_drop.p == 0.2 and conv.leaky_relu.negative_slope == 0.2
    res = K.GATConv(20, 16, 4, residual=True)
    assert sorted(res.state_dict()) == ["attn_l", "attn_r", "fc.weight", "res_fc.weight"]
    assert res.res_fc.weight.shape == (64, 20) and res.res_fc.bias is None
    same = K.GATConv(64, 16, 4, residual=True)          # equal widths: the identity, no parameter
    assert sorted(same.state_dict()) == ["attn_l", "attn_r", "fc.weight"]
    x = torch.randn(3, 64)
    assert same.res_fc(x) is x
    # xavier-normal with the gain of relu: std = gain * sqrt(2 / (fan_in + fan_out))
    big = K.GATConv(256, 64, 8)
    std = float(big.fc.weight.detach().std())
    want = torch.nn.init.calculate_gain("relu") * (2.0 / (256 + 512)) ** 0.5
    assert abs(std / want - 1) < 0.05
    assert float(big.fc.weight.detach().abs().max()) > 2.5 * want      # normal, not uniform (bound: 1.73 std)
    # round trip, and a foreign state_dict of the same layout loads strictly
    other = K.GATConv(20, 16, 4, residual=True)
    other.load_state_dict(res.state_dict(), strict=True)
    for k, v in res.state_dict().items():
        assert torch.equal(other.state_dict()[k], v)
    foreign = {"fc.weight": torch.randn(64, 20), "attn_l": torch.randn(1, 4, 16), "attn_r": torch.randn(1, 4, 16)}
    conv.load_state_dict(foreign, strict=True)
    assert torch.equal(conv.attn_r.detach(), foreign["attn_r"])
    with pytest.raises(NotImplementedError):
        K.GATConv((8, 8), 4, 2)
    with pytest.raises(ValueError):
        K.GATConv(8, 4, 2, negative_slope=-1.0)


def test_install_as_dgl_exposes_gatconv():
    K.install_as_dgl(force=True)
    from dgl.nn.pytorch.conv import GATConv, SAGEConv
    assert GATConv is K.GATConv and SAGEConv is K.SAGEConv
    assert "GATConv" in K.__all__
    with pytest.raises(NotImplementedError):          # the propagation model keeps refusing it
        K.KGATPropagation(10, 2, 8, 8, 2, 8, gnn_model="gat")


def _ring(n=5):
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(list(range(n)), [(i + 1) % n for i in range(n)])
    return g


def test_cpu_tensors_and_other_refusals():
    g = _ring()
    conv = K.GATConv(8, 4, 4)
    with pytest.raises(K.KGATLibraryError):           # no CPU fallback, supported shape
        conv(g, torch.randn(5, 8))
    with pytest.raises(K.KGATLibraryError):           # ... nor for the shapes the torch restatement serves
        K.GATConv(8, 5, 3)(g, torch.randn(5, 8))
    with pytest.raises(K.KGATLibraryError):
        autograd.gat_aggregate(g, torch.randn(5, 4, 4), torch.randn(5, 4), torch.randn(5, 4))
    with pytest.raises(NotImplementedError):
        conv(g, (torch.randn(5, 8), torch.randn(5, 8)))
    with pytest.raises(ValueError):
        conv(g, torch.randn(4, 8))
    with pytest.raises(ValueError):
        autograd.gat_aggregate(g, torch.randn(5, 4, 4), torch.randn(5, 3), torch.randn(5, 4))
    with pytest.raises(ValueError):
        autograd.gat_aggregate(g, torch.randn(5, 16), torch.randn(5, 4), torch.randn(5, 4))
    g.partition = object()
    with pytest.raises(K.DGLError):
        conv(g, torch.randn(5, 8))
    with pytest.raises(K.DGLError):
        autograd.gat_aggregate(g, torch.randn(5, 4, 4), torch.randn(5, 4), torch.randn(5, 4))
    # the (E, H) refusal of edge_softmax stays
    with pytest.raises(NotImplementedError):
        K.edge_softmax(_ring(), torch.randn(5, 4))


@pytest.mark.parametrize("hf, te", [(16, 256), (32, 256), (64, 256), (128, 128)])
def test_planted_graph_holds_every_finish_case(hf, te):
    """What tests/test_gpu_gat_shapes.py relies on: from indptr and the tile size alone, the (tile, slot) that owns each
    row and the number of tiles its chain runs on, as gat_finish_kernel derives them."""
    deg = _gat_ref.planted_degrees(te)
    src, dst = _gat_ref.graph_from_degrees(deg, 3)
    n, e = len(deg), int(deg.sum())
    assert _lib.load().kgat_spmm_tile_edges(e, hf) == te                  # the tile the call takes is the one assumed
    assert len(src) == e and np.array_equal(np.bincount(dst, minlength=n), deg) and src.min() >= 0 and src.max() < n
    assert not np.array_equal(dst, np.sort(dst))                          # edge ids are shuffled
    assert deg[0] == 0 and deg[-1] == 0 and (deg[1:-1] == 0).sum() >= 6
    indptr = np.concatenate([[0], np.cumsum(deg)])
    owners = _gat_ref.row_owners(indptr, te)
    for slot in (0, 1):
        have = {k for (_, s, k) in owners.values() if s == slot}
        assert have >= set(_gat_ref.CHAINS) | {0}, (slot, have)
    ends = indptr[1:][deg > 0]
    assert deg[1] == te and indptr[1] == 0                                # a row that is exactly tile 0
    assert any(deg[i] == deg[i + 1] == te // 2 and indptr[i] % te == 0 for i in range(n - 1))
    single = np.nonzero(deg == 1)[0]
    assert any(indptr[r] % te == 0 and deg[r - 1] == 1 for r in single)   # single-edge rows on both sides of a tile edge
    assert any(k >= _gat_ref.LONG_CHAIN and indptr[r + 1] % te == 0 for r, (_, s, k) in owners.items())
    assert any(k == 2 and indptr[r] % te == 0 and indptr[r + 1] % te == 0 for r, (_, s, k) in owners.items())
    assert (ends % te == 0).sum() >= 5
    assert e % te == 1 and deg[-2] == 1                                   # the last tile holds one edge, a row of its own
    # a wavefront of the finish holds 64 / LPR consecutive (tile, slot) items: one of them has a short and a long chain
    spw = 64 // (hf // 4)
    items = {2 * b + s: k for (b, s, k) in owners.values() if s >= 0}
    mixed = [w for w in range(0, 2 * -(-e // te), spw)
             if any(items.get(i, -1) >= _gat_ref.LONG_CHAIN for i in range(w, w + spw))
             and any(0 <= items.get(i, -1) < _gat_ref.LONG_CHAIN for i in range(w, w + spw))]
    assert mixed, "no wavefront with a short and a long chain"
    if spw > 2:                                                           # (two items are one tile: its first row ends inside it)
        assert any(any(1 <= items.get(i, -1) < _gat_ref.LONG_CHAIN for i in range(w, w + spw)) for w in mixed)


def test_per_element_metric():
    """term_scales against a loop over the edges, and scaled_error's two halves."""
    rng = np.random.default_rng(4)
    n, e, H, F, slope, p = 7, 30, 2, 3, 0.2, 0.5
    src, dst = rng.integers(0, n - 1, e), rng.integers(1, n, e)          # node 6 has no out-edges, node 0 no in-edges
    ft, el, er, g = (rng.standard_normal(s) for s in ((n, H, F), (n, H), (n, H), (n, H, F)))
    keep = rng.random((e, H)) < 0.5
    t = [torch.as_tensor(x) for x in (ft, el, er, g)]
    S = [x.numpy() for x in _gat_ref.term_scales(torch.as_tensor(src), torch.as_tensor(dst), n, *t, slope, torch.as_tensor(keep), p)]
    out = _gat_ref.gat_aggregate(torch.as_tensor(src), torch.as_tensor(dst), n, *t[:3], slope, torch.as_tensor(keep), p).numpy()
    want = [np.zeros((n, H, F)), np.zeros((n, H, F)), np.zeros((n, H)), np.zeros((n, H))]
    for h in range(H):
        z = el[src, h] + er[dst, h]
        s = np.where(z > 0, z, slope * z)
        for i in range(e):
            u, v = src[i], dst[i]
            a = np.exp(s[i]) / np.exp(s[dst == v]).sum()
            c = keep[i, h] / (1 - p)
            want[0][v, h] += c * a * np.abs(ft[u, h])
            want[1][u, h] += c * a * np.abs(g[v, h])
            t_ = a * (c * np.abs(g[v, h] * ft[u, h]).sum() + np.abs(g[v, h] * out[v, h]).sum()) * (1.0 if z[i] > 0 else slope)
            want[2][u, h] += t_
            want[3][v, h] += t_
    for a, b in zip(S, want):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    assert (S[0][0] == 0).all() and (S[3][0] == 0).all() and (S[1][6] == 0).all() and (S[2][6] == 0).all()
    assert _gat_ref.scaled_error([1.0, 0.0, 2.5], [1.0, 0.0, 2.0], [4.0, 0.0, 2.0]) == 0.25
    assert _gat_ref.scaled_error([0.0], [0.0], [0.0]) == 0.0
    with pytest.raises(AssertionError):
        _gat_ref.scaled_error([1.0, 1e-30], [1.0, 0.0], [1.0, 0.0])      # a value where no term exists


def test_restatement_is_the_per_node_softmax():
    """The reference of the GPU tests against a loop over destinations, in fp64, with and without a mask."""
    rng = np.random.default_rng(2)
    n, e, H, F = 9, 40, 3, 5
    src, dst = rng.integers(0, n, e), rng.integers(0, n - 1, e)       # node 8 has no in-edges
    ft, el, er = (torch.as_tensor(rng.standard_normal(s)) for s in ((n, H, F), (n, H), (n, H)))
    keep = torch.as_tensor(rng.random((e, H)) < 0.5)
    for mask in (None, keep):
        got = _gat_ref.gat_aggregate(torch.as_tensor(src), torch.as_tensor(dst), n, ft, el, er, 0.2, mask, 0.5)
        want = torch.zeros_like(ft)
        for v in range(n):
            ids = np.nonzero(dst == v)[0]
            if len(ids) == 0:
                continue
            a = torch.softmax(torch.nn.functional.leaky_relu(el[src[ids]] + er[v], 0.2), 0)     # (deg, H)
            if mask is not None:
                a = a * mask[ids].double() / 0.5
            want[v] = (a.unsqueeze(-1) * ft[src[ids]]).sum(0)
        assert (want[8] == 0).all() and torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    src, dst = _gat_ref.adversarial_graph()
    deg, odeg = np.bincount(dst, minlength=_gat_ref.N), np.bincount(src, minlength=_gat_ref.N)
    assert deg.max() == deg[_gat_ref.HUB_DST] and odeg.max() == odeg[_gat_ref.HUB_SRC] >= 4000
    pairs = src * _gat_ref.N + dst
    assert len(pairs) - len(np.unique(pairs)) >= 500
    assert _gat_ref.scale_error([1.0, 2.0, 4.5], [1.0, 2.0, 4.0]) == 0.125
