"""Host-side checks of the relational graph convolution (no GPU): the five ABI entries, their shape rule and argument
refusals (scratch one byte short, null pointers - before any device work), RelGraphConv's parameters and state_dict, the
dgl shim, every refusal of the Python layers, the gnn_model="rgcn" stack, and what the GPU tests' helper claims: the
restatement against a triple loop, and the features of the adversarial graph."""
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

import _rgcn_ref  # noqa: E402

NAMES = ("kgat_rgcn_supported", "kgat_rgcn_scratch_bytes", "kgat_rgcn_fwd_f32", "kgat_rgcn_bwd_x_f32",
         "kgat_rgcn_bwd_coef_f32")
ENTRIES = (("kgat_rgcn_fwd_f32", "rgcn_fwd", 0), ("kgat_rgcn_bwd_x_f32", "rgcn_bwd_x", 1),
           ("kgat_rgcn_bwd_coef_f32", "rgcn_bwd_coef", 2))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3

_BUF = C.create_string_buffer((1 << 16) + 16)    # a non-null, 16-byte aligned host address no call gets as far as using
P = (C.addressof(_BUF) + 15) // 16 * 16


def test_restatement_against_a_triple_loop():
    rng = np.random.default_rng(0)
    n, e, R, B, D = 12, 60, 4, 3, 5
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    src[:3], dst[:3] = (2, 2, 7), (2, 9, 9)                   # a self-loop; dst 9 twice
    src[3], dst[3] = src[4], dst[4]                           # a duplicate edge
    et = rng.integers(0, R, e)
    et[5] = R + 1                                             # outside [0, R): contributes nothing
    x, a = rng.standard_normal((n, D)), rng.standard_normal((R, B))
    g_Z, norm = rng.standard_normal((n, B, D)), rng.random(e) + 0.1
    for nm in (norm, None):
        got = _rgcn_ref.restate(n, src, dst, et, nm, x, a, g_Z)
        Z, gx, ga = _rgcn_ref.brute_force(n, src, dst, et, nm, x, a, g_Z)
        for name, want in (("Z", Z), ("g_x", gx), ("g_a", ga)):
            assert got[name].value.shape == want.shape, name
            assert np.abs(got[name].value - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
            assert (got[name].S >= np.abs(got[name].value) - 1e-12).all(), name      # |sum| <= sum of |terms|
        indeg, outdeg = np.bincount(dst[et < R], minlength=n), np.bincount(src[et < R], minlength=n)
        assert np.array_equal(got["Z"].n[:, 0, 0], indeg) and np.array_equal(got["g_x"].n[:, 0], B * outdeg)
        assert np.array_equal(got["g_a"].n[:, 0], D * np.bincount(et[et < R], minlength=R))
        assert got["Z"].bound().shape == Z.shape


def test_adversarial_graph_has_what_it_claims():
    lib = _lib.load()
    tiles = {D: lib.kgat_spmm_tile_edges(_rgcn_ref.N_EDGES, D) for D in (16, 32, 64, 128)}
    assert tiles[64] == 256                                                  # the short-run tile at D = 64
    src, dst, et = _rgcn_ref.adversarial_graph(set(tiles.values()))
    n, e = _rgcn_ref.N_NODES, _rgcn_ref.N_EDGES
    assert len(src) == len(dst) == len(et) == e and (e + tiles[64] - 1) // tiles[64] >= 8
    for rows in (dst, src):                                                  # forward and reversed walk
        deg = np.bincount(rows, minlength=n)
        indptr = np.concatenate([[0], np.cumsum(deg)])
        hub = int(np.argmax(deg))
        for te in set(tiles.values()):
            assert (indptr[hub + 1] - 1) // te - indptr[hub] // te >= 2      # the hub's chain: at least three tiles
            assert any(indptr[v + 1] % te == 0 and deg[v] > 0 and indptr[v + 1] < e for v in range(n))  # a row ends on a tile edge
        assert (deg == 0).sum() >= 10
    assert not np.array_equal(dst, np.sort(dst))                             # edge ids are shuffled
    assert (src == dst).sum() >= 3
    pairs = src * n + dst
    assert np.bincount(pairs).max() >= 3                                     # duplicate edges
    counts = np.bincount(et, minlength=_rgcn_ref.N_REL)
    assert counts[3] == 0 and counts[4] == 1 and counts[:3].min() > 100


def test_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "kgat_rgcn.hip" in _lib.SOURCES
    assert lib.kgat_version() == 16 and _lib.ABI_VERSION == 16
    for name, _, _ in ENTRIES:
        assert len(_lib.SIGNATURES[name][1]) == 16, name
    for name in ("rgcn_supported", "rgcn_forward", "rgcn_backward_x", "rgcn_backward_coef"):
        assert callable(getattr(ops, name))
    assert callable(autograd.rgcn_aggregate)
    # the scratch naming the closed tables of the other host tests rest on
    assert not any(n.endswith("_workspace_bytes") for n in NAMES)
    assert "void* scratch, size_t scratch_bytes" in header


def test_supported_is_the_shape_rule():
    lib = _lib.load()
    for D in (0, 4, 8, 16, 20, 32, 48, 64, 128, 256):
        for B in range(-1, 11):
            for R in (-1, 0, 1, 5, 41, 455, 456, 512, 513, 4096, 4097):
                want = D in (16, 32, 64, 128) and 1 <= B <= 8 and R >= 1 and R * B <= 4096
                assert lib.kgat_rgcn_supported(D, B, R) == int(want), (D, B, R)
    assert not ops.rgcn_supported(20, 4, 41) and not ops.rgcn_supported(64, 0, 41) and not ops.rgcn_supported(64, 9, 41)
    assert ops.rgcn_supported(64, 1, 4096) and not ops.rgcn_supported(64, 1, 4097)       # R * B = 4096 | 4097
    assert ops.rgcn_supported(16, 8, 512) and not ops.rgcn_supported(16, 8, 513)


def _call(lib, name, which, n=300, e=5000, D=64, B=4, R=5, ptr=P, scratch=P, short=0, **over):
    need = lib.kgat_rgcn_scratch_bytes(n, e, D, B, R, which)
    args = dict(n_nodes=n, n_edges=e, D=D, B=B, R=R)
    ptrs = [over.get("p%d" % i, ptr) for i in range(8)]
    rc = getattr(lib, name)(args["n_nodes"], args["n_edges"], D, B, R, *ptrs, scratch, need - short, None)
    return rc, (lib.kgat_last_error() or b"").decode(), need


@pytest.mark.parametrize("name, word, which", ENTRIES)
def test_scratch_one_byte_short_is_refused_before_device_work(name, word, which):
    lib = _lib.load()
    for D, B in ((64, 4), (16, 3), (128, 8)):
        rc, msg, need = _call(lib, name, which, D=D, B=B, short=1)
        assert need > 256 and rc == WORKSPACE, (name, rc, msg)
        assert word + ":" in msg and "scratch too small (%d < %d)" % (need - 1, need) in msg, msg
    rc, msg, _ = _call(lib, name, which, scratch=None)
    assert rc == WORKSPACE and word in msg
    rc, msg, _ = _call(lib, name, which, scratch=P + 4)                       # 16-byte alignment
    assert rc == BADARG and word in msg
    # the forward's partials hold B accumulator sets, the reversed walk's one
    assert lib.kgat_rgcn_scratch_bytes(300, 5000, 64, 8, 5, 0) > lib.kgat_rgcn_scratch_bytes(300, 5000, 64, 1, 5, 0)
    assert lib.kgat_rgcn_scratch_bytes(300, 5000, 64, 8, 5, 1) == lib.kgat_rgcn_scratch_bytes(300, 5000, 64, 1, 5, 1)
    # nothing edge-sized: far below one float per edge and basis at a benchmark-sized call
    assert lib.kgat_rgcn_scratch_bytes(100000, 3000000, 64, 4, 41, 0) < 3000000 * 4
    assert lib.kgat_rgcn_scratch_bytes(10, 20, 20, 4, 5, which) == 256 and lib.kgat_rgcn_scratch_bytes(-1, 20, 64, 4, 5, which) == 256
    assert lib.kgat_rgcn_scratch_bytes(10, 20, 64, 4, 5, 3) == 256


@pytest.mark.parametrize("name, word, which", ENTRIES)
def test_null_pointers_bad_sizes_and_shapes_are_refused(name, word, which):
    lib = _lib.load()
    # pointer positions 0..7: indptr, col, row_of, etype, norm (may be null), then the entry's three tensors
    for i in (0, 1, 2, 3, 5, 6, 7):
        rc, msg, _ = _call(lib, name, which, **{"p%d" % i: None})
        assert rc == BADARG and word in msg and "null" in msg, (name, i, rc, msg)
    rc, msg, _ = _call(lib, name, which, p4=None, short=1)                    # a null norm is an argument, not an error
    assert rc == WORKSPACE, (name, rc, msg)
    for over in (dict(n=-1), dict(e=-1), dict(D=0), dict(B=0), dict(R=0), dict(B=-2)):
        rc, msg, _ = _call(lib, name, which, **over)
        assert rc == BADARG and word in msg, (name, over, rc, msg)
    for over in (dict(D=20), dict(B=9), dict(R=4097, B=1), dict(R=513, B=8)):
        rc, msg, _ = _call(lib, name, which, **over)
        assert rc == UNSUPPORTED and word in msg, (name, over, rc, msg)


def _init_bound(fan_in, fan_out):
    return torch.nn.init.calculate_gain("relu") * (6.0 / (fan_in + fan_out)) ** 0.5


def test_relgraphconv_parameters_and_state_dict():
    torch.manual_seed(5)
    conv = K.RelGraphConv(20, 12, 7, num_bases=3)                                       # B < R
    assert sorted(conv.state_dict()) == ["h_bias", "w_comp", "weight"]
    assert conv.weight.shape == (3, 20, 12) and conv.w_comp.shape == (7, 3) and conv.h_bias.shape == (12,)
    assert float(conv.h_bias.detach().abs().max()) == 0.0
    # xavier-uniform with the gain of relu; torch's fans of a (B, in, out) tensor: fan_in = in * out, fan_out = B * out
    assert float(conv.weight.detach().abs().max()) <= _init_bound(20 * 12, 3 * 12)
    assert float(conv.weight.detach().abs().max()) > 0.8 * _init_bound(20 * 12, 3 * 12)
    assert float(conv.w_comp.detach().abs().max()) <= _init_bound(3, 7)
    full = K.RelGraphConv(20, 12, 7)                                                    # B == R: no w_comp
    assert sorted(full.state_dict()) == ["h_bias", "weight"] and full.weight.shape == (7, 20, 12) and full.num_bases == 7
    assert torch.equal(full.coefficients(), torch.eye(7)) and not full.coefficients().requires_grad
    for nb in (0, -1, 8, 100, None):                                                    # outside 1..R: R
        assert K.RelGraphConv(4, 4, 7, num_bases=nb).num_bases == 7
    nobias = K.RelGraphConv(20, 12, 7, num_bases=3, bias=False)
    assert sorted(nobias.state_dict()) == ["w_comp", "weight"]
    loop = K.RelGraphConv(20, 12, 7, num_bases=3, self_loop=True, dropout=0.25)
    assert sorted(loop.state_dict()) == ["h_bias", "loop_weight", "w_comp", "weight"]
    assert loop.loop_weight.shape == (20, 12) and float(loop.loop_weight.detach().abs().max()) <= _init_bound(20, 12)
    assert loop.dropout.p == 0.25 and loop.drop_p() == 0.25 and loop.eval().drop_p() == 0.0
    # a foreign state_dict of DGL's layout loads strictly
    foreign = {"weight": torch.randn(3, 20, 12), "w_comp": torch.randn(7, 3), "h_bias": torch.randn(12),
               "loop_weight": torch.randn(20, 12)}
    loop.load_state_dict(foreign, strict=True)
    assert torch.equal(loop.w_comp.detach(), foreign["w_comp"]) and torch.equal(loop.h_bias.detach(), foreign["h_bias"])
    with pytest.raises(RuntimeError):
        conv.load_state_dict(foreign, strict=True)                                      # no loop_weight there
    with pytest.raises(NotImplementedError):
        K.RelGraphConv(8, 8, 4, regularizer="bdd", num_bases=2)
    with pytest.raises(ValueError):
        K.RelGraphConv(8, 8, 4, regularizer="other")
    with pytest.raises(NotImplementedError):
        K.RelGraphConv((8, 8), 8, 4)


def test_install_as_dgl_exposes_relgraphconv():
    K.install_as_dgl(force=True)
    from dgl.nn.pytorch.conv import RelGraphConv
    assert RelGraphConv is K.RelGraphConv and "RelGraphConv" in K.__all__


def _ring(n=5):
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(list(range(n)), [(i + 1) % n for i in range(n)])
    return g


def test_cpu_tensors_and_other_refusals():
    g = _ring()
    et = torch.tensor([0, 1, 2, 0, 1])
    conv = K.RelGraphConv(16, 8, 3, num_bases=2)
    with pytest.raises(K.KGATLibraryError):           # no CPU fallback, supported shape
        conv(g, torch.randn(5, 16), et)
    with pytest.raises(K.KGATLibraryError):           # ... nor for the shapes the torch restatement serves
        K.RelGraphConv(20, 8, 3, num_bases=2)(g, torch.randn(5, 20), et)
    with pytest.raises(K.KGATLibraryError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et)
    with pytest.raises(K.KGATLibraryError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et, torch.rand(5, 1))
    with pytest.raises(NotImplementedError):          # tuple inputs
        conv(g, (torch.randn(5, 16), torch.randn(5, 16)), et)
    with pytest.raises(NotImplementedError):          # featureless input
        conv(g, torch.arange(5), et)
    with pytest.raises(ValueError):
        conv(g, torch.randn(4, 16), et)
    with pytest.raises(ValueError):
        conv(g, torch.randn(5, 8), et)
    with pytest.raises(ValueError):
        autograd.rgcn_aggregate(g, torch.randn(5, 2, 8), torch.randn(3, 2), et)
    with pytest.raises(ValueError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et[:4])
    with pytest.raises(ValueError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et, torch.rand(5, 2))
    with pytest.raises(TypeError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16, dtype=torch.float64), torch.randn(3, 2), et)
    with pytest.raises(TypeError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2).half(), et)
    with pytest.raises(TypeError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et.float())
    with pytest.raises(NotImplementedError):          # no gradient towards norm
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et, torch.rand(5, requires_grad=True))
    g.partition = object()
    with pytest.raises(K.DGLError):
        conv(g, torch.randn(5, 16), et)
    with pytest.raises(K.DGLError):
        autograd.rgcn_aggregate(g, torch.randn(5, 16), torch.randn(3, 2), et)


def test_propagation_model_builds_the_rgcn_stack():
    m = K.KGATPropagation(10, 2, 16, 16, 3, 16, dropout=0.0, gnn_model="rgcn")
    assert m._rgcn_stack() and not m._sage_stack() and not m._can_fuse_readout()
    assert [(layer.in_feat, layer.out_feat) for layer in m.layers] == [(16, 16), (16, 8), (8, 4)]
    for i, layer in enumerate(m.layers):
        assert isinstance(layer, K.RelGraphConv) and layer.num_rels == 2 and layer.num_bases == 2      # min(4, R)
        assert layer.self_loop and layer.bias and (layer.activation is None) == (i == 2)
        assert not hasattr(layer, "w_comp")
    m = K.KGATPropagation(10, 41, 16, 16, 2, 16, dropout=0.2, gnn_model="rgcn")
    assert [layer.num_bases for layer in m.layers] == [4, 4] and m.layers[0].w_comp.shape == (41, 4)
    assert m.layers[0].dropout.p == 0.2
    assert K.KGATPropagation(10, 41, 16, 16, 1, 16, gnn_model="rgcn", num_bases=8).layers[0].num_bases == 8
    with pytest.raises(ValueError):
        K.KGATPropagation(10, 2, 16, 16, 3, 16, gnn_model="rgcn", res_type="GCN")
    with pytest.raises(ValueError):
        K.KGATPropagation(10, 2, 16, 16, 3, 16, gnn_model="rgcn", node_dropout=0.1)
    with pytest.raises(ValueError):
        K.KGATPropagation(10, 2, 16, 16, 3, 16, gnn_model="rgcn", num_bases=0)
    with pytest.raises(NotImplementedError):          # the propagation model keeps refusing it
        K.KGATPropagation(10, 2, 8, 8, 2, 8, gnn_model="gat")
    g = _ring()
    g.partition = object()
    with pytest.raises(K.DGLError):
        K.KGATPropagation(5, 2, 16, 16, 1, 16, gnn_model="rgcn").gnn(g)


def test_training_example_takes_rgcn_and_its_conflicts(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat as tk
    a = tk.parse_args(["--gnn_model", "rgcn", "--num_bases", "8"])
    assert a.gnn_model == "rgcn" and a.num_bases == 8 and a.res_type == "Bi"
    assert not hasattr(tk.parse_args(["--gnn_model", "rgcn"]), "num_bases")              # the model's default: 4
    for argv in (["--res_type", "GCN"], ["--node_dropout", "0.1"], ["--explain", "3"], ["--attention_grad", "1"],
                 ["--num_bases", "0"], ["--gpus", "2"]):
        with pytest.raises(SystemExit):
            tk.parse_args(["--gnn_model", "rgcn"] + argv)
    capsys.readouterr()
