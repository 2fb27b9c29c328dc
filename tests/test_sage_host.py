"""Host-side checks of the GraphSAGE (mean) layer: the reference's graphsage model builds over this package, the
DGL surface (fn.copy_src / fn.copy_u / fn.mean, update_all, SAGEConv) refuses what it does not run, and the new C
entries validate their arguments before any device work.  No GPU needed."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, function as fn  # noqa: E402

REFERENCE = os.environ.get("KGAT_REFERENCE_DIR", "/root/reference")  # a checkout of the reference implementation


def _reference_models():
    path = os.path.join(REFERENCE, "models.py")
    if not os.path.exists(path):
        pytest.skip("reference checkout not present")
    K.install_as_dgl(force=True)
    spec = importlib.util.spec_from_file_location("_reference_models_sage", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_graphsage_model_builds():
    models = _reference_models()
    torch.manual_seed(0)
    m = models.Model(True, 64, "graphsage", 3, 64, 0.1, n_entities=50, n_relations=4, relation_dim=64)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("layers.")}
    want = {}
    for i, (d_in, d_out) in enumerate([(64, 64), (64, 32), (32, 16)]):
        for fc in ("fc_self", "fc_neigh"):
            want["layers.%d.%s.weight" % (i, fc)] = (d_out, d_in)
            want["layers.%d.%s.bias" % (i, fc)] = (d_out,)
    assert shapes == want
    assert all(isinstance(layer, K.SAGEConv) for layer in m.layers)
    assert [layer.activation for layer in m.layers] == [torch.nn.functional.relu, torch.nn.functional.relu, None]
    assert all(layer.feat_drop.p == 0.1 for layer in m.layers)
    # accelerate() takes the graphsage model (it raised TypeError on any layer without res_fc_2)
    assert K.accelerate(m) is m and m._kgat_accelerated


def test_accelerate_still_refuses_unknown_layers():
    class Odd(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.entity_embed = torch.nn.Embedding(4, 8)
            self.relation_embed = torch.nn.Embedding(2, 8)
            self.W_R = torch.nn.Parameter(torch.zeros(2, 8, 8))
            self.layers = torch.nn.ModuleList([torch.nn.Linear(8, 8)])

    with pytest.raises(TypeError):
        K.accelerate(Odd())


def test_sageconv_parameters_and_refusals():
    torch.manual_seed(1)
    conv = K.SAGEConv(20, 12, "mean", feat_drop=0.3)
    assert sorted(conv.state_dict()) == ["fc_neigh.bias", "fc_neigh.weight", "fc_self.bias", "fc_self.weight"]
    assert conv.fc_self.weight.shape == (12, 20) and conv.fc_neigh.bias.shape == (12,)
    # xavier-uniform with the gain of relu: |w| <= gain * sqrt(6 / (fan_in + fan_out))
    bound = torch.nn.init.calculate_gain("relu") * (6.0 / 32) ** 0.5
    assert float(conv.fc_self.weight.detach().abs().max()) <= bound and float(conv.fc_neigh.weight.detach().abs().max()) <= bound
    for agg in ("pool", "gcn", "lstm"):
        with pytest.raises(NotImplementedError):
            K.SAGEConv(8, 8, agg)
    with pytest.raises(NotImplementedError):
        K.SAGEConv((8, 8), 8, "mean")
    with pytest.raises(NotImplementedError):
        K.KGATPropagation(10, 2, 8, 8, 2, 8, gnn_model="gat")
    m = K.KGATPropagation(10, 2, 16, 16, 3, 16, dropout=0.0, gnn_model="graphsage")
    assert m._sage_stack() and not m._can_fuse_readout()
    assert [(layer._in_feats, layer._out_feats) for layer in m.layers] == [(16, 16), (16, 8), (8, 4)]


def test_function_aliases_and_update_all_refusals():
    assert fn.copy_u is fn.copy_src
    g = K.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
    g.ndata["h"] = torch.randn(5, 8)
    assert g.srcdata is g.ndata and g.dstdata is g.ndata
    with pytest.raises(K.KGATLibraryError):  # no CPU fallback
        g.update_all(fn.copy_src("h", "m"), fn.mean("m", "o"))
    with pytest.raises(K.KGATLibraryError):
        g.update_all(fn.copy_u("h", "m"), fn.sum("m", "o"))
    with pytest.raises(NotImplementedError):
        g.update_all(lambda e: {"m": e.src["h"]}, fn.mean("m", "o"))
    with pytest.raises(NotImplementedError):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.mean("m", "o"))
    with pytest.raises(K.DGLError):
        g.update_all(fn.copy_src("h", "m"), fn.mean("other", "o"))
    with pytest.raises(KeyError):
        g.update_all(fn.copy_src("nope", "m"), fn.mean("m", "o"))
    with pytest.raises(K.KGATLibraryError):
        K.SAGEConv(8, 8, "mean")(g, g.ndata["h"])


def test_sage_entries_refuse_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.kgat_copy_reduce_f32(-1, 0, 0, 0, 64, None, None, None, None, None, 1, None, 0, None) == -1
    assert b"copy_reduce" in lib.kgat_last_error()
    assert lib.kgat_copy_reduce_f32(4, 0, 0, 0, 64, None, None, None, None, None, 7, None, 0, None) == -1
    assert b"reduce" in lib.kgat_last_error()
    assert lib.kgat_copy_reduce_f32(4, 0, 0, 10, 64, None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.kgat_sage_dense_supported(64, 32) == 1 and lib.kgat_sage_dense_supported(20, 12) == 0
    assert lib.kgat_sage_dense_f32(10, 20, 12, None, None, None, None, None, None, 0, None, None, 0, None, 0, None) == -2
    assert b"sage_dense" in lib.kgat_last_error()
    assert lib.kgat_sage_dense_f32(10, 64, 64, None, None, None, None, None, None, 5, None, None, 0, None, 0, None) == -1
    assert lib.kgat_sage_dense_f32(10, 64, 64, None, None, None, None, None, None, 1, None, None, 0, None, 0, None) == -1
    assert lib.kgat_dropout_rows_f32(10, 8, None, None, 1.0, 0, None, None) == -1
    assert b"dropout_rows" in lib.kgat_last_error()
    assert lib.kgat_dropout_rows_f32(10, 8, None, None, 0.5, 0, None, None) == -1
    assert lib.kgat_sage_bwd_input_f32(10, 20, 12, None, None, None, None, None, None, None) == -2
    assert lib.kgat_sage_bwd_input_f32(10, 64, 32, None, None, None, None, None, None, None) == -1
    assert b"sage_bwd_input" in lib.kgat_last_error()
    assert lib.kgat_sage_bwd_weight_f32(100, 64, 32, None, None, None, None, None, None, 5, None) == -1
    assert b"n_partials" in lib.kgat_last_error()
    assert lib.kgat_sage_bwd_weight_f32(100, 20, 12, None, None, None, None, None, None, 2, None) == -2
