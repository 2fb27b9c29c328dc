"""KGAT's GCN and GraphSage aggregators (KGATConv res_type) without a GPU: parameters and state_dict keys per form, the
refusals (unknown res_type, graphsage + res_type, a partitioned graph), the C entries' host-side answers and the
example's --res_type parser."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, ops  # noqa: E402
from dgl_kgat_amd.graph import DGLError  # noqa: E402


def _model(res_type, **kw):
    return K.KGATPropagation(100, 5, input_node_dim=64, relation_dim=64, num_gnn_layers=3, n_hidden=64, dropout=0.1,
                             res_type=res_type, **kw)


@pytest.mark.parametrize("res_type,name,k", [("Bi", "res_fc_2", 1), ("GCN", "res_fc", 1), ("GraphSage", "res_fc", 2)])
def test_state_dict_keys_and_shapes_per_form(res_type, name, k):
    sd = _model(res_type).state_dict()
    layer_keys = sorted(key for key in sd if key.startswith("layers."))
    assert layer_keys == ["layers.%d.%s.weight" % (i, name) for i in range(3)]
    # widths 64 -> 64 -> 32 -> 16 (reference models.py:91-111); GraphSage's W acts on [h | h_N]
    assert [tuple(sd[key].shape) for key in layer_keys] == [(64, 64 * k), (32, 64 * k), (16, 32 * k)]
    assert sorted(key for key in sd if not key.startswith("layers.")) == ["W_R", "entity_embed.weight",
                                                                          "relation_embed.weight"]
    for layer in _model(res_type).layers:
        assert isinstance(layer, K.KGATConv) and layer._res_type == res_type
        lin = getattr(layer, name)
        assert lin.bias is None
        assert not hasattr(layer, "res_fc" if name == "res_fc_2" else "res_fc_2")


def test_graphsage_columns_act_on_h_then_h_neighbor():
    conv = K.KGATConv(16, 8, 0.0, "GraphSage")
    assert tuple(conv.res_fc.weight.shape) == (8, 32)
    conv = K.KGATConv(16, 8, 0.0, "GCN")
    assert tuple(conv.res_fc.weight.shape) == (8, 16)
    # torch's default init of nn.Linear: kaiming-uniform bound 1 / sqrt(fan_in)
    w = K.KGATConv(64, 64, 0.0, "GraphSage").res_fc.weight
    assert float(w.detach().abs().max()) <= 1.0 / 128 ** 0.5 + 1e-7


def test_unknown_res_type_and_graphsage_with_res_type_are_refused():
    for bad in ("gcn", "Sum", "", None):
        with pytest.raises(NotImplementedError):
            K.KGATConv(16, 16, 0.1, bad)
        with pytest.raises(NotImplementedError):
            _model(bad)
    for res_type in ("GCN", "GraphSage"):
        with pytest.raises(ValueError):
            _model(res_type, gnn_model="graphsage")
    assert len(_model("Bi", gnn_model="graphsage").layers) == 3


class _PartitionedGraph:
    """Stands in for a destination-range shard: the layer must refuse before touching it."""
    partition = object()

    @property
    def edata(self):
        raise AssertionError("the refusal must come first")


@pytest.mark.parametrize("res_type", ["GCN", "GraphSage"])
def test_partitioned_graph_with_a_new_form_raises(res_type):
    with pytest.raises(DGLError):
        K.KGATConv(16, 16, 0.0, res_type)(_PartitionedGraph(), torch.zeros(4, 16))
    with torch.no_grad(), pytest.raises(DGLError):
        _model(res_type).gnn(_PartitionedGraph())
    with pytest.raises(DGLError):
        _model(res_type).gnn(_PartitionedGraph(), fused=False)


def test_aggregator_entries_answer_without_gpu():
    lib = _lib.load()
    assert ops.FORMS == {"Bi": 0, "GCN": 1, "GraphSage": 2}
    wide = (16, 32, 64, 128)
    for form in (1, 2):
        for d_in in wide:
            for d_out in wide:
                assert lib.kgat_aggregator_supported(form, d_in, d_out) == 1
                assert lib.kgat_aggregator_bwd_supported(form, d_in, d_out) == 1
        for d_in, d_out in ((8, 8), (4, 16), (64, 8), (48, 64), (256, 64)):
            assert lib.kgat_aggregator_supported(form, d_in, d_out) == 0
            assert lib.kgat_aggregator_bwd_supported(form, d_in, d_out) == 0
    # form 0 is the Bi entries' coverage, the narrow one-lane-per-row widths included
    for d_in, d_out in ((8, 8), (64, 64), (4, 32), (128, 16)):
        assert lib.kgat_aggregator_supported(0, d_in, d_out) == lib.kgat_bi_interaction_supported(d_in, d_out) == 1
    assert lib.kgat_aggregator_bwd_supported(0, 8, 8) == lib.kgat_bi_interaction_bwd_input_supported(8, 8) == 0
    assert lib.kgat_aggregator_supported(3, 64, 64) == 0 and lib.kgat_aggregator_supported(-1, 64, 64) == 0
    # argument checks come before any device work
    fake = 256
    assert lib.kgat_aggregator_f32(1, -1, 64, 64, fake, fake, fake, 0.01, fake, None, 0, None, 0, None) == -1
    assert lib.kgat_aggregator_f32(2, 10, 8, 8, fake, fake, fake, 0.01, fake, None, 0, None, 0, None) == -2
    assert b"unsupported widths" in lib.kgat_last_error()
    assert lib.kgat_aggregator_train_f32(1, 10, 8, 8, fake, fake, fake, 0.01, 0.1, 1, 0, fake, None, 0, None, 0,
                                         None) == -2
    assert lib.kgat_aggregator_bwd_input_f32(2, 10, 64, 64, fake, fake, None, None, fake, None, None) == -1
    assert lib.kgat_aggregator_bwd_input_f32(1, 10, 8, 8, fake, fake, None, None, fake, None, None) == -2
    assert lib.kgat_aggregator_bwd_weight_f32(2, 10, 64, 64, fake, fake, fake, fake, 3, None) == -1
    assert lib.kgat_aggregator_deferred_f32(5, 10, 64, 64, fake, fake, fake, 0.01, fake, None, 0, None, 0, fake, 0, 0,
                                            fake, 256, None) == -1


def _train_kgat():
    spec = importlib.util.spec_from_file_location("_train_kgat_parser", os.path.join(ROOT, "examples", "train_kgat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_res_type_parser():
    tk = _train_kgat()
    assert tk.parse_args([]).res_type == "Bi"
    for res_type in ("Bi", "GCN", "GraphSage"):
        a = tk.parse_args(["--res_type", res_type, "--planted"])
        assert a.res_type == res_type and a.gnn_model == "kgat" and a.gpus == 1
    assert tk.parse_args(["--gnn_model", "graphsage"]).res_type == "Bi"
    assert tk.parse_args(["--gpus", "2"]).gpus == 2
    for argv in (["--res_type", "GCN", "--gnn_model", "graphsage"], ["--res_type", "GraphSage", "--gnn_model", "graphsage"],
                 ["--res_type", "GCN", "--gpus", "2"], ["--res_type", "GraphSage", "--gpus", "4"], ["--res_type", "gcn"]):
        with pytest.raises(SystemExit) as e:
            tk.parse_args(argv)
        assert e.value.code == 2
