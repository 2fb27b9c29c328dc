"""The KGAT paper's two-term Bi-Interaction aggregator (KGATConv res_type "Bi2") without a GPU: parameters and state_dict
keys, the refusals (unknown res_type, graphsage + Bi2, a partitioned graph, the example's parser), the kgat_bi2_* entries'
host-side answers, and what must not move (ops.FORMS, the aggregator entries' form table)."""
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


def test_state_dict_is_the_union_of_gcn_and_bi():
    sd = _model("Bi2").state_dict()
    layer_keys = sorted(key for key in sd if key.startswith("layers."))
    assert layer_keys == sorted(["layers.%d.res_fc.weight" % i for i in range(3)] +
                                ["layers.%d.res_fc_2.weight" % i for i in range(3)])
    shapes = [(64, 64), (32, 64), (16, 32)]  # widths 64 -> 64 -> 32 -> 16 (reference models.py:91-111)
    for i, shape in enumerate(shapes):
        assert tuple(sd["layers.%d.res_fc.weight" % i].shape) == shape
        assert tuple(sd["layers.%d.res_fc_2.weight" % i].shape) == shape
    assert sorted(key for key in sd if not key.startswith("layers.")) == ["W_R", "entity_embed.weight",
                                                                          "relation_embed.weight"]
    assert set(layer_keys) == (set(k for k in _model("GCN").state_dict() if k.startswith("layers.")) |
                               set(k for k in _model("Bi").state_dict() if k.startswith("layers.")))
    for layer in _model("Bi2").layers:
        assert isinstance(layer, K.KGATConv) and layer._res_type == "Bi2"
        assert layer.res_fc.bias is None and layer.res_fc_2.bias is None
    # a GCN + a Bi state_dict load into a Bi2 model as they are
    m = _model("Bi2")
    merged = dict(_model("Bi").state_dict())
    merged.update({k: v for k, v in _model("GCN").state_dict().items() if k.startswith("layers.")})
    m.load_state_dict(merged)


def test_layer_dense_reads_res_type_before_the_attributes():
    from dgl_kgat_amd.kgat_layer import BI2_FORM, RES_TYPES, _layer_dense
    conv = K.KGATConv(32, 16, 0.0, "Bi2")
    form, w, d_in, d_out = _layer_dense(conv)
    assert form == BI2_FORM == RES_TYPES["Bi2"] and form not in ops.FORMS.values()
    assert w[0] is conv.res_fc.weight and w[1] is conv.res_fc_2.weight and (d_in, d_out) == (32, 16)
    assert _layer_dense(K.KGATConv(32, 16, 0.0, "Bi"))[0] == ops.FORMS["Bi"]
    assert {k: v for k, v in RES_TYPES.items() if k != "Bi2"} == ops.FORMS


def test_refusals():
    for bad in ("gcn", "Sum", "", None, "bi2", "BI2"):
        with pytest.raises(NotImplementedError):
            K.KGATConv(16, 16, 0.1, bad)
        with pytest.raises(NotImplementedError):
            _model(bad)
    with pytest.raises(ValueError):
        _model("Bi2", gnn_model="graphsage")


class _PartitionedGraph:
    """Stands in for a destination-range shard: the layer must refuse before touching it."""
    partition = object()

    @property
    def edata(self):
        raise AssertionError("the refusal must come first")


def test_partitioned_graph_raises():
    with pytest.raises(DGLError):
        K.KGATConv(16, 16, 0.0, "Bi2")(_PartitionedGraph(), torch.zeros(4, 16))
    with torch.no_grad(), pytest.raises(DGLError):
        _model("Bi2").gnn(_PartitionedGraph())
    with pytest.raises(DGLError):
        _model("Bi2").gnn(_PartitionedGraph(), fused=False)


def test_cpu_layer_matches_the_formula():
    """The library-GEMM path of the layer (what runs off the kernels' widths) is the paper's eq. 8."""
    torch.manual_seed(0)
    conv = K.KGATConv(8, 4, 0.0, "Bi2").double()
    h, hn = torch.randn(5, 8, dtype=torch.float64), torch.randn(5, 8, dtype=torch.float64)
    got = conv._dense(h, hn, fused=False)
    lr = torch.nn.functional.leaky_relu
    want = lr((h + hn) @ conv.res_fc.weight.t(), 0.01) + lr((h * hn) @ conv.res_fc_2.weight.t(), 0.01)
    assert torch.allclose(got, want, rtol=0, atol=1e-14)


def test_bi2_entries_answer_without_gpu():
    lib = _lib.load()
    assert ops.FORMS == {"Bi": 0, "GCN": 1, "GraphSage": 2}
    assert lib.kgat_aggregator_supported(3, 64, 64) == 0 and lib.kgat_aggregator_bwd_supported(3, 64, 64) == 0
    wide = (16, 32, 64, 128)
    for d_in in wide:
        for d_out in wide:
            assert lib.kgat_bi2_supported(d_in, d_out) == 1 and lib.kgat_bi2_bwd_supported(d_in, d_out) == 1
    for d_in, d_out in ((8, 8), (4, 16), (64, 8), (48, 64), (256, 64)):
        assert lib.kgat_bi2_supported(d_in, d_out) == 0 and lib.kgat_bi2_bwd_supported(d_in, d_out) == 0
    # argument checks come before any device work: -1 bad arguments, -2 unsupported widths
    fake = 256
    assert lib.kgat_bi2_f32(-1, 64, 64, fake, fake, fake, fake, 0.01, fake, None, 0, None, 0, None) == -1
    assert lib.kgat_bi2_f32(10, 64, 64, fake, fake, None, fake, 0.01, fake, None, 0, None, 0, None) == -1
    assert lib.kgat_bi2_f32(10, 8, 8, fake, fake, fake, fake, 0.01, fake, None, 0, None, 0, None) == -2
    assert b"unsupported widths" in lib.kgat_last_error()
    assert lib.kgat_bi2_deferred_f32(10, 64, 64, fake, fake, fake, fake, 0.01, fake, None, 0, None, 0, fake, 0, 0, fake,
                                     100, None) == -1  # tile_edges not a power of two
    assert lib.kgat_bi2_deferred_f32(10, 48, 64, fake, fake, fake, fake, 0.01, fake, None, 0, None, 0, fake, 0, 0, fake,
                                     256, None) == -2
    assert lib.kgat_bi2_train_f32(10, 64, 64, fake, fake, fake, fake, 0.01, 0.1, 1, 0, fake, None, None, 0, None, 0,
                                  None) == -1  # no sign record
    assert b"sign record" in lib.kgat_last_error()
    assert lib.kgat_bi2_train_f32(10, 64, 64, fake, fake, fake, fake, 0.01, 1.0, 1, 0, fake, fake, None, 0, None, 0,
                                  None) == -1  # dropout probability 1
    assert lib.kgat_bi2_train_f32(10, 256, 64, fake, fake, fake, fake, 0.01, 0.1, 1, 0, fake, fake, None, 0, None, 0,
                                  None) == -2
    assert lib.kgat_bi2_bwd_pre_f32(10, 64, fake, None, None, None, None, 0, 0.01, 0.1, 1, 0, fake, 2 * fake, None) == -1
    assert lib.kgat_bi2_bwd_pre_f32(10, 256, fake, fake, None, None, None, 0, 0.01, 0.1, 1, 0, fake, 2 * fake, None) == -1
    assert lib.kgat_bi2_bwd_input_f32(10, 64, 64, fake, fake, fake, fake, fake, fake, fake, None, None) == -1
    assert lib.kgat_bi2_bwd_input_f32(10, 8, 8, fake, fake, fake, fake, fake, fake, fake, 2 * fake, None) == -2
    assert lib.kgat_bi2_bwd_weight_f32(10, 64, 64, fake, fake, fake, fake, fake, 2 * fake, 3, None) == -1  # n_partials
    assert lib.kgat_bi2_bwd_weight_f32(10, 64, 8, fake, fake, fake, fake, fake, 2 * fake, 1, None) == -2
    # zero rows: nothing to do
    assert lib.kgat_bi2_f32(0, 64, 64, None, None, None, None, 0.01, None, None, 0, None, 0, None) == 0
    # the Python wrappers refuse CPU tensors like their siblings
    with pytest.raises(_lib.KGATLibraryError):
        ops.aggregator(ops.BI2_FORM, torch.zeros(4, 16), torch.zeros(4, 16), (torch.zeros(16, 16), torch.zeros(16, 16)))
    assert (ops.aggregator_supported(ops.BI2_FORM, 64, 32) and ops.aggregator_bwd_supported(ops.BI2_FORM, 32, 16) and
            not ops.aggregator_supported(ops.BI2_FORM, 8, 8))


def _train_kgat():
    spec = importlib.util.spec_from_file_location("_train_kgat_parser_bi2", os.path.join(ROOT, "examples", "train_kgat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_parser_takes_bi2_and_refuses_what_it_cannot_run():
    tk = _train_kgat()
    a = tk.parse_args(["--res_type", "Bi2", "--planted"])
    assert a.res_type == "Bi2" and a.gnn_model == "kgat" and a.gpus == 1
    assert tk.parse_args([]).res_type == "Bi"
    for argv in (["--res_type", "Bi2", "--gnn_model", "graphsage"], ["--res_type", "Bi2", "--gpus", "2"],
                 ["--res_type", "bi2"]):
        with pytest.raises(SystemExit) as e:
            tk.parse_args(argv)
        assert e.value.code == 2
