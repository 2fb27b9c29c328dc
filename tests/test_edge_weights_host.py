"""Laplacian edge weights (use_attention=False, adj_type) and node dropout without a GPU: the two C-ABI entries are
declared at version 15, the numpy restatement of the edge mask, the constructor's refusals, the state_dict that must not
grow, and the example's parser."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, ops  # noqa: E402


def _model(**kw):
    return K.KGATPropagation(100, 5, input_node_dim=64, relation_dim=64, num_gnn_layers=3, n_hidden=64, dropout=0.1, **kw)


def test_header_declares_both_entries_at_version_15():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    for name in ("kgat_edge_norm_f32", "kgat_edge_dropout_f32"):
        assert name in declared and name in _lib.SIGNATURES
    assert "#define KGAT_ABI_VERSION 16" in header and _lib.ABI_VERSION == 16
    assert "KGAT_NORM_SI = 0" in header and "KGAT_NORM_BI = 1" in header
    assert ops.NORM_MODES == {"si": 0, "bi": 1}
    assert "kgat_edge_weights.hip" in _lib.SOURCES
    assert _lib.load().kgat_version() == 16


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 63 + 12345])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9])
def test_edge_keep_mask_is_the_row_mask_of_width_one(seed, p):
    for n_edges in (0, 1, 4099):
        got = ops.edge_keep_mask(seed, n_edges, p)
        assert got.shape == (n_edges,) and got.dtype == np.bool_
        assert np.array_equal(got, ops.dropout_keep_mask(seed, n_edges, 1, p).reshape(-1))
    if p == 0.0:
        assert ops.edge_keep_mask(seed, 4099, p).all()


def test_constructor_refusals():
    with pytest.raises(ValueError):
        _model(adj_type="xx")
    with pytest.raises(ValueError):
        _model(node_dropout=1.0)
    with pytest.raises(ValueError):
        _model(node_dropout=-0.1)
    with pytest.raises(ValueError):
        _model(gnn_model="graphsage", node_dropout=0.1)
    # what is allowed: every adj_type with or without attention, graphsage without node dropout
    for adj in ("si", "bi"):
        for att in (True, False):
            _model(use_attention=att, adj_type=adj, node_dropout=0.5)
    _model(gnn_model="graphsage", use_attention=False, adj_type="bi")


@pytest.mark.parametrize("res_type", ["Bi", "GCN", "GraphSage", "Bi2"])
def test_new_keywords_add_no_parameter_or_buffer(res_type):
    plain = _model(res_type=res_type)
    new = _model(res_type=res_type, use_attention=False, adj_type="bi", node_dropout=0.3)
    assert list(new.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in new.named_buffers()] == [n for n, _ in plain.named_buffers()] == []
    new.load_state_dict(plain.state_dict())


def _train_kgat():
    spec = importlib.util.spec_from_file_location("_train_kgat_parser_edge_weights",
                                                  os.path.join(ROOT, "examples", "train_kgat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_parser():
    tk = _train_kgat()
    a = tk.parse_args([])
    assert a.use_attention == 1 and a.adj_type == "si" and a.node_dropout == 0.0
    a = tk.parse_args(["--use_attention", "0", "--adj_type", "bi", "--node_dropout", "0.1"])
    assert a.use_attention == 0 and a.adj_type == "bi" and a.node_dropout == 0.1
    # (the run's JSON log records vars(args): all three are in it)
    assert {"use_attention", "adj_type", "node_dropout"} <= set(vars(a))
    for argv in (["--node_dropout", "0.1", "--gnn_model", "graphsage"], ["--node_dropout", "0.1", "--gpus", "2"],
                 ["--node_dropout", "1.0"], ["--adj_type", "xx"], ["--use_attention", "2"]):
        with pytest.raises(SystemExit) as e:
            tk.parse_args(argv)
        assert e.value.code == 2
