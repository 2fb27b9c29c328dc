"""KGAT's GCN and GraphSage aggregators (KGATConv res_type) on the MI355X: the aggregator kernels at every width pair
(no-grad, deferred, training and both backward kernels), the KGATPropagation stack (fused readout, surface path, the
product-only switch, the whole-stack training unit's gradients, a width off the kernels) and an end-to-end training
run.  References are float64 restatements of the paper's aggregators inside this file:
    GCN        LeakyReLU(W (h + h_N))          GraphSage  LeakyReLU(W [h | h_N])
with h_N = update_all(u_mul_e('h','w','m'), sum('m','h_neighbor')) (reference models.py:63)."""
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

from conftest import readout_abs_bar  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {"GCN": 1, "GraphSage": 2}
WIDTHS = (16, 32, 64, 128)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _scale_err(x, y):
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y)) / max(np.abs(y).max(), 1e-30)) if y.size else 0.0


def _np(t):
    return t.detach().double().cpu().numpy()


def _comb(form, h, hn):
    return h + hn if form == FORMS["GCN"] else np.concatenate([h, hn], 1)


def _leaky(z):
    return np.where(z >= 0, z, 0.01 * z)


def _normalize(z):
    return z / np.maximum(np.sqrt((z * z).sum(1, keepdims=True)), 1e-12)


def _edges(kind, n, rng):
    if kind == "hub":   # one destination with tens of thousands of in-edges among ordinary rows
        dst = np.concatenate([rng.integers(0, n, 6 * n), np.full(30000, 7)])
    elif kind == "noin":  # a third of the rows without in-edges
        dst = rng.integers(0, n, 6 * n)
        dst = dst[dst % 3 != 0]
    else:
        dst = rng.integers(0, n, 8 * n)
    return rng.integers(0, n, dst.size), dst


def _graph(n, src, dst, dev):
    import dgl_kgat_amd as K
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    g.readonly()
    return g


@pytest.mark.parametrize("kind", ["random", "hub", "noin"])
@pytest.mark.parametrize("form_name", ["GCN", "GraphSage"])
def test_aggregator_kernels_every_width(dev, form_name, kind):
    """Forward, deferred, training form and both backward kernels at every width pair against fp64 (1e-5 of each
    tensor's scale); two launches give the same bits; the deferred form is bit-identical to the plain one; the dropout
    mask is ops.dropout_keep_mask."""
    from dgl_kgat_amd import ops
    form = FORMS[form_name]
    rng = np.random.default_rng(17 + form)
    n = 1500
    src, dst = _edges(kind, n, rng)
    g = _graph(n, src, dst, dev)
    st = g._st
    csr = st.csr(dev)
    w = torch.as_tensor(rng.random(src.size).astype(np.float32) / 8, device=dev)
    w_csr = st.csr_weights(w)
    for d_in in WIDTHS:
        H = torch.randn(n, d_in, device=dev)
        HN = ops.spmm(csr.indptr, csr.col, csr.row_of, H, w_csr)
        h64, hn64 = _np(H), _np(HN)
        x64 = _comb(form, h64, hn64)
        for d_out in WIDTHS:
            assert ops.aggregator_supported(form, d_in, d_out) and ops.aggregator_bwd_supported(form, d_in, d_out)
            k = 2 * d_in if form == FORMS["GraphSage"] else d_in
            W = torch.randn(d_out, k, device=dev) / k ** 0.5
            z64 = _leaky(x64 @ _np(W).T)
            tag = (form_name, kind, d_in, d_out)
            # no-grad form: rows, normalised slice of a wider readout, ego block
            ro = torch.full((n, d_in + d_out + 4), 7.0, device=dev)
            z = ops.aggregator(form, H, HN, W, 0.01, norm_out=ro[:, d_in:d_in + d_out], self_out=ro[:, :d_in])
            assert _scale_err(_np(z), z64) <= 1e-5, tag
            assert _scale_err(_np(ro[:, d_in:d_in + d_out]), _normalize(z64)) <= 1e-5, tag
            assert torch.equal(ro[:, :d_in], H) and bool((ro[:, d_in + d_out:] == 7.0).all()), tag
            z2 = ops.aggregator(form, H, HN, W, 0.01)
            assert torch.equal(z, z2), tag
            # deferred: the aggregation's second launch left to the dense kernel - the same bits
            hn_d, rows = ops.spmm(csr.indptr, csr.col, csr.row_of, H, w_csr, defer_finish=True)
            ro_d = torch.full_like(ro, 7.0)
            z_d = ops.aggregator(form, H, hn_d, W, 0.01, norm_out=ro_d[:, d_in:d_in + d_out], self_out=ro_d[:, :d_in],
                                 deferred=rows)
            assert torch.equal(z_d, z) and torch.equal(ro_d, ro), tag
            # training form: LeakyReLU, hash dropout, normalised slice
            p, seed = 0.3, 1234 + d_out
            nrm = torch.empty(n, d_out, device=dev)
            y = ops.aggregator_train(form, H, HN, W, 0.01, p, seed, norm_out=nrm)
            keep = ops.dropout_keep_mask(seed, n, d_out, p)
            y64 = np.where(keep, z64 / (1 - p), 0.0)
            assert np.array_equal(_np(y) != 0, keep & (z64 != 0)), tag
            assert _scale_err(_np(y), y64) <= 1e-5 and _scale_err(_np(nrm), _normalize(y64)) <= 1e-5, tag
            assert torch.equal(y, ops.aggregator_train(form, H, HN, W, 0.01, p, seed)), tag
            # backward kernels
            gz = torch.randn(n, d_out, device=dev)
            gp64 = _np(gz) @ _np(W)
            t, gb = ops.aggregator_bwd_input(form, gz, W, H, HN)
            if form == FORMS["GCN"]:
                assert t is gb and _scale_err(_np(t), gp64) <= 1e-5, tag
            else:
                assert _scale_err(_np(t), gp64[:, d_in:]) <= 1e-5 and _scale_err(_np(gb), gp64[:, :d_in]) <= 1e-5, tag
            t2, gb2 = ops.aggregator_bwd_input(form, gz, W, H, HN)
            assert torch.equal(t, t2) and torch.equal(gb, gb2), tag
            gw = ops.aggregator_bwd_weight(form, gz, H, HN)
            assert tuple(gw.shape) == (d_out, k)
            assert _scale_err(_np(gw), _np(gz).T @ x64) <= 1e-5, tag
            assert torch.equal(gw, ops.aggregator_bwd_weight(form, gz, H, HN)), tag


# ---------------------------------------------------------------- the stack

def _setup(dev, res_type, dim=64, layers=3, dropout=0.0, seed=5):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth
    n, trip, n_rel = synth.collaborative_kg(300, 500, 400, 4, 12000, 6000, seed=3)
    torch.manual_seed(seed)
    model = K.KGATPropagation(n, n_rel, input_node_dim=dim, relation_dim=dim, num_gnn_layers=layers, n_hidden=dim,
                              dropout=dropout, res_type=res_type).to(dev)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
    return model, g, n, trip


def _readout_ref64(model, g, n, trip, masks=None, p=0.0):
    """[h0 | normalize(h1) | ...] in fp64 from the model's parameters and the graph's attention weights."""
    form = FORMS[model._res_type]
    src, dst = trip[:, 2], trip[:, 0]
    a = _np(g.edata["w"]).reshape(-1)
    h = _np(model.entity_embed.weight)
    cache = [h]
    for li, layer in enumerate(model.layers):
        hn = np.zeros_like(h)
        np.add.at(hn, dst, a[:, None] * h[src])
        z = _leaky(_comb(form, h, hn) @ _np(layer.res_fc.weight).T)
        if masks is not None:
            z = np.where(masks[li], z / (1 - p), 0.0)
        h = z
        cache.append(_normalize(h))
    return np.concatenate(cache, 1)


@pytest.mark.parametrize("res_type", ["GCN", "GraphSage"])
def test_stack_readout_fused_surface_and_switches(dev, res_type):
    from dgl_kgat_amd.options import options, override
    model, g, n, trip = _setup(dev, res_type)
    model.eval()
    assert model._can_fuse_readout()
    with torch.no_grad():
        out = model.gnn(g)
        surface = model.gnn(g, fused=False)
        with override(fuse_bi=True):
            out_fb = model.gnn(g)
        with override(gnn_defer_finish=not options.gnn_defer_finish):
            out_df = model.gnn(g)
    ref = _readout_ref64(model, g, n, trip)
    widths = [64, 64, 32, 16]
    o = 0
    for b, wd in enumerate(widths):
        err = _scale_err(_np(out[:, o:o + wd]), ref[:, o:o + wd])
        assert err <= readout_abs_bar(b), (res_type, b, err)
        assert _scale_err(_np(surface[:, o:o + wd]), ref[:, o:o + wd]) <= 1e-5, (res_type, b)
        o += wd
    # the product-only switch is skipped for these forms, never applied; the deferred finish gives the same bits
    assert torch.equal(out_fb, out) and torch.equal(out_df, out)


@pytest.mark.parametrize("res_type", ["GCN", "GraphSage"])
def test_stack_training_unit_gradients(dev, res_type):
    """_GNNTrain (the whole stack as one autograd unit, hash dropout) against torch fp64 autograd of the restatement."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.autograd import gnn_train
    model, g, n, trip = _setup(dev, res_type, dropout=0.2)
    model.train()
    form = FORMS[res_type]
    p, seed = 0.2, 99
    emb = model.entity_embed.weight
    weights = [layer.res_fc.weight for layer in model.layers]
    out = gnn_train(g, emb, weights, 0.01, p, seed, forms=[form] * 3)
    assert type(out.grad_fn).__name__.startswith("_GNNTrain")
    R = torch.randn(out.shape, device=dev)
    (out * R).sum().backward()
    # the model's own path takes the unit as well
    torch.manual_seed(0)
    assert type(model.gnn(g).grad_fn).__name__.startswith("_GNNTrain")
    masks = [ops.dropout_keep_mask(seed + li, n, w.shape[0], p) for li, w in enumerate(weights)]
    with torch.no_grad():
        ref_out = _readout_ref64(model, g, n, trip, masks, p)
    assert _scale_err(_np(out), ref_out) <= 1e-5
    # fp64 autograd of the restatement
    src = torch.as_tensor(trip[:, 2], device=dev)
    dst = torch.as_tensor(trip[:, 0], device=dev)
    a = g.edata["w"].detach().double().reshape(-1, 1)
    h = emb.detach().double().clone().requires_grad_(True)
    Ws = [w.detach().double().clone().requires_grad_(True) for w in weights]
    x, cache = h, [h]
    for li, W in enumerate(Ws):
        hn = torch.zeros_like(x).index_add_(0, dst, a * x[src])
        c = x + hn if form == FORMS["GCN"] else torch.cat([x, hn], 1)
        z = torch.nn.functional.leaky_relu(c @ W.t(), 0.01)
        x = torch.where(torch.as_tensor(masks[li], device=dev), z / (1 - p), torch.zeros_like(z))
        cache.append(torch.nn.functional.normalize(x, p=2, dim=1))
    (torch.cat(cache, 1) * R.double()).sum().backward()
    assert _scale_err(_np(emb.grad), _np(h.grad)) <= 1e-5
    for li, (w, W) in enumerate(zip(weights, Ws)):
        assert w.grad is not None and _scale_err(_np(w.grad), _np(W.grad)) <= 1e-5, li
    assert isinstance(model.layers[0], K.KGATConv)


@pytest.mark.parametrize("res_type", ["GCN", "GraphSage"])
def test_width_off_the_kernels_takes_the_fallback(dev, res_type):
    from dgl_kgat_amd import ops
    model, g, n, trip = _setup(dev, res_type, dim=8, layers=1)
    assert not ops.aggregator_supported(FORMS[res_type], 8, 8)
    model.eval()
    assert not model._can_fuse_readout()
    with torch.no_grad():
        out = model.gnn(g)
    ref = _readout_ref64(model, g, n, trip)
    assert _scale_err(_np(out[:, :8]), ref[:, :8]) == 0.0
    assert _scale_err(_np(out[:, 8:]), ref[:, 8:]) <= 1e-5
    # under autograd: the per-layer path, gradients reach the layer's weight and the embeddings
    model.train()
    loss = model.gnn(g).square().sum()
    loss.backward()
    assert model.layers[0].res_fc.weight.grad is not None and model.entity_embed.weight.grad is not None


@pytest.mark.parametrize("res_type", ["GCN", "GraphSage"])
def test_planted_structure_recall_rises_with_res_type(dev, res_type, tmp_path, capsys):
    """End to end in a child process (the example's global switches stay there): recall@20 on the planted held-out
    interactions leaves a random ranking within three short epochs - the bar of test_planted_structure_recall_rises."""
    log = tmp_path / ("train_%s.json" % res_type)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_kgat.py"), "--planted", "--epochs", "3", "--lr", "0.03",
           "--batch_size", "512", "--batch_size_kg", "512", "--eval_before", "--seed", "1234", "--res_type", res_type,
           "--log_json", str(log)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(log) as f:
        hist = json.load(f)["epochs"]
    rec = [h["test_recall"] for h in hist]
    val = [h["valid_recall"] for h in hist]
    with capsys.disabled():
        print("\n%s planted-structure run: test recall@20 by epoch %s, valid %s" % (
            res_type, ["%.4f" % x for x in rec], ["%.4f" % x for x in val]))
    assert rec[3] > 3.0 * rec[0] and rec[3] > rec[2] > rec[1]
    assert val[3] > 3.0 * val[0]
