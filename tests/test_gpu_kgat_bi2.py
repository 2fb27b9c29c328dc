"""The KGAT paper's two-term Bi-Interaction aggregator (KGATConv res_type "Bi2") on the MI355X: the kgat_bi2_* kernels at
every width pair (no-grad, deferred, training form with its sign record, backward head and both backward kernels), the
KGATPropagation stack (fused readout, surface path, the product-only switch, the whole-stack training unit's
gradients, a width off the kernels) and an end-to-end training run.  References are float64 restatements inside this
file of
    Z = LeakyReLU(W1 (h + h_N)) + LeakyReLU(W2 (h * h_N))        (Wang et al. 2019, eq. 8)
with h_N = update_all(u_mul_e('h','w','m'), sum('m','h_neighbor')) (reference models.py:63), W1 = res_fc.weight and
W2 = res_fc_2.weight.

Signs.  The backward needs LeakyReLU'(z1) and LeakyReLU'(z2) apart, which the training forward records (one byte per
element, bit 0 = z1 > 0, bit 1 = z2 > 0).  A recorded bit can differ from the fp64 sign only where the fp32 value is
within the forward bar (1e-5 of the term's scale) of zero; that is asserted.  The backward references then take their
slopes FROM THE RECORD, so that no comparison hinges on a near-zero sign: one flipped sign among ~3e5 elements would move
a whole gradient row by far more than 1e-5."""
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

WIDTHS = (16, 32, 64, 128)
SLOPE = 0.01


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


def _leaky(z):
    return np.where(z >= 0, z, SLOPE * z)


def _normalize(z):
    return z / np.maximum(np.sqrt((z * z).sum(1, keepdims=True)), 1e-12)


def _pre64(h, hn, W1, W2):
    """The two pre-activations in fp64."""
    return (h + hn) @ W1.T, (h * hn) @ W2.T


def _check_signs(signs, z1, z2, tag):
    """The recorded bits equal z64 > 0 wherever |z64| > 1e-5 * max|z64| of that term; returns the share of elements
    inside the band (a property of the inputs, not capped)."""
    s = signs.cpu().numpy()
    assert s.dtype == np.uint8 and s.shape == z1.shape and int(s.max(initial=0)) <= 3, tag
    inside = 0
    for bit, z in ((1, z1), (2, z2)):
        clear = np.abs(z) > 1e-5 * np.abs(z).max()
        assert np.array_equal(((s & bit) != 0)[clear], (z > 0)[clear]), (tag, bit)
        inside += int((~clear).sum())
    return inside / (2.0 * max(z1.size, 1))


def _slopes(signs):
    s = signs.cpu().numpy()
    return np.where(s & 1, 1.0, SLOPE), np.where(s & 2, 1.0, SLOPE)


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
def test_bi2_kernels_every_width(dev, kind, capsys):
    """Items 1-3: forward (plain, deferred, training with the sign record) and the three backward entries at every width
    pair against fp64, 1e-5 of each tensor's scale; repeat launches bit-identical; deferred = plain, bit for bit."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(23)
    n = 1500
    src, dst = _edges(kind, n, rng)
    g = _graph(n, src, dst, dev)
    st = g._st
    csr = st.csr(dev)
    w = torch.as_tensor(rng.random(src.size).astype(np.float32) / 8, device=dev)
    w_csr = st.csr_weights(w)
    worst = {}

    def note(name, err, tag):
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= 1e-5, (name, err, tag)

    band = 0.0
    for d_in in WIDTHS:
        H = torch.randn(n, d_in, device=dev)
        HN = ops.spmm(csr.indptr, csr.col, csr.row_of, H, w_csr)
        h64, hn64 = _np(H), _np(HN)
        for d_out in WIDTHS:
            assert ops.aggregator_supported(ops.BI2_FORM, d_in, d_out) and ops.aggregator_bwd_supported(ops.BI2_FORM, d_in, d_out)
            W1 = torch.randn(d_out, d_in, device=dev) / d_in ** 0.5
            W2 = torch.randn(d_out, d_in, device=dev) / d_in ** 0.5
            z1, z2 = _pre64(h64, hn64, _np(W1), _np(W2))
            z64 = _leaky(z1) + _leaky(z2)
            tag = (kind, d_in, d_out)
            # no-grad form: rows, normalised slice of a wider readout, ego block, padding untouched
            ro = torch.full((n, d_in + d_out + 4), 7.0, device=dev)
            z = ops.aggregator(ops.BI2_FORM, H, HN, (W1, W2), SLOPE, norm_out=ro[:, d_in:d_in + d_out], self_out=ro[:, :d_in])
            note("h_out", _scale_err(_np(z), z64), tag)
            note("norm", _scale_err(_np(ro[:, d_in:d_in + d_out]), _normalize(z64)), tag)
            assert torch.equal(ro[:, :d_in], H) and bool((ro[:, d_in + d_out:] == 7.0).all()), tag
            assert torch.equal(z, ops.aggregator(ops.BI2_FORM, H, HN, (W1, W2), SLOPE)), tag
            # deferred: the aggregation's second launch left to the dense kernel - the same bits
            hn_d, rows = ops.spmm(csr.indptr, csr.col, csr.row_of, H, w_csr, defer_finish=True)
            ro_d = torch.full_like(ro, 7.0)
            z_d = ops.aggregator(ops.BI2_FORM, H, hn_d, (W1, W2), SLOPE, norm_out=ro_d[:, d_in:d_in + d_out], self_out=ro_d[:, :d_in],
                          deferred=rows)
            assert torch.equal(z_d, z) and torch.equal(ro_d, ro), tag
            # training form: LeakyReLU per term, sum, hash dropout on the sum, normalised slice, sign record
            p, seed = 0.3, 1234 + d_out
            nrm = torch.empty(n, d_out, device=dev)
            y, signs = ops.aggregator_train(ops.BI2_FORM, H, HN, (W1, W2), SLOPE, p, seed, norm_out=nrm)
            keep = ops.dropout_keep_mask(seed, n, d_out, p)
            y64 = np.where(keep, z64 / (1 - p), 0.0)
            assert bool((_np(y)[~keep] == 0).all()), tag
            note("train", _scale_err(_np(y), y64), tag)
            note("train_norm", _scale_err(_np(nrm), _normalize(y64)), tag)
            y_b, signs_b = ops.aggregator_train(ops.BI2_FORM, H, HN, (W1, W2), SLOPE, p, seed)
            assert torch.equal(y, y_b) and torch.equal(signs, signs_b), tag
            band = max(band, _check_signs(signs, z1, z2, tag))
            # backward head from a given gradient: the slopes come from the record
            gA = torch.randn(n, d_out, device=dev)
            gB = torch.randn(n, d_out, device=dev)
            gN = torch.randn(n, d_out + 8, device=dev)[:, 4:4 + d_out]
            gz1, gz2 = ops.aggregator_bwd_pre(ops.BI2_FORM, y, signs, gA, gB, gN, SLOPE, p, seed)
            yv, gn = _np(y), _np(gN)
            nr = np.maximum(np.sqrt((yv * yv).sum(1, keepdims=True)), 1e-12)
            g64 = (gn - yv * ((yv * gn).sum(1, keepdims=True) / nr ** 2)) / nr + _np(gA) + _np(gB)
            g64 = np.where(keep, g64 / (1 - p), 0.0)
            s1, s2 = _slopes(signs)
            note("gz1", _scale_err(_np(gz1), g64 * s1), tag)
            note("gz2", _scale_err(_np(gz2), g64 * s2), tag)
            a1, a2 = ops.aggregator_bwd_pre(ops.BI2_FORM, y, signs, gA, gB, gN, SLOPE, p, seed)
            assert torch.equal(gz1, a1) and torch.equal(gz2, a2), tag
            # backward towards the inputs and the weights, from the kernel's own gz1 / gz2
            p1, p2 = _np(gz1) @ _np(W1), _np(gz2) @ _np(W2)
            t, gb = ops.aggregator_bwd_input(ops.BI2_FORM, (gz1, gz2), (W1, W2), H, HN)
            note("grad_agg", _scale_err(_np(t), p1 + p2 * h64), tag)
            note("grad_self", _scale_err(_np(gb), p1 + p2 * hn64), tag)
            t2, gb2 = ops.aggregator_bwd_input(ops.BI2_FORM, (gz1, gz2), (W1, W2), H, HN)
            assert torch.equal(t, t2) and torch.equal(gb, gb2), tag
            gw1, gw2 = ops.aggregator_bwd_weight(ops.BI2_FORM, (gz1, gz2), H, HN)
            assert tuple(gw1.shape) == tuple(gw2.shape) == (d_out, d_in)
            note("grad_W1", _scale_err(_np(gw1), _np(gz1).T @ (h64 + hn64)), tag)
            note("grad_W2", _scale_err(_np(gw2), _np(gz2).T @ (h64 * hn64)), tag)
            b1, b2 = ops.aggregator_bwd_weight(ops.BI2_FORM, (gz1, gz2), H, HN)
            assert torch.equal(gw1, b1) and torch.equal(gw2, b2), tag
    with capsys.disabled():
        print("\nBi2 kernels (%s): worst error / scale %s; largest share of pre-activations inside the sign band %.2e"
              % (kind, {k: "%.2e" % v for k, v in worst.items()}, band))


# ---------------------------------------------------------------- the stack

def _setup(dev, dim=64, layers=3, dropout=0.0, seed=5):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth
    n, trip, n_rel = synth.collaborative_kg(300, 500, 400, 4, 12000, 6000, seed=3)
    torch.manual_seed(seed)
    model = K.KGATPropagation(n, n_rel, input_node_dim=dim, relation_dim=dim, num_gnn_layers=layers, n_hidden=dim,
                              dropout=dropout, res_type="Bi2").to(dev)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
    return model, g, n, trip


def _readout_ref64(model, g, n, trip):
    """[h0 | normalize(h1) | ...] in fp64 from the model's parameters and the graph's attention weights (no dropout)."""
    src, dst = trip[:, 2], trip[:, 0]
    a = _np(g.edata["w"]).reshape(-1)
    h = _np(model.entity_embed.weight)
    cache = [h]
    for layer in model.layers:
        hn = np.zeros_like(h)
        np.add.at(hn, dst, a[:, None] * h[src])
        z1, z2 = _pre64(h, hn, _np(layer.res_fc.weight), _np(layer.res_fc_2.weight))
        h = _leaky(z1) + _leaky(z2)
        cache.append(_normalize(h))
    return np.concatenate(cache, 1)


def test_stack_readout_fused_surface_and_switches(dev, capsys):
    """Item 4.  The gate per block is 1e-5 of scale; the project's tighter per-layer bar (conftest.readout_abs_bar,
    1.5e-6 per layer, measured for "Bi") is asserted as well: measured on the MI355X, Bi2 holds it."""
    from dgl_kgat_amd.options import options, override
    model, g, n, trip = _setup(dev)
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
    errs = []
    for b, wd in enumerate(widths):
        err = _scale_err(_np(out[:, o:o + wd]), ref[:, o:o + wd])
        errs.append(err)
        with capsys.disabled():
            print("\nBi2 fused readout block %d: error / scale %.3e (bar %.3e)" % (b, err, readout_abs_bar(b)))
        assert err <= 1e-5, (b, err)
        assert _scale_err(_np(surface[:, o:o + wd]), ref[:, o:o + wd]) <= 1e-5, b
        o += wd
    for b, err in enumerate(errs):
        assert err <= readout_abs_bar(b), (b, err)
    assert torch.equal(out[:, :64], model.entity_embed.weight)
    # the product-only switch is skipped for this form, never applied; the deferred finish gives the same bits
    assert torch.equal(out_fb, out) and torch.equal(out_df, out)


def test_stack_training_unit_gradients(dev):
    """Item 5: _GNNTrain (the whole stack as one autograd unit, hash dropout, two weights per layer) against torch fp64
    autograd of the restatement, whose LeakyReLU slopes are the kernels' recorded ones."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.autograd import gnn_train
    model, g, n, trip = _setup(dev, dropout=0.2)
    model.train()
    p, seed = 0.2, 99
    emb = model.entity_embed.weight
    pairs = [(layer.res_fc.weight, layer.res_fc_2.weight) for layer in model.layers]
    out = gnn_train(g, emb, pairs, SLOPE, p, seed, forms=[ops.BI2_FORM] * 3)
    assert type(out.grad_fn).__name__.startswith("_GNNTrain")
    R = torch.randn(out.shape, device=dev)
    (out * R).sum().backward()
    # the model's own path takes the unit as well
    torch.manual_seed(0)
    assert type(model.gnn(g).grad_fn).__name__.startswith("_GNNTrain")
    masks = [ops.dropout_keep_mask(seed + li, n, w1.shape[0], p) for li, (w1, _) in enumerate(pairs)]
    # replay the layers through ops.aggregator_train (bit-reproducible kernels) for the sign records
    st = g._st
    csr = st.csr(dev)
    w_csr = st.csr_weights(g.edata["w"])
    records, x = [], emb.detach().contiguous()
    for li, (w1, w2) in enumerate(pairs):
        hn = ops.spmm(csr.indptr, csr.col, csr.row_of, x, w_csr)
        x, sg = ops.aggregator_train(ops.BI2_FORM, x, hn, (w1.detach().contiguous(), w2.detach().contiguous()), SLOPE, p,
                                     seed + li)
        records.append(sg)
    # fp64 autograd of the restatement with the recorded slopes; every record is within the forward bar of the fp64 sign
    src = torch.as_tensor(trip[:, 2], device=dev)
    dst = torch.as_tensor(trip[:, 0], device=dev)
    a = g.edata["w"].detach().double().reshape(-1, 1)
    h = emb.detach().double().clone().requires_grad_(True)
    Ws = [(w1.detach().double().clone().requires_grad_(True), w2.detach().double().clone().requires_grad_(True))
          for w1, w2 in pairs]
    x, cache = h, [h]
    for li, (W1, W2) in enumerate(Ws):
        hn = torch.zeros_like(x).index_add_(0, dst, a * x[src])
        z1, z2 = (x + hn) @ W1.t(), (x * hn) @ W2.t()
        _check_signs(records[li], _np(z1), _np(z2), ("layer", li))
        s1, s2 = _slopes(records[li])
        z = z1 * torch.as_tensor(s1, device=dev) + z2 * torch.as_tensor(s2, device=dev)
        x = torch.where(torch.as_tensor(masks[li], device=dev), z / (1 - p), torch.zeros_like(z))
        cache.append(torch.nn.functional.normalize(x, p=2, dim=1))
    ref = torch.cat(cache, 1)
    assert _scale_err(_np(out), _np(ref)) <= 1e-5
    (ref * R.double()).sum().backward()
    assert _scale_err(_np(emb.grad), _np(h.grad)) <= 1e-5
    for li, ((w1, w2), (W1, W2)) in enumerate(zip(pairs, Ws)):
        assert w1.grad is not None and _scale_err(_np(w1.grad), _np(W1.grad)) <= 1e-5, li
        assert w2.grad is not None and _scale_err(_np(w2.grad), _np(W2.grad)) <= 1e-5, li
    assert isinstance(model.layers[0], K.KGATConv)


def test_width_off_the_kernels_takes_the_fallback(dev):
    """Item 6."""
    from dgl_kgat_amd import ops
    model, g, n, trip = _setup(dev, dim=8, layers=1)
    assert not ops.aggregator_supported(ops.BI2_FORM, 8, 8)
    model.eval()
    assert not model._can_fuse_readout()
    with torch.no_grad():
        out = model.gnn(g)
    ref = _readout_ref64(model, g, n, trip)
    assert _scale_err(_np(out[:, :8]), ref[:, :8]) == 0.0
    assert _scale_err(_np(out[:, 8:]), ref[:, 8:]) <= 1e-5
    # under autograd: the per-layer path, gradients reach both weights and the embeddings
    model.train()
    loss = model.gnn(g).square().sum()
    loss.backward()
    layer = model.layers[0]
    assert layer.res_fc.weight.grad is not None and layer.res_fc_2.weight.grad is not None
    assert float(layer.res_fc.weight.grad.abs().sum()) > 0 and float(layer.res_fc_2.weight.grad.abs().sum()) > 0
    assert model.entity_embed.weight.grad is not None


def test_planted_structure_recall_rises_with_bi2(dev, tmp_path, capsys):
    """Item 7: end to end in a child process (the example's global switches stay there): recall@20 on the planted held-out
    interactions leaves a random ranking within three short epochs - the bar of test_planted_structure_recall_rises."""
    log = tmp_path / "train_Bi2.json"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_kgat.py"), "--planted", "--epochs", "3", "--lr", "0.03",
           "--batch_size", "512", "--batch_size_kg", "512", "--eval_before", "--seed", "1234", "--res_type", "Bi2",
           "--log_json", str(log)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(log) as f:
        hist = json.load(f)["epochs"]
    rec = [h["test_recall"] for h in hist]
    val = [h["valid_recall"] for h in hist]
    with capsys.disabled():
        print("\nBi2 planted-structure run: test recall@20 by epoch %s, valid %s" % (
            ["%.4f" % x for x in rec], ["%.4f" % x for x in val]))
    assert rec[3] > 3.0 * rec[0] and rec[3] > rec[2] > rec[1]
    assert val[3] > 3.0 * val[0]
