"""GraphSAGE (mean) on the MI355X: update_all(copy_src, sum | mean), the SAGE dense kernel, SAGEConv's forward and
its five gradients, the graphsage propagation stack (fused no-grad readout and the per-layer autograd path) and an
end-to-end training run.  References are float64 restatements of DGL 0.4.x SAGEConv inside this file."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _spmm_fwd_ref as fwd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _scale_err(x, y):
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y)) / max(np.abs(y).max(), 1e-30)) if y.size else 0.0


def _graph(n, src, dst, dev):
    import dgl_kgat_amd as K
    g = K.DGLGraph()
    g.add_nodes(n)
    g.add_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    g.readonly()
    g._st.csr(dev)
    return g


def _edges(kind, n, rng):
    """Edge lists with the shapes that stress the merge-path tiles."""
    if kind == "empty":
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "hub":   # a 10^5-edge destination among ordinary rows, a third of the rows without in-edges
        e = 60000
        dst = rng.integers(0, n, e)
        dst = dst[dst % 3 != 0]
        dst = np.concatenate([dst, np.full(100000, 7)])
        return rng.integers(0, n, dst.size), dst
    if kind == "runs":  # long runs: a few rows of thousands of edges, many of one or two, multi-edges
        dst = np.concatenate([np.repeat([1, 5, 9], [3000, 2500, 4100]), rng.integers(0, n, 20000)])
        src = rng.integers(0, n, dst.size)
        src[:50] = 3  # the same edge several times
        dst[:50] = 1
        return src, dst
    dst = rng.integers(0, n, 8 * n)
    return rng.integers(0, n, dst.size), dst


def _copy_reduce_ref(n, src, dst, X, reduce):
    X = np.asarray(X, np.float64)
    out = np.zeros((n, X.shape[1]))
    np.add.at(out, dst, X[src])
    if reduce == "mean":
        deg = np.bincount(dst, minlength=n).astype(np.float64)
        out /= np.maximum(deg, 1)[:, None]
    return out


@pytest.mark.parametrize("kind", ["random", "hub", "runs", "empty"])
@pytest.mark.parametrize("D", [8, 16, 20, 32, 64, 128])
def test_copy_reduce_matches_fp64_and_is_reproducible(dev, kind, D):
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(D * 7 + len(kind))
    n = 6000
    src, dst = _edges(kind, n, rng)
    g = _graph(n, src, dst, dev)
    csr = g._st.csr(dev)
    X = torch.randn(n, D, device=dev)
    Xh = X.cpu().numpy()
    for reduce in ("sum", "mean"):
        a = ops.copy_reduce(csr.indptr, csr.col, csr.row_of, X, reduce)
        b = ops.copy_reduce(csr.indptr, csr.col, csr.row_of, X, reduce)
        torch.cuda.synchronize()
        ref = _copy_reduce_ref(n, src, dst, Xh, reduce)
        assert torch.equal(a, b), (kind, D, reduce, "not bitwise reproducible")
        if src.size == 0:
            assert not a.any()
            continue
        assert _scale_err(a.cpu().numpy(), ref) <= 1e-6, (kind, D, reduce, _scale_err(a.cpu().numpy(), ref))
        deg = np.bincount(dst, minlength=n)
        # beside the tensor-scale bar: every row within gamma_{L+1} (sum) / gamma_{L+2} (mean: one division) of ITS sum
        # of |terms| (tests/_spmm_fwd_ref.py), so a wrong short row beside the hub row shows
        A = _copy_reduce_ref(n, src, dst, np.abs(Xh), reduce)
        fwd.check_gamma(a.cpu().numpy(), ref, A, deg, int(reduce == "mean"), "%s D=%d %s" % (kind, D, reduce))
        assert not a[torch.as_tensor(deg == 0, device=dev)].any()
        # a row range and its edge range (what a destination shard launches)
        ip = csr.indptr.cpu().numpy()
        for row0, nr in ((0, 1), (5, 1200), (1777, n - 1777)):
            sub = ops.copy_reduce(csr.indptr, csr.col, csr.row_of, X, reduce, rows=(row0, nr),
                                  e_range=(int(ip[row0]), int(ip[row0 + nr])))
            err = float(np.abs(sub.cpu().numpy() - ref[row0:row0 + nr]).max()) / max(np.abs(ref).max(), 1e-30)
            assert err <= 1e-6, (kind, D, reduce, row0, err)
            fwd.check_gamma(sub.cpu().numpy(), ref[row0:row0 + nr], A[row0:row0 + nr], deg[row0:row0 + nr],
                            int(reduce == "mean"), "%s D=%d %s rows [%d, +%d)" % (kind, D, reduce, row0, nr))


def test_update_all_copy_src_mean_and_its_backward(dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import function as fn
    rng = np.random.default_rng(3)
    n = 3000
    src, dst = _edges("runs", n, rng)
    g = _graph(n, src, dst, dev)
    x = torch.randn(n, 24, device=dev, requires_grad=True)
    for reduce, red in (("mean", fn.mean), ("sum", fn.sum)):
        gl = g.local_var()
        gl.srcdata["h"] = x
        gl.update_all(fn.copy_u("h", "m"), red("m", "o"))
        out = gl.dstdata["o"]
        gout = torch.randn_like(out)
        (gx,) = torch.autograd.grad(out, x, gout)
        xd = x.detach().double().cpu().requires_grad_(True)
        s, d = torch.as_tensor(src), torch.as_tensor(dst)
        ref = torch.zeros(n, 24, dtype=torch.float64).index_add_(0, d, xd[s])
        if reduce == "mean":
            ref = ref / torch.bincount(d, minlength=n).clamp(min=1).double()[:, None]
        (gref,) = torch.autograd.grad(ref, xd, gout.double().cpu())
        assert _scale_err(out.detach().cpu(), ref.detach()) <= 1e-6
        assert _scale_err(gx.cpu(), gref) <= 1e-6
    with pytest.raises(NotImplementedError):
        gl.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"), apply_node_func=lambda nodes: nodes)
    assert isinstance(K.SAGEConv(24, 16, "mean"), nn.Module)


WIDTHS = (16, 32, 64, 128)


@pytest.mark.parametrize("act", [None, "relu"])
def test_sage_dense_every_width(dev, act):
    from dgl_kgat_amd import ops
    n = 2000 + 13
    torch.manual_seed(5)
    for d_in in WIDTHS:
        for d_out in WIDTHS:
            H, HN = torch.randn(n, d_in, device=dev), torch.randn(n, d_in, device=dev)
            Ws, Wn = torch.randn(d_out, d_in, device=dev) / d_in ** 0.5, torch.randn(d_out, d_in, device=dev) / d_in ** 0.5
            bs, bn = torch.randn(d_out, device=dev), torch.randn(d_out, device=dev)
            buf = torch.zeros(n, d_in + d_out + 4, device=dev)
            z = ops.sage_dense(H, HN, Ws, Wn, bs, bn, act, norm_out=buf[:, d_in:d_in + d_out], self_out=buf[:, :d_in])
            pre = (H.double() @ Ws.double().T + HN.double() @ Wn.double().T + bs.double() + bn.double())
            ref = pre.clamp(min=0) if act == "relu" else pre
            assert _scale_err(z.cpu(), ref.cpu()) <= 1e-5, (d_in, d_out, act)
            assert _scale_err(buf[:, d_in:d_in + d_out].cpu(), F.normalize(ref, dim=1).cpu()) <= 1e-5
            assert torch.equal(buf[:, :d_in], H) and not buf[:, d_in + d_out:].any()


def test_sageconv_fallback_width_goes_through_linear(dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    assert not ops.sage_dense_supported(20, 12)
    rng = np.random.default_rng(11)
    n = 2500
    src, dst = _edges("hub", n, rng)
    g = _graph(n, src, dst, dev)
    torch.manual_seed(2)
    conv = K.SAGEConv(20, 12, "mean", activation=torch.relu).to(dev)
    x = torch.randn(n, 20, device=dev)
    out = conv(g, x)
    p = {k: v.double().cpu() for k, v in conv.state_dict().items()}
    hn = torch.as_tensor(_copy_reduce_ref(n, src, dst, x.cpu().numpy(), "mean"))
    ref = torch.relu(x.double().cpu() @ p["fc_self.weight"].T + p["fc_self.bias"] + hn @ p["fc_neigh.weight"].T +
                     p["fc_neigh.bias"])
    assert _scale_err(out.detach().cpu(), ref) <= 1e-5


def _sage_ref64(n, src, dst, h, Ws, bs, Wn, bn, mask, p, act):
    """float64 torch restatement of DGL 0.4.x SAGEConv(mean) with the given dropout mask."""
    hd = h * mask / (1.0 - p) if p > 0 else h
    s, d = torch.as_tensor(src), torch.as_tensor(dst)
    hn = torch.zeros_like(hd).index_add_(0, d, hd[s]) / torch.bincount(d, minlength=n).clamp(min=1).double()[:, None]
    rst = hd @ Ws.T + bs + hn @ Wn.T + bn
    return torch.relu(rst) if act else rst


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("d_in,d_out,act", [(64, 64, True), (64, 32, True), (32, 16, False), (20, 12, True)])
def test_sageconv_forward_and_gradients(dev, p, d_in, d_out, act):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(d_in + d_out)
    n = 4000
    src, dst = _edges("hub", n, rng)
    g = _graph(n, src, dst, dev)
    torch.manual_seed(7)
    conv = K.SAGEConv(d_in, d_out, "mean", feat_drop=p, activation=F.relu if act else None).to(dev).train()
    h = torch.randn(n, d_in, device=dev, requires_grad=True)
    seed = 987654321
    out = conv(g, h, seed=seed)
    gout = torch.randn_like(out)
    params = [h, conv.fc_self.weight, conv.fc_neigh.weight, conv.fc_self.bias, conv.fc_neigh.bias]
    grads = torch.autograd.grad(out, params, gout)
    mask = torch.as_tensor(ops.dropout_keep_mask(seed, n, d_in, p)).double()
    ref_in = [t.detach().double().cpu().requires_grad_(True) for t in params]
    ref = _sage_ref64(n, src, dst, ref_in[0], ref_in[1], ref_in[3], ref_in[2], ref_in[4], mask, p, act)
    ref_grads = torch.autograd.grad(ref, ref_in, gout.double().cpu())
    assert _scale_err(out.detach().cpu(), ref.detach()) <= 1e-5, (p, d_in, d_out)
    for name, a, b in zip(("h", "W_self", "W_neigh", "b_self", "b_neigh"), grads, ref_grads):
        assert _scale_err(a.cpu(), b) <= 1e-5, (name, p, d_in, d_out, _scale_err(a.cpu(), b))


def _stack_ref64(g_src, g_dst, n, model):
    """The readout [h0 | normalize(h1) | ...] of a graphsage stack in float64 on the device (no dropout)."""
    s, d = g_src, g_dst
    deg = torch.bincount(d, minlength=n).clamp(min=1).double()[:, None]
    h = model.entity_embed.weight.detach().double()
    cache = [h]
    for layer in model.layers:
        W = {k: v.detach().double() for k, v in layer.state_dict().items()}
        hn = torch.zeros_like(h).index_add_(0, d, h[s]) / deg
        h = h @ W["fc_self.weight"].T + W["fc_self.bias"] + hn @ W["fc_neigh.weight"].T + W["fc_neigh.bias"]
        if layer.activation is not None:
            h = torch.relu(h)
        cache.append(F.normalize(h, dim=1))
    return torch.cat(cache, 1)


def test_graphsage_stack_full_size(dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth
    from conftest import blocks_rel_err_inf
    n, trip, R = synth.amazon_book_ckg(scale=1.0)
    torch.manual_seed(3)
    m = K.KGATPropagation(n, R, 64, 64, 3, 64, dropout=0.1, gnn_model="graphsage").to(dev).eval()
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        fused = m.gnn(g)
        per_layer = m.gnn(g, fused=False)
    torch.cuda.synchronize()
    widths = [64, 64, 32, 16]
    assert fused.shape == (n, 176)
    assert float((fused - per_layer).abs().max()) <= 1e-6
    src = torch.as_tensor(trip[:, 2], device=dev)
    dst = torch.as_tensor(trip[:, 0], device=dev)
    ref = _stack_ref64(src, dst, n, m)
    deg = torch.bincount(dst, minlength=n)
    hubs = torch.topk(deg, 32).indices
    rows = torch.cat([hubs, torch.randint(0, n, (4000,), device=dev), torch.nonzero(deg == 0)[:32, 0]])
    x, y = fused[rows].double().cpu().numpy(), ref[rows].cpu().numpy()
    assert blocks_rel_err_inf(x, y, widths) <= 1e-5
    assert torch.equal(fused[:, :64], m.entity_embed.weight)


def test_accelerate_reference_shaped_graphsage_model(dev):
    """compat.accelerate on a model with the reference Model's layout and its graphsage layers (a paraphrase of
    models.py:72-111,135-168): the routed gnn gives the model's own loop's readout, training gives finite gradients."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth

    class RefModel(nn.Module):
        def __init__(self, n, R, d):
            super().__init__()
            self._use_KG, self._n_entities, self._n_relations = True, n, R
            self.entity_embed, self.relation_embed = nn.Embedding(n, d), nn.Embedding(R, d)
            self.W_R = nn.Parameter(torch.empty(R, d, d))
            nn.init.xavier_uniform_(self.W_R, gain=nn.init.calculate_gain("relu"))
            self.layers = nn.ModuleList([K.SAGEConv(d, d, aggregator_type="mean", feat_drop=0.1, activation=F.relu),
                                         K.SAGEConv(d, d // 2, aggregator_type="mean", feat_drop=0.1, activation=F.relu),
                                         K.SAGEConv(d // 2, d // 4, aggregator_type="mean", feat_drop=0.1,
                                                    activation=None)])

        def compute_attention(self, g):
            return K.edge_softmax(g, torch.zeros(g.number_of_edges(), 1, device=self.W_R.device))

        def gnn(self, g, x):
            g = g.local_var()
            h = self.entity_embed(g.ndata["id"])
            cache = [h]
            for layer in self.layers:
                h = layer(g, h)
                cache.append(F.normalize(h, p=2, dim=1))
            return torch.cat(cache, 1)

    n, trip, R = synth.amazon_book_ckg(scale=0.02)
    torch.manual_seed(4)
    m = RefModel(n, R, 32).to(dev).eval()
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        own = m.gnn(g, None)
    assert K.accelerate(m) is m
    with torch.no_grad():
        g.edata["w"] = m.compute_attention(g)
        routed = m.gnn(g, None)
    assert float((own - routed).abs().max()) <= 1e-6
    m.train()
    out = m.gnn(g, None)
    loss = (out[:100] * out[100:200]).sum()
    loss.backward()
    for name, p_ in m.named_parameters():
        if name in ("W_R", "relation_embed.weight"):
            continue
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), name
    assert float(m.layers[0].fc_self.weight.grad.abs().sum()) > 0


def test_planted_structure_recall_rises_graphsage(dev, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--planted", "--gnn_model", "graphsage", "--epochs", "3", "--lr", "0.03", "--batch_size",
                            "512", "--batch_size_kg", "512", "--eval_before", "--seed", "1234"])
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\ngraphsage planted-structure run: test recall@20 by epoch %s, CF loss %s" % (
            ["%.4f" % r for r in rec], ["%.3f" % h["cf_loss"] for h in hist[1:]]))
    assert rec[3] > 3.0 * rec[0]
    assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
