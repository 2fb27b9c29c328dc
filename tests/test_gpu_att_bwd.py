"""The backward of the attention logits (kgat_att_score_bwd_f32) and the differentiable attention built on it.

References are float64: torch-fp64 autograd of a restatement of ``_att_score`` + a per-destination softmax, computed on
the CPU from the SAME fp32 inputs as the device run.  Gate 1 (the project's "at most 10 x the CPU fp32 run" tripwire):
per tensor, the scale error max|got - ref64| / max|ref64| of the device result may be at most 10 times that of
torch-CPU fp32 autograd of the same restatement on the same inputs - the factor covers another summation order and
nothing else.  Both figures are printed before the assertion.  On top of it, inputs whose result is exact in fp32 (one
non-zero logit gradient; small integers with T = 0) are compared for equality: one dropped or doubled edge among 30,000
is invisible to a relative bar and shows there."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 6                      # relations the model scores; the graph also carries types R and R + 1
N = 2000
BOTH, HEADS, TAILS, NONE = (0, 900), (900, 1000), (1000, 1950), (1950, 2000)   # node roles by id range
BIG_HEAD, BIG_REL, BIG_COUNT = 17, 3, 300     # one (head, relation) group with more than 256 positions
PAIR, PAIR_REL = (1003, 5), 4                 # one edge repeated ten times
SINGLE_REL, EMPTY_REL, WIDE_REL = 2, 1, 0
WIDTHS = [16, 32, 64, 128]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _adversarial():
    rng = np.random.default_rng(77)
    tails = np.concatenate([np.arange(*BOTH), np.arange(*TAILS)])
    heads = np.concatenate([np.arange(*BOTH), np.arange(*HEADS)])
    parts = []

    def add(n, rel, src=None, dst=None):
        s = rng.choice(tails, n) if src is None else np.broadcast_to(src, n)
        d = rng.choice(heads, n) if dst is None else np.broadcast_to(dst, n)
        parts.append(np.stack([s, d, np.broadcast_to(rel, n)], 1))
    add(20000, WIDE_REL)                                    # thousands of groups: hundreds of tiles, many workgroups
    add(1, SINGLE_REL)
    add(BIG_COUNT, BIG_REL, src=rng.choice(tails, BIG_COUNT, replace=False), dst=BIG_HEAD)
    add(3000, BIG_REL)
    add(10, PAIR_REL, src=PAIR[0], dst=PAIR[1])
    add(3000, PAIR_REL)
    add(3000, 5)
    loops = rng.choice(np.arange(*BOTH), 40, replace=False)
    add(40, rng.choice([0, 3, 4, 5], 40), src=loops, dst=loops)
    add(500, rng.choice([R, R + 1], 500))                   # never scored
    e = np.concatenate(parts)
    e = e[rng.permutation(len(e))]
    return e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), e[:, 2].astype(np.int32)


GRAPH_SPECS = {
    "adversarial": (N, _adversarial),
    "empty": (5, lambda: (np.zeros(0, np.int32),) * 3),
    "single_edge": (3, lambda: (np.array([2], np.int32), np.array([0], np.int32), np.array([4], np.int32))),
}


class _Graph:
    def __init__(self, name, dev):
        from dgl_kgat_amd import synth
        self.n, make = GRAPH_SPECS[name]
        self.src, self.dst, self.et = make()
        self.e = len(self.src)
        trip = np.stack([self.dst, self.et, self.src], 1).astype(np.int32).reshape(-1, 3)   # [h, r, t]: t -> h
        self.g = synth.build_graph(self.n, trip, dev)
        self.dev = dev

    def statics(self):
        from dgl_kgat_amd.graph import att_bwd_statics
        st = self.g._st
        groups = st.rel_groups(self.g.edata["type"], R, self.dev)
        return st, groups, att_bwd_statics(groups, st.n_nodes)

    def backward(self, ent, W, rel, gamma_eid):
        """The operator on logit gradients given in edge-id order."""
        from dgl_kgat_amd import ops
        st, groups, s = self.statics()
        return ops.att_score_bwd(st.n_nodes, s.n_scored, groups.n_groups, groups.perm, groups.src_g, groups.gid, s.gstart,
                                 groups.gptr, groups.g_node, s.node_ptr, s.node_col, s.node_row, s.node_wsrc, ent, W, rel,
                                 gamma_eid)


@pytest.fixture(scope="module")
def graphs(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Graph(name, dev)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ references
def logits_ref(ent, W, rel, src, dst, et):
    """_att_score of models.py:135-144 per relation; edges of a type outside [0, R) keep the logit 0."""
    out = torch.zeros(len(src), dtype=ent.dtype)
    for r in range(R):
        idx = (et == r).nonzero().reshape(-1)
        if idx.numel():
            t_r, h_r = ent[src[idx]] @ W[r], ent[dst[idx]] @ W[r]
            out = out.index_add(0, idx, (t_r * torch.tanh(h_r + rel[r])).sum(-1))
    return out


def softmax_ref(logits, dst, n):
    m = torch.full((n,), -math.inf, dtype=logits.dtype).scatter_reduce(0, dst, logits.detach(), "amax")
    ex = torch.exp(logits - m[dst])
    return ex / torch.zeros(n, dtype=logits.dtype).index_add(0, dst, ex)[dst]


def _ids(G):
    return (torch.as_tensor(G.src.astype(np.int64)), torch.as_tensor(G.dst.astype(np.int64)),
            torch.as_tensor(G.et.astype(np.int64)))


def grads_ref(G, functional, params32, dtype):
    """torch-CPU autograd (`dtype`) of functional(params, src, dst, et) w.r.t. every entry of params32 (fp32 arrays)."""
    ps = [torch.as_tensor(p).to(dtype).requires_grad_(True) for p in params32]
    out = functional(ps, *_ids(G))
    return [g.double().numpy() for g in torch.autograd.grad(out, ps, allow_unused=False)]


def scale_err(got, ref64):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    m = np.abs(ref64).max()
    return float(np.abs(got - ref64).max() / m) if m > 0 else float(np.abs(got).max())


def gate1(what, names, got, cpu32, ref64, floor=0.0):
    figures = [(n, scale_err(g, r), max(scale_err(c, r), floor)) for n, g, c, r in zip(names, got, cpu32, ref64)]
    for n, e_dev, e_cpu in figures:
        print("%s %-16s device %.3e   cpu-fp32 %.3e   ratio %.2f" % (what, n, e_dev, e_cpu, e_dev / max(e_cpu, 1e-300)))
    for n, e_dev, e_cpu in figures:
        assert e_dev <= 10.0 * e_cpu, "%s %s: device %.3e > 10 x cpu-fp32 %.3e" % (what, n, e_dev, e_cpu)


def _inputs(n, d, seed):
    rng = np.random.default_rng(seed)
    return ((0.5 * rng.standard_normal((n, d))).astype(np.float32),
            (rng.standard_normal((R, d, d)) / math.sqrt(d)).astype(np.float32),
            (0.5 * rng.standard_normal((R, d))).astype(np.float32))


def _dev(arrs, dev):
    return [torch.as_tensor(a, device=dev) for a in arrs]


_OP_CACHE = {}


def op_case(G, d):
    """Inputs, logit gradients (edge-id order) and the two CPU references of the operator at width d, computed once."""
    key = (id(G), d)
    if key not in _OP_CACHE:
        params = _inputs(G.n, d, 100 + d)
        gamma = np.random.default_rng(200 + d).standard_normal(G.e).astype(np.float32)

        def functional(ps, src, dst, et):
            return (logits_ref(ps[0], ps[1], ps[2], src, dst, et) * torch.as_tensor(gamma).to(ps[0].dtype)).sum()
        _OP_CACHE[key] = (params, gamma, grads_ref(G, functional, params, torch.float64),
                          grads_ref(G, functional, params, torch.float32))
    return _OP_CACHE[key]


NAMES = ("grad_ent", "grad_W_R", "grad_rel")


# ------------------------------------------------------------------------------------------------ the graph
def test_graph_set_is_what_it_claims(graphs, dev):
    G = graphs("adversarial")
    assert G.n == N and 29000 <= G.e <= 31000
    cnt = np.bincount(G.et, minlength=R + 2)
    assert cnt[EMPTY_REL] == 0 and cnt[SINGLE_REL] == 1 and cnt[R] + cnt[R + 1] == 500 and cnt[R] and cnt[R + 1]
    assert np.sum((G.dst == BIG_HEAD) & (G.et == BIG_REL)) > 256
    assert np.sum((G.src == PAIR[0]) & (G.dst == PAIR[1]) & (G.et == PAIR_REL)) >= 10
    assert np.sum((G.src == G.dst) & (G.et < R)) >= 40
    out_deg, in_deg = np.bincount(G.src, minlength=N), np.bincount(G.dst, minlength=N)
    assert np.all(out_deg[slice(*NONE)] == 0) and np.all(in_deg[slice(*NONE)] == 0)
    assert np.all(in_deg[slice(*TAILS)] == 0) and np.all(out_deg[slice(*TAILS)] > 0)
    assert np.all(out_deg[slice(*HEADS)] == 0) and np.all(in_deg[slice(*HEADS)] > 0)
    # the wide relation: more than 16 groups per tile x several tiles per workgroup x several workgroups, so its
    # weight-gradient partials cross workgroups (the dense kernel gives a workgroup about four tiles on a small graph)
    st, groups, s = G.statics()
    gptr = groups.gptr.cpu().numpy()
    assert s.n_scored == G.e - 500 and groups.n_groups == gptr[R]
    wide_groups = gptr[WIDE_REL + 1] - gptr[WIDE_REL]
    assert wide_groups > 16 * 4 * 8
    assert gptr[EMPTY_REL + 1] == gptr[EMPTY_REL] and gptr[SINGLE_REL + 1] - gptr[SINGLE_REL] == 1
    assert graphs("empty").e == 0 and graphs("single_edge").e == 1


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("d", WIDTHS)
def test_operator_against_fp64(graphs, dev, d):
    G = graphs("adversarial")
    params, gamma, ref64, cpu32 = op_case(G, d)
    got = G.backward(*_dev(params, dev), torch.as_tensor(gamma, device=dev))
    assert [tuple(t.shape) for t in got] == [(N, d), (R, d, d), (R, d)]
    gate1("operator d=%d" % d, NAMES, got, cpu32, ref64)


@pytest.mark.parametrize("d", [16, 64])
def test_empty_and_single_edge_graphs(graphs, dev, d):
    G = graphs("empty")
    params = _inputs(G.n, d, 5)
    got = G.backward(*_dev(params, dev), torch.zeros(0, dtype=torch.float32, device=dev))
    assert all(not t.any() for t in got) and got[0].shape == (G.n, d)
    G = graphs("single_edge")
    params = _inputs(G.n, d, 6)
    gamma = np.array([1.5], np.float32)

    def functional(ps, src, dst, et):
        return (logits_ref(ps[0], ps[1], ps[2], src, dst, et) * 1.5).sum()
    ref64 = grads_ref(G, functional, params, torch.float64)
    got = G.backward(*_dev(params, dev), torch.as_tensor(gamma, device=dev))
    # gate 1; with so few terms the CPU's fp32 result can be exact to rounding, so its figure counts as no less than
    # u = 2^-24, half an ulp of the largest element (what a correctly rounded result is allowed)
    gate1("single edge d=%d" % d, NAMES, got, grads_ref(G, functional, params, torch.float32), ref64, floor=2.0 ** -24)
    g_ent, g_w, g_rel = [t.cpu().numpy() for t in got]
    assert not g_ent[1].any() and not np.delete(g_w, 4, 0).any() and not np.delete(g_rel, 4, 0).any()


# ------------------------------------------------------------------------------------------------ 2. exact structure
def test_one_nonzero_logit_gradient_touches_two_rows_and_one_relation(graphs, dev):
    G = graphs("adversarial")
    d = 64
    params = _inputs(N, d, 9)
    e0 = int(np.nonzero((G.et == 5) & (G.src != G.dst))[0][3])
    gamma = np.zeros(G.e, np.float32)
    gamma[e0] = 0.75
    g_ent, g_w, g_rel = [t.cpu().numpy() for t in G.backward(*_dev(params, dev), torch.as_tensor(gamma, device=dev))]
    rows = np.ones(N, bool)
    rows[[G.src[e0], G.dst[e0]]] = False
    assert not g_ent[rows].any() and g_ent[G.src[e0]].any() and g_ent[G.dst[e0]].any()
    assert not np.delete(g_w, 5, 0).any() and not np.delete(g_rel, 5, 0).any() and g_w[5].any() and g_rel[5].any()


def _counting_inputs(G, d):
    rng = np.random.default_rng(31)
    ent = rng.integers(-1, 2, (N, d)).astype(np.int64)
    ent[np.unique(G.dst)] = 0                                   # every head-role node: T = tanh(0 + 0) = 0
    W = (rng.integers(-1, 2, (R, d, d)) * (rng.random((R, d, d)) < 0.25)).astype(np.int64)
    gamma = rng.integers(-1, 2, G.e).astype(np.int64)
    return ent, W, np.zeros((R, d), np.int64), gamma


def test_counting_case_is_exact(graphs, dev):
    from dgl_kgat_amd import ops
    G = graphs("adversarial")
    d = 32
    ent, W, rel, gamma = _counting_inputs(G, d)
    assert ent[slice(*TAILS)].any() and np.abs(gamma[G.src >= TAILS[0]]).sum() > 5000
    # integer reference, with the sums of absolute values every partial sum is bounded by
    g_ent, g_rel, bound = np.zeros((N, d), np.int64), np.zeros((R, d), np.int64), 0
    for r in range(R):
        idx = np.nonzero(G.et == r)[0]
        A, A_abs = np.zeros((N, d), np.int64), np.zeros((N, d), np.int64)
        np.add.at(A, G.dst[idx], gamma[idx, None] * ent[G.src[idx]])
        np.add.at(A_abs, G.dst[idx], np.abs(gamma[idx, None] * ent[G.src[idx]]))
        dP, dP_abs = A @ W[r], A_abs @ np.abs(W[r])
        g_rel[r] = dP.sum(0)
        g_ent += dP @ W[r].T
        bound = max(bound, dP_abs.sum(0).max(), (dP_abs @ np.abs(W[r]).T).max() * R)
    assert bound < 2 ** 24 and np.abs(g_rel).max() > 100 and np.abs(g_ent).max() > 100
    dparams = _dev([ent.astype(np.float32), W.astype(np.float32), rel.astype(np.float32)], dev)
    # the forward's logits on this input are exactly 0 (T = 0, so V = W_r T = 0)
    st, groups, s = G.statics()
    logits = ops.att_score_split(st.n_nodes, groups.rel_ptr, groups.perm, groups.src_g, groups.pos_g, groups.gid, groups.gptr,
                                 groups.g_node, groups.n_groups, *dparams, want_csr=False, folded=True)[0]
    assert not logits.any()
    got = [t.cpu().numpy() for t in G.backward(*dparams, torch.as_tensor(gamma.astype(np.float32), device=dev))]
    assert np.array_equal(got[2], g_rel.astype(np.float32))
    assert np.array_equal(got[0], g_ent.astype(np.float32))      # head rows: the integers; every other row: 0
    assert not got[0][slice(*TAILS)].any() and not got[0][slice(*NONE)].any()
    assert not got[1].any()                                      # A^T (x) T and ent[h]^T (x) dP both vanish


def test_unscored_edges_change_no_bit(graphs, dev):
    G = graphs("adversarial")
    d = 64
    params, gamma, _, _ = op_case(G, d)
    dparams = _dev(params, dev)
    a = G.backward(*dparams, torch.as_tensor(gamma, device=dev))
    other = gamma.copy()
    other[G.et >= R] = 1e6 * (1.0 + np.arange(int(np.sum(G.et >= R)), dtype=np.float32))
    b = G.backward(*dparams, torch.as_tensor(other, device=dev))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize("d", WIDTHS)
def test_two_calls_give_the_same_bits(graphs, dev, d):
    G = graphs("adversarial")
    params, gamma, _, _ = op_case(G, d)
    dparams, dgamma = _dev(params, dev), torch.as_tensor(gamma, device=dev)
    a = G.backward(*dparams, dgamma)
    torch.empty(1 << 22, device=dev).fill_(float("nan"))   # (whatever the allocator hands out next is not zeros)
    b = G.backward(*dparams, dgamma)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 4. autograd
def _model(dev, d, n_layers=2, res_type="Bi", seed=0):
    import dgl_kgat_amd as K
    torch.manual_seed(seed)
    model = K.KGATPropagation(N, R, input_node_dim=d, relation_dim=d, num_gnn_layers=n_layers, n_hidden=d, dropout=0.0,
                              res_type=res_type)
    with torch.no_grad():   # (the default embedding initialisation saturates nothing, but keep the scales of test 1)
        model.entity_embed.weight.mul_(0.5)
        model.relation_embed.weight.mul_(0.5)
    return model.to(dev).train()


def test_differentiable_attention_values_and_gradients(graphs, dev):
    G = graphs("adversarial")
    model = _model(dev, 64)
    with torch.no_grad():
        plain = model.compute_attention(G.g)
        same = model.compute_attention(G.g, differentiable=True)
    assert type(same) is torch.Tensor and same.grad_fn is None and torch.equal(plain, same)
    w = model.compute_attention(G.g, differentiable=True)
    assert type(w) is torch.Tensor and w.grad_fn is not None and w.shape == (G.e, 1)
    assert torch.equal(w.detach(), model.compute_attention(G.g))     # the default, with gradients enabled: detached
    assert not model.compute_attention(G.g).requires_grad
    coef = np.random.default_rng(3).standard_normal(G.e).astype(np.float32)
    tensors = (model.entity_embed.weight, model.W_R, model.relation_embed.weight)
    got = torch.autograd.grad((w.reshape(-1) * torch.as_tensor(coef, device=dev)).sum(), tensors)

    def functional(ps, src, dst, et):
        a = softmax_ref(logits_ref(ps[0], ps[1], ps[2], src, dst, et), dst, N)
        return (a * torch.as_tensor(coef).to(a.dtype)).sum()
    params = [t.detach().cpu().numpy() for t in tensors]
    gate1("attention d=64", ("entity_embed", "W_R", "relation_embed"), got,
          grads_ref(G, functional, params, torch.float32), grads_ref(G, functional, params, torch.float64))


def test_only_the_requested_gradients_come_back(graphs, dev):
    from dgl_kgat_amd import autograd
    G = graphs("adversarial")
    ent, W, rel = _dev(_inputs(N, 32, 12), dev)
    rel.requires_grad_(True)
    seen = []
    orig = autograd._KGATAttention.backward

    def spy(ctx, grad):
        out = orig(ctx, grad)
        seen.append(out)
        return out
    autograd._KGATAttention.backward = staticmethod(spy)
    try:
        w = autograd.kgat_attention(G.g, ent, W, rel)
        w.square().sum().backward()
    finally:
        autograd._KGATAttention.backward = staticmethod(orig)
    assert len(seen) == 1 and seen[0][0] is None and seen[0][1] is None and seen[0][2] is not None
    assert all(x is None for x in seen[0][3:])
    assert ent.grad is None and W.grad is None and rel.grad is not None and rel.grad.abs().sum() > 0


def test_lazy_setting_does_not_reach_the_differentiable_result(graphs, dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd.lazy import LazyEdgeWeights
    G = graphs("adversarial")
    model = _model(dev, 16)
    prev = K.enable_lazy_edge_weights(True)
    try:
        assert isinstance(model.compute_attention(G.g), LazyEdgeWeights)
        w = model.compute_attention(G.g, differentiable=True)
        assert type(w) is torch.Tensor and w.grad_fn is not None
        with torch.no_grad():
            assert type(model.compute_attention(G.g, differentiable=True)) is torch.Tensor
    finally:
        K.enable_lazy_edge_weights(prev)


def test_unsupported_widths_take_the_torch_restatement(graphs, dev):
    """d = k = 8 is outside att_score_bwd_supported: same gradients to rounding from the restatement."""
    from dgl_kgat_amd import autograd, ops
    G = graphs("adversarial")
    assert not ops.att_score_bwd_supported(N, 8, 8, R)
    params = _inputs(N, 8, 14)
    tensors = [t.requires_grad_(True) for t in _dev(params, dev)]
    coef = np.random.default_rng(4).standard_normal(G.e).astype(np.float32)
    w = autograd.kgat_attention(G.g, *tensors)
    got = torch.autograd.grad((w.reshape(-1) * torch.as_tensor(coef, device=dev)).sum(), tensors)

    def functional(ps, src, dst, et):
        a = softmax_ref(logits_ref(ps[0], ps[1], ps[2], src, dst, et), dst, N)
        return (a * torch.as_tensor(coef).to(a.dtype)).sum()
    gate1("restatement d=8", ("ent", "W_R", "rel"), got, grads_ref(G, functional, params, torch.float32),
          grads_ref(G, functional, params, torch.float64))


# ------------------------------------------------------------------------------------------------ 5. end to end
def _layer_weight(layer, res_type):
    return layer.res_fc_2.weight if res_type == "Bi" else layer.res_fc.weight


@pytest.mark.parametrize("res_type", ["Bi", "GCN"])
def test_end_to_end_gradients(graphs, dev, res_type):
    G = graphs("adversarial")
    model = _model(dev, 16, n_layers=2, res_type=res_type, seed=5)
    rng = np.random.default_rng(8)
    u, p, n = (rng.integers(BOTH[0], BOTH[1], 512) for _ in range(3))
    ids = [torch.as_tensor(x.astype(np.int32), device=dev) for x in (u, p, n)]
    tensors = [model.entity_embed.weight, model.W_R, model.relation_embed.weight] + \
              [_layer_weight(layer, res_type) for layer in model.layers]
    names = ["entity_embed", "W_R", "relation_embed", "layer0", "layer1"]

    def device_grads(differentiable):
        model.zero_grad(set_to_none=True)
        g = G.g.local_var()
        g.edata["w"] = model.compute_attention(g, differentiable=differentiable)
        loss = model.get_loss(model.gnn(g, g.ndata["id"]), *ids)
        loss.backward()
        return [t.grad for t in tensors]
    got = device_grads(True)
    assert all(t is not None for t in got)
    lam = model._reg_lambda_gnn
    lu, lp, ln = (torch.as_tensor(x.astype(np.int64)) for x in (u, p, n))

    def functional(ps, src, dst, et):
        a = softmax_ref(logits_ref(ps[0], ps[1], ps[2], src, dst, et), dst, N)
        h = ps[0]
        outs = [h]
        for wl in ps[3:]:
            hn = torch.zeros_like(h).index_add(0, dst, a[:, None] * h[src])
            h = F.leaky_relu((h * hn if res_type == "Bi" else h + hn) @ wl.t(), 0.01)
            outs.append(F.normalize(h, p=2, dim=1))
        emb = torch.cat(outs, 1)
        s, pp, nn_ = emb[lu], emb[lp], emb[ln]
        cf = -F.logsigmoid((s * pp).sum(1) - (s * nn_).sum(1)).mean()
        return cf + lam * sum((v.pow(2).sum(1) / 2.0).mean() for v in (s, pp, nn_))
    params = [t.detach().cpu().numpy() for t in tensors]
    gate1("end to end %s" % res_type, names, got, grads_ref(G, functional, params, torch.float32),
          grads_ref(G, functional, params, torch.float64))
    plain = device_grads(False)
    assert plain[1] is None and plain[2] is None and plain[0] is not None and plain[3] is not None


def test_node_dropout_still_refuses_differentiable_weights(graphs, dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd.graph import DGLError
    G = graphs("adversarial")
    torch.manual_seed(0)
    model = K.KGATPropagation(N, R, input_node_dim=16, relation_dim=16, num_gnn_layers=1, n_hidden=16, dropout=0.0,
                              node_dropout=0.2).to(dev).train()
    g = G.g.local_var()
    g.edata["w"] = model.compute_attention(g, differentiable=True)
    with pytest.raises(DGLError):
        model.gnn(g, g.ndata["id"])


# ------------------------------------------------------------------------------------------------ 6. the example
def _train_kgat():
    spec = importlib.util.spec_from_file_location("_train_kgat_att_bwd", os.path.join(ROOT, "examples", "train_kgat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("attention_grad", [1, 0])
def test_example_trains_the_attention_only_when_asked(attention_grad):
    import dgl_kgat_amd as K
    tk = _train_kgat()
    before = K.enable_lazy_edge_weights(False)
    try:
        hist = tk.main(["--planted", "--epochs", "1", "--max_iters", "2", "--lr", "0.001", "--dropout_rate", "0.0",
                        "--attention_grad", str(attention_grad)])
    finally:
        after = K.enable_lazy_edge_weights(before)
    rec = hist[-1]
    assert math.isfinite(rec["kg_loss"]) and math.isfinite(rec["cf_loss"]) and rec["cf_iters"] == 2
    if attention_grad:
        assert rec["cf_W_R_change"] > 0
        assert after is False           # main() left the process-wide lazy setting as it found it
    else:
        assert rec["cf_W_R_change"] == 0
