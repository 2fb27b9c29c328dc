"""The TransE kernels (csrc/kgat_transe.hip) and the CFKG / CKE models on the device: loss and gradients against float64
under tests/_transr_ref's per-row metric and bar, the bits of the three training routes, the memory contract, link
prediction without a projection, and the two baselines end to end on the planted CKG."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import _kg_rank_ref as KR
import _transe_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SCALE = 2.5


def t32(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", [c.name for c in T.TRANSE_CASES])
def test_loss_and_gradients_against_float64(name):
    """Loss, grad_ent, grad_rel of the one call and of the two halves (grad_scale 2.5) against float64: a row passes
    within max(its floor, 2 x the CPU fp32 restatement's largest row error of that tensor); the two halves at
    grad_scale 1 have the bits of the one call.  Measured on MI355X, worst over the cases, error / bar (1 = the bar) -
    grad_ent 0.43 (4-xavier-N524289), grad_rel 0.46, both forms alike; the device's largest row
    error over the restatement's largest: grad_ent 0.45 .. 1.25, grad_rel 0.34 .. 1.48 (the printed lines of a run)."""
    from dgl_kgat_amd import ops
    c = next(c for c in T.TRANSE_CASES if c.name == name)
    batch, (ent, rel), ref, rs = T.transe_case_data(name)
    assert ops.transe_supported(c.N, c.d, c.R, c.B)
    ids = [t32(x) for x in batch]
    ent_d, rel_d = ent.to(DEV), rel.to(DEV)
    loss1, ge1, gr1 = ops.transe_loss_grad(*ids, ent_d, rel_d, T.REG_LAMBDA)
    loss2, ws = ops.transe_forward(*ids, ent_d, rel_d, T.REG_LAMBDA)
    ge_one, gr_one = ops.transe_backward(*ids, (ent.shape, rel.shape), ws, grad_scale=torch.ones(1, device=DEV))
    ge2, gr2 = ops.transe_backward(*ids, (ent.shape, rel.shape), ws, grad_scale=torch.full((1,), SCALE, device=DEV))
    assert _same_bits(loss1, loss2) and _same_bits(ge1, ge_one) and _same_bits(gr1, gr_one)
    floors = T.transe_floors(ref, c.d)
    err_rs = T.transe_errors(ref, (rs.grad_ent, rs.grad_rel))
    for tag, grads, scale in (("one call", (ge1, gr1), 1.0), ("halves x2.5", (ge2, gr2), SCALE)):
        err = T.transe_errors(ref, [g.cpu().numpy() for g in grads], scale)
        ratios = [T.bar_ratio(e, e_rs, f) for e, e_rs, f in zip(err, err_rs, floors)]
        vs_rs = [float(np.max(e) / max(np.max(e_rs), 1e-300)) for e, e_rs in zip(err, err_rs)]
        print("transe %s %s: error / bar grad_ent %.3f grad_rel %.3f; device / restatement %.2f %.2f; loss %.7f (fp64 %.7f)"
              % (name, tag, ratios[0], ratios[1], vs_rs[0], vs_rs[1], float(loss1), ref.loss))
        assert all(r <= 1.0 for r in ratios), (name, tag, ratios)
    assert T.loss_ok(float(loss1), rs.loss, ref.loss), (float(loss1), rs.loss, ref.loss)
    # rows outside the batch, relations without a sample: exactly zero
    assert not ge1[torch.as_tensor(ref.run_ent == 0, device=DEV)].any() and not gr1[torch.as_tensor(ref.run_rel == 0, device=DEV)].any()


def _phase_batches(c, n_it):
    cols = [np.stack(x) for x in zip(*[T.transr_batch(c.N, c.R, c.B, seed=40 + i, high_ids=c.high_ids) for i in range(n_it)])]
    if c.hub:
        cols[0][:, :300] = cols[0][:, :1]
    return [torch.as_tensor(x, device=DEV).to(torch.int32) for x in cols]


def _model(c, params):
    import dgl_kgat_amd as K
    m = K.CFKG(c.N, c.R, dim=c.d, reg_lambda_kg=T.REG_LAMBDA)
    with torch.no_grad():
        m.entity_embed.weight.copy_(params[0])
        m.relation_embed.weight.copy_(params[1])
    return m.to(DEV)


def _run_route(c, params, ids, route):
    import dgl_kgat_amd as K
    m = _model(c, params)
    fused_opt = route in ("phase", "steps")
    opt = K.FusedAdam(m.parameters(), lr=0.01) if fused_opt else torch.optim.Adam(m.parameters(), lr=0.01)
    n_it = ids[0].shape[0]
    if route == "phase":
        losses = m.kg_phase(*ids, opt)
    elif route == "steps":
        losses = torch.stack([m.kg_step(*(t[i] for t in ids), opt).clone() for i in range(n_it)])
    else:
        out = []
        for i in range(n_it):
            loss = m.transE(*(t[i] for t in ids))
            loss.backward()
            opt.step()
            opt.zero_grad()
            out.append(loss.detach().clone())
        losses = torch.stack(out)
    assert m.entity_embed.weight.grad is None and m.relation_embed.weight.grad is None
    state = []
    for p in (m.entity_embed.weight, m.relation_embed.weight):
        st = opt.state[p]
        assert int(st["step"]) == n_it
        state += [p.detach(), st["exp_avg"], st["exp_avg_sq"]]
    return [losses] + state


@pytest.mark.parametrize("name", [c.name for c in T.PHASE_CASES])
def test_three_routes_have_the_same_bits(name):
    """After four iterations: parameters, both moments, step counts and losses bit for bit equal between kg_phase (the
    fused iteration), a loop over kg_step with FusedAdam, and transE(...).backward(); torch.optim.Adam.step(); two runs
    of kg_phase bit-identical; ``.grad`` None on both parameters after every route."""
    c = next(c for c in T.TRANSE_CASES if c.name == name)
    _, params, _, _ = T.transe_case_data(name)
    ids = _phase_batches(c, 4)
    runs = {route: _run_route(c, params, ids, route) for route in ("phase", "steps", "autograd")}
    again = _run_route(c, params, ids, "phase")
    names = ("losses", "ent", "ent.exp_avg", "ent.exp_avg_sq", "rel", "rel.exp_avg", "rel.exp_avg_sq")
    assert torch.isfinite(runs["phase"][0]).all() and not torch.equal(runs["phase"][1].cpu(), params[0])
    for other, got in (("steps", runs["steps"]), ("autograd", runs["autograd"]), ("phase again", again)):
        for what, a, b in zip(names, runs["phase"], got):
            assert _same_bits(a, b), "%s: %s differs between kg_phase and %s" % (name, what, other)


def test_kg_phase_without_the_fused_route_leaves_grad_none_too():
    """The one ``.grad`` behaviour of CFKG on the routes the bits test does not take: torch.optim.Adam through kg_phase
    (the kg_step loop), and the torch restatement at a batch beyond the kernels' limit."""
    from dgl_kgat_amd import ops
    c = T.TRANSE_CASES[1]
    _, params, _, _ = T.transe_case_data(c.name)
    m = _model(c, params)
    ids = _phase_batches(c, 2)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    m.entity_embed.weight.grad = torch.ones_like(m.entity_embed.weight)
    losses = m.kg_phase(*ids, opt)
    assert losses.shape == (2,) and m.entity_embed.weight.grad is None and m.relation_embed.weight.grad is None
    big = [t.reshape(1, -1).repeat(1, 2) for t in ids]          # 2 x 2 x 1,200 = 4,800 samples: beyond 2,730
    assert not ops.transe_supported(c.N, c.d, c.R, big[0].shape[1])
    losses = m.kg_phase(*big, opt)
    assert losses.shape == (1,) and m.entity_embed.weight.grad is None and m.relation_embed.weight.grad is None


TRANSE_CONTRACT = [(900, 3, 5, 20), (3000, 41, 2730, 64)]      # (n, R, B, d): a small and the largest batch


@pytest.mark.parametrize("n, n_rel, B, d", TRANSE_CONTRACT)
def test_memory_contract(n, n_rel, B, d):
    """The three promises of include/kgat_hip.h for the new entries: scratch of exactly kgat_transe_scratch_bytes between
    guard bands, outputs fully overwritten, nothing read before it is written (poisoned scratch and outputs give the
    clean pass's bits).  Two consecutive fused steps on one state: the second step's tag must not take the first's words."""
    import test_gpu_memory_contract as mc
    from dgl_kgat_amd import ops
    dev = torch.device(DEV)
    rng = np.random.default_rng(60 + B)
    ids = [mc.t32(rng.integers(0, hi, (2, B)), dev) for hi in (n, n_rel, n, n)]
    ids[0][:, : B // 3] = 7                                        # a popular head: a long run of one row
    ent0, rel0 = mc.tf(rng.standard_normal((n, d)), dev), mc.tf(rng.standard_normal((n_rel, d)), dev)
    scale = mc.tf([0.37], dev)

    def run(alloc):
        h, r, pt, nt = (t[0] for t in ids)
        loss, ws = ops.transe_forward(h, r, pt, nt, ent0, rel0, 1e-3)
        g_ent, g_rel = ops.transe_backward(h, r, pt, nt, (ent0.shape, rel0.shape), ws, grad_scale=scale)
        one = ops.transe_loss_grad(h, r, pt, nt, ent0, rel0, 1e-3)
        out = dict(loss=loss.reshape(1), g_ent=g_ent, g_rel=g_rel, loss1=one[0].reshape(1), g_ent1=one[1], g_rel1=one[2])
        params = [ent0.clone(), rel0.clone()]
        m, v = [torch.zeros_like(t) for t in params], [torch.zeros_like(t) for t in params]
        state = ops.TransEAdamState(n, d, n_rel, B, dev)
        sorted_all, stride = ops.transe_presort(*ids, n, n_rel)
        arr_m, arr_v = (C.c_void_p * 2)(*[t.data_ptr() for t in m]), (C.c_void_p * 2)(*[t.data_ptr() for t in v])
        losses = alloc((2,), torch.float32)
        for i in range(2):
            ops.transe_adam_step(ids[0][i], ids[1][i], ids[2][i], ids[3][i], sorted_all[i * stride:(i + 1) * stride], *params,
                                 arr_m, arr_v, [i + 1] * 2, 1e-2, 0.9, 0.999, 1e-8, 1e-3, losses[i:i + 1], state)
        assert state.tag == 2
        out["losses"] = losses
        for nm, ts in (("p", params), ("m", m), ("v", v)):
            out.update({"%s%d" % (nm, i): t for i, t in enumerate(ts)})
        return out
    mc.check_contract("transe (%d, %d, %d, %d)" % (n, n_rel, B, d),
                      ["kgat_transe_forward_f32", "kgat_transe_backward_f32", "kgat_transe_loss_grad_f32",
                       "kgat_transe_presort_f32", "kgat_transe_adam_step_f32"], run, dev)


# ------------------------------------------------------------------------------------------------ link prediction
def _unit_dyadic(rng, n, d):
    """Rows with sixteen elements of +-1/4 (d >= 16): norm exactly 1, so normalize() leaves them as they are and every
    score n2 - 2 q.p is exact in fp32."""
    x = np.zeros((n, d))
    for i in range(n):
        x[i, rng.choice(d, 16, replace=False)] = rng.choice([-0.25, 0.25], 16)
    return x


def _cfkg_with(ent, rel):
    import dgl_kgat_amd as K
    m = K.CFKG(ent.shape[0], rel.shape[0], dim=ent.shape[1])
    with torch.no_grad():
        m.entity_embed.weight.copy_(torch.as_tensor(ent))
        m.relation_embed.weight.copy_(torch.as_tensor(rel))
    return m.to(DEV)


@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("d", [16, 64])
def test_kg_rank_without_projection_equals_brute_force_on_exact_arithmetic(d, side):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(70 + d)
    N, n_rel, n_q = 400, 3, 90
    ent, rel = _unit_dyadic(rng, N, d), _unit_dyadic(rng, n_rel, d)
    ent[5] = 0.0                                                    # a zero row: n2 = 0
    ent[300:320] = ent[17]                                          # ties with one true answer
    trip = np.stack([rng.integers(0, N, n_q), rng.integers(0, n_rel, n_q), rng.integers(0, N, n_q)], 1)
    trip[:6, 2 if side == "tail" else 0] = 17
    extra = np.stack([rng.integers(0, N, 600), rng.integers(0, n_rel, 600), rng.integers(0, N, 600)], 1)
    allt = np.concatenate([trip, extra])
    known = K.KnownTriples(allt[:, 0], allt[:, 1], allt[:, 2], N, n_rel, device=DEV)
    model = _cfkg_with(ent, rel)
    with ops.KernelTimer() as timer:
        got = model.kg_rank(trip[:, 0], trip[:, 1], trip[:, 2], known=known, side=side)
    torch.cuda.synchronize()
    seen = timer.summary()
    assert len(seen["transr_rank"]) == len(np.unique(trip[:, 1])) and "transr_project" not in seen     # the kernel counted
    sign = 1.0 if side == "tail" else -1.0
    anchor, answer = (trip[:, 0], trip[:, 2]) if side == "tail" else (trip[:, 2], trip[:, 0])
    Q = ent[anchor] + sign * rel[trip[:, 1]]
    S = (ent * ent).sum(1)[None, :] - 2.0 * (Q @ ent.T)             # float64 on dyadic values: exact
    exc = np.zeros(S.shape, bool)
    sets = {}
    for h, r, t in allt:
        key, val = ((h, r), t) if side == "tail" else ((t, r), h)
        sets.setdefault(key, set()).add(val)
    for j, (a, r) in enumerate(zip(anchor, trip[:, 1])):
        exc[j, list(sets[(a, r)])] = True
    lt, eq = KR.brute_counts(S, answer, exc)
    assert np.array_equal(got.lt.cpu().numpy(), lt) and np.array_equal(got.eq.cpu().numpy(), eq)
    assert eq[:6].min() >= 15                                       # the copies of row 17 tie


@pytest.mark.parametrize("side", ["tail", "head"])
def test_kg_rank_without_projection_lies_in_the_band(side):
    """Real-valued parameters, true answers placed at random among N = 300 entities: the counts lie inside the float64
    band of tests/_kg_rank_ref (tau from the fp32 restatement of the direct score, with W_r = I)."""
    import dgl_kgat_amd as K
    N, d, n_rel, n_q = 300, 64, 4, 120
    g = torch.Generator().manual_seed(71)
    ent, rel = torch.randn(N, d, generator=g), torch.randn(n_rel, d, generator=g)
    rng = np.random.default_rng(72)
    trip = np.stack([rng.integers(0, N, n_q), rng.integers(0, n_rel - 1, n_q), rng.integers(0, N, n_q)], 1)
    anchor, answer = (trip[:, 0], trip[:, 2]) if side == "tail" else (trip[:, 2], trip[:, 0])
    S64, worst, eye = np.empty((n_q, N)), 0.0, torch.eye(d, dtype=torch.float64)
    for r in np.unique(trip[:, 1]):
        sel = np.flatnonzero(trip[:, 1] == r)
        S64[sel] = KR.direct_scores(ent, eye, rel[r], anchor[sel], side, 0, N)
        s32 = KR.direct_scores(ent, eye, rel[r], anchor[sel], side, 0, N, dtype=torch.float32)
        worst = max(worst, float(np.abs(s32 - S64[sel]).max()))
    tau = max(KR.TAU_FLOOR, KR.FACTOR * worst)
    exc = np.zeros(S64.shape, bool)
    lt_lo, lt_hi = KR.band(S64, answer, exc, tau)
    case = types.SimpleNamespace(lt_lo=lt_lo, lt_hi=lt_hi, open_share=float((lt_lo != lt_hi).mean()))
    got = _cfkg_with(ent.numpy(), rel.numpy()).kg_rank(trip[:, 0], trip[:, 1], trip[:, 2], side=side)
    print("kg_rank CFKG %s: tau %.3e, band open for %.2f %%, median lt %d" % (side, tau, 100 * case.open_share,
                                                                               np.median(got.lt.cpu().numpy())))
    KR.check_band(case, got.lt.cpu().numpy(), got.eq.cpu().numpy())


def test_kg_phase_raises_the_filtered_mrr():
    """300 iterations of CFKG's KG phase on the planted CKG of the harness, interactions included: the filtered MRR of a
    fixed sample of training triples must rise (only the direction is asserted; measured 0.0146 -> 0.1530, MR 185.6 ->
    27.4, hits@10 0.021 -> 0.459)."""
    import dgl_kgat_amd as K
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    ds = K.CKGDataset(train_kgat.planted_data_dir(n_users=200, n_items=150, n_attrs=12, per_user=12, seed=5))
    trip = ds.train_KG_triplet.astype(np.int64)
    torch.manual_seed(0)
    model = K.CFKG(ds.n_KG_entity, ds.n_KG_relation, dim=32).to(DEV)
    opt = K.FusedAdam(model.parameters(), lr=0.01)
    rng = np.random.default_rng(0)
    sample = trip[rng.choice(len(trip), 256, replace=False)]
    known = K.KnownTriples(trip[:, 0], trip[:, 1], trip[:, 2], ds.n_KG_entity, ds.n_KG_relation, device=DEV)
    before = model.kg_metrics(sample[:, 0], sample[:, 1], sample[:, 2], known=known)
    n_it, bs = 300, 256
    idx = torch.as_tensor(rng.integers(0, len(trip), (n_it, bs)), device=DEV)
    cols = torch.as_tensor(trip, device=DEV).to(torch.int32)
    neg = torch.as_tensor(rng.integers(0, ds.n_KG_entity, (n_it, bs)), device=DEV).to(torch.int32)
    losses = model.kg_phase(cols[:, 0][idx], cols[:, 1][idx], cols[:, 2][idx], neg, opt)
    after = model.kg_metrics(sample[:, 0], sample[:, 1], sample[:, 2], known=known)
    print("CFKG filtered MRR of 256 training triples: %.4f -> %.4f (MR %.1f -> %.1f, hits@10 %.3f -> %.3f), loss %.4f -> %.4f"
          % (before["mrr"], after["mrr"], before["mr"], after["mr"], before["hits@10"], after["hits@10"],
             float(losses[0]), float(losses[-1])))
    assert after["mrr"] > before["mrr"]


# ------------------------------------------------------------------------------------------------ end to end
# the arguments of test_gpu_train_ops.test_planted_structure_recall_rises
PLANTED_ARGS = ["--planted", "--epochs", "3", "--lr", "0.03", "--batch_size", "512", "--batch_size_kg", "512", "--eval_before",
                "--seed", "1234"]


@pytest.mark.parametrize("model", ["cfkg", "cke"])
def test_planted_structure_recall_rises(model, capsys):
    """examples/train_kgat.py --model {cfkg, cke} --planted with the arguments of
    test_gpu_train_ops.test_planted_structure_recall_rises, under its criterion: untrained test recall@20 inside
    (0.005, 0.05) - a random ranking -, more than 3 x that after the last epoch, losses falling.  Measured on MI355X
    (test recall@20, untrained then per epoch) - cfkg: 0.0174 -> 0.0270, 0.0895, 0.3495 (KG loss 0.5795, 0.4387, 0.3596);
    cke: 0.0221 -> 0.2437, 0.4102, 0.4480 (CF loss 0.575, 0.347, 0.310; KG loss falling).  With nn.Embedding's N(0, 1) tables
    CKE stayed at 0.0200 -> 0.0192, 0.0237, 0.0319 (CF loss 6.11 -> 2.38): its tables are Xavier-initialised for that reason."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--model", model] + PLANTED_ARGS)
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\n--model %s planted-structure run: test recall@20 by epoch %s, valid %s, KG loss %s%s" % (
            model, ["%.4f" % r for r in rec], ["%.4f" % h["valid_recall"] for h in hist], ["%.4f" % h["kg_loss"] for h in hist[1:]],
            ", CF loss %s" % ["%.4f" % h["cf_loss"] for h in hist[1:]] if model == "cke" else ""))
    assert len(hist) == 4 and 0.005 < rec[0] < 0.05                # untrained: a random ranking
    assert rec[3] > 3.0 * rec[0]
    assert hist[3]["kg_loss"] < hist[1]["kg_loss"]
    if model == "cke":
        assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
