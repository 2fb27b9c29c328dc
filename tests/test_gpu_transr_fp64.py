"""The TransR and BPR training kernels (kgat_transr.hip, kgat_bpr.hip) against float64 under a per-row metric.

Reference, metric, bars, batch builders and the list of cases: tests/_transr_ref.py (checked without a GPU by
tests/test_transr_ref_host.py).  The restatement of the bars is ``transr_ref(..., dtype=torch.float32)`` /
``bpr_ref(..., dtype=torch.float32)`` on the CPU, never one of the fused kernels.  A row passes when its error is within
max(its floor, 2 x the restatement's largest row error of that tensor).

Measured on an MI355X when the test was written (largest row error of the device / of the restatement, the larger of
the one-call form and forward + backward x 2.5; loss: |L - L64| / |L64|; last column: the worst row's error as a fraction
of its bar, over both forms).  Cases are named by width; N = 700, R = 9, B = 1,200, Xavier-like values unless stated:

    case                         loss                grad_ent            grad_W              grad_rel            worst/bar
    4x4                          4.6e-09 / 4.6e-09   7.4e-07 / 8.8e-07   2.3e-07 / 1.8e-07   2.8e-07 / 1.4e-07   0.42
    8x8                          2.5e-08 / 2.5e-08   4.8e-07 / 7.2e-07   1.4e-07 / 1.5e-07   1.6e-07 / 1.2e-07   0.28
    20x12                        1.8e-08 / 1.8e-08   3.5e-07 / 3.9e-07   1.3e-07 / 2.3e-07   2.0e-07 / 3.0e-07   0.15
    12x20                        1.1e-07 / 2.9e-08   3.5e-07 / 3.5e-07   1.9e-07 / 2.5e-07   1.8e-07 / 2.0e-07   0.13
    64x64                        7.4e-08 / 7.4e-08   4.1e-07 / 4.3e-07   1.8e-07 / 1.9e-07   3.0e-07 / 3.0e-07   0.07
    16x48                        3.7e-08 / 3.7e-08   4.8e-07 / 3.6e-07   2.1e-07 / 2.3e-07   2.0e-07 / 2.7e-07   0.10
    48x16                        4.5e-08 / 2.7e-08   5.4e-07 / 4.6e-07   1.9e-07 / 1.6e-07   2.2e-07 / 2.8e-07   0.15
    68x36                        9.6e-09 / 6.6e-08   3.9e-07 / 3.8e-07   2.2e-07 / 2.5e-07   2.2e-07 / 2.9e-07   0.08
    100x60                       4.7e-08 / 4.7e-08   5.7e-07 / 4.2e-07   2.0e-07 / 2.2e-07   2.9e-07 / 3.9e-07   0.07
    128x4                        9.2e-08 / 1.7e-08   1.4e-06 / 8.8e-07   2.9e-07 / 4.5e-07   3.6e-07 / 2.7e-07   0.44
    4x128                        9.3e-09 / 1.2e-07   3.8e-07 / 4.8e-07   1.4e-07 / 1.8e-07   1.4e-07 / 1.7e-07   0.04
    64x128                       7.3e-08 / 5.7e-09   5.4e-07 / 4.1e-07   2.3e-07 / 3.4e-07   2.6e-07 / 2.2e-07   0.04
    128x64                       2.5e-08 / 2.5e-08   4.4e-07 / 5.2e-07   2.2e-07 / 2.9e-07   3.5e-07 / 3.8e-07   0.08
    80x48                        4.2e-08 / 4.2e-08   3.9e-07 / 4.4e-07   3.0e-07 / 4.1e-07   2.5e-07 / 4.3e-07   0.07
    128x128                      3.3e-08 / 4.8e-08   4.7e-07 / 4.6e-07   2.2e-07 / 2.5e-07   3.8e-07 / 3.7e-07   0.05
    64x64-scaled                 7.4e-08 / 7.4e-08   4.1e-07 / 4.3e-07   1.8e-07 / 1.9e-07   3.0e-07 / 3.0e-07   0.07
    20x12-scaled                 1.8e-08 / 1.8e-08   3.5e-07 / 3.9e-07   1.3e-07 / 2.3e-07   2.0e-07 / 3.0e-07   0.15
    80x48-scaled                 4.2e-08 / 4.2e-08   3.9e-07 / 4.4e-07   3.0e-07 / 4.1e-07   2.5e-07 / 4.3e-07   0.07
    64x64-zeros                  1.7e-08 / 1.7e-08   4.1e-07 / 4.3e-07   2.1e-07 / 3.3e-07   3.0e-07 / 3.0e-07   0.07
    20x12-zeros                  4.6e-08 / 2.1e-08   3.2e-07 / 3.7e-07   1.3e-07 / 2.3e-07   2.0e-07 / 2.6e-07   0.14
    80x48-zeros                  4.0e-08 / 3.7e-08   4.4e-07 / 4.4e-07   2.6e-07 / 2.4e-07   4.4e-07 / 3.2e-07   0.13
    8x8-B1                       2.7e-07 / 2.7e-07   4.4e-07 / 5.4e-07   2.7e-07 / 3.5e-07   1.3e-07 / 1.5e-07   0.30
    8x8-B2                       5.7e-08 / 5.7e-08   4.1e-07 / 2.4e-07   2.8e-07 / 2.0e-07   4.2e-07 / 4.2e-07   0.42
    8x8-B3                       1.6e-07 / 3.2e-07   5.9e-07 / 5.9e-07   5.5e-07 / 2.8e-07   5.6e-07 / 3.8e-07   0.56
    8x8-B4                       6.5e-08 / 1.3e-07   3.4e-07 / 4.0e-07   2.6e-07 / 3.2e-07   2.2e-07 / 3.9e-07   0.22
    8x8-B5                       3.2e-08 / 8.2e-08   4.0e-07 / 6.2e-07   2.1e-07 / 3.6e-07   2.5e-07 / 5.8e-07   0.27
    8x8-B2730                    2.7e-08 / 8.7e-08   4.6e-07 / 4.6e-07   1.3e-07 / 1.7e-07   2.9e-07 / 2.5e-07   0.31
    64x64-B1                     1.3e-07 / 1.3e-07   3.4e-07 / 2.5e-07   1.4e-07 / 2.6e-07   3.0e-07 / 1.8e-07   0.07
    64x64-B2                     5.4e-08 / 1.1e-07   4.9e-07 / 1.7e-07   3.1e-07 / 2.6e-07   3.5e-07 / 3.5e-07   0.08
    64x64-B3                     6.1e-08 / 7.5e-08   4.6e-07 / 3.5e-07   2.9e-07 / 2.3e-07   5.3e-07 / 2.7e-07   0.12
    64x64-B4                     8.3e-08 / 1.5e-07   3.2e-07 / 3.3e-07   1.8e-07 / 1.9e-07   2.4e-07 / 4.1e-07   0.05
    64x64-B5                     4.7e-08 / 1.7e-08   6.1e-07 / 4.3e-07   4.6e-07 / 2.0e-07   5.9e-07 / 2.5e-07   0.14
    64x64-B2730                  1.9e-09 / 8.1e-08   2.9e-07 / 3.2e-07   2.4e-07 / 2.1e-07   4.7e-07 / 4.7e-07   0.11
    8x8-R1                       1.2e-07 / 1.2e-07   5.9e-07 / 6.1e-07   2.9e-08 / 8.7e-08   2.6e-08 / 8.5e-08   0.32
    64x64-R1                     4.2e-08 / 1.2e-07   4.6e-07 / 4.9e-07   2.2e-08 / 9.3e-08   3.3e-08 / 1.1e-07   0.06
    8x8-R1025-B300               4.2e-08 / 8.5e-08   7.3e-07 / 8.3e-07   6.2e-07 / 7.0e-07   7.0e-07 / 8.0e-07   0.45
    8x8-R4096-B300               1.4e-08 / 1.4e-08   6.9e-07 / 7.8e-07   1.2e-06 / 7.9e-07   1.1e-06 / 1.1e-06   0.74
    4x4-N524288                  8.4e-09 / 8.4e-09   9.5e-07 / 1.0e-06   2.4e-07 / 1.6e-07   2.9e-07 / 3.5e-07   0.46
    4x4-N524289                  7.0e-08 / 4.0e-08   7.2e-07 / 7.3e-07   3.2e-07 / 5.0e-07   1.5e-07 / 5.6e-07   0.49
    bpr-N700-F16-B1365           9.8e-09 / 9.8e-09   9.8e-07 / 7.7e-07                                                          0.63
    bpr-N700-F16-B1366           9.2e-08 / 1.1e-08   4.6e-07 / 8.9e-07                                                          0.26
    bpr-N700-F176-B4000          3.6e-08 / 3.6e-08   7.4e-07 / 9.3e-07                                                          0.40
    worst ratio to the bar per tensor class: grad_ent 0.49, grad_W 0.74, grad_rel 0.56, grad 0.63

The device sits where an honest fp32 run sits at every width and in every regime.  What the cases did expose: at
R = 4,096 (the largest relation count the kernels take) grad_W and grad_rel were garbage (row errors of 1e+1 and 1e+23):
the chunk table is built four keys per thread by 1,024 threads, and its total, chunk_ptr[n_rel], was left to a thread
whose first key is n_rel - none at 4,096.  Fixed in small_sort_body (kgat_transr.hip); the row above is after the fix.
"""
import numpy as np
import pytest
import torch

import _transr_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _report(name, what, tensors, errs_dev, errs_rs, floors):
    ratios = []
    for tensor, e, s, fl in zip(tensors, errs_dev, errs_rs, floors):
        ratio = T.bar_ratio(e, s, fl)
        ratios.append(ratio)
        print("[fp64] %-30s %-9s %-8s device %.3e  restatement %.3e  floor(max) %.3e  worst row / bar %.3f"
              % (name, what, tensor, e.max(), s.max(), np.max(fl), ratio))
    return ratios


TENSORS = ("grad_ent", "grad_W", "grad_rel")


@pytest.mark.parametrize("name", [c.name for c in T.TRANSR_CASES])
def test_transr_kernels_against_float64(dev, name):
    """transr_loss_grad, its loss-only form, and transr_forward + transr_backward (upstream gradient 2.5): loss and the
    three gradients against float64 per row, exact zeros where nothing is added, the same bits on a second call."""
    from dgl_kgat_amd import ops
    c = next(c for c in T.TRANSR_CASES if c.name == name)
    batch, params, ref, rs = T.transr_case_data(name)
    assert ops.transr_supported(c.N, c.d, c.k, c.R, c.B)
    ids = [torch.as_tensor(t, dtype=torch.int32, device=dev) for t in batch]
    ent, W, rel = (p.to(dev) for p in params)
    floors = T.floors(ref, c.d, c.k)
    failures = []

    # 1. loss + gradients in one call
    out = ops.transr_loss_grad(*ids, ent, W, rel, T.REG_LAMBDA)
    again = ops.transr_loss_grad(*ids, ent, W, rel, T.REG_LAMBDA)
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    loss = float(out[0])
    grads = [g.double().cpu().numpy() for g in out[1:]]
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
    print("[fp64] %-30s loss      device %.3e  restatement %.3e  (relative to |L64|)"
          % (name, abs(loss - ref.loss) / abs(ref.loss), abs(rs.loss - ref.loss) / abs(ref.loss)))
    if not T.loss_ok(loss, rs.loss, ref.loss):
        failures.append(("loss", loss, ref.loss))
    ratios = _report(name, "loss_grad", TENSORS, T.transr_errors(ref, grads),
                     T.transr_errors(ref, (rs.grad_ent, rs.grad_W, rs.grad_rel)), floors)
    failures += [("loss_grad", t, r) for t, r in zip(TENSORS, ratios) if not r <= 1.0]

    # 2. the loss-only entry
    only = ops.transr_loss_grad(*ids, ent, W, rel, T.REG_LAMBDA, want_grad=False)
    assert only[1] is None and torch.equal(only[0], out[0])

    # 3. forward, then backward with the gradient that arrives at the loss
    f_loss, ws = ops.transr_forward(*ids, ent, W, rel, T.REG_LAMBDA)
    assert torch.equal(f_loss, out[0])
    scale = 2.5
    back = ops.transr_backward(*ids, ((c.N, c.d), (c.R, c.d, c.k)), ws,
                               grad_scale=torch.tensor(scale, dtype=torch.float32, device=dev))
    grads_b = [g.double().cpu().numpy() for g in back]
    rs_scaled = [(torch.as_tensor(g, dtype=torch.float32) * scale).double().numpy()
                 for g in (rs.grad_ent, rs.grad_W, rs.grad_rel)]
    ratios = _report(name, "fwd+bwd", TENSORS, T.transr_errors(ref, grads_b, scale),
                     T.transr_errors(ref, rs_scaled, scale), floors)
    failures += [("fwd+bwd", t, r) for t, r in zip(TENSORS, ratios) if not r <= 1.0]
    assert not failures, failures


@pytest.mark.parametrize("name", [c.name for c in T.PHASE_CASES])
def test_kg_phase_same_bits_as_kg_step_at_every_width(dev, name):
    """kg_phase (split MFMA partials, gradient rows and partials summed inside the Adam launch) and a loop over
    kg_step, both with FusedAdam, three iterations on the builder's batch and two shuffles of it: the same parameters,
    moments and losses bit for bit - which carries the float64 verdict on transr_loss_grad over to the phase form."""
    import dgl_kgat_amd as K
    c = next(c for c in T.TRANSR_CASES if c.name == name)
    batch, params, _, _ = T.transr_case_data(name)
    rng = np.random.default_rng(5)
    perms = [np.arange(c.B), rng.permutation(c.B), rng.permutation(c.B)]
    ids = [torch.as_tensor(np.stack([t[p] for p in perms]), dtype=torch.int32, device=dev) for t in batch]
    results = []
    for mode in ("phase", "steps"):
        m = K.KGATPropagation(c.N, c.R, c.d, c.k, 1, 8, dropout=0.0).to(dev)
        kg = (m.entity_embed.weight, m.W_R, m.relation_embed.weight)
        with torch.no_grad():
            for p, v in zip(kg, params):
                p.copy_(v)
        opt = K.FusedAdam(m.parameters(), lr=0.01)
        if mode == "phase":
            losses = m.kg_phase(*ids, opt, reg_lambda_kg=T.REG_LAMBDA).tolist()
        else:
            losses = [float(m.kg_step(ids[0][i], ids[1][i], ids[2][i], ids[3][i], opt, reg_lambda_kg=T.REG_LAMBDA))
                      for i in range(len(perms))]
        results.append((losses, [p.detach().clone() for p in kg], [opt.state[p]["exp_avg"].clone() for p in kg],
                        [opt.state[p]["exp_avg_sq"].clone() for p in kg], [float(opt.state[p]["step"]) for p in kg]))
    a, b = results
    assert a[0] == b[0] and np.isfinite(a[0]).all(), (a[0], b[0])
    assert a[4] == b[4] == [3.0, 3.0, 3.0]
    for la, lb in zip(a[1:4], b[1:4]):
        for x, y in zip(la, lb):
            assert torch.equal(x, y)


@pytest.mark.parametrize("n,F_,B,structured", T.BPR_CASES)
def test_bpr_kernels_against_float64_per_row(dev, n, F_, B, structured):
    """kgat_bpr_loss_f32 + kgat_bpr_grad_f32 with an upstream gradient of 2.5 against float64: per row, relative to
    the accumulated magnitude of the row's contributions, floor (run + 8) U; exact zeros outside the batch."""
    from dgl_kgat_amd import ops
    batch, emb, ref, rs = T.bpr_case_data(n, F_, B, structured)
    e = emb.to(dev)
    ids = [torch.as_tensor(t, dtype=torch.int32, device=dev) for t in batch]
    s = T.BPR_SCALE
    outs = []
    for _ in range(2):
        loss, coef, ws = ops.bpr_loss(e, *ids, 1e-5)
        grad = ops.bpr_grad(e, *ids, coef, 1e-5, grad_scale=torch.tensor(s, dtype=torch.float32, device=dev), workspace=ws)
        outs.append((loss.clone(), grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    loss, grad = float(outs[0][0]), outs[0][1].double().cpu().numpy()
    rs_grad = (torch.as_tensor(rs.grad, dtype=torch.float32) * s).double().numpy()
    name = "bpr-N%d-F%d-B%d" % (n, F_, B)
    print("[fp64] %-30s loss      device %.3e  restatement %.3e  (relative to |L64|)"
          % (name, abs(loss - ref.loss) / abs(ref.loss), abs(rs.loss - ref.loss) / abs(ref.loss)))
    ratio, = _report(name, "loss+grad", ("grad",), [T.row_err(grad, s * ref.grad, s * ref.A)],
                     [T.row_err(rs_grad, s * ref.grad, s * ref.A)], [(ref.run + 8) * T.U])
    assert T.loss_ok(loss, rs.loss, ref.loss), (loss, rs.loss, ref.loss)
    assert ratio <= 1.0, ratio
