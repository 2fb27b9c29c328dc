"""The float64 references of tests/_transr_ref.py, checked where no GPU is needed: they equal the module's own torch
restatements, the per-row metric catches what the whole-tensor bar let through, and the fp32 restatement on the CPU
meets every bar on every case the device test runs (the inputs are fair)."""
import numpy as np
import pytest
import torch

import _transr_ref as T
from conftest import rel_err_inf


def _module(N, R, d, k, params):
    import dgl_kgat_amd as K
    m = K.KGATPropagation(N, R, d, k, 1, 8, dropout=0.0).double()
    with torch.no_grad():
        for p, v in zip((m.entity_embed.weight, m.W_R, m.relation_embed.weight), params):
            p.copy_(v.double())
    return m


@pytest.mark.parametrize("d,k", [(8, 8), (20, 12), (64, 64)])
def test_transr_ref_equals_the_module_restatement(d, k):
    N, R, B = 700, 9, 1200
    batch = T.transr_batch(N, R, B)
    params = T.transr_params(N, R, d, k, "xavier", batch)
    ref = T.transr_ref(*params, *batch, T.REG_LAMBDA)
    m = _module(N, R, d, k, params)
    ids = [torch.as_tensor(t) for t in batch]
    loss = m.transR(*ids, reg_lambda_kg=T.REG_LAMBDA, fused=False)
    grads = torch.autograd.grad(loss, (m.entity_embed.weight, m.W_R, m.relation_embed.weight))
    assert abs(ref.loss - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for got, want in zip((ref.grad_ent, ref.grad_W, ref.grad_rel), grads):
        assert rel_err_inf(got, want.numpy()) <= 1e-12
    # the per-occurrence rows add up to the gradients (what the accumulations of magnitudes are built from)
    back = np.zeros_like(ref.grad_ent)
    np.add.at(back, ref.ids3, ref.gx)
    assert rel_err_inf(back, ref.grad_ent) <= 1e-12
    assert np.all(ref.A_ent >= np.abs(ref.grad_ent) * (1 - 1e-12)) and np.all(ref.A_W >= np.abs(ref.grad_W) * (1 - 1e-9))
    assert np.all(ref.A_rel >= np.abs(ref.grad_rel) * (1 - 1e-12))


@pytest.mark.parametrize("n,F_,B,structured", T.BPR_CASES)
def test_bpr_ref_equals_the_module_restatement(n, F_, B, structured):
    batch, emb, ref, _ = T.bpr_case_data(n, F_, B, structured)
    m = _module(n, 4, 8, 8, T.transr_params(n, 4, 8, 8, "xavier", None))
    m._reg_lambda_gnn = 1e-5
    e = emb.double().requires_grad_(True)
    loss = m.get_loss(e, *[torch.as_tensor(t) for t in batch], fused=False)
    loss.backward()
    assert abs(ref.loss - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert rel_err_inf(ref.grad, e.grad.numpy()) <= 1e-12
    assert np.all(ref.A >= np.abs(ref.grad) * (1 - 1e-12))


def test_batch_builder_plants_what_it_says():
    h, r, pt, nt = T.transr_batch(700, 9, 1200)
    assert np.bincount(r, minlength=9).tolist() == list(T.REL_RUNS) + [1200 - sum(T.REL_RUNS)]
    cnt = np.bincount(np.stack([h, pt, nt], 1).reshape(-1), minlength=700)
    assert cnt[:10].tolist() == list(T.ENT_RUNS[:10]) and cnt[699] == 65 and (cnt == 0).sum() >= 200
    assert (pt == nt).sum() >= 25 and (h == pt).sum() >= 15 and ((h == pt) & (pt == nt)).sum() >= 5
    for N in (524288, 524289):
        hh, _, pp, nn_ = T.transr_batch(N, 9, 1200, high_ids=True)
        ids = np.concatenate([hh, pp, nn_])
        assert ids.max() == N - 1 and ids.min() == 0 and np.all((ids == 0) | (ids >= N - 700))
    u, p, q = T.bpr_batch(700, 4000, True)
    cnt = np.bincount(np.concatenate([u, p, q]), minlength=700)
    assert (p == 5).sum() == 1500 and (u == 7).sum() == 70 and cnt[[11, 12, 13, 14]].tolist() == [31, 32, 33, 64]
    assert (u == 9).sum() == (p == 9).sum() == (q == 9).sum() == 1 and cnt[699] == 5


def test_row_metric_catches_what_the_tensor_bar_let_through():
    """The hub batch of test_transr_hub_batch (one entity heads 300 samples and is the tail of 100), with a 65-run
    planted: three corruptions of the float64 entity gradient, each beyond the per-row bar; two of them inside the old
    whole-tensor bar rel_err_inf < 2e-5."""
    torch.manual_seed(11)
    n, R, B, d, k = 3000, 7, 1024, 64, 64
    h, r, pt, nt = (torch.randint(0, hi, (B,)) for hi in (n, R, n, n))
    h[:300] = 42
    pt[300:400] = 42
    for t in (h, pt, nt):
        t[t == 77] = 78
    nt[400:465] = 77
    batch = [t.numpy() for t in (h, r, pt, nt)]
    params = T.transr_params(n, R, d, k, "xavier", batch)
    ref = T.transr_ref(*params, *batch, T.REG_LAMBDA)
    rs = T.transr_ref(*params, *batch, T.REG_LAMBDA, dtype=torch.float32)
    floor = T.floors(ref, d, k)[0]
    err_rs = T.row_err(rs.grad_ent, ref.grad_ent, ref.A_ent)

    def new_bar(g):
        return T.bar_ratio(T.row_err(g, ref.grad_ent, ref.A_ent), err_rs, floor)

    assert ref.run_ent[42] == 400 and ref.run_ent[77] == 65
    assert new_bar(rs.grad_ent) <= 1.0 and new_bar(ref.grad_ent) == 0.0
    hub_scale = np.abs(ref.grad_ent[42]).max()
    assert hub_scale == np.abs(ref.grad_ent).max()
    # (a) one of the 65 contributions of the 65-run row is missing
    a = ref.grad_ent.copy()
    a[77] -= ref.gx[np.flatnonzero(ref.ids3 == 77)[30]]
    # (b) 1e-5 of the hub row's scale on a row with one occurrence
    b_ = ref.grad_ent.copy()
    single = int(np.flatnonzero(ref.run_ent == 1)[0])
    b_[single, 3] += 1e-5 * hub_scale
    # (c) a row outside the batch is not exactly zero
    c = ref.grad_ent.copy()
    outside = int(np.flatnonzero(ref.run_ent == 0)[0])
    c[outside, 0] = 1e-30
    for name, g in (("a", a), ("b", b_), ("c", c)):
        print("corruption (%s): ratio to the per-row bar %.3g, rel_err_inf %.3g" % (name, new_bar(g), rel_err_inf(g, ref.grad_ent)))
        assert new_bar(g) > 1.0, name
    assert rel_err_inf(b_, ref.grad_ent) < 2e-5 and rel_err_inf(c, ref.grad_ent) < 2e-5


@pytest.mark.parametrize("name", [c.name for c in T.TRANSR_CASES])
def test_fp32_restatement_meets_every_transr_bar(name):
    """The inputs are fair: the fp32 restatement on the CPU is finite, exactly zero where nothing is added, and inside
    every bar of the device test.  Prints its row errors as multiples of the floors."""
    c = next(c for c in T.TRANSR_CASES if c.name == name)
    _, _, ref, rs = T.transr_case_data(name)
    assert np.isfinite(ref.loss) and all(np.isfinite(g).all() for g in (ref.grad_ent, ref.grad_W, ref.grad_rel))
    assert T.loss_ok(rs.loss, rs.loss, ref.loss)
    errs = T.transr_errors(ref, (rs.grad_ent, rs.grad_W, rs.grad_rel))
    for tensor, e, fl in zip(("grad_ent", "grad_W", "grad_rel"), errs, T.floors(ref, c.d, c.k)):
        print("[restatement] %-28s %-8s row_err %.3e = %.3f of its floor" % (name, tensor, e.max(), np.max(e / fl)))
        assert np.isfinite(e).all() and T.bar_ratio(e, e, fl) <= 1.0
    # untouched rows exist in every case with a table larger than the batch, and they are zero in the reference
    assert np.all(ref.grad_ent[ref.run_ent == 0] == 0) and np.all(ref.grad_W[ref.run_rel == 0] == 0)


@pytest.mark.parametrize("n,F_,B,structured", T.BPR_CASES)
def test_fp32_restatement_meets_every_bpr_bar(n, F_, B, structured):
    _, _, ref, rs = T.bpr_case_data(n, F_, B, structured)
    e = T.row_err(rs.grad, ref.grad, ref.A)
    fl = (ref.run + 8) * T.U
    print("[restatement] bpr %s row_err %.3e = %.3f of its floor" % ((n, F_, B), e.max(), np.max(e / fl)))
    assert np.isfinite(e).all() and T.bar_ratio(e, e, fl) <= 1.0 and T.loss_ok(rs.loss, rs.loss, ref.loss)
