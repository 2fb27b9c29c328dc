"""Float64 reference of the TransE loss (the reference's `transR`, models.py:114-133, with the projection removed), plain
torch on the CPU, with what a per-row bound needs; with ``dtype=torch.float32`` the fp32 comparator on the CPU ("the
restatement").  The batch builders, the row metric and the bar rule are tests/_transr_ref.py's: TransE is TransR with
every W_R[r] = I and d = k, so an entity row's floor is ``floors(ref, d, d)[0]`` and a relation row's ``floors(ref, d,
d)[2]``, and a row passes within max(its floor, 2 x the restatement's largest row error of that tensor).

The cases are the smallest at which the kernels take another path: every lane-group size (d <= 64: 16 lanes per sample,
<= 128: 32, <= 256: 64) with whole and partly idle groups; batches of 1-5 samples and the largest batch (2,730: the
presort has ONE size class, so its edge is the limit itself); 1, 9 and the largest relation count; node counts on either
side of the sort key's 32-bit packing; one entity heading 300 samples; samples whose three entities coincide (the
builder's five, in every batch of 600 samples or more - on rows that other samples feed too: alone such a sample leaves
a gradient that is rounding in float64 as well, with no magnitude to bound it against); rows at the 1e-12 clamp; rows
scaled by 2^+-20."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from _transr_ref import REG_LAMBDA, U, FACTOR, _np64, bar_ratio, floors, loss_ok, row_err, transr_batch  # noqa: F401


def transe_ref(ent, rel, h, r, pos_t, neg_t, reg_lambda, dtype=torch.float64):
    ent, rel = (torch.as_tensor(t).detach().cpu().to(dtype).clone().requires_grad_(True) for t in (ent, rel))
    h, r, pos_t, neg_t = (torch.as_tensor(t).detach().cpu().long() for t in (h, r, pos_t, neg_t))
    n, (n_rel, d), b = ent.shape[0], rel.shape, h.numel()
    ids3 = torch.stack([h, pos_t, neg_t], 1).reshape(-1)      # occurrence 3 s + (0, 1, 2) = head, positive, negative
    x = ent.index_select(0, ids3)
    x.retain_grad()
    er = rel.index_select(0, r)
    er.retain_grad()
    u = F.normalize(x.view(b, 3, d), p=2, dim=2)
    h_vec, pos_vec, neg_vec = u[:, 0], u[:, 1], u[:, 2]
    r_vec = F.normalize(er, p=2, dim=1)
    pos_score = (h_vec + r_vec - pos_vec).pow(2).sum(1, keepdim=True)
    neg_score = (h_vec + r_vec - neg_vec).pow(2).sum(1, keepdim=True)
    loss = (-F.logsigmoid(neg_score - pos_score)).mean()
    reg = sum((v.pow(2).sum(1) / 2.0).mean() for v in (h_vec, r_vec, pos_vec, neg_vec))
    total = loss + reg_lambda * reg
    total.backward()
    with torch.no_grad():
        A_ent = torch.zeros(n, d, dtype=torch.float64).index_add_(0, ids3, x.grad.abs().double())
        A_rel = torch.zeros(n_rel, d, dtype=torch.float64).index_add_(0, r, er.grad.abs().double())
    return types.SimpleNamespace(
        loss=float(total.detach().double()), grad_ent=_np64(ent.grad), grad_rel=_np64(rel.grad), A_ent=A_ent.numpy(),
        A_rel=A_rel.numpy(), run_ent=np.bincount(ids3.numpy(), minlength=n), run_rel=np.bincount(r.numpy(), minlength=n_rel))


def transe_floors(ref, d):
    """Per-row floors of grad_ent and grad_rel: tests/_transr_ref.floors with k = d."""
    f = floors(ref, d, d)
    return f[0], f[2]


def transe_errors(ref, grads, scale=1.0):
    """row_err of (grad_ent, grad_rel) against `scale` x the float64 gradients."""
    return [row_err(g, scale * w, scale * A) for g, w, A in zip(grads, (ref.grad_ent, ref.grad_rel), (ref.A_ent, ref.A_rel))]


def transe_batch(c):
    h, r, pt, nt = transr_batch(c.N, c.R, c.B, high_ids=c.high_ids)
    if c.hub:           # one entity heads 300 samples of the batch
        h[:300] = h[0]
    return h, r, pt, nt


def transe_params(c, batch, seed=22):
    """ent, rel (fp32 torch, CPU).  "scaled": rows times 2^-20 or 2^+20; "zeros": an all-zero entity row and an all-zero
    relation row that the batch uses (the max(norm, 1e-12) clamp: large, finite gradients)."""
    g = torch.Generator().manual_seed(seed)
    ent = torch.randn(c.N, c.d, generator=g) * 0.05
    rel = torch.randn(c.R, c.d, generator=g) * 0.3
    h, r, pt, nt = batch
    if c.regime == "scaled":
        ent *= torch.exp2(40.0 * torch.randint(0, 2, (c.N, 1), generator=g).float() - 20.0)
        rel *= torch.exp2(40.0 * torch.randint(0, 2, (c.R, 1), generator=g).float() - 20.0)
    elif c.regime == "zeros":
        ent[int(h[0])] = 0.0
        ent[int(pt[-1])] = 0.0
        rel[int(r[0])] = 0.0
    elif c.regime != "xavier":
        raise ValueError(c.regime)
    return ent, rel


def _case(d, regime="xavier", N=700, R=9, B=1200, high_ids=False, hub=False):
    name = "%d-%s-N%d-R%d-B%d%s" % (d, regime, N, R, B, "-hub" if hub else "")
    return types.SimpleNamespace(name=name, d=d, regime=regime, N=N, R=R, B=B, high_ids=high_ids, hub=hub)


MAX_BATCH, MAX_REL = 2730, 4096
TRANSE_CASES = [_case(d) for d in (4, 8, 20, 64, 128, 256)]
TRANSE_CASES += [_case(d, regime) for regime in ("scaled", "zeros") for d in (20, 64)]
TRANSE_CASES += [_case(d, B=b) for d in (8, 64) for b in (1, 2, 3, 5)]
TRANSE_CASES += [_case(20, B=MAX_BATCH), _case(64, hub=True)]
TRANSE_CASES += [_case(8, R=1), _case(8, R=MAX_REL, B=300)]
TRANSE_CASES += [_case(4, N=524288, high_ids=True), _case(4, N=524289, high_ids=True)]
PHASE_CASES = [c for c in TRANSE_CASES if c.name in ("4-xavier-N700-R9-B1200", "20-xavier-N700-R9-B1200", "64-xavier-N700-R9-B1200-hub",
                                                      "256-xavier-N700-R9-B1200", "8-xavier-N700-R4096-B300", "8-xavier-N700-R9-B3")]


@functools.lru_cache(maxsize=None)
def transe_case_data(name):
    """(batch, parameters, float64 reference, fp32 restatement) of a case: computed once, shared, never written to."""
    c = next(c for c in TRANSE_CASES if c.name == name)
    batch = transe_batch(c)
    params = transe_params(c, batch)
    return batch, params, transe_ref(*params, *batch, REG_LAMBDA), transe_ref(*params, *batch, REG_LAMBDA, dtype=torch.float32)
