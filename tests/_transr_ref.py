"""Float64 references of the two training losses, plain torch on the CPU, with what a per-row bound needs.

``transr_ref`` restates reference models.py:114-133 exactly as ``KGATPropagation.transR(fused=False)`` does, and keeps
the gathered rows, the projections and the gathered relation rows as autograd leaves, so that ONE backward yields the
three gradients, the per-occurrence gradient rows, and the accumulations of their magnitudes that the kernels' sums are
bounded against.  ``bpr_ref`` does the same for ``get_loss(fused=False)`` (reference models.py:170-178).  With
``dtype=torch.float32`` both are the fp32 comparator on the CPU ("the restatement" of the bars below).

``row_err`` is the metric: per leading-index row (an entity, a relation) the largest |got - want| over the row, divided
by the row's largest accumulated magnitude - a row is one sum, and fp32 summation bounds the error of a sum by the sum
of |terms|, not by the largest element of some other row.  A row whose accumulation is zero everywhere (an entity not
in the batch, an unused relation) must be exactly zero.

The bars (``U`` = 2^-24; one rounding per addition of the longest chain a term passes through):
    entity row with `run` occurrences       (run + d + k + 8) U
    relation r's block of grad_W            (3 n_r + d + k + 8) U
    relation r's row of grad_rel            (n_r + k + 8) U
    a BPR gradient row                      (run + 8) U
and a row passes when its error is within max(its floor, 2 x the restatement's largest row error of that tensor);
the loss when |L - L64| <= max(8 U, 2 x the restatement's) x |L64|.  The factor 2 is conftest.parity_8c's.

The batch builders and the list of cases live here too: the host test (fp32 restatement against every bar, no GPU) and
the device test walk the same cases.

At the end: the layout of the per-batch block that the KG phase's presort writes, restated (the host test tabulates it
against the library's size entry, the device test decodes blocks with it), and what the block must hold, from numpy."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FACTOR = 2.0
REG_LAMBDA = 0.01


def _np64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def transr_ref(ent, W_R, rel, h, r, pos_t, neg_t, reg_lambda, dtype=torch.float64):
    ent, W_R, rel = (torch.as_tensor(t).detach().cpu().to(dtype).clone().requires_grad_(True) for t in (ent, W_R, rel))
    h, r, pos_t, neg_t = (torch.as_tensor(t).detach().cpu().long() for t in (h, r, pos_t, neg_t))
    n, (n_rel, d, k), b = ent.shape[0], W_R.shape, h.numel()
    ids3 = torch.stack([h, pos_t, neg_t], 1).reshape(-1)      # occurrence 3 s + (0, 1, 2) = head, positive, negative
    x = ent.index_select(0, ids3)
    x.retain_grad()
    a = torch.bmm(x.view(b, 3, d), W_R.index_select(0, r))    # (B, 3, k)
    a.retain_grad()
    er = rel.index_select(0, r)
    er.retain_grad()
    u = F.normalize(a, p=2, dim=2)
    h_vec, pos_vec, neg_vec = u[:, 0], u[:, 1], u[:, 2]
    r_vec = F.normalize(er, p=2, dim=1)
    pos_score = (h_vec + r_vec - pos_vec).pow(2).sum(1, keepdim=True)
    neg_score = (h_vec + r_vec - neg_vec).pow(2).sum(1, keepdim=True)
    loss = (-F.logsigmoid(neg_score - pos_score)).mean()
    reg = sum((v.pow(2).sum(1) / 2.0).mean() for v in (h_vec, r_vec, pos_vec, neg_vec))
    total = loss + reg_lambda * reg
    total.backward()
    gx, ga, ger = x.grad, a.grad.reshape(3 * b, k), er.grad
    with torch.no_grad():
        A_ent = torch.zeros(n, d, dtype=torch.float64).index_add_(0, ids3, gx.abs().double())
        A_rel = torch.zeros(n_rel, k, dtype=torch.float64).index_add_(0, r, ger.abs().double())
        A_W = torch.zeros(n_rel, d, k, dtype=torch.float64)
        r3 = r.repeat_interleave(3)
        xa, gaa = x.detach().abs().double(), ga.abs().double()
        for q in torch.unique(r).tolist():
            sel = r3 == q
            A_W[q] = xa[sel].t() @ gaa[sel]
    return types.SimpleNamespace(
        loss=float(total.detach().double()), grad_ent=_np64(ent.grad), grad_W=_np64(W_R.grad), grad_rel=_np64(rel.grad),
        x=_np64(x), gx=_np64(gx), ga=_np64(ga), ger=_np64(ger), A_ent=A_ent.numpy(), A_W=A_W.numpy(), A_rel=A_rel.numpy(),
        ids3=ids3.numpy(), run_ent=np.bincount(ids3.numpy(), minlength=n), run_rel=np.bincount(r.numpy(), minlength=n_rel))


def bpr_ref(emb, u, p, n, reg_lambda, dtype=torch.float64):
    emb = torch.as_tensor(emb).detach().cpu().to(dtype).clone().requires_grad_(True)
    u, p, n = (torch.as_tensor(t).detach().cpu().long() for t in (u, p, n))
    b = u.numel()
    ids3 = torch.cat([u, p, n])
    rows = emb.index_select(0, ids3)
    rows.retain_grad()
    s, pp, nn_ = rows[:b], rows[b:2 * b], rows[2 * b:]
    cf = -F.logsigmoid((s * pp).sum(1) - (s * nn_).sum(1)).mean()
    reg = sum((v.pow(2).sum(1) / 2.0).mean() for v in (s, pp, nn_))
    total = cf + reg_lambda * reg
    total.backward()
    A = torch.zeros(emb.shape, dtype=torch.float64).index_add_(0, ids3, rows.grad.abs().double())
    return types.SimpleNamespace(loss=float(total.detach().double()), grad=_np64(emb.grad), A=A.numpy(),
                                 run=np.bincount(ids3.numpy(), minlength=emb.shape[0]))


def row_err(got, want, A):
    """Per leading-index row: max |got - want| over the row / the row's largest A; a row with A == 0 everywhere must be
    exactly zero in `got` (else inf)."""
    got, want, A = (np.asarray(t, np.float64).reshape(np.shape(A)[0], -1) for t in (got, want, A))
    err, scale = np.abs(got - want).max(axis=1), A.max(axis=1)
    out = np.zeros(len(scale))
    nz = scale > 0
    out[nz] = err[nz] / scale[nz]
    out[~nz & (np.abs(got).max(axis=1) != 0)] = np.inf
    out[np.isnan(err)] = np.inf
    return out


def floors(ref, d, k):
    """The per-row floors of grad_ent, grad_W, grad_rel for a transr_ref result."""
    return ((ref.run_ent + d + k + 8) * U, (3 * ref.run_rel + d + k + 8) * U, (ref.run_rel + k + 8) * U)


def bar_ratio(err_dev, err_rs, floor):
    """Worst ratio of a row's error to its bar max(floor of the row, FACTOR x the restatement's largest row error)."""
    return float(np.max(err_dev / np.maximum(floor, FACTOR * float(np.max(err_rs)))))


def loss_ok(got, rs, want):
    return abs(got - want) <= max(8 * U, FACTOR * abs(rs - want) / abs(want)) * abs(want)


# ------------------------------------------------------------------------------------------------ batch builders
REL_RUNS = (64, 1, 3, 0, 63, 65, 128, 129)       # relations 0..7 (an empty one in the middle); the rest go to the last
ENT_RUNS = (17, 1, 2, 15, 16, 63, 64, 80, 81, 400, 65)   # local entities 0..9 and, the 65-run, the last id


def _plant(slots, runs, pool, rng):
    """Fill the free (-1) entries of the (B, 3) id table: `runs` = [(id, count, column or None)] at random free places
    of the allowed column(s), every other free entry a random draw from `pool`."""
    for ident, count, col in runs:
        free = np.argwhere(slots < 0) if col is None else np.argwhere(slots[:, col] < 0)
        pick = free[rng.choice(len(free), count, replace=False)]
        if col is None:
            slots[pick[:, 0], pick[:, 1]] = ident
        else:
            slots[pick[:, 0], col] = ident
    free = slots < 0
    slots[free] = rng.choice(pool, int(free.sum()))
    return slots


def transr_batch(N, R, B, seed=20, high_ids=False):
    """h, r, pos_t, neg_t (int64 numpy) of one KG batch.  With R >= 9 and B >= 600 the relation run lengths are exactly
    REL_RUNS (the rest in relation R - 1); with B >= 600 the entity run lengths of eleven planted entities are exactly
    ENT_RUNS, entity 0 among them, the 65-run on entity N - 1, spread over the three roles at random; 20 samples have
    pos_t == neg_t, 10 h == pos_t, 5 all three equal.  Smaller batches keep the first entity (a head), the last (a
    positive tail), the first and the last relation, and no coincidence of the two tails.  The other entities are drawn from 400 ids,
    so that rows outside the batch exist.  high_ids: every id but 0 among the largest of N."""
    rng = np.random.default_rng(seed)
    span = min(N, 700)
    local = np.arange(span)
    planted = np.concatenate([local[:len(ENT_RUNS) - 1], local[-1:]])
    others = np.setdiff1d(local, planted)
    pool = rng.choice(others, min(400, len(others)), replace=False) if len(others) else planted
    slots = np.full((B, 3), -1, np.int64)
    # the coincidences first, on ids of the pool
    small = B < 600
    n_pn, n_hp, n_all = (0, 0, 0) if small else (20, 10, 5)
    s = 0
    for cnt, kind in ((n_all, "all"), (n_pn, "pn"), (n_hp, "hp")):
        for _ in range(cnt):
            a, b_, c = rng.choice(pool, 3)
            slots[s] = {"all": (a, a, a), "pn": (a, b_, b_), "hp": (a, a, c)}[kind]
            s += 1
    if not small:
        runs = [(int(e), int(c), None) for e, c in zip(planted, ENT_RUNS)]
    else:
        runs = [(int(local[0]), min(2, B), 0), (int(local[-1]), min(3, B), 1)]
    _plant(slots, runs, pool, rng)
    if small:
        # With pos_t == neg_t the gradients at the head and at the relation row vanish ANALYTICALLY (what is left of
        # them is rounding, in float64 too), so a row that only such a sample feeds has no magnitude to be bounded
        # against: the small batches, where one sample can be all a row gets, keep the two tails apart.
        same = slots[:, 1] == slots[:, 2]
        slots[same, 2] = np.where(slots[same, 1] == pool[0], pool[1], pool[0])
    if R >= 9 and B >= 600:
        r = np.concatenate([np.full(c, q) for q, c in enumerate(REL_RUNS)] + [np.full(B - sum(REL_RUNS), R - 1)])
    else:
        r = rng.integers(0, R, B)
        r[0] = R - 1
        r[-1] = 0
    perm = rng.permutation(B)                       # samples in random order: the sorts have work to do
    slots, r = slots[perm], r[rng.permutation(B)]
    if N > span:                                    # local ids -> the table's: 0 stays, the others move to the top
        slots = np.where(slots == 0, 0, slots + (N - span)) if high_ids else np.where(slots == span - 1, N - 1, slots)
    return slots[:, 0].copy(), r.astype(np.int64), slots[:, 1].copy(), slots[:, 2].copy()


def transr_params(N, R, d, k, regime, batch, seed=21):
    """ent, W_R, rel (fp32 torch, CPU).  "xavier": ent x 0.05, W ~ sqrt(2 / (d + k)); "scaled": rows of ent times
    2^-20 .. 2^+10 (the loss does not move, the gradients scale inversely); "zeros": three entity rows of the batch and
    one used relation row set to zero (the max(norm, 1e-12) clamp: large, finite gradients)."""
    g = torch.Generator().manual_seed(seed)
    ent = torch.randn(N, d, generator=g) * 0.05
    W = torch.randn(R, d, k, generator=g) * (2.0 / (d + k)) ** 0.5
    rel = torch.randn(R, k, generator=g) * 0.3
    if regime == "scaled":
        ent *= torch.exp2(torch.randint(-20, 11, (N, 1), generator=g).float())
    elif regime == "zeros":
        h, r, pt, nt = batch
        ids3 = np.stack([h, pt, nt], 1).reshape(-1)
        cnt = np.bincount(ids3, minlength=N)
        order = np.argsort(-cnt, kind="stable")
        picks = [int(order[0]), int(np.flatnonzero(cnt == 16)[0]) if (cnt == 16).any() else int(order[1]), int(h[0])]
        ent[picks] = 0.0
        used = np.bincount(r, minlength=R)
        rel[int(np.flatnonzero(used == 63)[0]) if (used == 63).any() else int(r[0])] = 0.0
    elif regime != "xavier":
        raise ValueError(regime)
    return ent, W, rel


WIDTHS = [(4, 4), (8, 8), (20, 12), (12, 20), (64, 64), (16, 48), (48, 16), (68, 36), (100, 60), (128, 4), (4, 128),
          (64, 128), (128, 64), (80, 48), (128, 128)]
REGIME_WIDTHS = [(64, 64), (20, 12), (80, 48)]
EDGE_WIDTHS = [(8, 8), (64, 64)]


def _case(d, k, regime="xavier", N=700, R=9, B=1200, high_ids=False):
    name = "%dx%d-%s-N%d-R%d-B%d" % (d, k, regime, N, R, B)
    return types.SimpleNamespace(name=name, d=d, k=k, regime=regime, N=N, R=R, B=B, high_ids=high_ids)


TRANSR_CASES = [_case(d, k) for d, k in WIDTHS]
TRANSR_CASES += [_case(d, k, regime) for regime in ("scaled", "zeros") for d, k in REGIME_WIDTHS]
TRANSR_CASES += [_case(d, k, B=b) for d, k in EDGE_WIDTHS for b in (1, 2, 3, 4, 5, 2730)]
TRANSR_CASES += [_case(d, k, R=1) for d, k in EDGE_WIDTHS]
TRANSR_CASES += [_case(8, 8, R=1025, B=300), _case(8, 8, R=4096, B=300)]
TRANSR_CASES += [_case(4, 4, N=524288, high_ids=True), _case(4, 4, N=524289, high_ids=True)]
# (every width, and the largest relation count: its chunk table is the one whose total no thread's four keys reach)
PHASE_CASES = TRANSR_CASES[:len(WIDTHS)] + [c for c in TRANSR_CASES if c.R == 4096]


@functools.lru_cache(maxsize=None)
def transr_case_data(name):
    """(batch, parameters, float64 reference, fp32 restatement) of a case: computed once, shared, never written to."""
    c = next(c for c in TRANSR_CASES if c.name == name)
    batch = transr_batch(c.N, c.R, c.B, high_ids=c.high_ids)
    params = transr_params(c.N, c.R, c.d, c.k, c.regime, batch)
    ref = transr_ref(*params, *batch, REG_LAMBDA)
    rs = transr_ref(*params, *batch, REG_LAMBDA, dtype=torch.float32)
    return batch, params, ref, rs


def transr_errors(ref, grads, scale=1.0):
    """row_err of (grad_ent, grad_W, grad_rel) against `scale` x the float64 gradients."""
    return [row_err(g, scale * w, scale * A) for g, w, A in zip(grads, (ref.grad_ent, ref.grad_W, ref.grad_rel),
                                                                 (ref.A_ent, ref.A_W, ref.A_rel))]


# -- BPR
def bpr_batch(n, B, structured, seed=30):
    """u, p, q (int64 numpy).  structured: one row the positive of 1,500 samples, one user the source of 70, one row
    once in each role, runs of exactly 31, 32, 33 and 64, and the last row (a run that ends at the last sorted
    position); else the draw of test_bpr_loss_and_gradient_vs_torch (users from a third of the rows, five samples whose
    positive is their source) with the last row present."""
    rng = np.random.default_rng(seed + B)
    if not structured:
        u, p, q = rng.integers(0, max(n // 3, 1), B), rng.integers(0, n, B), rng.integers(0, n, B)
        p[:5] = u[:5]
        q[B // 2] = n - 1
        return u, p, q
    slots = np.full((B, 3), -1, np.int64)
    runs = [(5, 1500, 1), (7, 70, 0), (9, 1, 0), (9, 1, 1), (9, 1, 2), (11, 31, None), (12, 32, None), (13, 33, None),
            (14, 64, None), (n - 1, 5, None)]
    pool = rng.choice(np.arange(20, n - 1), 450, replace=False)
    _plant(slots, runs, pool, rng)
    return slots[:, 0].copy(), slots[:, 1].copy(), slots[:, 2].copy()


BPR_CASES = [(700, 16, 1365, False), (700, 16, 1366, False), (700, 176, 4000, True)]
BPR_SCALE = 2.5


@functools.lru_cache(maxsize=None)
def bpr_case_data(n, F_, B, structured):
    batch = bpr_batch(n, B, structured)
    emb = torch.randn(n, F_, generator=torch.Generator().manual_seed(n + F_ + B))
    return batch, emb, bpr_ref(emb, *batch, 1e-5), bpr_ref(emb, *batch, 1e-5, dtype=torch.float32)


# -- the presort's per-batch block (kgat_transr_presort_f32), restated
CHUNK = 64       # samples per chunk of the weight-gradient partials


def align256(nbytes):
    return (int(nbytes) + 255) // 256 * 256


def max_chunks(batch, n_rel):
    """The most chunks a batch's chunk table can hold: one per started CHUNK samples of every relation."""
    return batch // CHUNK + n_rel + 1


def sorted_block_layout(batch, n_rel):
    """name -> (byte offset, dtype, element count) of the pieces of one batch's block, and the block's size in bytes:
    256-aligned pieces in this order."""
    pieces = [("order", np.int32, batch), ("seg", np.int32, n_rel + 2), ("chunk_ptr", np.int32, n_rel + 2),
              ("chunks", np.int32, 2 * max_chunks(batch, n_rel)), ("sorted_ids", np.int32, 3 * batch),
              ("row_order", np.int32, 3 * batch), ("inv_pos", np.int32, 3 * batch), ("run_len", np.int32, 3 * batch)]
    lay, off = {}, 0
    for name, dtype, count in pieces:
        lay[name] = (off, dtype, count)
        off += align256(count * np.dtype(dtype).itemsize)
    return lay, off


def decode_sorted_block(block, batch, n_rel):
    """The pieces of one batch's block (a uint8 numpy array of the block's size) as int32 arrays; `chunks` as (n, 2)."""
    lay, nbytes = sorted_block_layout(batch, n_rel)
    assert block.dtype == np.uint8 and block.size == nbytes
    out = {name: block[off:off + 4 * count].view(np.int32) for name, (off, _, count) in lay.items()}
    out["chunks"] = out["chunks"].reshape(-1, 2)
    return types.SimpleNamespace(**out)


def presort_expected(h, r, pos_t, neg_t, n_rel):
    """What the presort must leave for one batch, from numpy's stable sorts (a stable sort's output is unique).  Only
    the first chunk_ptr[n_rel] entries of `chunks`, and seg[0 .. n_rel], are defined."""
    h, r, pos_t, neg_t = (np.asarray(t, np.int64) for t in (h, r, pos_t, neg_t))
    order = np.argsort(r, kind="stable")
    rs = r[order]
    seg = np.searchsorted(rs, np.arange(n_rel + 1), side="left")
    counts = np.bincount(r, minlength=n_rel)
    n_chunks = (counts + CHUNK - 1) // CHUNK
    chunk_ptr = np.concatenate([[0], np.cumsum(n_chunks)])
    chunks = np.array([(v, seg[v] + CHUNK * j) for v in range(n_rel) for j in range(n_chunks[v])], np.int64).reshape(-1, 2)
    ids = np.stack([h, pos_t, neg_t], 1).reshape(-1)
    row_order = np.argsort(ids, kind="stable")
    sorted_ids = ids[row_order]
    inv_pos = np.empty_like(row_order)
    inv_pos[row_order] = np.arange(len(ids))
    starts = np.flatnonzero(np.concatenate([[True], sorted_ids[1:] != sorted_ids[:-1]]))
    run_len = np.zeros(len(ids), np.int64)
    run_len[starts] = np.diff(np.append(starts, len(ids)))
    return types.SimpleNamespace(order=order, seg=seg, chunk_ptr=chunk_ptr, chunks=chunks, sorted_ids=sorted_ids,
                                 row_order=row_order, inv_pos=inv_pos, run_len=run_len)
