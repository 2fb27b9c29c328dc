"""Float64 restatement of TransR link prediction (kg_eval / csrc/kgat_transr_rank.hip), plain torch / numpy on the CPU.

``project_ref`` is the projection  u = a / max(|a|, 1e-12),  a = e W_r,  out = u + sign * rel / max(|rel|, 1e-12)  with
what a per-row bound needs.  ``direct_scores`` is the score of reference models.py:120-126 in its DIRECT form,
sum_j (u_h + u_r - u_t)_j^2, for every (query, candidate) pair - not the  n2 - 2 q.p  identity the kernel sweeps
with.  ``brute_counts`` counts lt / eq over a score matrix, ``band`` gives the two counts a rank may lie between.
With ``dtype=torch.float32`` the first two are "the CPU fp32 restatement" of the bars below.

The projection's bar (``U`` = 2^-24).  Column j of a row is  a_j = sum_i e_i W_ij,  a chain of d fused multiply-adds:
|da_j| <= d U A_j with A_j = sum_i |e_i| |W_ij|.  The norm adds k squares (k U relative on |a|^2, half of it after the
root), the root, the division, the relation term's own normalisation and the final addition are a handful of roundings
more: 8 covers them.  Normalising divides by |a|, so an error da reaches the output as da / |a|: the row's scale is
    S = max(1, |A|_2 / |a|_2)
(1 is the size of a unit vector's largest possible element; |A| / |a| > 1 measures how much the row's products
cancel).  ``project_row_err`` is max_j |got - want| / S per row, and its floor
    (d + k + 8) U
in the manner of _transr_ref's (run + d + k + 8) U.  n2 = sum_j u_j^2 of the normalised row carries the norm's error
twice plus its own k additions: floor (2 k + 8) U against its value 1; a row whose a is exactly zero has u = 0 and
n2 = 0 exactly.  A row passes within max(its floor, 2 x the restatement's largest row error); 2 is
conftest.parity_8c's factor.  The output of such a zero row is the relation term alone, sign * rel / |rel| in fp32:
the sum of k squares (k U relative on |rel|^2, k / 2 U after the root), the root and the division (1 U each) on
elements of size <= 1, plus the fp32 representation of the inputs the float64 value is formed from:
(k / 2 + 3) U, held to ZERO_ROW_BAR = (k + 8) U.

The band.  Two implementations of the score that are both correct to a tolerance tau can disagree about
s_i < s_t only where |s_i - s_t| <= tau.  So for the fp64 scores s64 and every query
    lt_lo = #{ s64_i <  s64_t - tau },    lt_hi = #{ s64_i <= s64_t + tau }      (i not filtered, i != t)
and a correct (lt, eq) obeys  lt_lo <= lt <= lt + eq <= lt_hi.  tau = max(TAU_FLOOR, 2 x the largest |s32 - s64| of the
fp32 restatement of the direct form over all pairs of the case).  TAU_FLOOR is what NO fp32 implementation can avoid:
the three unit vectors u_h, u_r, u_t are stored in fp32 (each element off by up to U |u_j|), which moves
s = |v|^2, v = u_h + u_r - u_t, |v| <= 3, by up to 2 sum_j |v_j| U (|u_h| + |u_r| + |u_t|)_j <= 2 * 3 * 3 U = 18 U,
and the sum itself is rounded at least once at its size <= 9: 9 U more; 27 U, rounded up to
    TAU_FLOOR = 32 U = 1.9e-6.
kg_complete.  Every distance it returns is one fp32 score and is held to |d32 - d64| <= tau, the band's tolerance, with
no factor.  Its order is held to the same tau: two entities may change places only where their fp64 distances lie
within tau of each other, so the fp64 distance of the entity returned at place j is within tau of the j-th smallest
fp64 distance, |D64[returned_j] - sorted(D64)[j]| <= tau.  (The shortcut |q|^2 + 1 - 2 q.p puts 1 for |p|^2; the fp64
reference's p is a unit vector too, so no extra term is owed for it.)
A band is only a test where it is narrow: the share of queries with lt_lo != lt_hi must stay <= BAND_CAP = 2 %
(asserted by every test that uses it)."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FACTOR = 2.0
TAU_FLOOR = 32 * U
BAND_CAP = 0.02


def zero_row_bar(k):
    return (k + 8) * U


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).detach().cpu().to(dtype)


def project_ref(ent, W_r, rel_row=None, sign=1.0, ids=None, rows=None, dtype=torch.float64):
    """out (n, k), n2 (n,), S (n,) - the row scale of the bar - as float64 numpy; computed in `dtype`."""
    ent, W_r = _t(ent, dtype), _t(W_r, dtype)
    if ids is not None:
        x = ent[torch.as_tensor(np.asarray(ids)).long()]
    else:
        lo, hi = (0, ent.shape[0]) if rows is None else rows
        x = ent[lo:hi]
    a = x @ W_r
    u = F.normalize(a, p=2, dim=1, eps=1e-12)
    n2 = (u * u).sum(1)
    out = u if rel_row is None else u + float(sign) * F.normalize(_t(rel_row, dtype).unsqueeze(0), p=2, dim=1, eps=1e-12)
    A = x.abs().double() @ W_r.abs().double()
    na = a.double().norm(dim=1)
    S = torch.where(na > 0, A.norm(dim=1) / na.clamp(min=1e-300), torch.ones_like(na)).clamp(min=1.0)
    return out.double().numpy(), n2.double().numpy(), S.numpy()


def project_row_err(got, want, S):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max(axis=1) / np.asarray(S, np.float64)
    err[np.isnan(err)] = np.inf
    return err


def project_floor(d, k):
    return (d + k + 8) * U


def n2_floor(k):
    return (2 * k + 8) * U


def direct_scores(ent, W_r, rel_row, anchor, side, lo, hi, dtype=torch.float64, chunk=16):
    """S[q, c] = sum_j (u_h + u_r - u_t)_j^2 in `dtype` for the queries `anchor` (the heads for side="tail", the tails
    for side="head") against the candidates [lo, hi) in the open slot.  float64 numpy."""
    ent, W_r, rel_row = _t(ent, dtype), _t(W_r, dtype), _t(rel_row, dtype)
    u_c = F.normalize(ent[lo:hi] @ W_r, p=2, dim=1, eps=1e-12)
    u_a = F.normalize(ent[torch.as_tensor(np.asarray(anchor)).long()] @ W_r, p=2, dim=1, eps=1e-12)
    u_r = F.normalize(rel_row.unsqueeze(0), p=2, dim=1, eps=1e-12)
    out = np.empty((u_a.shape[0], hi - lo), np.float64)
    for b in range(0, u_a.shape[0], chunk):
        a = u_a[b:b + chunk].unsqueeze(1)
        v = (a + u_r - u_c.unsqueeze(0)) if side == "tail" else (u_c.unsqueeze(0) + u_r - a)
        out[b:b + chunk] = v.pow(2).sum(2).double().numpy()
    return out


def brute_counts(S, t_pos, excluded):
    """lt, eq of every row of the score matrix S against its column t_pos; `excluded` (bool, same shape) marks the
    filtered candidates (the true answer is left out whatever it says)."""
    S = np.asarray(S)
    rows = np.arange(S.shape[0])
    st = S[rows, t_pos][:, None]
    on = ~np.asarray(excluded, bool)
    on[rows, t_pos] = False
    return ((S < st) & on).sum(1), ((S == st) & on).sum(1)


def band(S64, t_pos, excluded, tau):
    S64 = np.asarray(S64, np.float64)
    rows = np.arange(S64.shape[0])
    st = S64[rows, t_pos][:, None]
    on = ~np.asarray(excluded, bool)
    on[rows, t_pos] = False
    return ((S64 < st - tau) & on).sum(1), ((S64 <= st + tau) & on).sum(1)


def loop_counts(ent, W_R, rel, triples, known, side, lo, hi):
    """The literal statement, one triple and one candidate at a time, in float64: (lt, eq) lists."""
    ent, W_R, rel = (np.asarray(x, np.float64) for x in (ent, W_R, rel))

    def unit(x):
        return x / max(np.sqrt((x * x).sum()), 1e-12)

    def score(h, r, t):
        v = unit(ent[h] @ W_R[r]) + unit(rel[r]) - unit(ent[t] @ W_R[r])
        return float((v * v).sum())

    lts, eqs = [], []
    for h, r, t in triples:
        true = score(h, r, t)
        lt = eq = 0
        for c in range(lo, hi):
            cand = (h, r, c) if side == "tail" else (c, r, t)
            if c == (t if side == "tail" else h) or cand in known:
                continue
            s = score(*cand)
            lt += s < true
            eq += s == true
        lts.append(lt)
        eqs.append(eq)
    return lts, eqs


def metrics_ref(ranks, hits):
    ranks = [float(x) for x in ranks]
    out = {"mr": sum(ranks) / len(ranks), "mrr": sum(1.0 / x for x in ranks) / len(ranks), "n": len(ranks)}
    for k in hits:
        out["hits@%d" % k] = sum(x <= k for x in ranks) / len(ranks)
    return out


# ------------------------------------------------------------------------------------------------ end-to-end cases
N_REL = 5          # relation 4 has triples and no query
E2E_SIZES = (300, 5000)
E2E_WIDTHS = ((16, 16), (64, 64), (64, 32))
N_QUERIES = 120


def ckg_layout(N):
    """users | items | attribute entities"""
    n_users, n_items = N // 3, (2 * N) // 5
    return n_users, n_items, N - n_users - n_items


@functools.lru_cache(maxsize=None)
def e2e_params(N, d, k, seed=11):
    g = torch.Generator().manual_seed(seed + N + 7 * d + k)
    ent = torch.randn(N, d, generator=g)
    W_R = torch.randn(N_REL, d, k, generator=g) * (2.0 / (d + k)) ** 0.5
    rel = torch.randn(N_REL, k, generator=g)
    return ent, W_R, rel


@functools.lru_cache(maxsize=None)
def random_ckg(N, d, k, fitted=True, seed=5):
    """fitted=False: heads and tails both drawn at random - true answers anywhere in the score distribution (used at
    N = 300, where the cap holds for them too).  fitted=True: (triples (M, 3) int64 with duplicates, item range) of a CKG that the Gaussian parameters e2e_params(N, d, k)
    FIT, as a trained embedding fits its graph: relation 0 user -> item, 1 item -> attribute, 2 item -> item,
    3 attribute -> item with random heads and, per head, a tail drawn among the best-scoring fiftieth of the
    relation's tail range; relation 4 anything -> anything at random (it gets no query).
    Why fitted: a band of half-width tau around s_t is open with probability about 2 tau x (the density of candidate
    scores at s_t).  For a true answer placed at random that density is N / (the spread of the scores, about 1):
    3 % of the queries at N = 5000 and tau = 3e-6, above BAND_CAP.  In the best fiftieth of the candidates - where
    link prediction metrics are decided - the scores lie an order of magnitude further apart."""
    rng = np.random.default_rng(seed + N)
    ent, W_R, rel = (x.double() for x in e2e_params(N, d, k))
    nu, ni, na = ckg_layout(N)
    users, items, attrs = (0, nu), (nu, nu + ni), (nu + ni, N)
    parts = []
    for r, a, b in [(0, users, items), (1, items, attrs), (2, items, items), (3, attrs, items)]:
        heads = rng.integers(*a, N // 2)
        q = F.normalize(ent[torch.as_tensor(heads)] @ W_R[r], dim=1) + F.normalize(rel[r:r + 1], dim=1)
        score = -(q @ F.normalize(ent[b[0]:b[1]] @ W_R[r], dim=1).t()).numpy()     # the order of |q - p|^2, |p| = 1
        top = max(3, (b[1] - b[0]) // 50)
        best = np.argpartition(score, top - 1, axis=1)[:, :top]
        tails = b[0] + best[np.arange(len(heads)), rng.integers(0, top, len(heads))]
        if not fitted:
            tails = rng.integers(*b, len(heads))
        parts.append(np.stack([heads, np.full(len(heads), r), tails], 1))
    parts.append(np.stack([rng.integers(0, N, 2 * N), np.full(2 * N, N_REL - 1), rng.integers(0, N, 2 * N)], 1))
    trip = np.concatenate(parts)
    trip = np.concatenate([trip, trip[rng.integers(0, len(trip), N // 2)]])       # repeated triples
    return trip.astype(np.int64), items


def e2e_queries(N, d, k, side, items_only, fitted=True, n=N_QUERIES, seed=3):
    """n triples of relations 0..3 (drawn from the CKG, in mixed relation order) whose answer on `side` lies in the
    candidate range."""
    trip, items = random_ckg(N, d, k, fitted)
    rng = np.random.default_rng(seed + N)
    ans = trip[:, 2] if side == "tail" else trip[:, 0]
    ok = trip[:, 1] < N_REL - 1
    if items_only:
        ok &= (ans >= items[0]) & (ans < items[1])
    pick = rng.choice(np.flatnonzero(ok), n, replace=False)
    return trip[pick]


@functools.lru_cache(maxsize=None)
def e2e_case(N, d, k, side, items_only, fitted=True):
    """Everything a band test needs, computed once: queries, candidate range, fp64 scores per query (rows of the
    candidate range), the excluded mask, tau, and the band."""
    trip, items = random_ckg(N, d, k, fitted)
    ent, W_R, rel = e2e_params(N, d, k)
    q = e2e_queries(N, d, k, side, items_only, fitted)
    lo, hi = items if items_only else (0, N)
    anchor = q[:, 0] if side == "tail" else q[:, 2]
    answer = q[:, 2] if side == "tail" else q[:, 0]
    S64 = np.empty((len(q), hi - lo))
    worst = 0.0
    for r in np.unique(q[:, 1]):
        sel = np.flatnonzero(q[:, 1] == r)
        S64[sel] = direct_scores(ent, W_R[r], rel[r], anchor[sel], side, lo, hi)
        s32 = direct_scores(ent, W_R[r], rel[r], anchor[sel], side, lo, hi, dtype=torch.float32)
        worst = max(worst, float(np.abs(s32 - S64[sel]).max()))
    known = {}
    for h, r, t in trip:
        key, val = ((h, r), t) if side == "tail" else ((t, r), h)
        known.setdefault(key, set()).add(val)
    excluded = np.zeros(S64.shape, bool)
    for j, (a, r) in enumerate(zip(anchor, q[:, 1])):
        ids = np.array([x for x in known.get((a, r), ()) if lo <= x < hi], np.int64)
        excluded[j, ids - lo] = True
    tau = max(TAU_FLOOR, FACTOR * worst)
    lt_lo, lt_hi = band(S64, answer - lo, excluded, tau)
    return types.SimpleNamespace(N=N, d=d, k=k, side=side, lo=lo, hi=hi, triples=q, S64=S64, excluded=excluded, tau=tau,
                                 restatement_err=worst, lt_lo=lt_lo, lt_hi=lt_hi, t_pos=answer - lo,
                                 open_share=float((lt_lo != lt_hi).mean()))


def check_band(case, lt, eq):
    """lt_lo <= lt <= lt + eq <= lt_hi for every query, and the band narrow enough to mean something."""
    lt, eq = np.asarray(lt, np.int64), np.asarray(eq, np.int64)
    assert case.open_share <= BAND_CAP, ("the band is open for %.1f %% of the queries" % (100 * case.open_share))
    bad = ~((case.lt_lo <= lt) & (eq >= 0) & (lt + eq <= case.lt_hi))
    assert not bad.any(), (int(bad.sum()), lt[bad][:5], eq[bad][:5], case.lt_lo[bad][:5], case.lt_hi[bad][:5])


def make_model(K, N, d, k, device):
    """A KGATPropagation that carries the case's parameters."""
    ent, W_R, rel = e2e_params(N, d, k)
    model = K.KGATPropagation(N, N_REL, input_node_dim=d, relation_dim=k, num_gnn_layers=1, n_hidden=16, dropout=0.0)
    with torch.no_grad():
        model.entity_embed.weight.copy_(ent)
        model.W_R.copy_(W_R)
        model.relation_embed.weight.copy_(rel)
    return model.to(device)
