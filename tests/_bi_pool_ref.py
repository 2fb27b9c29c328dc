"""Bi-Interaction pooling restated in numpy (a helper, no test): forward and backward in float64 (or, for the exactness
checks, in float32), the error bounds the device is held to, and the worlds of feature sets the GPU tests share.

A pooled set is ``[extra[m]] + list(items[m])`` (extra first, left out where negative); lists are multisets."""
import numpy as np


def set_lists(indptr, ids, items, extra=None):
    """The pooled sets as one flat id array in set order (extra first) with its offsets: (f, ptr)."""
    indptr, ids, items = np.asarray(indptr, np.int64), np.asarray(ids, np.int64), np.asarray(items, np.int64)
    parts = []
    for m, j in enumerate(items):
        own = ids[indptr[j]:indptr[j + 1]]
        if extra is not None and extra[m] >= 0:
            own = np.concatenate([[int(extra[m])], own])
        parts.append(own)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    f = np.concatenate(parts).astype(np.int64) if ptr[-1] else np.zeros(0, np.int64)
    return f, ptr


def _segment_sum(rows, ptr):
    """Row sums of the segments ptr[m]:ptr[m + 1] of `rows`, each added up from +0 (empty segments: zero; a segment of
    terms that are all -0 sums to +0, as an accumulator that starts at +0 does)."""
    out = np.zeros((len(ptr) - 1,) + rows.shape[1:], rows.dtype)
    full = np.flatnonzero(np.diff(ptr) > 0)
    if len(full):
        out[full] = np.add.reduceat(rows, ptr[full], axis=0) + rows.dtype.type(0)
    return out


def forward(V, w, f, ptr, dtype=np.float64):
    """(S, bi, lin, sq) of the sets (f, ptr) in `dtype`."""
    V = np.asarray(V, dtype)
    rows = V[f]
    S = _segment_sum(rows, ptr)
    Q = _segment_sum(rows * rows, ptr)
    bi = (S * S - Q) * dtype(0.5)
    lin = _segment_sum(np.asarray(w, dtype)[f], ptr) if w is not None else np.zeros(len(ptr) - 1, dtype)
    return S, bi, lin, Q.sum(1)


def brute_bi(V, own):
    """sum_{a<b} v_a * v_b over the positions of one set, literally."""
    V = np.asarray(V, np.float64)
    out = np.zeros(V.shape[1])
    for a in range(len(own)):
        for b in range(a + 1, len(own)):
            out += V[own[a]] * V[own[b]]
    return out


def _by_feature(f, n_nodes):
    order = np.argsort(f, kind="stable")
    counts = np.bincount(f, minlength=n_nodes)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), counts


def backward(V, f, ptr, S, g_bi, g_lin, g_sq, dtype=np.float64):
    """(grad_V, grad_w): grad_V[x] = sum over the occurrences of x in the sets m of g_bi[m] (S[m] - v_x) + 2 g_sq[m] v_x,
    grad_w[x] = sum of g_lin[m] over the same occurrences; any of the three incoming gradients may be None (zero)."""
    V = np.asarray(V, dtype)
    n, d = V.shape
    M = len(ptr) - 1
    set_of = np.repeat(np.arange(M), np.diff(ptr))
    g_bi = np.zeros((M, d), dtype) if g_bi is None else np.asarray(g_bi, dtype)
    g_lin = np.zeros(M, dtype) if g_lin is None else np.asarray(g_lin, dtype)
    g_sq = np.zeros(M, dtype) if g_sq is None else np.asarray(g_sq, dtype)
    rows = V[f]
    terms = g_bi[set_of] * (np.asarray(S, dtype)[set_of] - rows) + (dtype(2) * g_sq[set_of])[:, None] * rows
    order, fptr, _ = _by_feature(f, n)
    return _segment_sum(terms[order], fptr), _segment_sum(g_lin[set_of][order], fptr)


def forward_bounds(V, w, f, ptr):
    """Per-element bounds of the fp32 forward against fp64, n the set's length:
    bi: (n + 4) 2^-24 ((sum |v|)^2 + sum v^2); S, lin, sq: (n + 4) 2^-24 sum |term|."""
    V = np.asarray(V, np.float64)
    n = np.diff(ptr).astype(np.float64)
    rows = V[f]
    A = _segment_sum(np.abs(rows), ptr)
    Q = _segment_sum(rows * rows, ptr)
    u = (n + 4.0) * 2.0 ** -24
    lin = u * _segment_sum(np.abs(np.asarray(w, np.float64))[f], ptr) if w is not None else np.zeros(len(n))
    return {"S": u[:, None] * A, "bi": u[:, None] * (A * A + Q), "lin": lin, "sq": u * Q.sum(1)}


def backward_bounds(V, f, ptr, g_bi, g_lin, g_sq):
    """grad_V: (h + n + 4) 2^-24 x the sum of the absolute values of its terms - |g_bi| (sum_set |v| + |v_x|) +
    2 |g_sq| |v_x| per occurrence - with h the hits of the row and n the longest set among them; grad_w: (h + 4) 2^-24
    sum |g_lin|."""
    V = np.asarray(V, np.float64)
    N, d = V.shape
    M = len(ptr) - 1
    set_of = np.repeat(np.arange(M), np.diff(ptr))
    rows = np.abs(V[f])
    A = _segment_sum(rows, ptr)
    g_bi = np.zeros((M, d)) if g_bi is None else np.abs(np.asarray(g_bi, np.float64))
    g_lin = np.zeros(M) if g_lin is None else np.abs(np.asarray(g_lin, np.float64))
    g_sq = np.zeros(M) if g_sq is None else np.abs(np.asarray(g_sq, np.float64))
    terms = g_bi[set_of] * (A[set_of] + rows) + (2.0 * g_sq[set_of])[:, None] * rows
    order, fptr, h = _by_feature(f, N)
    longest = np.zeros(N)
    np.maximum.at(longest, f, np.diff(ptr)[set_of].astype(np.float64))
    u = (h + longest + 4.0) * 2.0 ** -24
    return {"grad_V": u[:, None] * _segment_sum(terms[order], fptr), "grad_w": (h + 4.0) * 2.0 ** -24 * _segment_sum(g_lin[set_of][order], fptr),
            "abs_terms": _segment_sum(terms[order], fptr)}


# ------------------------------------------------------------------------------------------------ the shared worlds
N_TERNARY = 1000          # features [0, 1000): the ids of the 1,000-long list; exact inputs there are in {-1, 0, 1}
N_NODES = 1200            # features [1000, 1200) double as the users (the extras)
HUB = 7
LONG = 1000
AT_255, AT_256 = 1198, 1199   # (hub world) features in exactly 255 and 256 lists: either side of the 256-source threshold
N_DRAW = 1198             # random list entries come from [0, N_DRAW): _draw


def list_lengths(d):
    """The set lengths the tests must hit, counting the extra: 0, 1, 2; G - 1, G, G + 1 with G = 256 / d the lane groups
    of a wavefront; 4 G - 1, 4 G, 4 G + 1 - the rows a wavefront has in flight (four per group), where the kernels' loop
    takes another turn; 63, 64, 65 and 1,000."""
    G = 256 // d
    return sorted({0, 1, 2, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 63, 64, 65, LONG})


_worlds = {}


def _draw(rng, n):
    """n list entries: each with equal chance a {-1, 0, 1} row or a row of multiples of 1/4 up to 2."""
    return np.where(rng.random(n) < 0.5, rng.integers(0, N_TERNARY, n), rng.integers(N_TERNARY, N_DRAW, n))


def world(d, hub=False):
    """(indptr, ids, cases): items whose lists have every length of list_lengths(d) and one less (so that each length is
    met with and without an extra), an item with a repeated id, 40 random items; with `hub`, 1,100 short items more and
    feature HUB in every list.
    cases: item position -> what it is."""
    key = (d, hub)
    if key in _worlds:
        return _worlds[key]
    rng = np.random.default_rng(1000 + d)
    want = list_lengths(d)
    lens = sorted(set(want) | {x - 1 for x in want if x >= 1})
    lists = []
    for n in lens:
        if n >= LONG - 1:
            own = rng.permutation(N_TERNARY)[:n]          # distinct ternary features
        else:
            own = _draw(rng, n)
        lists.append(own)
    dup = len(lists)
    lists.append(np.array([1100, 3, 1100, 1150, 3, 3]))   # a multiset
    for _ in range(40):
        lists.append(_draw(rng, rng.integers(1, 41)))
    if hub:
        # 1,100 two-to-four-entry items: the hub's reversed list passes 1,024 entries (several looks per wavefront)
        for t in range(1100):
            lists.append(np.array([int(rng.integers(N_TERNARY, N_DRAW))] + [AT_255] * (t < 255) + [AT_256] * (t < 256)))
        lists = [np.concatenate([own[:len(own) // 2], [HUB], own[len(own) // 2:]]) for own in lists]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ids = np.concatenate(lists).astype(np.int64)
    _worlds[key] = (indptr, ids, {"by_len": dict(zip(lens, range(len(lens)))), "dup": dup, "n_items": len(lists)})
    return _worlds[key]


def batch(d, n_sets, hub=False, seed=0):
    """(items, extra) of n_sets pooled sets over world(d, hub).  In order, as far as n_sets reaches: the 1,000-long list
    with an extra that is in it; every length with and without an extra; the multiset item with an extra from its own
    list; one item five times, split across the two halves of the batch, under one repeated user; random sets."""
    indptr, ids, info = world(d, hub)
    rng = np.random.default_rng(seed + 17 * n_sets + d)
    by_len = info["by_len"]
    users = np.arange(N_TERNARY, N_NODES)
    head = []
    long_item = by_len[LONG - 1]
    head.append((long_item, int(ids[indptr[long_item] + 5])))          # length 1,000 counting an extra that is in the list
    head.append((by_len[0], -1))                                       # the empty set
    head.append((by_len[0], 1003))                                     # length 1: the extra alone
    for n in sorted(by_len):
        head.append((by_len[n], -1))
        if n < LONG:
            head.append((by_len[n], int(users[rng.integers(len(users))]) if n < LONG - 1 else int(rng.integers(N_TERNARY))))
    head.append((info["dup"], 3))
    head = head[:n_sets]
    rest = n_sets - len(head)
    items = rng.integers(0, info["n_items"], rest)
    items = np.where(np.isin(items, [by_len[LONG - 1], by_len[LONG]]), info["dup"], items)   # (the long lists: in the head only)
    extra = np.where(rng.random(rest) < 0.2, -1, users[rng.integers(0, len(users), rest)])
    if rest >= 10:
        five = info["dup"] + 3
        spots = np.concatenate([rng.choice(rest // 2, 3, replace=False), rest // 2 + rng.choice(rest - rest // 2, 2, replace=False)])
        items[spots] = five
        extra[spots] = 1111                                            # ... under the same user
        extra[rng.choice(rest, min(rest, 8), replace=False)] = 1111
    it = np.concatenate([[h[0] for h in head], items]).astype(np.int32)
    ex = np.concatenate([[h[1] for h in head], extra]).astype(np.int32)
    return it, ex


def exact_values(rng, d, w=True):
    """V with rows [0, 1000) in {-1, 0, 1} and the others multiples of 1/4 in [-2, 2]; w_lin multiples of 1/4 in [-2, 2]."""
    V = np.empty((N_NODES, d), np.float32)
    V[:N_TERNARY] = rng.integers(-1, 2, (N_TERNARY, d))
    V[N_TERNARY:] = rng.integers(-8, 9, (N_NODES - N_TERNARY, d)) / 4.0
    return V, (rng.integers(-8, 9, N_NODES) / 4.0).astype(np.float32) if w else None


def exact_grads(rng, n_sets, d):
    return ((rng.integers(-8, 9, (n_sets, d)) / 4.0).astype(np.float32), (rng.integers(-8, 9, n_sets) / 4.0).astype(np.float32),
            (rng.integers(-8, 9, n_sets) / 4.0).astype(np.float32))


def real_values(rng, d):
    """N(0, 1) rows, every seventh scaled by 1e-2 and every eleventh by 30."""
    V = rng.standard_normal((N_NODES, d))
    V[::7] *= 1e-2
    V[::11] *= 30.0
    return V.astype(np.float32), rng.standard_normal(N_NODES).astype(np.float32)
