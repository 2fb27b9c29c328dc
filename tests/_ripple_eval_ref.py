"""Restatements for the fused RippleNet evaluation sweep (a helper, no test): the contract of include/kgat_hip.h in
numpy float64, the keys pass replayed in fp32 in the header's order, the ranking rule, and the two exact input
families (uniform and saturated softmax) of tests/test_gpu_ripple_eval.py.

An input set is a dict: ent (n_nodes, d), rel (n_rel, d * d), W (d, d) float32; mem_h / mem_r / mem_t
(n_users, n_hop, M) integers; item_lo, n_items; mode 0..3 (ripple_models.UPDATE_MODES); all_hops."""
import numpy as np

N_USERS = 40
MODES = ("replace", "plus", "replace_transform", "plus_transform")


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise over float32 arrays: the product is exact in float64, the sum is
    taken with its rounding error (TwoSum) and rounded to odd, which the final rounding to float32 then cannot see."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = np.atleast_1d(s).view(np.int64).copy()
    e, s1 = np.atleast_1d(e), np.atleast_1d(s)
    inexact = e != 0
    toward = inexact & ((e > 0) != (s1 > 0))       # the exact sum is smaller in magnitude than its rounding
    bits[toward] -= 1
    bits[inexact] |= 1
    return bits.view(np.float64).astype(np.float32).reshape(np.shape(s))


def keys32(inp, users):
    """The key table of kgat_eval_ripple_keys_f32, (len(users), n_hop, M, d) float32: per element one fmaf chain in
    ascending column order from 0."""
    ent, d = inp["ent"], inp["ent"].shape[1]
    R = inp["rel"].reshape(-1, d, d)
    users = np.asarray(users, dtype=np.int64)
    h, r = inp["mem_h"][users], inp["mem_r"][users]            # (U, H, M)
    Rr, hr = R[r], ent[h]                                        # (U, H, M, d, d), (U, H, M, d)
    acc = np.zeros(hr.shape, dtype=np.float32)
    for c in range(d):
        acc = fma32(Rr[..., c], hr[..., c:c + 1].repeat(d, -1), acc)
    return acc


def scores64(inp, users):
    """y (len(users), n_items) in float64: the contract of the header, nothing else."""
    ent = inp["ent"].astype(np.float64)
    d = ent.shape[1]
    R = inp["rel"].astype(np.float64).reshape(-1, d, d)
    W = inp["W"].astype(np.float64)
    users = np.asarray(users, dtype=np.int64)
    lo, n_items, mode = inp["item_lo"], inp["n_items"], inp["mode"]
    n_hop = inp["mem_h"].shape[1]
    v = np.broadcast_to(ent[lo:lo + n_items], (len(users), n_items, d))
    o_list = []
    for k in range(n_hop):
        h, r, t = (inp[name][users, k] for name in ("mem_h", "mem_r", "mem_t"))
        key = np.einsum("umac,umc->uma", R[r], ent[h])
        s = np.einsum("uma,uia->uim", key, v)
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        o = np.einsum("uim,umc->uic", p, ent[t])
        o_list.append(o)
        x = o if mode in (0, 2) else v + o
        v = x if mode < 2 else np.einsum("ac,uic->uia", W, x)
    z = sum(o_list) if inp["all_hops"] else o_list[-1]
    return (v * z).sum(-1)


def ranked(y, train_lists, K):
    """The lists of the entry for scores y (users, items): training items dropped, (y descending with -0 = +0, position
    ascending), K entries, -1 / -inf padding.  Returns (items int32, scores float32)."""
    n_users, n_items = y.shape
    items = np.full((n_users, K), -1, dtype=np.int32)
    scores = np.full((n_users, K), -np.inf, dtype=np.float32)
    for u in range(n_users):
        keep = np.ones(n_items, dtype=bool)
        keep[np.asarray(train_lists[u], dtype=np.int64)] = False
        pos = np.nonzero(keep)[0]
        order = pos[np.argsort(-(y[u, pos] + 0.0), kind="stable")][:K]
        items[u, :len(order)] = order
        scores[u, :len(order)] = y[u, order]
    return items, scores


def csr(train_lists):
    ptr = np.zeros(len(train_lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(x) for x in train_lists])
    flat = np.concatenate([np.sort(np.asarray(x, dtype=np.int32)) for x in train_lists]) if len(train_lists) else np.zeros(0, np.int32)
    return ptr, flat.astype(np.int32)


def random_train_lists(seed, n_users, n_items, most=9):
    rng = np.random.default_rng(seed)
    most = max(0, min(most, n_items - 1))
    return [np.sort(rng.choice(n_items, int(rng.integers(0, most + 1)), replace=False)) for _ in range(n_users)]


def _relations(rng, n_rel, n_hop, M):
    return np.sort(rng.integers(0, n_rel, (N_USERS, n_hop, M)), axis=2)


def uniform_inputs(seed, n_items, d, M, n_hop, mode, all_hops, order=None):
    """relation_emb = 0: every logit is 0 and, M a power of two, p = 1 / M exactly.  Rows in {-1, 0, 1}, W in {-1, 0, 1}
    with two entries per row: every value below is a multiple of 2^-6 under 2^5 and every partial sum of y a multiple of
    2^-12 under 2^11 - representable.  `order`: column 0 of the item rows is +position / -position / 0, the users' tail
    rows are one node with row e_0 and the model is `plus`, one hop: y = <v_0 + e_0, e_0> = v_0[0] + 1."""
    assert M & (M - 1) == 0
    rng = np.random.default_rng(seed)
    f = np.float32
    n_nodes, n_rel = N_USERS + n_items + 100, 5
    ent = rng.integers(-1, 2, (n_nodes, d)).astype(f)
    W = np.zeros((d, d), dtype=f)
    for a in range(d):
        W[a, rng.choice(d, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
    mem_h = rng.integers(0, n_nodes, (N_USERS, n_hop, M))
    mem_t = rng.integers(0, n_nodes, (N_USERS, n_hop, M))
    if order is not None:
        assert mode == 1 and n_hop == 1
        pos = np.arange(n_items, dtype=f)
        ent[N_USERS:N_USERS + n_items, 0] = {"ascending": pos, "descending": -pos, "equal": 0 * pos}[order]
        ent[n_nodes - 1] = 0
        ent[n_nodes - 1, 0] = 1
        mem_t[:] = n_nodes - 1
    return dict(ent=ent, rel=np.zeros((n_rel, d * d), dtype=f), W=W, mem_h=mem_h, mem_r=_relations(rng, n_rel, n_hop, M),
                mem_t=mem_t, item_lo=N_USERS, n_items=n_items, mode=mode, all_hops=all_hops)


def saturated_inputs(seed, n_items, d, M, n_hop, mode, all_hops):
    """R_r = I.  The last q = d / 4 columns are selector columns Q.  An item row is a e_c, a in 1..4, c outside Q.  The
    head row of slot i of hop 1 is 0 on its own columns C_i (the columns outside Q dealt over the slots, another deal per
    variant) and -256 on the others: for every item exactly one slot has logit 0, the others <= -256, whose exponential
    is 0 in fp32 - p is one-hot and the slot depends on the item.  Tail rows are small integers outside Q and a one-hot
    on Q; W maps Q to Q by a permutation and nothing else to Q, so v_1 restricted to Q is a one-hot in every mode; the
    head rows of hop 2 are 0 outside Q and 0 / -256 on Q in the same way: the second hop's logits are 0 or -256 as
    well.  Everything is an integer below 2^23."""
    rng = np.random.default_rng(seed)
    f = np.float32
    q = d // 4
    nq = d - q
    G = 4                                                    # variants of the deal
    n_heads = 2 * G * M
    n_tails = 60
    n_nodes = N_USERS + n_items + n_heads + n_tails
    n_rel = 5
    ent = np.zeros((n_nodes, d), dtype=f)
    item = slice(N_USERS, N_USERS + n_items)
    ent[item] = 0
    ent[np.arange(N_USERS, N_USERS + n_items), rng.integers(0, nq, n_items)] = rng.integers(1, 5, n_items)
    ent[:N_USERS] = rng.integers(-1, 2, (N_USERS, d))
    head0 = N_USERS + n_items
    for hop in range(2):
        cols = np.arange(nq) if hop == 0 else np.arange(nq, d)
        for g in range(G):
            deal = rng.permutation(len(cols)) if len(cols) >= M else rng.permutation(M)[:len(cols)]
            rows = ent[head0 + (hop * G + g) * M:head0 + (hop * G + g + 1) * M]
            rows[:, cols] = -256
            rows[deal % M, cols] = 0                         # column cols[j] belongs to slot deal[j] mod M
    tail0 = head0 + n_heads
    ent[tail0:, :nq] = rng.integers(-2, 3, (n_tails, nq))
    ent[np.arange(tail0, n_nodes), nq + rng.integers(0, q, n_tails)] = 1
    W = rng.integers(-1, 2, (d, d)).astype(f)
    W[nq:] = 0
    W[nq + np.arange(q), nq + rng.permutation(q)] = 1
    mem_h = np.zeros((N_USERS, n_hop, M), dtype=np.int64)
    for u in range(N_USERS):
        for k in range(n_hop):
            mem_h[u, k] = head0 + (k * G + (u + k) % G) * M + rng.permutation(M)
    mem_t = rng.integers(tail0, n_nodes, (N_USERS, n_hop, M))
    rel = np.tile(np.eye(d, dtype=f).reshape(1, -1), (n_rel, 1))
    return dict(ent=ent, rel=rel, W=W, mem_h=mem_h, mem_r=_relations(rng, n_rel, n_hop, M), mem_t=mem_t, item_lo=N_USERS,
                n_items=n_items, mode=mode, all_hops=all_hops)
