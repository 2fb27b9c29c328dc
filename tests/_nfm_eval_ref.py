"""numpy restatement of the fused NFM evaluation sweep (kgat_nfm_eval_topk_f32; a helper, no test): inputs, float64
keys, the ranked lists of the stated total order and the rounding bound of the arithmetic stated in include/kgat_hip.h."""
import numpy as np

U = 2.0 ** -24     # unit roundoff of fp32


def gamma(n):
    """n roundings in a row: (1 + u)^n - 1 <= n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def exact_inputs(seed, n_rows, n_items, d, hidden, order="random"):
    """Small integers everywhere: every product and sum below is exact in fp32, and keys tie often.  V, P in {-2..2},
    W1 in {-1, 0, 1}, C, h, lin, user_const integers.  `order`: "ascending" / "descending" add a multiple of the item
    position to lin that exceeds the spread of the MLP term (the keys of EVERY user then ascend / descend with the
    position); "equal": h = 0 and one lin for all items (every key of a user is the same)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    inp = dict(V=rng.integers(-2, 3, (n_rows, d)).astype(f), W1=rng.integers(-1, 2, (hidden, d)).astype(f),
               P=rng.integers(-2, 3, (n_items, d)).astype(f), C=rng.integers(-3, 4, (n_items, hidden)).astype(f),
               h=rng.integers(-2, 3, hidden).astype(f), lin=rng.integers(-2, 3, n_items).astype(f),
               const=rng.integers(-5, 6, n_rows).astype(f))
    if order == "equal":
        inp["h"][:] = 0
        inp["lin"][:] = 3
    elif order != "random":
        s = mlp_term(inp, np.arange(n_rows))
        step = 2.0 ** np.ceil(np.log2(2 * np.abs(s).max() + 8))
        pos = np.arange(n_items) if order == "ascending" else np.arange(n_items)[::-1]
        inp["lin"] = (inp["lin"] + step * pos).astype(f)
        assert step * n_items < 2 ** 23
    return inp


def pre_activation(inp, rows):
    """pre[u, i, j] in float64 (and the sum of magnitudes the chain's bound needs)."""
    V, W1, P, C = (inp[k].astype(np.float64) for k in ("V", "W1", "P", "C"))
    a = W1[None, :, :] * V[rows][:, None, :]                       # (users, hidden, d)
    pre = np.einsum("ujc,ic->uij", a, P) + C[None]
    mag = np.einsum("ujc,ic->uij", np.abs(a), np.abs(P)) + np.abs(C)[None]
    return pre, mag


def mlp_term(inp, rows):
    pre, _ = pre_activation(inp, rows)
    return np.maximum(pre, 0.0) @ inp["h"].astype(np.float64)


def keys_and_bounds(inp, rows, with_const=True):
    """(key, score, key_bound, score_bound) in float64, (users, items) each.  Roundings counted on the stated order:
    a = fl(W1 v) and the chain of d fmas from C give pre to gamma(d + 1) (sum_c |W1 v P| + |C|); relu adds none; a
    half's sum is hidden / 2 fmas from 0, the two halves one addition: gamma(hidden / 2 + 1) on sum_j |h_j| relu_j,
    applied to the perturbed relu; the key and the score are one addition each."""
    d, hidden = inp["W1"].shape[1], inp["W1"].shape[0]
    pre, mag = pre_activation(inp, rows)
    h = np.abs(inp["h"].astype(np.float64))
    e_pre = gamma(d + 1) * mag
    relu = np.maximum(pre, 0.0)
    s = relu @ inp["h"].astype(np.float64)
    g2 = gamma(hidden // 2 + 1)
    e_s = (1.0 + g2) * (e_pre @ h) + g2 * (relu @ h)
    lin = inp["lin"].astype(np.float64)[None]
    key = s + lin
    e_key = e_s + U * (np.abs(s) + np.abs(lin) + e_s)
    if not with_const:
        return key, key, e_key, e_key
    const = inp["const"].astype(np.float64)[rows][:, None]
    score = key + const
    e_score = e_key + U * (np.abs(key) + np.abs(const) + e_key)
    return key, score, e_key, e_score


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if ptr[-1] else np.zeros(0, dtype=np.int32)
    return ptr, flat


def ranked(key, score, train_lists, K):
    """The lists of the stated order: key descending (fp32 compare, -0 = +0), equal keys by ascending position - a
    stable descending sort -, training items removed, -1 / -inf padding.  key, score: (users, items)."""
    n_users, n_items = key.shape
    items = np.full((n_users, K), -1, dtype=np.int32)
    scores = np.full((n_users, K), -np.inf, dtype=np.float32)
    k32 = key.astype(np.float32)
    for r in range(n_users):
        order = np.argsort(-(k32[r] + np.float32(0.0)), kind="stable")
        seen = np.zeros(n_items, dtype=bool)
        seen[np.asarray(train_lists[r], dtype=np.int64)] = True
        order = order[~seen[order]][:K]
        items[r, :len(order)] = order
        scores[r, :len(order)] = score[r, order].astype(np.float32)
    return items, scores


def random_train_lists(seed, n_users, n_items, most=12):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n_items, size=min(n_items, int(rng.integers(0, most + 1))), replace=False)) for _ in range(n_users)]
