"""numpy restatement of the top-4 reducer (kgat_spmm_umule_max4_f32) and of the ranked attention-path search built on
it (dgl_kgat_amd.explain.attention_paths(top=2..4)).  Every candidate is one fp32 multiply and a selection never rounds,
so the device results must equal these bit for bit."""
import numpy as np

from _max_ref import csr_order


def _ascending_bits(x):
    """uint64 keys (below 2^32) that order as the float32 values do: the bit pattern with the sign bit set for x >= 0
    and all bits flipped for x < 0.  (-0.0 would sort below 0.0: the caller has made them one.)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint64)


def spmm_max4(n_nodes, src, dst, X, w=None):
    """(out, arg_eid, arg_pos, arg_slot), each (n_nodes, Q, 4): the four largest of {w[e] * X[src[e], q, s]} over the
    in-edges e of v and the slots s (w=None: X[src[e], q, s]), in order, with the winners' bits, edge ids, CSR positions
    and source slots.  (a, i, r) beats (b, k, s) iff a > b, or a == b and (i < k, or i == k and r < s); -0.0 ties with
    0.0; inside a row the CSR positions are sorted by edge id, so one order serves both id forms.  A node without
    in-edges: out 0, args -1, slot 255.  X is (n_nodes, Q, 4), w in edge-id order.

    Per query column: one lexsort over (row, -value, id, slot) of the 4 E candidates, whose first four per row are the
    answer.  The candidates are laid out in (row, id, slot) order, so a stable sort by (row, -value) is that lexsort;
    the two keys are packed into one 64-bit integer (_ascending_bits), which sorts several times faster."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    X = np.asarray(X, np.float32)
    assert X.ndim == 3 and X.shape[2] == 4
    Q, E = X.shape[1], len(src)
    out = np.zeros((n_nodes, Q, 4), np.float32)
    arg_eid = np.full((n_nodes, Q, 4), -1, np.int32)
    arg_pos = np.full((n_nodes, Q, 4), -1, np.int32)
    arg_slot = np.full((n_nodes, Q, 4), 255, np.uint8)
    if E == 0:
        return out, arg_eid, arg_pos, arg_slot
    order = csr_order(src, dst)
    s, d = src[order], dst[order]
    wv = None if w is None else np.asarray(w, np.float32).reshape(-1)[order]
    deg = np.bincount(d, minlength=n_nodes)
    rows = np.nonzero(deg > 0)[0]
    starts = 4 * (np.cumsum(deg) - deg)[rows]
    first4 = (starts[:, None] + np.arange(4)[None, :]).reshape(-1)    # every row with an in-edge has >= 4 candidates
    row_key = np.repeat(d, 4).astype(np.uint64) << np.uint64(32)
    for q in range(Q):
        prod = X[s, q, :] if wv is None else wv[:, None] * X[s, q, :]   # (E, 4): position-major, slot-minor
        assert prod.dtype == np.float32
        flat = prod.reshape(-1)
        neg = -flat + np.float32(0.0)                                 # -0.0 and 0.0 become one key
        win = np.argsort(row_key | _ascending_bits(neg), kind="stable")[first4]   # indices into the flat candidates
        out[rows, q] = flat[win].reshape(-1, 4)
        arg_pos[rows, q] = (win // 4).reshape(-1, 4)
        arg_eid[rows, q] = order[win // 4].reshape(-1, 4)
        arg_slot[rows, q] = (win % 4).reshape(-1, 4)
    return out, arg_eid, arg_pos, arg_slot


def rank_walks(score):
    """(ranked_score, ranked_len, ranked_slot), each (Q, top), of score (Q, L, top): the best `top` walks over all
    lengths by (score descending, length ascending, slot ascending); length 0 / slot -1 / score 0 where none is left."""
    Q, L, top = score.shape
    flat = score.reshape(Q, L * top)
    idx = np.argsort(-flat, axis=1, kind="stable")[:, :top]
    ranked = np.take_along_axis(flat, idx, axis=1)
    some = ranked > 0
    return ranked, np.where(some, idx // top + 1, 0).astype(np.int64), np.where(some, idx % top, -1).astype(np.int64)


def attention_paths_top(n_nodes, src, dst, w, users, items, max_len=3, top=4):
    """(score, edges, nodes, ranked_score, ranked_len, ranked_slot) as explain.attention_paths(top=top) returns them:
    the k-best max-times recurrence over walks that start at items[q] and end at users[q], multiplying in the kernel's
    order (w_e * B_{l-1}[src e, q, s]), and the backtrack through the (edge, slot) back-pointers."""
    src = np.asarray(src, np.int64)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    Q, L = len(users), max_len
    B = np.zeros((n_nodes, Q, 4), np.float32)
    B[items, np.arange(Q), 0] = 1.0
    score = np.zeros((Q, L, top), np.float32)
    edges = np.full((Q, L, top, L), -1, np.int64)
    nodes = np.full((Q, L, top, L + 1), -1, np.int64)
    back = []
    for hop in range(L):
        B, A, _, S = spmm_max4(n_nodes, src, dst, B, w)
        back.append((A, S))
        score[:, hop] = B[users, np.arange(Q), :top]
    for q in range(Q):
        for hop in range(L):
            for r in range(top):
                if score[q, hop, r] == 0:
                    continue
                at, slot = int(users[q]), r
                nodes[q, hop, r, hop + 1] = at
                for j in range(hop, -1, -1):
                    e, slot = int(back[j][0][at, q, slot]), int(back[j][1][at, q, slot])
                    at = int(src[e])
                    edges[q, hop, r, j] = e
                    nodes[q, hop, r, j] = at
    return (score, edges, nodes) + rank_walks(score)
