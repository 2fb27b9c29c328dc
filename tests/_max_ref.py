"""numpy restatement of the max reducer (kgat_spmm_umule_max_f32) and of the attention-path search built on it
(dgl_kgat_amd.explain.attention_paths).  Every message is one fp32 multiply and `max` never rounds, so the device
results must equal these bit for bit."""
import numpy as np


def csr_order(src, dst):
    """Positions of the destination-major CSR: edges sorted by (dst, edge id).  order[p] = edge id at position p."""
    dst = np.asarray(dst, np.int64)
    return np.lexsort((np.arange(len(dst)), dst))


def spmm_max(n_nodes, src, dst, X, w=None):
    """(out, arg_eid, arg_pos): out[v, j] = max over in-edges e of v of w[e] * X[src[e], j] (w=None: X[src[e], j]) with
    the bits of the winner; among equal products the smallest edge id wins (== the smallest CSR position: positions are
    sorted by edge id inside a row).  A node without in-edges: out 0, arg -1.  w in edge-id order."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    X = np.asarray(X, np.float32)
    D, E = X.shape[1], len(src)
    out = np.zeros((n_nodes, D), np.float32)
    arg_eid = np.full((n_nodes, D), -1, np.int32)
    arg_pos = np.full((n_nodes, D), -1, np.int32)
    if E == 0:
        return out, arg_eid, arg_pos
    order = csr_order(src, dst)
    s, d = src[order], dst[order]
    prod = X[s] if w is None else (np.asarray(w, np.float32).reshape(-1)[order][:, None] * X[s])
    assert prod.dtype == np.float32
    deg = np.bincount(d, minlength=n_nodes)
    rows = np.nonzero(deg > 0)[0]
    starts = (np.cumsum(deg) - deg)[rows]
    top = np.maximum.reduceat(prod, starts, axis=0)                   # (rows, D)
    seg = np.repeat(np.arange(len(rows)), deg[rows])                  # sorted position -> index into rows
    cand = np.where(prod == top[seg], np.arange(E, dtype=np.int32)[:, None], np.int32(E))   # -0.0 == 0.0: a tie
    pos = np.minimum.reduceat(cand, starts, axis=0)
    assert (pos < E).all()
    out[rows] = np.take_along_axis(prod, pos, axis=0)                 # the winner's bits
    arg_pos[rows] = pos
    arg_eid[rows] = order[pos]
    return out, arg_eid, arg_pos


def attention_paths(n_nodes, src, dst, w, users, items, max_len=3):
    """(score, edges, nodes, best_len) as explain.attention_paths returns them: the max-times DP over walks that start
    at items[q] and end at users[q], multiplying in the kernel's order (w_e * B_{l-1}[src e]), and the backtrack
    through the argmax edges."""
    src = np.asarray(src, np.int64)
    Q, L = len(users), max_len
    B = np.zeros((n_nodes, Q), np.float32)
    B[np.asarray(items, np.int64), np.arange(Q)] = 1.0
    score = np.zeros((Q, L), np.float32)
    edges = np.full((Q, L, L), -1, np.int64)
    nodes = np.full((Q, L, L + 1), -1, np.int64)
    args = []
    for hop in range(L):
        B, A, _ = spmm_max(n_nodes, src, dst, B, w)
        args.append(A)
        score[:, hop] = B[np.asarray(users, np.int64), np.arange(Q)]
    for q in range(Q):
        for hop in range(L):
            if score[q, hop] == 0:
                continue
            at = int(users[q])
            nodes[q, hop, hop + 1] = at
            for j in range(hop, -1, -1):
                e = int(args[j][at, q])
                at = int(src[e])
                edges[q, hop, j] = e
                nodes[q, hop, j] = at
    best_len = np.where(score.max(1) > 0, score.argmax(1) + 1, 0) if Q else np.zeros(0, np.int64)
    return score, edges, nodes, best_len.astype(np.int64)
