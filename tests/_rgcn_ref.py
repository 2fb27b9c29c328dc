"""What the relational-convolution tests share (a helper, no test): a numpy fp64 restatement of the three quantities the
kgat_rgcn_* entries compute, from the COO, with the per-element sum of absolute terms S and term count n that the tests'
error bounds are made of, and the adversarial graph the GPU tests walk.

    Z[v, b, :]  = sum_{e: u->v} norm[e] a[etype[e], b] x[u, :]
    g_x[u, :]   = sum_{u->e} sum_b norm[e] a[etype[e], b] g_Z[dst e, b, :]
    g_a[r, b]   = sum_{e: etype[e] = r} norm[e] <x[src e, :], g_Z[dst e, b, :]>

An edge whose type is outside [0, R) contributes nothing, as in the kernels."""
import numpy as np

N_NODES = 300
N_EDGES = 2000
N_REL = 5          # relation 3 has no edge, relation 4 exactly one


class Restated:
    """value, S (sum of |terms|) and n (terms per element, broadcastable) of one quantity."""

    def __init__(self, value, S, n):
        self.value, self.S, self.n = value, S, n

    def bound(self):
        """Higham's bound for n fp32 terms added in any order, each a product with two roundings: (n + 4) 2^-24 S."""
        return (self.n + 4.0) * 2.0 ** -24 * self.S


def restate(n_nodes, src, dst, et, norm, x, a, g_Z=None):
    """Z (and g_x, g_a when g_Z is given) as Restated, all fp64.  norm None: 1."""
    src, dst, et = (np.asarray(t, dtype=np.int64) for t in (src, dst, et))
    x, a = np.asarray(x, dtype=np.float64), np.asarray(a, dtype=np.float64)
    R, B = a.shape
    D = x.shape[1]
    nm = np.ones(len(src)) if norm is None else np.asarray(norm, dtype=np.float64).reshape(-1)
    ok = (et >= 0) & (et < R)
    src, dst, et, nm = src[ok], dst[ok], et[ok], nm[ok]
    c = nm[:, None] * a[et]                                               # (E, B)
    terms = c[:, :, None] * x[src][:, None, :]                            # (E, B, D)
    Z, SZ = np.zeros((n_nodes, B, D)), np.zeros((n_nodes, B, D))
    np.add.at(Z, dst, terms)
    np.add.at(SZ, dst, np.abs(terms))
    out = {"Z": Restated(Z, SZ, np.bincount(dst, minlength=n_nodes).astype(np.float64)[:, None, None])}
    if g_Z is not None:
        g = np.asarray(g_Z, dtype=np.float64)[dst]                        # (E, B, D)
        t = c[:, :, None] * g
        gx, Sx = np.zeros((n_nodes, D)), np.zeros((n_nodes, D))
        np.add.at(gx, src, t.sum(1))
        np.add.at(Sx, src, np.abs(t).sum(1))
        out["g_x"] = Restated(gx, Sx, B * np.bincount(src, minlength=n_nodes).astype(np.float64)[:, None])
        p = nm[:, None, None] * x[src][:, None, :] * g                    # (E, B, D)
        ga, Sa = np.zeros((R, B)), np.zeros((R, B))
        np.add.at(ga, et, p.sum(2))
        np.add.at(Sa, et, np.abs(p).sum(2))
        out["g_a"] = Restated(ga, Sa, D * np.bincount(et, minlength=R).astype(np.float64)[:, None])
    return out


def brute_force(n_nodes, src, dst, et, norm, x, a, g_Z):
    """The same three by loops over edges, bases and columns (python floats, i.e. fp64): what `restate` is checked against."""
    R, B = len(a), len(a[0])
    D = len(x[0])
    Z = [[[0.0] * D for _ in range(B)] for _ in range(n_nodes)]
    gx = [[0.0] * D for _ in range(n_nodes)]
    ga = [[0.0] * B for _ in range(R)]
    for e in range(len(src)):
        u, v, r = int(src[e]), int(dst[e]), int(et[e])
        if not 0 <= r < R:
            continue
        w = 1.0 if norm is None else float(norm[e])
        for b in range(B):
            for d in range(D):
                Z[v][b][d] += w * float(a[r][b]) * float(x[u][d])
                gx[u][d] += w * float(a[r][b]) * float(g_Z[v][b][d])
                ga[r][b] += w * float(x[u][d]) * float(g_Z[v][b][d])
    return np.array(Z), np.array(gx), np.array(ga)


def adversarial_graph(tile_edges, seed=0):
    """(src, dst, etype) int64 arrays in a shuffled edge-id order, N_NODES nodes, N_EDGES edges, N_REL relations, for
    the walks' tile sizes `tile_edges` (kgat_spmm_tile_edges at the widths tested: 256 and 128 edges):

    * node 0 is a destination hub of 700 in-edges: its row spans at least three tiles of the forward walk, a finish
      chain; node 1's 68 in-edges then end the row at CSR position 768, a tile edge of every size in `tile_edges`;
    * node 1 is a source hub of 748 out-edges behind node 0's 20, so the reversed walk has the same two features;
    * nodes 290 .. 299 have no edge at all; (0, 0), (5, 5) and (6, 6) are self-loops; (7, 8) occurs three times;
    * relation 3 has no edge and relation 4 owns exactly one."""
    rng = np.random.default_rng(seed)
    lo, hi = 2, 290                                     # ordinary nodes
    deg0, deg1 = 700, 68
    for te in tile_edges:
        assert (deg0 + deg1) % te == 0 and deg0 > 2 * te and N_EDGES >= 8 * te - te + 1, te
    edges = [(0, 0)]
    edges += [(int(s), 0) for s in rng.integers(lo, hi, deg0 - 1)]            # into the hub
    edges += [(int(s), 1) for s in rng.integers(lo, hi, deg1)]                # row 1 ends on the tile edge
    edges += [(1, int(t)) for t in rng.integers(lo, hi, 748)]                 # out of the source hub
    edges += [(0, int(t)) for t in rng.integers(lo, hi, 19)]                  # out-degree of node 0: 20 with its self-loop
    edges += [(5, 5), (6, 6), (7, 8), (7, 8), (7, 8)]
    rest = N_EDGES - len(edges)
    edges += list(zip(rng.integers(lo, hi, rest).tolist(), rng.integers(lo, hi, rest).tolist()))
    edges = np.array(edges, dtype=np.int64)[rng.permutation(N_EDGES)]
    src, dst = edges[:, 0].copy(), edges[:, 1].copy()
    et = rng.integers(0, 3, N_EDGES)
    et[int(rng.integers(0, N_EDGES))] = 4
    # what the docstring claims
    indeg, outdeg = np.bincount(dst, minlength=N_NODES), np.bincount(src, minlength=N_NODES)
    assert len(src) == N_EDGES and indeg[0] == deg0 and indeg[0] + indeg[1] == deg0 + deg1
    assert outdeg[0] == 20 and outdeg[0] + outdeg[1] == 768
    assert (indeg[290:] == 0).all() and (outdeg[290:] == 0).all()
    assert (et == 3).sum() == 0 and (et == 4).sum() == 1
    return src, dst, et.astype(np.int64)


def dyadic_inputs(n_nodes, n_edges, D, B, R, seed, with_norm=True):
    """x, g_Z small integers, a in {0, +-0.5, +-1, 2}, norm in {0.25, 0.5, 1} (or None): every product of the three is a
    multiple of GRANULARITY, so fp32 sums whose absolute terms stay below 2^24 granules are exact in any order."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (n_nodes, D)).astype(np.float32)
    g_Z = rng.integers(-3, 4, (n_nodes, B, D)).astype(np.float32)
    a = rng.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0], dtype=np.float32), (R, B))
    norm = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), n_edges) if with_norm else None
    return x, g_Z, a, norm


GRANULARITY = 0.125   # norm (1/4) x a (1/2) x integer
