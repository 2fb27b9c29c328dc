"""Planted graphs, exact-arithmetic inputs and the two checkers of the forward aggregation tests
(tests/test_sparse_forward_host.py, tests/test_gpu_sparse_forward.py).  numpy only; no device, no test.

Two bars, neither of them measured:

* ``check_equal``: on ``exact_inputs`` (X in {+-1, +-2, +-3}, w in {1/4, 1/2, 1, 2}) every product is a multiple of
  1/4 and every partial sum of a row, in ANY order and grouping, is a multiple of 1/4 of magnitude <= A = sum |w||x|;
  while 4 A < 2^24 (``assert_exact``) all of them are fp32 numbers, so an fp32 kernel must return the float64 result
  itself.  One dropped, doubled or misplaced edge moves an element by at least 1/4.
* ``check_gamma``: on real inputs a sum of L rounded products (or L fmas) in any order is within gamma_{L+1} A of the
  exact value, gamma_k = k u / (1 - k u), u = 2^-24, with L the row's own in-degree - a bound per ROW, so a short row
  beside a hub row is held to its own few ulps."""
import numpy as np

U = 2.0 ** -24
K_LONG_CHAIN = 8    # kgat_spmm_plan.h kLongChain: a row cut by this many tile boundaries is finished by a whole wavefront

SMALL_DEGREES = (1, 2, 3, 4, 5, 7, 8, 9)


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------ the plan's rule, restated
def tile_rule(D, e):
    """kgat_spmm_plan.h merge_plan restated for a lane-group width D (4 ... 256): (class, run length C, tile edges).
    Short runs while they give at most 4,096 tiles, else - rows of 64 and 128 bytes only - half-length runs while those
    give at most 16,384 tiles, else full-length runs."""
    lpr = D // 4
    assert D % 4 == 0 and lpr in (1, 2, 4, 8, 16, 32, 64), D
    threads = 128 if lpr <= 8 else 256
    nsub = threads // lpr
    full = 64 if lpr >= 8 else {4: 32, 2: 16, 1: 8}[lpr]
    short = max(full // 4, 4)
    half = full // 2 if lpr in (4, 8) else full

    def tiles(c):
        return -(-e // (nsub * c)) if e > 0 else 0
    if tiles(short) <= 4096:
        return "short", short, nsub * short
    if tiles(half) <= 16384 and half != full:
        return "half", half, nsub * half
    return "full", full, nsub * full


# (D: ((short tile, largest e), (half tile, largest e) or None, full tile)) - the table of DESIGN.md section 31
CLASS_TABLE = {
    4: ((512, 2_097_152), None, 1024),
    8: ((256, 1_048_576), None, 1024),
    16: ((256, 1_048_576), (512, 8_388_608), 1024),
    32: ((256, 1_048_576), (512, 8_388_608), 1024),
    64: ((256, 1_048_576), None, 1024),
    128: ((128, 524_288), None, 512),
    256: ((64, 262_144), None, 256),
}


# The graphs of the GPU file, keyed by (tile edges, e_min): the run lengths C of every width the graph serves.
GRAPH_SPECS = {
    (512, 0): (4,),                        # D = 4, short
    (256, 0): (4, 8, 16),                  # D = 8, 16, 32, 64 and the generic widths, short
    (128, 0): (16,),                       # D = 128, short
    (64, 0): (16,),                        # D = 256, short
    (512, 1_048_577): (16, 32, 64),        # D = 16, 32 half; D = 128 full
    (1024, 1_048_577): (16, 64),           # D = 8, 64 full
    (1024, 2_097_153): (8,),               # D = 4 full
    (256, 262_145): (64,),                 # D = 256 full
    (1024, 8_388_609): (32, 64),           # D = 16, 32 full: the only large graph (fill degrees up to 1,677)
}


def graph_seed(TE, e_min):
    return 1000 + TE + e_min % 997


# ------------------------------------------------------------------------------------------------ planted graph
def planted_csr(TE, C, e_min, seed, fill=None):
    """The graph of ``planted_graph`` with its CSR arrays and the rows of its structures:
    dict(n, e, src, dst (edge-id order), deg, indptr, col, eid (CSR position -> edge id), rows={name: (lo, hi)}).
    Within a row the edge ids ascend, so a stable sort by destination (ops.csr_from_coo) reproduces `col` and `eid`."""
    rng = np.random.default_rng(seed)
    Cs = sorted(set(np.atleast_1d(C).tolist()))
    assert TE >= 64 and all(2 <= c <= TE for c in Cs)
    if fill is None:
        fill = max(16, e_min // 5000)
    deg, rows = [], {}

    def put(name, ds):
        rows[name] = (len(deg), len(deg) + len(ds))
        deg.extend(int(d) for d in ds)
    put("head", [0, TE - 3, 3])                   # row 2 ends exactly on the first tile boundary
    put("one_tile", [TE])                         # exactly tile 1
    put("hub", [12 * TE + 5])                     # starts on a boundary, cut by 12 more
    put("ones", [1] * (2 * TE + 7))
    put("empty", [0] * 50)
    put("runs", [d for c in Cs for d in (c - 1, c, c + 1) for _ in range(6)])
    put("small", [d for d in SMALL_DEGREES for _ in range(6)])
    put("chain", [3 * TE + 1, 0, 0])
    pad = -sum(deg) % TE
    put("pad", [pad if pad else TE])
    put("aligned", [2 * TE])                      # starts exactly on a boundary
    lo = len(deg)
    total = sum(deg)
    while total <= e_min:
        d = int(rng.integers(0, fill + 1))
        deg.append(d)
        total += d
    rows["fill"] = (lo, len(deg))
    t = 5
    while (total + t) % 4 == 0 or (total + t) % TE == 0:
        t += 1
    put("tail", [0, t, 0, 0])
    deg = np.asarray(deg, np.int64)
    n, e = len(deg), int(deg.sum())
    indptr = np.concatenate([[0], np.cumsum(deg)])
    dst_csr = np.repeat(np.arange(n), deg)
    col = rng.integers(0, n, e)
    col[:8] = dst_csr[:8]                         # the first eight CSR positions are self-loops
    perm = rng.permutation(e)
    eid = perm[np.lexsort((perm, dst_csr))]       # a random id for every position, ascending within each row
    src, dst = np.empty(e, np.int32), np.empty(e, np.int32)
    src[eid], dst[eid] = col, dst_csr
    return dict(n=n, e=e, src=src, dst=dst, deg=deg, indptr=indptr.astype(np.int64), col=col.astype(np.int32),
                eid=eid.astype(np.int32), rows=rows, TE=TE, Cs=Cs)


def planted_graph(TE, C, e_min, seed, fill=None):
    """(n, src, dst, deg): a graph built from an explicit in-degree sequence whose structures sit at known CSR positions
    relative to the tile size TE and the run length C (an int, or the run lengths of every width the graph serves):
    row 0 empty; TE-3 and 3 (a row ending exactly on a tile boundary); TE (exactly one tile); 12 TE + 5 (cut by 12 >=
    kLongChain boundaries); 2 TE + 7 rows of degree 1; 50 empty rows; six rows each of degree C-1, C, C+1, 1, 2, 3, 4, 5,
    7, 8, 9; 3 TE + 1 (a short chain) and two empty rows; a pad row up to the next boundary and a 2 TE row starting on it;
    random degrees in [0, fill] until e_min is passed; 0, t, 0, 0 with t >= 5 such that the last tile is ragged and
    e % 4 != 0.  Random sources (parallel edges), self-loops on the first eight CSR positions, edge ids shuffled."""
    g = planted_csr(TE, C, e_min, seed, fill)
    return g["n"], g["src"], g["dst"], g["deg"]


def exact_inputs(n, e, D, seed):
    """X (n, D) from {+-1, +-2, +-3} - never zero, so no dropped edge is invisible - and w (e,) from {1/4, 1/2, 1, 2}."""
    rng = np.random.default_rng(seed)
    X = rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), size=(n, D))
    w = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), size=e)
    return np.ascontiguousarray(X, np.float32), np.ascontiguousarray(w, np.float32)


def assert_exact(A, X=None):
    """On the float64 reference alone: with A = sum |w||x| per element, 4 A < 2^24 makes every partial sum (a multiple
    of 1/4 no larger than A) an fp32 number in any order; for the mul_self forms the product with |X[v]| as well.
    Returns 4 max A."""
    A = np.asarray(A, np.float64)
    top = 4.0 * float(A.max()) if A.size else 0.0
    assert top < 2 ** 24, top
    if X is not None:
        assert A.size == 0 or 4.0 * float((A * np.abs(np.asarray(X, np.float64))).max()) < 2 ** 24
    return top


def check_equal(got, ref, what):
    """`got` IS the float64 reference, element for element (exact inputs); prints and returns the mismatch count."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int(np.count_nonzero(got.astype(np.float64) != ref))
    print("[fwd exact] %-58s mismatches %d of %d" % (what, bad, ref.size))
    assert bad == 0, (what, bad, np.argwhere(got.astype(np.float64) != ref)[:4].tolist())
    return bad


def check_gamma(got, ref, A, L, extra, what):
    """|got - ref| <= gamma_{L + 1 + extra} A per element (L per row: the row's in-degree), exact zeros where A == 0.
    extra = 1 for mul_self (one more product; A = sum |w||x| |X[v]|) and for the mean (one division; A = sum |x| / deg).
    Prints and returns the worst |err| / bound."""
    L = np.asarray(L)
    got, ref, A = (np.asarray(t, np.float64).reshape(len(L), -1) for t in (got, ref, A))
    assert got.shape == ref.shape == A.shape, (what, got.shape, ref.shape, A.shape)
    assert np.all(np.isfinite(got)), what
    assert np.all(got[A == 0] == 0), (what, "elements without terms must be exact zeros")
    bound = gamma(L + 1 + extra)[:, None] * A
    err = np.abs(got - ref)
    nz = bound > 0
    ratio = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    print("[fwd gamma] %-58s worst |err| / bound = %.4f" % (what, ratio))
    assert np.all(err <= bound), (what, ratio)
    return ratio


def mean_exact(sum64, deg):
    """The mean the kernels state (reduce_fin, copy_finish_kernel): the exact fp32 sum divided, correctly rounded in
    fp32, by max(deg, 1)."""
    s = np.asarray(sum64, np.float64).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), np.asarray(sum64, np.float64))
    return s / np.maximum(np.asarray(deg), 1).astype(np.float32)[:, None]


def seq_sum32(n, rows_of_pos, col, X, w_csr, mult=None):
    """A sequential fp32 sum in CSR order, one rounded product and one rounded addition per position: the plain
    restatement the host test mutates.  `rows_of_pos`: the row every position is credited to; `mult`: 0 drops a
    position, 2 doubles it."""
    w = np.asarray(w_csr, np.float32)
    if mult is not None:
        w = w * np.asarray(mult, np.float32)
    out = np.zeros((n, X.shape[1]), np.float32)
    np.add.at(out, np.asarray(rows_of_pos, np.int64), w[:, None] * np.asarray(X, np.float32)[col])
    return out
