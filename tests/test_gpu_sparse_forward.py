"""The FORWARD aggregation against float64 on planted graphs, in every tile class of kgat_spmm_plan.h:
``kgat_spmm_umule_sum_f32`` (every algorithm and flag form), ``defer_finish`` + the deferred aggregator,
``kgat_spmm_bi_fused_f32`` and ``kgat_copy_reduce_f32``.

No bar here is measured.  Every case runs twice (tests/_spmm_fwd_ref.py):

* on ``exact_inputs`` - X in {+-1, +-2, +-3}, w in {1/4, 1/2, 1, 2}, ``assert_exact`` on the float64 reference first -
  every partial sum in any order is an fp32 number, so the device result must BE the float64 result (``check_equal``):
  one dropped, doubled or misplaced edge among 12,293 shows, which no relative bar can see;
* on standard-normal X and uniform w the result is within gamma_{L+1+extra} of the sum of |terms|, L the row's own
  in-degree (``check_gamma``): a short row beside a hub row is held to its own few ulps.

Each form is called twice and the two results must have the same bits.  The graphs (``planted_graph``) put a row end on
a tile boundary, a one-tile row, a row cut by 12 boundaries (the whole-wavefront finish), a short chain, more degree-1
rows than the fused form's LDS row buffer holds, empty rows inside and at the end of the range, rows around the run
length and the four-edge group, a ragged last tile and e % 4 != 0 at known positions of the tile size its widths take;
every case asserts the class it runs in (``kgat_spmm_tile_edges`` for D in 16 ... 128, the plan's rule restated for
D = 4, 8, 256).  CELLS at the end is the closed table of (entry, form, class) cells; test_every_cell_has_a_case fails
for a cell no case list reaches.  The worst |err| / bound ratios are printed: information, not thresholds."""
import numpy as np
import pytest
import torch

import _spmm_fwd_ref as R
from oracle import kgat_oracle as orc

pytestmark = pytest.mark.gpu

TILE_WIDTHS = (16, 32, 64, 128)   # kgat_spmm_plan.h TileWidths: the widths kgat_spmm_tile_edges answers for

# (D, class) -> the graph whose tile size that width takes in that class (tests/_spmm_fwd_ref.py GRAPH_SPECS)
SLOTS = {
    (4, "short"): (512, 0), (8, "short"): (256, 0), (16, "short"): (256, 0), (32, "short"): (256, 0),
    (64, "short"): (256, 0), (128, "short"): (128, 0), (256, "short"): (64, 0),
    (16, "half"): (512, 1_048_577), (32, "half"): (512, 1_048_577),
    (4, "full"): (1024, 2_097_153), (8, "full"): (1024, 1_048_577), (64, "full"): (1024, 1_048_577),
    (16, "full"): (1024, 8_388_609), (32, "full"): (1024, 8_388_609), (128, "full"): (512, 1_048_577),
    (256, "full"): (256, 262_145),
}
GENERIC_WIDTHS = (1, 12, 20, 100)  # no lane-group geometry: the generic kernel, on the TE = 256 graph
BIG = (1024, 8_388_609)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def tf(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def t32(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)


def leaky_half(p):
    """LeakyReLU of slope 1/2: exact in fp32 and in float64."""
    return np.where(p >= 0, p, 0.5 * p)


class _Graph:
    """One planted graph on the host and on the device, its inputs (one X as wide as the widest D it serves: a case of
    width D takes the first D columns) and its float64 references, each computed once and left unchanged."""

    def __init__(self, key, dev):
        from dgl_kgat_amd import ops
        self.key, self.dev = key, dev
        self.TE, self.e_min = key
        g = R.planted_csr(self.TE, R.GRAPH_SPECS[key], self.e_min, R.graph_seed(*key))
        self.n, self.e, self.deg, self.rows, self.ip = g["n"], g["e"], g["deg"], g["rows"], g["indptr"]
        self.src, self.dst, self.eid_h = g["src"], g["dst"], g["eid"]
        self.indptr, self.col, self.eid, self.row_of = ops.csr_from_coo(self.n, t32(self.src, dev), t32(self.dst, dev))
        assert np.array_equal(self.col.cpu().numpy(), g["col"]) and np.array_equal(self.eid.cpu().numpy(), g["eid"])
        assert np.array_equal(self.indptr.cpu().numpy(), g["indptr"])
        self.W = max([d for (d, _), k in SLOTS.items() if k == key] + (list(GENERIC_WIDTHS) if key == (256, 0) else []))
        self._in, self._ref, self._dev = {}, {}, {}

    def inputs(self, kind):
        """(X (n, W), w (e,) in edge-id order) on the host."""
        if kind not in self._in:
            if kind == "exact":
                self._in[kind] = R.exact_inputs(self.n, self.e, self.W, 7 + self.TE)
            else:
                rng = np.random.default_rng(9 + self.TE)
                self._in[kind] = (rng.standard_normal((self.n, self.W)).astype(np.float32), rng.random(self.e).astype(np.float32))
        return self._in[kind]

    def ref(self, kind, D, unit_w=False):
        """(sum w x, sum |w||x|) in float64, (n, D); unit_w: the copy reducer's w = 1."""
        k = (kind, unit_w)
        if k not in self._ref:
            X, w = self.inputs(kind)
            w = np.ones_like(w) if unit_w else w
            both = np.concatenate([X, np.abs(X)], 1)
            spmm = orc.spmm_u_mul_e_sum_sparse if self.e > 100_000 else orc.spmm_u_mul_e_sum
            out = spmm(self.n, self.src, self.dst, both, w)      # w >= 0: the second half is the sum of |terms|
            self._ref[k] = (out[:, :self.W], out[:, self.W:])
        ref, A = self._ref[k]
        return ref[:, :D], A[:, :D]

    def X(self, kind, D):
        """(host (n, D), device tensor)."""
        if (kind, D) not in self._dev:
            x = np.ascontiguousarray(self.inputs(kind)[0][:, :D])
            self._dev[(kind, D)] = (x, tf(x, self.dev))
        return self._dev[(kind, D)]

    def w(self, kind):
        """Device weights (edge-id order, CSR order)."""
        if ("w", kind) not in self._dev:
            w = self.inputs(kind)[1]
            self._dev[("w", kind)] = (tf(w, self.dev), tf(w[self.eid_h], self.dev))
        return self._dev[("w", kind)]

    def shards(self):
        """name -> (lo, hi): the row ranges of the issue's list."""
        h, (o0, o1), (z0, z1) = self.rows["hub"][0], self.rows["ones"], self.rows["empty"]
        return {"starts at the hub": (h, o0 + 100), "ends with the hub": (1, h + 1), "the hub alone": (h, h + 1),
                "the degree-1 stretch": (o0, o1), "only empty rows": (z0 + 3, z1 - 3), "the last rows": (self.n - 30, self.n)}

    def e_range(self, lo, hi):
        return int(self.ip[lo]), int(self.ip[hi])


@pytest.fixture(scope="module")
def graphs(dev):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = _Graph(key, dev)
        return cache[key]
    return get


RATIOS = {}   # cell -> worst |err| / bound over the cases that ran (printed by the last test)


def _note(cell, ratio):
    RATIOS[cell] = max(RATIOS.get(cell, 0.0), ratio)


def assert_class(D, e, cls, TE=None):
    """The class (and tile size) a call over `e` edges takes at width D: the restated rule, and the library's own answer
    where it gives one."""
    from dgl_kgat_amd import _lib
    got_cls, C, te = R.tile_rule(D, e)
    if D in TILE_WIDTHS:
        assert int(_lib.load().kgat_spmm_tile_edges(e, D)) == te, (D, e, te)
    print("[fwd class] D=%d e=%d: %s runs of %d, tiles of %d edges" % (D, e, got_cls, C, te))
    assert got_cls == cls and (TE is None or te == TE), (D, e, got_cls, te, cls, TE)
    return te


def no_tiles(D, G):
    """A width without a lane-group geometry: the generic kernel, one wavefront per row - no tiles, no class."""
    from dgl_kgat_amd import _lib
    assert D % 4 != 0 or D // 4 not in (1, 2, 4, 8, 16, 32, 64)
    assert int(_lib.load().kgat_spmm_tile_edges(G.e, D)) == 0
    print("[fwd class] D=%d e=%d: no lane-group geometry - the generic kernel (on the short-class graph of tile %d)" % (D, G.e, G.TE))


def _twice(f):
    a, b = f(), f()
    assert torch.equal(a, b), "two calls differ"
    return a.cpu().numpy()


def _compare(kind, got, ref, A, L, extra, what, cell):
    if kind == "exact":
        R.check_equal(got, ref, what)
    else:
        _note(cell, R.check_gamma(got, ref, A, L, extra, what))


# ------------------------------------------------------------------------- 1. kgat_spmm_umule_sum_f32, whole graph
SPMM_CASES = ([(D, cls, algo) for (D, cls) in SLOTS for algo in ("merge", "merge1")]
              + [(D, "short", algo) for (D, cls) in SLOTS if cls == "short" for algo in ("rows", "rows+order", "generic")]
              + [(D, "short", "generic-width") for D in GENERIC_WIDTHS])
W_ORDERS, SELF = ("csr", "eid"), ("plain", "mul_self")


@pytest.mark.parametrize("D,cls,algo", SPMM_CASES)
def test_spmm_whole_graph(dev, graphs, D, cls, algo):
    """Weights in CSR order and in edge-id order, with and without mul_self, exact and bounded."""
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)] if algo != "generic-width" else (256, 0))
    if algo != "generic-width":
        assert_class(D, G.e, cls, G.TE)
    else:
        no_tiles(D, G)
    kw = dict(algo="generic" if algo == "generic-width" else algo.split("+")[0])
    if algo == "rows+order":
        kw["order"] = ops.row_order_by_degree(G.indptr)
    for kind in ("exact", "real"):
        (Xh, Xd), (w_e, w_csr) = G.X(kind, D), G.w(kind)
        ref, A = G.ref(kind, D)
        if kind == "exact":
            R.assert_exact(A, Xh)
        for wo in W_ORDERS:
            for ms in SELF:
                wkw = dict(eid=G.eid) if wo == "eid" else {}
                got = _twice(lambda: ops.spmm(G.indptr, G.col, G.row_of, Xd, w_e if wo == "eid" else w_csr,
                                              mul_self=ms == "mul_self", **wkw, **kw))
                assert got.shape == (G.n, D)
                mul = ms == "mul_self"
                _compare(kind, got, ref * Xh if mul else ref, A * np.abs(Xh) if mul else A, G.deg, int(mul),
                         "spmm %s %s/%s D=%d %s %s" % (algo, wo, ms, D, cls, kind), ("spmm", "%s/%s/%s" % (algo, wo, ms), cls))


SELF_OUT_CASES = [(64, "short"), (64, "full"), (16, "short"), (16, "half")]


@pytest.mark.parametrize("D,cls", SELF_OUT_CASES)
def test_spmm_self_out(dev, graphs, D, cls):
    """self_out (mul_self, merge): `out` has the bits of the call without it - which is held to float64 here -, the slice
    of the wider poisoned buffer equals X, nothing outside the slice is touched."""
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)])
    assert_class(D, G.e, cls, G.TE)
    for kind in ("exact", "real"):
        (Xh, Xd), (_, w_csr) = G.X(kind, D), G.w(kind)
        ref, A = G.ref(kind, D)
        plain = ops.spmm(G.indptr, G.col, G.row_of, Xd, w_csr, mul_self=True, algo="merge")
        wide = torch.full((G.n, D + 24), float("nan"), device=dev)
        got = ops.spmm(G.indptr, G.col, G.row_of, Xd, w_csr, mul_self=True, algo="merge", self_out=wide[:, 8:8 + D])
        assert torch.equal(got, plain) and torch.equal(wide[:, 8:8 + D], Xd)
        assert bool(torch.isnan(wide[:, :8]).all()) and bool(torch.isnan(wide[:, 8 + D:]).all())
        _compare(kind, got.cpu().numpy(), ref * Xh, A * np.abs(Xh), G.deg, 1,
                 "spmm self_out D=%d %s %s" % (D, cls, kind), ("spmm", "self_out", cls))


# ------------------------------------------------------------------------------------------- 2. row-range shards
SHARD_WIDTHS = [(4, "short"), (16, "short"), (64, "short"), (128, "short")]
SHARD_ALGOS = ("merge", "rows")


def _shard_list(G, D):
    """[(name, lo, hi, class)]: every shard of a small graph is in the short class."""
    return [(name, lo, hi, "short") for name, (lo, hi) in G.shards().items()]


def _big_shard(G):
    """Rows [r, n) of the 8.5 M-edge graph, r > 0 the first fill row: more than 1,048,576 edges, fewer than 8,388,609."""
    lo = G.rows["fill"][0]
    assert lo > 0 and 1_048_576 < G.e - int(G.ip[lo]) <= 8_388_608
    return lo, G.n


@pytest.mark.parametrize("algo", SHARD_ALGOS)
@pytest.mark.parametrize("D,cls", SHARD_WIDTHS)
def test_spmm_row_range_shards(dev, graphs, D, cls, algo):
    """rows= / e_range=: shards that start at, end with and consist of the 12 TE + 5 hub row, the degree-1 stretch, only
    empty rows (e0 == e1: zeros) and the last rows, against ref[lo:hi]."""
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)])
    for name, lo, hi, scls in _shard_list(G, D):
        e0, e1 = G.e_range(lo, hi)
        assert_class(D, e1 - e0, scls)
        assert (e0 == e1) == (name == "only empty rows")
        for kind in ("exact", "real"):
            (Xh, Xd), (_, w_csr) = G.X(kind, D), G.w(kind)
            ref, A = G.ref(kind, D)
            if kind == "exact":
                R.assert_exact(A, Xh)
            got = _twice(lambda: ops.spmm(G.indptr, G.col, G.row_of, Xd, w_csr, rows=(lo, hi - lo), e_range=(e0, e1), algo=algo))
            assert got.shape == (hi - lo, D)
            _compare(kind, got, ref[lo:hi], A[lo:hi], G.deg[lo:hi], 0,
                     "spmm shard %s: %s D=%d %s" % (algo, name, D, kind), ("spmm", "shard/" + algo, scls))


@pytest.mark.parametrize("algo", SHARD_ALGOS)
@pytest.mark.parametrize("D", [16, 32])
def test_spmm_half_class_shard_with_a_row_offset(dev, graphs, D, algo):
    from dgl_kgat_amd import ops
    G = graphs(BIG)
    lo, hi = _big_shard(G)
    e0, e1 = G.e_range(lo, hi)
    assert_class(D, e1 - e0, "half", 512)
    for kind in ("exact", "real"):
        (Xh, Xd), (_, w_csr) = G.X(kind, D), G.w(kind)
        ref, A = G.ref(kind, D)
        if kind == "exact":
            R.assert_exact(A, Xh)
        got = _twice(lambda: ops.spmm(G.indptr, G.col, G.row_of, Xd, w_csr, rows=(lo, hi - lo), e_range=(e0, e1), algo=algo))
        _compare(kind, got, ref[lo:hi], A[lo:hi], G.deg[lo:hi], 0,
                 "spmm shard %s: [%d, n) of 8.4 M D=%d %s" % (algo, lo, D, kind), ("spmm", "shard/" + algo, "half"))


# ------------------------------------------------------- 3. defer_finish + the deferred aggregator (Bi, identity W)
DEFER_CASES = [(16, "short"), (16, "half"), (64, "short"), (64, "full")]


def _deferred_identity(ops, G, Xd, w_csr, D, dev):
    hn = torch.full((G.n, D), float("nan"), device=dev)   # a deferred row taken from `out` would show
    hn, left = ops.spmm(G.indptr, G.col, G.row_of, Xd, w_csr, out=hn, algo="merge", defer_finish=True)
    assert left.tile_edges == R.tile_rule(D, G.e)[2]
    assert bool(torch.isnan(hn).any()), "no row was deferred"
    return ops.aggregator(ops.FORMS["Bi"], Xd, hn, torch.eye(D, device=dev), negative_slope=0.5, deferred=left)


@pytest.mark.parametrize("D,cls", DEFER_CASES)
def test_spmm_deferred_finish_identity_aggregator(dev, graphs, D, cls):
    """W = I and a LeakyReLU of slope 1/2: products with 1 and 0 and the halving are exact, so Z is LeakyReLU_1/2 of
    ref * X - the very bits on exact inputs, the rows the tiles cut (formed by the dense kernel) included."""
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)])
    assert_class(D, G.e, cls, G.TE)
    for kind in ("exact", "real"):
        (Xh, Xd), (_, w_csr) = G.X(kind, D), G.w(kind)
        ref, A = G.ref(kind, D)
        if kind == "exact":
            R.assert_exact(A, Xh)
        Z = _twice(lambda: _deferred_identity(ops, G, Xd, w_csr, D, dev))
        _compare(kind, Z, leaky_half(ref * Xh), A * np.abs(Xh), G.deg, 1,
                 "defer_finish + Bi(I) D=%d %s %s" % (D, cls, kind), ("spmm", "defer_finish+aggregator", cls))


# ------------------------------------------------------------------------------------ 4. kgat_spmm_bi_fused_f32
FUSED_CASES = [(64, 64, "short"), (64, 64, "full"), (32, 16, "short"), (32, 16, "half")]


@pytest.mark.parametrize("d_in,d_out,cls", FUSED_CASES)
def test_spmm_bi_fused(dev, graphs, d_in, d_out, cls):
    """The same bits as the two-launch sequence (spmm(mul_self) - held to float64 above - then bi_interaction), whole
    graph and a shard that holds the hub and the degree-1 stretch; at (64, 64) with W2 = I and slope 1/2, h is
    LeakyReLU_1/2 of ref * X exactly, the rows spilled past the LDS row buffer (the degree-1 stretch) included."""
    from dgl_kgat_amd import ops
    from test_gpu_parity import _fused_vs_two_launches
    G = graphs(SLOTS[(d_in, cls)])
    assert_class(d_in, G.e, cls, G.TE)
    rng = np.random.default_rng(60 + d_in)
    W2 = tf(rng.standard_normal((d_out, d_in)) / np.sqrt(d_in), dev)
    h0, o1 = G.rows["hub"][0], G.rows["ones"][1]
    for kind in ("exact", "real"):
        (Xh, Xd), (_, w_csr) = G.X(kind, d_in), G.w(kind)
        ref, A = G.ref(kind, d_in)
        if kind == "exact":
            R.assert_exact(A, Xh)
        _fused_vs_two_launches(ops, G.indptr, G.col, G.row_of, Xd, w_csr, W2, dev, self_copy=True)
        _fused_vs_two_launches(ops, G.indptr, G.col, G.row_of, Xd, w_csr, W2, dev, lo=h0, hi=o1 + 20)
        # the two-launch side of that equality, tied to float64 in this very case
        prod = ops.spmm(G.indptr, G.col, G.row_of, Xd, w_csr, mul_self=True).cpu().numpy()
        cell = ("bi_fused", "%dx%d" % (d_in, d_out), cls)
        _compare(kind, prod, ref * Xh, A * np.abs(Xh), G.deg, 1, "two-launch side D=%d %s %s" % (d_in, cls, kind), cell)
        if d_in == d_out:
            h = _twice(lambda: ops.spmm_bi_fused(G.indptr, G.col, G.row_of, Xd, w_csr, torch.eye(d_in, device=dev), 0.5))
            _compare(kind, h, leaky_half(ref * Xh), A * np.abs(Xh), G.deg, 1,
                     "bi_fused W2=I D=%d %s %s" % (d_in, cls, kind), cell)


# ---------------------------------------------------------------------------------------- 5. kgat_copy_reduce_f32
COPY_CASES = [(D, cls) for (D, cls) in SLOTS if D in TILE_WIDTHS] + [(20, "short")]
COPY_SHARD_WIDTHS = [(16, "short"), (64, "short"), (128, "short"), (20, "short")]
REDUCES = ("sum", "mean")


def _copy_compare(G, kind, reduce, got, lo, hi, D, what, cell):
    ref, A = G.ref(kind, D, unit_w=True)
    ref, A, deg = ref[lo:hi], A[lo:hi], G.deg[lo:hi]
    if kind == "exact":
        R.check_equal(got, ref if reduce == "sum" else R.mean_exact(ref, deg), what)
    else:
        d = np.maximum(deg, 1)[:, None].astype(np.float64)
        ref, A, extra = (ref, A, 0) if reduce == "sum" else (ref / d, A / d, 1)
        _note(cell, R.check_gamma(got, ref, A, deg, extra, what))
    if reduce == "mean":
        assert np.all(got[deg == 0] == 0)


@pytest.mark.parametrize("D,cls", COPY_CASES)
def test_copy_reduce_whole_graph(dev, graphs, D, cls):
    """Exact inputs (w = 1): the sum is the float64 sum and the mean its correctly rounded fp32 quotient; real inputs under
    gamma_{L+1} (sum) and gamma_{L+2} (mean).  D = 20: the generic kernel."""
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)] if D in TILE_WIDTHS else (256, 0))
    if D in TILE_WIDTHS:
        assert_class(D, G.e, cls, G.TE)
    else:
        no_tiles(D, G)
    for kind in ("exact", "real"):
        Xh, Xd = G.X(kind, D)
        if kind == "exact":
            R.assert_exact(G.ref(kind, D, unit_w=True)[1])
        for reduce in REDUCES:
            got = _twice(lambda: ops.copy_reduce(G.indptr, G.col, G.row_of, Xd, reduce))
            _copy_compare(G, kind, reduce, got, 0, G.n, D, "copy_reduce %s D=%d %s %s" % (reduce, D, cls, kind),
                          ("copy_reduce", reduce, cls))


@pytest.mark.parametrize("D,cls", COPY_SHARD_WIDTHS)
def test_copy_reduce_row_range_shards(dev, graphs, D, cls):
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)] if D in TILE_WIDTHS else (256, 0))
    for name, lo, hi, scls in _shard_list(G, D):
        e0, e1 = G.e_range(lo, hi)
        if D in TILE_WIDTHS:
            assert_class(D, e1 - e0, scls)
        for kind in ("exact", "real"):
            Xh, Xd = G.X(kind, D)
            for reduce in REDUCES:
                got = _twice(lambda: ops.copy_reduce(G.indptr, G.col, G.row_of, Xd, reduce, rows=(lo, hi - lo), e_range=(e0, e1)))
                assert got.shape == (hi - lo, D)
                _copy_compare(G, kind, reduce, got, lo, hi, D, "copy_reduce shard %s: %s D=%d %s" % (reduce, name, D, kind),
                              ("copy_reduce", "shard/" + reduce, scls))


@pytest.mark.parametrize("D", [16, 32])
def test_copy_reduce_half_class_shard_with_a_row_offset(dev, graphs, D):
    from dgl_kgat_amd import ops
    G = graphs(BIG)
    lo, hi = _big_shard(G)
    e0, e1 = G.e_range(lo, hi)
    assert_class(D, e1 - e0, "half", 512)
    for kind in ("exact", "real"):
        Xh, Xd = G.X(kind, D)
        for reduce in REDUCES:
            got = _twice(lambda: ops.copy_reduce(G.indptr, G.col, G.row_of, Xd, reduce, rows=(lo, hi - lo), e_range=(e0, e1)))
            _copy_compare(G, kind, reduce, got, lo, hi, D, "copy_reduce shard %s: [%d, n) of 8.4 M D=%d %s" % (reduce, lo, D, kind),
                          ("copy_reduce", "shard/" + reduce, "half"))


# ------------------------------------------------------------------------------------------------------ 6. counts
@pytest.mark.parametrize("D,cls", list(SLOTS))
def test_every_form_counts_edges(dev, graphs, D, cls):
    """w = 1, X = 1: every form returns the in-degree (small integers add exactly in any order); the mean returns 1, and 0
    for the rows without in-edges."""
    from dgl_kgat_amd import ops
    G = graphs(SLOTS[(D, cls)])
    assert_class(D, G.e, cls, G.TE)
    X1, w1 = torch.ones((G.n, D), device=dev), torch.ones(G.e, device=dev)
    want = np.broadcast_to(G.deg[:, None].astype(np.float32), (G.n, D))
    algos = ("merge", "merge1") + (("rows", "generic") if cls == "short" else ())
    for algo in algos:
        for eid in (None, G.eid):
            for mul in (False, True):
                got = ops.spmm(G.indptr, G.col, G.row_of, X1, w1, eid=eid, mul_self=mul, algo=algo).cpu().numpy()
                assert np.array_equal(got, want), (algo, eid is not None, mul)
    if cls == "short":
        got = ops.spmm(G.indptr, G.col, G.row_of, X1, w1, algo="rows", order=ops.row_order_by_degree(G.indptr))
        assert np.array_equal(got.cpu().numpy(), want)
    if (D, cls) in SELF_OUT_CASES:
        wide = torch.zeros((G.n, D + 8), device=dev)
        got = ops.spmm(G.indptr, G.col, G.row_of, X1, w1, mul_self=True, algo="merge", self_out=wide[:, 4:4 + D])
        assert np.array_equal(got.cpu().numpy(), want) and bool((wide[:, 4:4 + D] == 1).all())
    if (D, cls) in DEFER_CASES:
        assert np.array_equal(_deferred_identity(ops, G, X1, w1, D, dev).cpu().numpy(), want)
    if (D, D, cls) in FUSED_CASES:
        h = ops.spmm_bi_fused(G.indptr, G.col, G.row_of, X1, w1, torch.eye(D, device=dev), 0.5)
        assert np.array_equal(h.cpu().numpy(), want)
    if D in TILE_WIDTHS:
        assert np.array_equal(ops.copy_reduce(G.indptr, G.col, G.row_of, X1, "sum").cpu().numpy(), want)
        mean = ops.copy_reduce(G.indptr, G.col, G.row_of, X1, "mean").cpu().numpy()
        assert np.array_equal(mean, np.broadcast_to((G.deg > 0)[:, None].astype(np.float32), (G.n, D)))
    for name, (lo, hi) in G.shards().items():
        kw = dict(rows=(lo, hi - lo), e_range=G.e_range(lo, hi))
        for algo in SHARD_ALGOS:
            assert np.array_equal(ops.spmm(G.indptr, G.col, G.row_of, X1, w1, algo=algo, **kw).cpu().numpy(), want[lo:hi]), (name, algo)
        if D in TILE_WIDTHS:
            assert np.array_equal(ops.copy_reduce(G.indptr, G.col, G.row_of, X1, "sum", **kw).cpu().numpy(), want[lo:hi]), name


def test_generic_widths_count_edges(dev, graphs):
    from dgl_kgat_amd import ops
    G = graphs((256, 0))
    for D in GENERIC_WIDTHS:
        X1, w1 = torch.ones((G.n, D), device=dev), torch.ones(G.e, device=dev)
        want = np.broadcast_to(G.deg[:, None].astype(np.float32), (G.n, D))
        assert np.array_equal(ops.spmm(G.indptr, G.col, G.row_of, X1, w1).cpu().numpy(), want)
        assert np.array_equal(ops.spmm(G.indptr, G.col, G.row_of, X1, w1, eid=G.eid, mul_self=True).cpu().numpy(), want)
        assert np.array_equal(ops.copy_reduce(G.indptr, G.col, G.row_of, X1, "sum").cpu().numpy(), want)


# ------------------------------------------------------------------------------------------ the closed cell table
ALL, SHORT = ("short", "half", "full"), ("short",)
_SPMM_FLAGS = ["%s/%s" % (wo, ms) for wo in W_ORDERS for ms in SELF]
CELLS = {
    # (entry, algorithm or flag form): the classes it must be reached in, by an exact and a bounded check each
    **{("spmm", "%s/%s" % (algo, f)): ALL for algo in ("merge", "merge1") for f in _SPMM_FLAGS},
    **{("spmm", "%s/%s" % (algo, f)): SHORT for algo in ("rows", "rows+order", "generic", "generic-width") for f in _SPMM_FLAGS},
    ("spmm", "self_out"): ALL,
    ("spmm", "shard/merge"): ("short", "half"),
    ("spmm", "shard/rows"): ("short", "half"),
    ("spmm", "defer_finish+aggregator"): ALL,
    ("bi_fused", "64x64"): ("short", "full"),
    ("bi_fused", "32x16"): ("short", "half"),
    ("copy_reduce", "sum"): ALL,
    ("copy_reduce", "mean"): ALL,
    ("copy_reduce", "shard/sum"): ("short", "half"),
    ("copy_reduce", "shard/mean"): ("short", "half"),
}


def _cells_of_the_case_lists():
    """The cells the parametrize lists above reach; every case of them runs its exact AND its bounded check."""
    got = set()
    for D, cls, algo in SPMM_CASES:
        got |= {("spmm", "%s/%s" % (algo, f), cls) for f in _SPMM_FLAGS}
    got |= {("spmm", "self_out", cls) for _, cls in SELF_OUT_CASES}
    got |= {("spmm", "shard/" + a, cls) for _, cls in SHARD_WIDTHS for a in SHARD_ALGOS}
    got |= {("spmm", "shard/" + a, "half") for a in SHARD_ALGOS}            # test_spmm_half_class_shard_with_a_row_offset
    got |= {("spmm", "defer_finish+aggregator", cls) for _, cls in DEFER_CASES}
    got |= {("bi_fused", "%dx%d" % (di, do), cls) for di, do, cls in FUSED_CASES}
    got |= {("copy_reduce", r, cls) for _, cls in COPY_CASES for r in REDUCES}
    got |= {("copy_reduce", "shard/" + r, cls) for _, cls in COPY_SHARD_WIDTHS for r in REDUCES}
    got |= {("copy_reduce", "shard/" + r, "half") for r in REDUCES}         # test_copy_reduce_half_class_shard_with_a_row_offset
    return got


def test_every_cell_has_a_case():
    want = {(entry, form, cls) for (entry, form), classes in CELLS.items() for cls in classes}
    got = _cells_of_the_case_lists()
    assert not want - got, "cells without a case: %s" % sorted(want - got)
    assert not got - want, "cases outside the table: %s" % sorted(got - want)
    # every merge width of the table runs in every class it has
    for D, (_, half, _) in R.CLASS_TABLE.items():
        for cls in ("short", "full") + (("half",) if half else ()):
            assert (D, cls, "merge") in SPMM_CASES and (D, cls, "merge1") in SPMM_CASES, (D, cls)
    for D in TILE_WIDTHS:
        assert all((D, cls) in COPY_CASES for cls in ("short", "full")), D
    ran = {c: r for c, r in RATIOS.items()}
    for cell in sorted(ran):
        print("[fwd worst ratio] %-14s %-28s %-6s %.4f" % (cell + (ran[cell],)))
    assert all(c in want for c in ran), sorted(set(ran) - want)
