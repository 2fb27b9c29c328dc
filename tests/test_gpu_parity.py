"""GPU parity tests: the HIP path (through the C ABI / ctypes) against the CPU oracle on the
same seeded inputs, the committed golden fixtures, edge cases, and size-independent
properties at the benchmark's full size.  Tolerance for fp32 device results vs the fp64
oracle: 1e-4 relative - elementwise with SURVEY 8c's floor (conftest.rel_err) for the softmax,
relative to the sum of |terms| for the aggregation (conftest.sum_err: hub rows add thousands
of fp32 products), relative to the tensor's scale for logits and multi-layer outputs
(conftest.rel_err_inf); integer / index outputs are bit-exact."""
import numpy as np
import pytest
import torch

from conftest import (readout_abs_bar, GOLDEN_CASES, blocks, blocks_rel_err_inf, load_golden, parity_8c, parity_8c_robust, rel_err,
                      rel_err_inf, sum_err)
import _spmm_fwd_ref as fwd
from oracle import c_oracle as co
from oracle import kgat_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    import dgl_kgat_amd
    return dgl_kgat_amd


def t32(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)


def tf(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def random_graph(seed, n, e, hub=0, isolated_tail=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, e)
    dst = rng.integers(0, max(n - isolated_tail, 1), e)
    if hub:
        dst[rng.choice(e, min(hub, e), replace=False)] = min(3, n - 1)
    return src.astype(np.int32), dst.astype(np.int32)


GRAPHS = [
    ("empty", 5, 0, 0, 0),
    ("single_edge", 3, 1, 0, 0),
    ("tiny", 7, 20, 0, 2),
    ("ragged", 300, 5000, 0, 40),
    ("hub", 500, 20000, 9000, 100),
    ("all_one_row", 64, 7000, 7000, 0),
    ("wide", 5000, 60000, 3000, 0),
]


@pytest.mark.parametrize("name,n,e,hub,iso", GRAPHS)
def test_csr_from_coo_bit_exact(K, dev, name, n, e, hub, iso):
    from dgl_kgat_amd import ops
    src, dst = random_graph(1, n, e, hub, iso)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    oi, oc, oe = orc.csr_from_coo(n, src, dst)
    assert np.array_equal(indptr.cpu().numpy(), oi)
    assert np.array_equal(col.cpu().numpy(), oc)
    assert np.array_equal(eid.cpu().numpy(), oe)
    assert np.array_equal(row_of.cpu().numpy(), dst[oe])
    if e:
        pos = ops.invert_permutation(eid).cpu().numpy()
        assert np.array_equal(pos[oe], np.arange(e))
        order = ops.row_order_by_degree(indptr).cpu().numpy()
        deg = np.diff(oi)
        assert sorted(order.tolist()) == list(range(n))
        assert np.all(np.diff(deg[order]) <= 0)
        assert np.array_equal(order, np.argsort(-deg.astype(np.int64), kind="stable"))


def test_csr_large_ids_three_radix_passes(K, dev):
    from dgl_kgat_amd import ops
    n, e = 200_000, 300_000  # 18-bit node ids -> three 8-bit passes
    src, dst = random_graph(2, n, e, hub=50_000)
    indptr, col, eid, _ = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    oi, oc, oe = co.csr_from_coo(n, src, dst)
    assert np.array_equal(indptr.cpu().numpy(), oi) and np.array_equal(eid.cpu().numpy(), oe)
    assert np.array_equal(col.cpu().numpy(), oc)


def _csr_bit_exact(ops, dev, n, src, dst):
    """All four outputs of csr_from_coo against numpy (stable argsort, bincount)."""
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    oe = np.argsort(dst, kind="stable")
    oi = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    assert np.array_equal(indptr.cpu().numpy(), oi)
    assert np.array_equal(eid.cpu().numpy(), oe)
    assert np.array_equal(col.cpu().numpy(), src[oe])
    assert np.array_equal(row_of.cpu().numpy(), dst[oe])


SORT_CLASS_SIZES = [(1 << 20) - 1, 1 << 20, (1 << 20) + 1]  # 256 keys per block below 2^20 keys, 4,096 from there on


@pytest.mark.parametrize("e", SORT_CLASS_SIZES)
def test_csr_sort_size_classes(K, dev, e):
    """Both sides of the sort's switch of tile (a ragged last block of 255 keys, of 1 key, whole blocks), two passes."""
    from dgl_kgat_amd import ops
    src, dst = random_graph(3, 3000, e, hub=300_000, isolated_tail=100)
    _csr_bit_exact(ops, dev, 3000, src, dst)


@pytest.mark.parametrize("e", SORT_CLASS_SIZES)
def test_group_by_relation_sort_size_classes(K, dev, e):
    from dgl_kgat_amd import ops
    n_rel = 41
    et = np.random.default_rng(e).integers(-2, n_rel + 3, e).astype(np.int32)  # [-2, 43]: types outside [0, R) included
    rel_ptr, perm = ops.group_by_relation(t32(et, dev), n_rel)
    key = np.where((et >= 0) & (et < n_rel), et, n_rel)
    assert np.array_equal(rel_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_rel + 1)[:n_rel])]))
    assert np.array_equal(perm.cpu().numpy(), np.argsort(key, kind="stable"))


@pytest.mark.parametrize("n", SORT_CLASS_SIZES)
def test_row_order_by_degree_sort_size_classes(K, dev, n):
    """2^20 rows: degrees 0 .. 40, some rows of 65,534 .. 65,537 and one of 300,000 in-edges (the key holds a degree
    up to 65,535; larger ones tie there and keep their row order)."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(n)
    deg = rng.integers(0, 41, n).astype(np.int64)
    deg[rng.choice(n, 9, replace=False)] = [65534, 65535, 65536, 65537, 300_000, 65535, 65536, 70_000, 65534]
    indptr = np.concatenate([[0], np.cumsum(deg)])
    assert indptr[-1] < 2 ** 31
    order = ops.row_order_by_degree(t32(indptr, dev)).cpu().numpy()
    assert np.array_equal(order, np.argsort(-np.minimum(deg, 65535), kind="stable"))


def test_csr_large_ids_four_radix_passes(K, dev):
    """Node ids of 25 bits: four 8-bit passes, so the ping-pong buffers start on the other side than with three."""
    from dgl_kgat_amd import ops
    n, e = (1 << 24) + 1000, 5000
    rng = np.random.default_rng(4)
    low, high = rng.integers(0, 51, e), rng.integers((1 << 24) - 50, (1 << 24) + 1000, e)
    dst = np.where(rng.random(e) < 0.5, low, high).astype(np.int32)
    assert dst.min() <= 50 and dst.max() >= 1 << 24 and np.any((dst < 1 << 24) & (dst >= (1 << 24) - 50))
    src = rng.integers(0, n, e).astype(np.int32)
    _csr_bit_exact(ops, dev, n, src, dst)


@pytest.mark.parametrize("n_rel,e", [(1, 10), (5, 5000), (41, 70000), (300, 9000)])
def test_group_by_relation_bit_exact(K, dev, n_rel, e):
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(n_rel)
    et = rng.integers(-2, n_rel + 3, e).astype(np.int32)  # includes types outside [0, R)
    rel_ptr, perm = ops.group_by_relation(t32(et, dev), n_rel)
    orp, operm = orc.group_by_relation(et, n_rel)
    assert np.array_equal(rel_ptr.cpu().numpy(), orp)
    assert np.array_equal(perm.cpu().numpy(), operm)


@pytest.mark.parametrize("D", [1, 4, 8, 12, 16, 32, 64, 128, 256, 100])
@pytest.mark.parametrize("name,n,e,hub,iso", GRAPHS)
def test_spmm_vs_oracle(K, dev, D, name, n, e, hub, iso):
    from dgl_kgat_amd import ops
    src, dst = random_graph(3, n, e, hub, iso)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((n, D)).astype(np.float32)
    w = rng.random(e).astype(np.float32)
    ref = orc.spmm_u_mul_e_sum(n, src, dst, X, w)
    ref_abs = orc.spmm_u_mul_e_sum(n, src, dst, np.abs(X), w)  # w >= 0: sum of |terms|
    ref_self, ref_self_abs = ref * X, ref_abs * np.abs(X)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    Xd, wd = tf(X, dev), tf(w, dev)
    w_csr = ops.gather(eid, wd) if e else wd
    algos = ["generic"] + (["merge", "merge1", "rows"] if D in (4, 8, 16, 32, 64, 128, 256) else [])
    deg = np.bincount(dst, minlength=n)
    for algo in algos:
        # beside the relative bar: every row within gamma_{L+1} of ITS sum of |terms| (tests/_spmm_fwd_ref.py)
        what = "%s D=%d %s " % (name, D, algo)
        out = ops.spmm(indptr, col, row_of, Xd, w_csr, algo=algo).cpu().numpy()
        assert out.shape == (n, D)
        assert sum_err(out, ref, ref_abs) < TOL, (algo, "csr-order w")
        fwd.check_gamma(out, ref, ref_abs, deg, 0, what + "csr-order w")
        out = ops.spmm(indptr, col, row_of, Xd, wd, eid=eid, algo=algo).cpu().numpy()
        assert sum_err(out, ref, ref_abs) < TOL, (algo, "edge-id-order w")
        fwd.check_gamma(out, ref, ref_abs, deg, 0, what + "edge-id-order w")
        out = ops.spmm(indptr, col, row_of, Xd, w_csr, algo=algo, mul_self=True).cpu().numpy()
        assert sum_err(out, ref_self, ref_self_abs) < TOL, (algo, "mul_self")
        fwd.check_gamma(out, ref_self, ref_self_abs, deg, 1, what + "mul_self")
        # destinations without in-edges are written as exact zeros, on a dirty output buffer
        dirty = torch.full((n, D), 7.0, device=dev)
        ops.spmm(indptr, col, row_of, Xd, w_csr, out=dirty, algo=algo)
        assert np.all(dirty.cpu().numpy()[np.diff(indptr.cpu().numpy()) == 0] == 0)
    if "rows" in algos and e:
        order = ops.row_order_by_degree(indptr)
        out = ops.spmm(indptr, col, row_of, Xd, w_csr, algo="rows", order=order).cpu().numpy()
        assert sum_err(out, ref, ref_abs) < TOL
        fwd.check_gamma(out, ref, ref_abs, deg, 0, "%s D=%d rows, ordered" % (name, D))
        # the rows kernel adds in CSR order with one fma per edge: bit-exact vs the C restatement
        cref = co.spmm(n, indptr.cpu().numpy(), col.cpu().numpy(), None, X, w_csr.cpu().numpy())
        assert np.array_equal(out, cref)
        # reproducible: two launches of the merge kernel give identical bits
        a = ops.spmm(indptr, col, row_of, Xd, w_csr, algo="merge")
        b = ops.spmm(indptr, col, row_of, Xd, w_csr, algo="merge")
        assert torch.equal(a, b)


@pytest.mark.parametrize("D", [4, 8, 16, 32, 64, 128, 256])
def test_spmm_long_runs_every_width(K, dev, D):
    """Launches over few edges take a quarter of the run length (kgat_spmm_plan.h: short_run_len), so
    the graphs above exercise the short runs; this one (4.3 M edges, hubs and empty rows included) is past them
    at every width: the full run length at D = 4, 8, 64, 128 and 256, the HALF-length runs at D = 16 and 32,
    whose full-length kernels take more than 8,388,608 edges - tests/test_gpu_sparse_forward.py runs those
    (and every other class of every width) on its 8.4 M-edge graph, at exact and worst-case bars."""
    from dgl_kgat_amd import _lib, ops
    n, e = 20000, 4_300_000
    cls, _, te = fwd.tile_rule(D, e)
    assert (cls, te) == (("half", 512) if D in (16, 32) else ("full", fwd.CLASS_TABLE[D][2])), (D, cls, te)
    if D in (16, 32, 64, 128):   # the widths the library answers for: half at 16 and 32, full at 64 (1,024) and 128 (512)
        assert int(_lib.load().kgat_spmm_tile_edges(e, D)) == te
    src, dst = random_graph(31, n, e, hub=600_000, isolated_tail=500)
    rng = np.random.default_rng(32)
    X = rng.standard_normal((n, D)).astype(np.float32)
    w = rng.random(e).astype(np.float32)
    ref = orc.spmm_u_mul_e_sum_sparse(n, src, dst, X, w)
    ref_abs = orc.spmm_u_mul_e_sum_sparse(n, src, dst, np.abs(X), w)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    w_csr = ops.gather(eid, tf(w, dev))
    for algo in ("merge", "merge1"):
        out = ops.spmm(indptr, col, row_of, tf(X, dev), w_csr, algo=algo)
        assert sum_err(out.cpu().numpy(), ref, ref_abs) < TOL, algo
        assert torch.equal(out, ops.spmm(indptr, col, row_of, tf(X, dev), w_csr, algo=algo))
    out = ops.spmm(indptr, col, row_of, tf(X, dev), w_csr, mul_self=True).cpu().numpy()
    assert sum_err(out, ref * X, ref_abs * np.abs(X)) < TOL
    assert np.all(out[np.diff(indptr.cpu().numpy()) == 0] == 0)


def test_spmm_row_range_shard(K, dev):
    """Destination-range shard: rows [lo, hi) with their CSR position range (multi-GPU layout)."""
    from dgl_kgat_amd import ops
    n, e, D = 700, 30000, 64
    src, dst = random_graph(5, n, e, hub=8000, isolated_tail=30)
    rng = np.random.default_rng(6)
    X = rng.standard_normal((n, D)).astype(np.float32)
    w = rng.random(e).astype(np.float32)
    ref = orc.spmm_u_mul_e_sum(n, src, dst, X, w)
    ref_abs = orc.spmm_u_mul_e_sum(n, src, dst, np.abs(X), w)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    ip = indptr.cpu().numpy()
    w_csr = ops.gather(eid, tf(w, dev))
    for lo, hi in [(0, 3), (3, 4), (4, 250), (250, 700), (690, 700)]:
        for algo in ["merge", "merge1", "rows", "generic"]:
            out = ops.spmm(indptr, col, row_of, tf(X, dev), w_csr, rows=(lo, hi - lo),
                           e_range=(int(ip[lo]), int(ip[hi])), algo=algo).cpu().numpy()
            assert out.shape == (hi - lo, D)
            assert sum_err(out, ref[lo:hi], ref_abs[lo:hi]) < TOL, (lo, hi, algo)
            fwd.check_gamma(out, ref[lo:hi], ref_abs[lo:hi], np.diff(ip)[lo:hi], 0, "shard [%d, %d) %s" % (lo, hi, algo))


@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_spmm_self_copy_epilogue(K, dev, D):
    """kgat_spmm_umule_sum_f32's self_out: the h * h_N launch also writes X[v] into a column slice of
    a wider buffer (the ego block of the readout) - same bits in `out` as without it, every row of the
    slice equal to X (rows finished in a tile, rows finished by the finish launch, rows without
    in-edges), nothing outside the slice touched; whole graph and a row-range shard."""
    from dgl_kgat_amd import ops
    n, e = 3000, 90000
    src, dst = random_graph(50 + D, n, e, hub=20000, isolated_tail=40)
    rng = np.random.default_rng(51)
    X = tf(rng.standard_normal((n, D)).astype(np.float32), dev)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    w_csr = tf(rng.random(e).astype(np.float32), dev)
    ip = indptr.cpu().numpy()
    for lo, hi in [(0, n), (5, 1700)]:
        kw = dict(rows=(lo, hi - lo), e_range=(int(ip[lo]), int(ip[hi])))
        plain = ops.spmm(indptr, col, row_of, X, w_csr, mul_self=True, **kw)
        wide = torch.full((hi - lo, D + 24), 7.0, device=dev)
        got = ops.spmm(indptr, col, row_of, X, w_csr, mul_self=True, self_out=wide[:, 8:8 + D], **kw)
        assert torch.equal(got, plain)
        assert torch.equal(wide[:, 8:8 + D], X[lo:hi])
        assert bool((wide[:, :8] == 7.0).all()) and bool((wide[:, 8 + D:] == 7.0).all())
    with pytest.raises(Exception):   # the copy reads the row the product reads: it needs KGAT_SPMM_MUL_SELF
        ops.spmm(indptr, col, row_of, X, w_csr, self_out=torch.empty((n, D), device=dev))


FUSED_WIDTHS = [(64, 64), (64, 32), (64, 16), (32, 32), (32, 16), (16, 16)]


def _fused_vs_two_launches(ops, indptr, col, row_of, X, w_csr, W2, dev, lo=None, hi=None, self_copy=False):
    """kgat_spmm_bi_fused_f32 against kgat_spmm_umule_sum_f32(MUL_SELF) + kgat_bi_interaction_f32 on the same
    inputs: the same bits in h_out and in the normalised slice, nothing outside the slice touched."""
    n, d_in = X.shape
    d_out = W2.shape[0]
    kw = {}
    if lo is not None:
        ip = indptr.cpu().numpy()
        kw = dict(rows=(lo, hi - lo), e_range=(int(ip[lo]), int(ip[hi])))
    rows = n if lo is None else hi - lo
    prod = ops.spmm(indptr, col, row_of, X, w_csr, mul_self=True, **kw)
    wide_a = torch.full((rows, d_out + 24), 9.0, device=dev)
    h_a = ops.bi_interaction(prod, W2, 0.01, norm_out=wide_a[:, 8:8 + d_out])
    wide_b = torch.full((rows, d_out + 24), 9.0, device=dev)
    ego = torch.full((rows, d_in + 8), 5.0, device=dev) if self_copy else None
    h_b = ops.spmm_bi_fused(indptr, col, row_of, X, w_csr, W2, 0.01, norm_out=wide_b[:, 8:8 + d_out],
                            self_out=None if ego is None else ego[:, 4:4 + d_in], **kw)
    assert torch.equal(h_a, h_b), float((h_a - h_b).abs().max())
    assert torch.equal(wide_a, wide_b)
    if ego is not None:
        assert torch.equal(ego[:, 4:4 + d_in], X if lo is None else X[lo:hi])
        assert bool((ego[:, :4] == 5.0).all()) and bool((ego[:, 4 + d_in:] == 5.0).all())
    # norm-only form (the last layer of the readout): h_out not wanted
    wide_c = torch.full((rows, d_out + 24), 9.0, device=dev)
    assert ops.spmm_bi_fused(indptr, col, row_of, X, w_csr, W2, 0.01, norm_out=wide_c[:, 8:8 + d_out], want_h=False,
                             **kw) is None
    assert torch.equal(wide_a, wide_c)
    return h_b, wide_b[:, 8:8 + d_out]


@pytest.mark.parametrize("d_in,d_out", FUSED_WIDTHS)
@pytest.mark.parametrize("name,n,e,hub,iso", GRAPHS)
def test_spmm_bi_fused_vs_two_launches_and_oracle(K, dev, d_in, d_out, name, n, e, hub, iso):
    """S1 + B1 + B2 in one launch (reference models.py:63-66 + :165): the same bits as the two-launch
    sequence, and within the aggregation's / bi-interaction's bars of the fp64 oracle; graphs with empty
    rows, a hub row spanning many tiles, a single row holding every edge, no edges at all."""
    from dgl_kgat_amd import ops
    src, dst = random_graph(7, n, e, hub, iso)
    rng = np.random.default_rng(8)
    X = rng.standard_normal((n, d_in)).astype(np.float32)
    w = rng.random(e).astype(np.float32)
    W2 = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    w_csr = ops.gather(eid, tf(w, dev)) if e else tf(w, dev)
    h, nrm = _fused_vs_two_launches(ops, indptr, col, row_of, tf(X, dev), w_csr, tf(W2, dev), dev, self_copy=True)
    hn = orc.spmm_u_mul_e_sum(n, src, dst, X, w)
    ref = orc.bi_interaction(X, hn, W2)
    assert rel_err_inf(h.cpu().numpy(), ref) < 1e-5
    assert rel_err_inf(nrm.cpu().numpy(), orc.l2_normalize(ref)) < 1e-4
    deg = np.diff(indptr.cpu().numpy())
    assert np.all(h.cpu().numpy()[deg == 0] == 0) and np.all(nrm.cpu().numpy()[deg == 0] == 0)
    assert np.all(np.isfinite(nrm.cpu().numpy()))


@pytest.mark.parametrize("d_in,d_out", [(64, 64), (64, 32), (32, 16)])
def test_spmm_bi_fused_long_runs_spill_and_shards(K, dev, d_in, d_out):
    """Large enough (3.3 M edges) for the full run length; a stretch of degree-1 rows so that tiles span far
    more rows than the LDS row buffer holds (the spill path through the global scratch), a stretch of empty
    rows inside a tile's range, a 600 k-edge hub (a boundary row finished by the long-chain path of the
    finish launch); whole graph, row-range shards (short and mid run lengths), repeated launch = same bits."""
    from dgl_kgat_amd import ops
    n, e = 30000, 3_300_000
    rng = np.random.default_rng(90 + d_in)
    src, dst = random_graph(91, n, e, hub=600_000, isolated_tail=500)
    # rows 20000..24999: exactly one in-edge each (5,000 rows in ~5 tiles), rows 25000..25999 then empty
    keep = (dst < 20000) | (dst >= 26000)
    src, dst = src[keep], dst[keep]
    src = np.concatenate([src, rng.integers(0, n, 5000).astype(np.int32)])
    dst = np.concatenate([dst, np.arange(20000, 25000, dtype=np.int32)])
    e = len(src)
    X = tf(rng.standard_normal((n, d_in)).astype(np.float32), dev)
    W2 = tf((rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32), dev)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    w_csr = tf(rng.random(e).astype(np.float32), dev)
    h, _ = _fused_vs_two_launches(ops, indptr, col, row_of, X, w_csr, W2, dev, self_copy=True)
    h2, _ = _fused_vs_two_launches(ops, indptr, col, row_of, X, w_csr, W2, dev)
    assert torch.equal(h, h2)
    for lo, hi in [(0, 5), (5, 9000), (19990, 26010), (24000, n), (n - 3, n)]:
        _fused_vs_two_launches(ops, indptr, col, row_of, X, w_csr, W2, dev, lo=lo, hi=hi, self_copy=(lo == 5))


def test_gnn_one_launch_layers_same_bits(K, dev, monkeypatch):
    """Model.gnn with KGAT_FUSE_BI=1 (every layer one kgat_spmm_bi_fused_f32 launch, ego block written by the
    first) against the default two launches per layer: the same bits in the whole readout."""
    from dgl_kgat_amd import synth
    n, trip, R = synth.amazon_book_ckg(scale=0.05)
    torch.manual_seed(3)
    model = K.KGATPropagation(n, R, 64, 64, 3, 64, dropout=0.0).to(dev)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
        from dgl_kgat_amd import options
        with options.override(fuse_bi=False):
            two = model.gnn(g)
        with options.override(fuse_bi=True):
            one = model.gnn(g)
    assert torch.equal(one, two), float((one - two).abs().max())


def test_spmm_bi_fused_refuses_what_it_cannot_do(K, dev):
    from dgl_kgat_amd import ops
    assert ops.spmm_bi_fused_supported(64, 64) and ops.spmm_bi_fused_supported(32, 16)
    assert not ops.spmm_bi_fused_supported(128, 128) and not ops.spmm_bi_fused_supported(16, 32)
    assert not ops.spmm_bi_fused_supported(8, 8)
    n, e = 50, 300
    src, dst = random_graph(3, n, e)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    X, w = torch.randn(n, 128, device=dev), torch.rand(e, device=dev)
    with pytest.raises(Exception):
        ops.spmm_bi_fused(indptr, col, row_of, X, w, torch.randn(128, 128, device=dev))
    X = torch.randn(n, 64, device=dev)
    wide = torch.empty((n, 70), device=dev)
    with pytest.raises(Exception):   # a normalised slice that is not 16-byte aligned
        ops.spmm_bi_fused(indptr, col, row_of, X, w, torch.randn(64, 64, device=dev), norm_out=wide[:, 3:67])


@pytest.mark.parametrize("name,n,e,hub,iso", GRAPHS)
def test_edge_softmax_vs_oracle(K, dev, name, n, e, hub, iso):
    from dgl_kgat_amd import ops
    if e == 0:
        pytest.skip("no edges")
    src, dst = random_graph(7, n, e, hub, iso)
    rng = np.random.default_rng(8)
    s = (rng.standard_normal(e) * 4).astype(np.float32)
    s[: min(e, 4)] = [80.0, -80.0, 0.0, -0.0][: min(e, 4)]
    ref = orc.edge_softmax(n, dst, s)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    out, out_csr = ops.edge_softmax(indptr, row_of, eid, tf(s, dev), want_out=True, want_csr=True)
    out, out_csr = out.cpu().numpy(), out_csr.cpu().numpy()
    assert np.all(np.isfinite(out))
    assert rel_err(out, ref) < TOL
    assert np.array_equal(out_csr, out[eid.cpu().numpy()])
    # CSR-ordered input gives the same bits
    s_csr = ops.gather(eid, tf(s, dev))
    out2, _ = ops.edge_softmax(indptr, row_of, eid, s_csr, in_csr_order=True, want_out=True)
    assert np.array_equal(out2.cpu().numpy(), out)
    # every non-empty destination's weights sum to one; shift invariance per destination
    sums = np.zeros(n)
    np.add.at(sums, dst, out.astype(np.float64))
    assert np.allclose(sums[np.bincount(dst, minlength=n) > 0], 1.0, atol=1e-5)
    shift = rng.standard_normal(n).astype(np.float32)[dst] * 3
    out3, _ = ops.edge_softmax(indptr, row_of, eid, tf(s + shift, dev))
    assert rel_err(out3.cpu().numpy(), ref) < 5e-4  # the shifted fp32 logits round differently
    # reproducible bit for bit
    out4, _ = ops.edge_softmax(indptr, row_of, eid, tf(s, dev))
    assert np.array_equal(out4.cpu().numpy(), out)


@pytest.mark.parametrize("e", [1, 15, 16, 17, 1023, 1024, 1025, 2048, 70001])
def test_edge_softmax_range_boundaries_and_hubs(K, dev, e):
    """Rows cut by the 512-position wavefront ranges of the 8-positions-per-lane form every call here takes (incl.
    rows spanning many ranges and a row that is the whole graph; the 1,024-position form: test_gpu_softmax_wide.py),
    sizes around the lane / range granularity, destination-range sub-ranges (shards), and agreement with the
    independent three-pass implementation."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(100 + e)
    n = 300
    for layout in ("one_row", "hubs", "short"):
        if layout == "one_row":
            dst = np.full(e, 7, np.int32)
        elif layout == "hubs":  # a few rows hold almost everything, the rest are short
            dst = rng.choice(np.array([3, 150, 299], np.int32), e, p=[0.6, 0.3, 0.1]).astype(np.int32)
            dst[rng.random(e) < 0.05] = rng.integers(0, n, int((rng.random(e) < 0.05).sum()) or 1)[0]
        else:
            dst = rng.integers(0, n, e).astype(np.int32)
        src = rng.integers(0, n, e).astype(np.int32)
        s = (rng.standard_normal(e) * 5).astype(np.float32)
        ref = orc.edge_softmax(n, dst, s)
        indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
        out, out_csr = ops.edge_softmax(indptr, row_of, eid, tf(s, dev), want_out=True, want_csr=True)
        assert rel_err(out.cpu().numpy(), ref) < TOL, layout
        assert torch.equal(out_csr, out[eid.long()])
        old, old_csr = ops.edge_softmax(indptr, row_of, eid, tf(s, dev), want_out=True, want_csr=True, three_pass=True)
        assert rel_err(out.cpu().numpy(), old.cpu().numpy()) < 1e-5, layout
        # a destination-range shard: positions [indptr[lo], indptr[hi]) only
        ip = indptr.cpu().numpy()
        for lo, hi in ((0, n), (3, 151), (150, 300), (7, 8)):
            e0, e1 = int(ip[lo]), int(ip[hi])
            if e1 == e0:
                continue
            _, part_csr = ops.edge_softmax(indptr, row_of, eid, ops.gather(eid, tf(s, dev)), in_csr_order=True,
                                           e_range=(e0, e1), want_out=False, want_csr=True)
            # (other range boundaries: the cut rows are combined in another association)
            assert rel_err(part_csr[e0:e1].cpu().numpy(), out_csr[e0:e1].cpu().numpy()) < 1e-6, (layout, lo, hi)


@pytest.mark.parametrize("length", [1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 63, 64, 65, 120, 127, 128, 129, 136, 248, 256, 264,
                                    511, 512, 513, 520, 1000, 1500, 5000])
def test_edge_softmax_lane_structures(K, dev, length):
    """Rows of one length at every alignment against the sweep's geometry: 8 positions per lane, DPP rows of
    16 lanes (segments starting / ending at lanes 15 | 16, 31 | 32, 47 | 48), 512-position ranges (rows cut
    once, rows spanning several ranges, a range that is one row), shifted by a prefix row of 0 .. 13
    positions; against an fp64 segment softmax, CSR-ordered and index-mapped input giving the same bits."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(1000 + length)
    for off in (0, 1, 5, 8, 13):
        n_rows = max(3, min(4000 // length + 2, 700))
        dst = np.concatenate([np.zeros(off, np.int32), np.repeat(np.arange(1, n_rows + 1, dtype=np.int32), length),
                              np.full(3, n_rows + 2, np.int32)])  # (row n_rows + 1 has no in-edges)
        e, n = len(dst), n_rows + 4
        src = rng.integers(0, n, e).astype(np.int32)
        s = (rng.standard_normal(e) * 4).astype(np.float32)
        indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
        out, out_csr = ops.edge_softmax(indptr, row_of, eid, tf(s, dev), want_out=True, want_csr=True)
        x = s.astype(np.float64)
        m = np.full(n, -np.inf)
        np.maximum.at(m, dst, x)
        ex = np.exp(x - m[dst])
        z = np.zeros(n)
        np.add.at(z, dst, ex)
        ref = ex / z[dst]
        got = out.cpu().numpy()
        assert np.all(np.isfinite(got)) and np.max(np.abs(got - ref) / np.maximum(ref, 1e-3)) < 2e-6, (length, off)
        assert torch.equal(out_csr, out[eid.long()])
        _, csr_in = ops.edge_softmax(indptr, row_of, eid, ops.gather(eid, tf(s, dev)), in_csr_order=True, want_out=False,
                                     want_csr=True)
        assert torch.equal(csr_in, out_csr), (length, off)


def test_edge_softmax_known_answers(K, dev):
    from dgl_kgat_amd import ops
    src = np.array([1, 2, 3, 0], np.int32)
    dst = np.array([0, 0, 2, 3], np.int32)
    indptr, col, eid, row_of = ops.csr_from_coo(5, t32(src, dev), t32(dst, dev))
    a, _ = ops.edge_softmax(indptr, row_of, eid, tf([0.3, 0.3, -7.0, 80.0], dev))
    assert np.array_equal(a.cpu().numpy(), np.array([0.5, 0.5, 1.0, 1.0], np.float32))


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_att_score_golden(K, dev, case):
    """Attention logits against the outputs of the reference's own _att_score (F1)."""
    from dgl_kgat_amd import ops
    g = load_golden(case)
    n, R = g["n"], g["R"]
    src, dst, et = t32(g["src"], dev), t32(g["dst"], dev), t32(g["etype"], dev)
    rel_ptr, perm = ops.group_by_relation(et, R)
    sg, dg = ops.gather(perm, src), ops.gather(perm, dst)
    _, _, eid, _ = ops.csr_from_coo(n, src, dst)
    pos = ops.gather(perm, ops.invert_permutation(eid))
    d = g["entity_embed"].shape[1]
    algos = ["generic"] + (["mfma", "mfma_chunk"]
                           if d == g["W_R"].shape[2] and d in (16, 32, 64, 128) else [])
    for algo in algos:
        logits, logits_csr = ops.att_score(n, rel_ptr, perm, sg, dg, tf(g["entity_embed"], dev),
                                           tf(g["W_R"], dev), tf(g["relation_embed"], dev), pos_g=pos,
                                           algo=algo)
        logits = logits.cpu().numpy()
        for r in range(R):
            assert rel_err(logits[g["att_eids_%d" % r]], g["att_score_%d" % r].reshape(-1)) < TOL, (algo, r)
        assert np.array_equal(logits_csr.cpu().numpy(), logits[eid.cpu().numpy()])


@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_att_score_mfma_vs_oracle(K, dev, d):
    from dgl_kgat_amd import ops
    n, e, R = 900, 40000, 7
    src, dst = random_graph(9, n, e, hub=3000)
    rng = np.random.default_rng(10)
    et = rng.integers(-1, R + 1, e).astype(np.int32)  # some edges outside [0, R): logit 0
    et[rng.choice(e, e // 2, replace=False)] = 2     # one large relation (> one 1024-edge chunk)
    ent = rng.standard_normal((n, d)).astype(np.float32)
    W = (rng.random((R, d, d)).astype(np.float32) - 0.5) * (2.0 / np.sqrt(d))
    rel = rng.standard_normal((R, d)).astype(np.float32)
    ref = orc.att_score(ent, W, rel, src, dst, et)
    rel_ptr, perm = ops.group_by_relation(t32(et, dev), R)
    sg, dg = ops.gather(perm, t32(src, dev)), ops.gather(perm, t32(dst, dev))
    # mfma = persistent-wavefront kernel (d <= 64) / chunk kernel (d = 128); mfma_chunk = the workgroup-chunk
    # kernel AUTO falls back to (d = 128, > 4,096 relations, tables of 4 GiB and more) at every width
    for algo in ["mfma", "mfma_chunk", "generic"]:
        logits, _ = ops.att_score(n, rel_ptr, perm, sg, dg, tf(ent, dev), tf(W, dev), tf(rel, dev), algo=algo)
        logits = logits.cpu().numpy()
        assert np.all(logits[(et < 0) | (et >= R)] == 0)
        # the softmax that consumes the logits is sensitive to their ABSOLUTE error
        assert rel_err_inf(logits, ref) < 1e-5, algo


@pytest.mark.parametrize("algo", ["mfma", "mfma_chunk"])
def test_att_score_named_mfma_refuses_other_widths(K, dev, algo):
    """A caller who names an MFMA kernel at a (d, k) it does not cover is refused, not handed the generic kernel."""
    from dgl_kgat_amd import ops
    n, e, R, d, k = 50, 400, 3, 12, 20
    src, dst = random_graph(14, n, e)
    et = np.random.default_rng(15).integers(0, R, e).astype(np.int32)
    rel_ptr, perm = ops.group_by_relation(t32(et, dev), R)
    sg, dg = ops.gather(perm, t32(src, dev)), ops.gather(perm, t32(dst, dev))
    ent, W, rel = (torch.zeros(s, device=dev) for s in ((n, d), (R, d, k), (R, k)))
    with pytest.raises(ops.KGATLibraryError) as info:
        ops.att_score(n, rel_ptr, perm, sg, dg, ent, W, rel, algo=algo)
    assert "att_score: the MFMA kernel covers d == k in {16,32,64,128}, got d=12 k=20" in str(info.value)
    logits, _ = ops.att_score(n, rel_ptr, perm, sg, dg, ent, W, rel, algo="generic")   # the kernel that does cover it
    assert logits.shape == (e,) and not logits.any()


def test_att_wrappers_refuse_a_wrong_ent_shape_alike(K, dev):
    """The three wrappers check their parameters through one helper: an `ent` of the wrong height is a ValueError
    from each, in the same words (tests/test_att_host.py has the one-kernel wrapper's, without a device)."""
    from dgl_kgat_amd import ops
    n, e, R, d = 100, 10, 2, 16
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)   # noqa: E731
    ent, W, rel = (torch.zeros(s, device=dev) for s in ((n + 1, d), (R, d, d), (R, d)))
    calls = [lambda: ops.att_score(n, i32(R + 1), i32(e), i32(e), i32(e), ent, W, rel),
             lambda: ops.att_score_split(n, i32(R + 1), i32(e), i32(e), i32(e), i32(e), i32(R + 1), i32(4), 4, ent, W, rel),
             lambda: ops.att_score_fused(n, i32(R + 1), i32(e), i32(e), i32(e), i32(e), i32(R + 1), i32(4), i32(3, 4),
                                         i32(R + 1), ent, W, rel, rec_g=i32(e))]
    for call in calls:
        with pytest.raises(ValueError) as info:
            call()
        assert "ent has shape (101, 16), expected (100, 16)" in str(info.value)


def _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev):
    """The structure DGLGraph.rel_groups builds: CSR-ordered edges grouped stably by relation."""
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    rel_ptr, idx = ops.group_by_relation(ops.gather(eid, t32(et, dev)), R)
    perm, src_g, dst_g = ops.gather(idx, eid), ops.gather(idx, col), ops.gather(idx, row_of)
    return rel_ptr, perm, src_g, dst_g, idx


@pytest.mark.parametrize("d", [16, 32, 64])
def test_att_split_head_groups(K, dev, d):
    """Head-group structure bit-exact vs the oracle; split attention == one-kernel attention
    bit for bit (same arithmetic per edge) and within tolerance of the fp64 oracle."""
    from dgl_kgat_amd import ops
    n, e, R = 700, 30000, 6
    src, dst = random_graph(12, n, e, hub=4000, isolated_tail=20)
    rng = np.random.default_rng(13)
    et = rng.integers(-1, R + 1, e).astype(np.int32)
    et[rng.choice(e, e // 2, replace=False)] = 3
    et[et == 1] = 2  # an empty relation in the middle
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    ogid, ogptr, ognode = orc.head_groups(rel_ptr.cpu().numpy(), dst_g.cpu().numpy())
    scored = int(rel_ptr[-1])
    assert n_groups == len(ognode) == int(ogptr[-1])
    assert np.array_equal(gid.cpu().numpy()[:scored], ogid[:scored])
    # positions of never-scored edges carry group id 0: the tail kernels read the ids of a whole
    # 16-position tile past the last relation's end and index the per-group table with them
    assert scored < e and np.all(gid.cpu().numpy()[scored:] == 0)
    assert np.array_equal(gptr.cpu().numpy(), ogptr) and np.array_equal(g_node.cpu().numpy()[:n_groups], ognode)
    # every scored position's group has its (relation, destination)
    perm_h, et_g = perm.cpu().numpy(), et[perm.cpu().numpy()]
    assert np.array_equal(ognode[ogid[:scored]], dst[perm_h[:scored]])
    assert np.all(np.diff(ogid[:scored]) >= 0) and np.all(et_g[:scored][1:] >= et_g[:scored][:-1])
    ent = rng.standard_normal((n, d)).astype(np.float32)
    W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
    rel = rng.standard_normal((R, d)).astype(np.float32)
    ref = orc.att_score(ent, W, rel, src, dst, et)
    split, split_csr = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups,
                                           tf(ent, dev), tf(W, dev), tf(rel, dev))
    full, full_csr = ops.att_score(n, rel_ptr, perm, src_g, dst_g, tf(ent, dev), tf(W, dev), tf(rel, dev),
                                   pos_g=pos_g, algo="mfma")
    assert torch.equal(split, full) and torch.equal(split_csr, full_csr)
    split = split.cpu().numpy()
    assert np.all(split[(et < 0) | (et >= R)] == 0)
    assert rel_err_inf(split, ref) < 1e-5
    _, _, eid, _ = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    assert np.array_equal(split_csr.cpu().numpy(), split[eid.cpu().numpy()])
    # folded form: W_r tanh(.) once per group, a d-length dot per edge - another contraction
    # order, so fp32 rounding apart from the others, same tolerance against the oracle
    for want_eid in (True, False):
        fold, fold_csr = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups,
                                             tf(ent, dev), tf(W, dev), tf(rel, dev), folded=True, want_eid=want_eid)
        assert rel_err_inf(fold_csr.cpu().numpy(), ref[eid.cpu().numpy()]) < 1e-5
        if want_eid:
            assert torch.equal(fold_csr, fold[eid.long()])
            assert np.all(fold.cpu().numpy()[(et < 0) | (et >= R)] == 0)
        else:
            assert fold is None


@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("cap", [64, 256])
def test_att_fused_tiles_and_logits(K, dev, d, cap):
    """Fused folded form: the tile table is bit-exact against the oracle's restatement, and the
    logits agree with the two-launch folded form to fp32 rounding and with the fp64 oracle."""
    from dgl_kgat_amd import ops
    n, e, R = 700, 30000, 6
    src, dst = random_graph(12, n, e, hub=4000, isolated_tail=20)
    rng = np.random.default_rng(13)
    et = rng.integers(-1, R + 1, e).astype(np.int32)
    et[rng.choice(e, e // 2, replace=False)] = 3
    et[et == 1] = 2  # an empty relation in the middle
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    tiles, rel_tptr, part_tptr = ops.fold_tiles(rel_ptr, gid, gptr, n_groups, cap=cap, n_parts=37, cost=(64, 12, 466))
    o_tiles, o_tptr = orc.fold_tiles(rel_ptr.cpu().numpy(), gid.cpu().numpy(), gptr.cpu().numpy(), cap)
    assert np.array_equal(rel_tptr.cpu().numpy(), o_tptr)
    n_tiles = int(o_tptr[-1])
    assert n_tiles <= tiles.shape[0] and np.array_equal(tiles.cpu().numpy()[:n_tiles], o_tiles)
    assert np.all(o_tiles[:, 3] - o_tiles[:, 2] <= cap)
    # the cost-balanced split over workgroups: bit-exact against its restatement, monotone, complete
    o_parts = orc.fold_tile_parts(o_tiles, o_tptr, 37, (64, 12, 466))
    assert np.array_equal(part_tptr.cpu().numpy(), o_parts) and o_parts[0] == 0 and o_parts[-1] == n_tiles
    assert np.all(np.diff(o_parts) >= 0)
    ent = rng.standard_normal((n, d)).astype(np.float32)
    W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
    rel = rng.standard_normal((R, d)).astype(np.float32)
    ref = orc.att_score(ent, W, rel, src, dst, et)
    fold, fold_csr = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups,
                                         tf(ent, dev), tf(W, dev), tf(rel, dev), folded=True)
    for want_eid in (True, False):
        fused, fused_csr = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                               tf(ent, dev), tf(W, dev), tf(rel, dev), want_eid=want_eid,
                                               part_tptr=part_tptr)
        # (another lane split of the d-length dot product than the two-launch form: fp32 rounding apart)
        assert rel_err_inf(fused_csr.cpu().numpy(), fold_csr.cpu().numpy()) < 2e-6
        if want_eid:
            assert torch.equal(fused_csr, fused[ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))[2].long()])
        # which workgroup computes a tile does not enter its arithmetic: any split gives the same bits
        even = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                   tf(ent, dev), tf(W, dev), tf(rel, dev), want_eid=False)[1]
        assert torch.equal(even, fused_csr)
        # grouped-order output (coalesced stores; what the propagation path takes): the same values at
        # the grouped positions, alone or beside the scattered outputs, never-scored positions zero
        rec = ops.att_pack_records(rel_ptr, gptr, gid, src_g)
        rec_h, n_scored = rec.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, int(rel_ptr[-1])
        assert np.array_equal(rec_h & 0x0FFFFFFF, src_g.cpu().numpy())
        rel_of = np.searchsorted(rel_ptr.cpu().numpy(), np.arange(n_scored), side="right") - 1
        assert np.array_equal(rec_h[:n_scored] >> 28, (gid.cpu().numpy()[:n_scored] - gptr.cpu().numpy()[rel_of]) & 15)
        assert np.all(rec_h[n_scored:] >> 28 == 0)
        for kw in (dict(want_eid=False, want_csr=False), dict(want_eid=want_eid, want_csr=True)):
            g_out = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                        tf(ent, dev), tf(W, dev), tf(rel, dev), part_tptr=part_tptr, rec_g=rec,
                                        want_grouped=True, **kw)
            assert torch.equal(g_out[2], fused_csr[pos_g.long()])
            assert kw["want_csr"] is False or torch.equal(g_out[1], fused_csr)
            assert float(g_out[2][n_scored:].abs().max()) == 0 if n_scored < e else True
    assert rel_err_inf(fused_csr.cpu().numpy(), ref[ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))[2].cpu().numpy()]) < 1e-5


def test_att_fused_small_and_single_relation(K, dev):
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(78)
    for n, e, R, lo in ((50, 1, 1, 0), (50, 63, 2, 0), (90, 65, 3, -1), (300, 1000, 1, 0), (300, 4097, 5, -2)):
        src, dst = rng.integers(0, n, e).astype(np.int32), rng.integers(0, max(n // 3, 1), e).astype(np.int32)
        et = rng.integers(lo, R, e).astype(np.int32)
        rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
        gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
        tiles, rel_tptr, part_tptr = ops.fold_tiles(rel_ptr, gid, gptr, n_groups, cap=64)
        d = 32
        ent = rng.standard_normal((n, d)).astype(np.float32)
        W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
        rel = rng.standard_normal((R, d)).astype(np.float32)
        ref = orc.att_score(ent, W, rel, src, dst, et)
        fused, fused_csr = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                               tf(ent, dev), tf(W, dev), tf(rel, dev), part_tptr=part_tptr)
        _, _, eid, _ = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
        assert rel_err_inf(fused.cpu().numpy(), ref) < 1e-5, (n, e, R)
        assert np.all(fused.cpu().numpy()[et < 0] == 0)
        assert torch.equal(fused_csr, fused[eid.long()])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_att_fused_product_forms(K, dev, d):
    """The default products of the fused kernel (d = 32, 64) and of the two-launch folded form's
    head kernel (d = 128) - three bf16 pieces per fp32 operand, six piece products in the fp32
    accumulator of the bf16 MFMA - against the fp32-MFMA products and the fp64 oracle: no further
    from fp64 than the fp32 form, under 8c and in absolute terms, also when the operands span
    forty orders of magnitude (every piece keeps the fp32 exponent range)."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(2024 + d)
    n, e, R = 3000, 60000, 7
    src, dst = random_graph(31, n, e, hub=3000, isolated_tail=10)
    et = rng.integers(0, R, e).astype(np.int32)
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    tiles, rel_tptr, part_tptr = ops.fold_tiles(rel_ptr, gid, gptr, n_groups, n_parts=19)
    W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
    rel = rng.standard_normal((R, d)).astype(np.float32)
    W0, rel0 = W, rel
    for case in ("normal", "wide range", "tiny", "signed zeros", "all positive", "large W", "small T"):
        ent = rng.standard_normal((n, d)).astype(np.float32)
        W, rel = W0, rel0
        if case == "all positive":   # same-sign operands everywhere: a one-sided error per product would add up
            ent, W, rel = np.abs(ent), np.abs(W0) * np.float32(0.25), np.abs(rel0) * np.float32(0.1)
        elif case == "large W":      # |W| near 1: d-term sums of O(1) products, tanh saturating
            W = np.sign(W0) * (np.float32(0.75) + np.float32(0.25) * np.abs(W0) * np.float32(np.sqrt(d)))
        if case == "wide range":   # rows scaled by 2^-60 .. 2^+10; elements by up to 2^-12 more
            ent *= np.exp2(rng.integers(-60, 11, (n, 1))).astype(np.float32)
            ent *= np.exp2(-rng.integers(0, 13, (n, d))).astype(np.float32)
        elif case == "tiny":       # around the subnormal boundary: products vanish, logits = 0 + rounding
            ent *= np.float32(1e-37)
        elif case == "signed zeros":
            ent[rng.random((n, d)) < 0.5] = -0.0
        elif case == "small T":    # |tanh| ~ 1e-3 everywhere (small embeddings AND small relation vectors): the second
            ent *= np.float32(1e-3)  # product's two fp16 pieces of a tanh value must still carry 22 bits of it
            rel = rel0 * np.float32(1e-3)
        ref = orc.att_score(ent, W, rel, src, dst, et)
        got = {}
        for f32p in (False, True):
            if d <= 64:
                out = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                          tf(ent, dev), tf(W, dev), tf(rel, dev), want_csr=False,
                                          part_tptr=part_tptr, f32_products=f32p)[0]
            else:
                out = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups, tf(ent, dev),
                                          tf(W, dev), tf(rel, dev), want_csr=False, folded=True, f32_products=f32p)[0]
            got[f32p] = out.cpu().numpy()
            assert np.isfinite(got[f32p]).all()
        if d == 128:   # the fused one-launch form at d = 128 has the piece products only: same bar
            out = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                      tf(ent, dev), tf(W, dev), tf(rel, dev), want_csr=False, part_tptr=part_tptr)[0]
            fused128 = out.cpu().numpy()
            assert np.isfinite(fused128).all()
            sc_ = max(float(np.abs(ref).max()), 1e-30)
            print("[att products d=128 %-12s] fused kernel (fp16 pieces, 3 piece products): max|err|/max|ref| %.3e  mean %.3e"
                  "  (fp32 products %.3e  mean %.3e)" % (case, np.abs(fused128 - ref).max() / sc_,
                                                       np.abs(fused128 - ref).mean() / sc_,
                                                       np.abs(got[True] - ref).max() / sc_, np.abs(got[True] - ref).mean() / sc_))
            assert np.abs(fused128 - ref).max() <= max(2.0 * np.abs(got[True] - ref).max(),
                                                       2e-7 * max(float(np.abs(ref).max()), 1e-30)), case
        scale = max(float(np.abs(ref).max()), 1e-30)
        e_new, e_f32 = np.abs(got[False] - ref).max(), np.abs(got[True] - ref).max()
        print("[att products d=%d %-12s] max|err|/max|ref|: bf16 pieces %.3e  fp32 products %.3e ; 8c %.3e  %.3e"
              % (d, case, e_new / scale, e_f32 / scale, rel_err(got[False], ref), rel_err(got[True], ref)))
        assert e_new <= max(2.0 * e_f32, 2e-7 * scale), (case, e_new, e_f32)
        assert rel_err(got[False], ref) <= max(1e-4, 2.0 * rel_err(got[True], ref)), case
        if case in ("all positive", "large W"):
            # round-to-nearest pieces: the dropped piece products are two-signed and below one fp32 ulp of
            # a product, so same-sign sums do not drift: the mean signed error stays far below the fp32
            # chain's rounding level, and the piece form is no worse than the fp32-MFMA form
            bias = abs(float(np.mean(got[False].astype(np.float64) - ref))) / scale
            bias32 = abs(float(np.mean(got[True].astype(np.float64) - ref))) / scale   # (shares the tanh evaluation)
            print("    mean signed error / max|ref|: bf16 pieces %.3e  fp32 products %.3e" % (bias, bias32))
            assert e_new <= 1.0 * e_f32 + 1e-7 * scale and bias <= max(2.0 * bias32, 3e-8), (case, e_new, e_f32, bias)


@pytest.mark.parametrize("d", [64, 128])
def test_att_fused_timed_entry(K, dev, d):
    """kgat_att_score_fused_timed_f32 (measurement aid): the bits of the plain launch, and for every workgroup with a
    tile range a start tick before its end tick inside one launch-long window."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(5 + d)
    n, e, R = 2000, 50000, 6
    src, dst = random_graph(77, n, e, hub=2500, isolated_tail=5)
    et = rng.integers(0, R, e).astype(np.int32)
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    tiles, rel_tptr, part_tptr = ops.fold_tiles(rel_ptr, gid, gptr, n_groups, n_parts=37, cost=ops.fold_tile_cost(d))
    ent = tf(rng.standard_normal((n, d)).astype(np.float32), dev)
    W = tf(((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32), dev)
    rel = tf(rng.standard_normal((R, d)).astype(np.float32), dev)
    plain = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr, ent, W, rel,
                                part_tptr=part_tptr)
    clocks = torch.zeros(2 * 37, dtype=torch.int64, device=dev)
    timed = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr, ent, W, rel,
                                part_tptr=part_tptr, part_clocks=clocks)
    assert torch.equal(plain[0], timed[0]) and torch.equal(plain[1], timed[1])
    c = clocks.cpu().numpy().reshape(-1, 2)
    assert (c[:, 0] > 0).all() and (c[:, 1] >= c[:, 0]).all()
    assert c[:, 1].max() - c[:, 0].min() < 100 * 1000 * 50      # all inside 50 ms of 100 MHz ticks
    with pytest.raises(Exception):
        ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr, ent, W, rel,
                            part_tptr=None, part_clocks=clocks)


def test_att_folded_d128(K, dev):
    """d = k = 128: W_r (64 KB) lives in LDS, 32 floats per lane in the per-edge dot."""
    from dgl_kgat_amd import ops
    n, e, R, d = 900, 40000, 5, 128
    src, dst = random_graph(21, n, e, hub=3000, isolated_tail=10)
    rng = np.random.default_rng(22)
    et = rng.integers(-1, R + 1, e).astype(np.int32)
    et[et == 2] = 3  # an empty relation
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    ent = rng.standard_normal((n, d)).astype(np.float32)
    W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
    rel = rng.standard_normal((R, d)).astype(np.float32)
    ref = orc.att_score(ent, W, rel, src, dst, et)
    assert ops.att_score_folded_supported(n, d, d, R) and not ops.att_score_split_supported(n, d, d, R)
    fold, fold_csr = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups,
                                         tf(ent, dev), tf(W, dev), tf(rel, dev), folded=True)
    _, _, eid, _ = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    assert rel_err_inf(fold.cpu().numpy(), ref) < 1e-5
    assert np.all(fold.cpu().numpy()[(et < 0) | (et >= R)] == 0)
    assert torch.equal(fold_csr, fold[eid.long()])
    full, _ = ops.att_score(n, rel_ptr, perm, src_g, dst_g, tf(ent, dev), tf(W, dev), tf(rel, dev), pos_g=pos_g)
    assert rel_err_inf(fold.cpu().numpy(), full.cpu().numpy()) < 1e-5
    # the one-launch fused form at d = 128 (round 3): same V rows, the per-edge dot split over 8 lanes
    # as in the two-launch form's tail kernel; every output order, any split of the tiles, small caps
    assert ops.att_score_fused_supported(n, d, d, R)
    for cap, n_parts in ((64, 5), (256, 37)):
        tiles, rel_tptr, part_tptr = ops.fold_tiles(rel_ptr, gid, gptr, n_groups, cap=cap, n_parts=n_parts,
                                                    cost=ops.fold_tile_cost(d))
        fe, fc, fg = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr,
                                         tf(ent, dev), tf(W, dev), tf(rel, dev), part_tptr=part_tptr, want_grouped=True)
        assert rel_err_inf(fe.cpu().numpy(), ref) < 1e-5 and rel_err_inf(fe.cpu().numpy(), fold.cpu().numpy()) < 2e-6
        assert np.all(fe.cpu().numpy()[(et < 0) | (et >= R)] == 0)
        assert torch.equal(fc, fe[eid.long()]) and torch.equal(fg, fc[pos_g.long()])
        only_g = ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr, tf(ent, dev),
                                     tf(W, dev), tf(rel, dev), want_eid=False, want_csr=False, want_grouped=True)[2]
        assert torch.equal(only_g, fg)   # equal tile counts per workgroup instead of the cost split: same bits
    with pytest.raises(Exception, match="bf16-piece products only"):
        ops.att_score_fused(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr, tf(ent, dev), tf(W, dev),
                            tf(rel, dev), f32_products=True)


@pytest.mark.parametrize("d,k", [(8, 8), (16, 32), (32, 8), (8, 5), (16, 17)])
def test_att_folded_small_widths(K, dev, d, k):
    """Folded form without an MFMA tile shape (one thread per group): d in {8,16,32}, any k <= 32 -
    BASELINE configs[0] is d = k = 8 - against the fp64 oracle and the generic per-edge kernel."""
    from dgl_kgat_amd import ops
    n, e, R = 600, 20000, 6
    src, dst = random_graph(41, n, e, hub=3000, isolated_tail=10)
    rng = np.random.default_rng(42)
    et = rng.integers(-1, R + 1, e).astype(np.int32)
    et[et == 4] = 3  # an empty relation
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    ent = rng.standard_normal((n, d)).astype(np.float32)
    W = ((rng.random((R, d, k)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
    rel = rng.standard_normal((R, k)).astype(np.float32)
    ref = orc.att_score(ent, W, rel, src, dst, et)
    assert ops.att_score_folded_supported(n, d, k, R)
    fold, fold_csr = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups,
                                         tf(ent, dev), tf(W, dev), tf(rel, dev), folded=True)
    _, _, eid, _ = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    assert rel_err_inf(fold.cpu().numpy(), ref) < 1e-5
    assert np.all(fold.cpu().numpy()[(et < 0) | (et >= R)] == 0)
    assert torch.equal(fold_csr, fold[eid.long()])
    gen, _ = ops.att_score(n, rel_ptr, perm, src_g, dst_g, tf(ent, dev), tf(W, dev), tf(rel, dev), algo="generic")
    assert rel_err_inf(fold.cpu().numpy(), gen.cpu().numpy()) < 1e-5


def test_att_folded_ragged_tail_positions(K, dev):
    """Folded form on edge counts that are not multiples of the 64-position wavefront chunk, with
    and without an unscored tail, and one relation only."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(77)
    for n, e, R, lo in ((50, 1, 1, 0), (50, 63, 2, 0), (90, 65, 3, -1), (300, 1000, 1, 0), (300, 4097, 5, -2)):
        src, dst = rng.integers(0, n, e).astype(np.int32), rng.integers(0, max(n // 3, 1), e).astype(np.int32)
        et = rng.integers(lo, R, e).astype(np.int32)
        rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
        gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
        d = 32
        ent = rng.standard_normal((n, d)).astype(np.float32)
        W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
        rel = rng.standard_normal((R, d)).astype(np.float32)
        ref = orc.att_score(ent, W, rel, src, dst, et)
        fold, fold_csr = ops.att_score_split(n, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups,
                                             tf(ent, dev), tf(W, dev), tf(rel, dev), folded=True)
        _, _, eid, _ = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
        assert rel_err_inf(fold.cpu().numpy(), ref) < 1e-5, (n, e, R)
        assert np.all(fold.cpu().numpy()[et < 0] == 0)
        assert torch.equal(fold_csr, fold[eid.long()])


def _model_from_golden(K, g, dev):
    d, k = g["entity_embed"].shape[1], g["W_R"].shape[2]
    hidden = g["W2"][0].shape[0]
    m = K.KGATPropagation(g["n"], g["R"], input_node_dim=d, relation_dim=k, num_gnn_layers=len(g["W2"]),
                          n_hidden=hidden, dropout=0.0)
    sd = {"entity_embed.weight": g["entity_embed"], "relation_embed.weight": g["relation_embed"], "W_R": g["W_R"]}
    for i, W2 in enumerate(g["W2"]):
        sd["layers.%d.res_fc_2.weight" % i] = W2
    m.load_state_dict({k_: torch.as_tensor(v) for k_, v in sd.items()})
    return m.to(dev)


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_layer_surface_and_fused_vs_reference_glue(K, dev, case):
    """The reference's call sequence over the drop-in surface, and the fused path, against the
    outputs of the reference's own compute_attention / gnn glue (F2)."""
    from dgl_kgat_amd import synth
    g = load_golden(case)
    model = _model_from_golden(K, g, dev)
    graph = synth.build_graph(g["n"], g["triplets"], dev)
    with torch.no_grad():
        a_surface = model.compute_attention_surface(graph)
        a_fused = model.compute_attention(graph)
        assert a_surface.shape == a_fused.shape == (len(g["src"]), 1)
        assert rel_err(a_surface.cpu().numpy(), g["attention"]) < TOL
        assert rel_err(a_fused.cpu().numpy(), g["attention"]) < TOL
        graph.edata["w"] = a_fused
        widths = [g["entity_embed"].shape[1]] + [W2.shape[0] for W2 in g["W2"]]
        # the same step by the C/OpenMP fp32 oracle: the 8c metric of the device result is bounded by
        # what a CPU fp32 forward shows against the reference's own fp64 outputs
        indptr_c, col_c, eid_c = co.csr_from_coo(g["n"], g["src"], g["dst"])
        a_c = co.edge_softmax(g["n"], indptr_c, eid_c,
                              co.att_score(g["entity_embed"], g["W_R"], g["relation_embed"], g["src"], g["dst"], g["etype"]))
        parity_8c(case + " attention", a_fused.cpu().numpy().reshape(-1), a_c, g["attention"].reshape(-1))
        h_c, cache_c = g["entity_embed"].astype(np.float32), [g["entity_embed"].astype(np.float32)]
        for W2 in g["W2"]:
            h_c = co.bi_interaction(h_c, co.spmm(g["n"], indptr_c, col_c, eid_c, h_c, a_c), W2)
            cache_c.append(co.l2_normalize(h_c))
        out_c = np.concatenate(cache_c, 1)
        for fused in (False, True):
            out = model.gnn(graph, fused=fused)
            assert out.shape == g["gnn_out"].shape
            assert blocks_rel_err_inf(out.cpu().numpy(), g["gnn_out"], widths) < TOL, fused
            for bi, (x, c, y) in enumerate(zip(blocks(out.cpu().numpy(), widths), blocks(out_c, widths),
                                               blocks(g["gnn_out"], widths))):
                # robust statistics instead of a 4 x bar on the maximum (conftest.parity_8c_robust): high quantile
                # within 1.5 x and mean within 1.25 x of the CPU fp32 run's, tensor scale within 1e-5, the maximum
                # only as a 10 x tripwire
                parity_8c_robust("%s readout block %d (%s)" % (case, bi, "fused" if fused else "surface"), x, c, y,
                                 abs_bar=readout_abs_bar(bi))
        h = model.entity_embed(graph.ndata["id"])
        for i, layer in enumerate(model.layers):
            h = layer(graph, h, fused=False)
            assert rel_err_inf(h.cpu().numpy(), g["layer_out_%d" % i]) < TOL
    assert "att_w" not in graph.edata and "h_neighbor" not in graph.ndata  # local_var did not leak


@pytest.mark.parametrize("d_in,d_out", [(64, 64), (64, 32), (32, 16), (16, 16), (128, 64), (16, 128), (128, 128),
                                        (8, 8), (4, 4), (16, 8), (8, 16), (32, 4), (4, 32)])
def test_bi_interaction_vs_oracle(K, dev, d_in, d_out):
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(d_in + d_out)
    for n in (1, 15, 16, 17, 1000, 40001):
        P = rng.standard_normal((n, d_in)).astype(np.float32)
        P[n // 2] = 0  # an all-zero row must normalise to zeros (eps clamp), not NaN
        W2 = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
        ref = orc.bi_interaction(np.ones_like(P), P, W2)
        wide = torch.full((n, d_out + 24), 9.0, device=dev)
        h = ops.bi_interaction(tf(P, dev), tf(W2, dev), 0.01, norm_out=wide[:, 8:8 + d_out])
        assert rel_err_inf(h.cpu().numpy(), ref) < 1e-5
        got_n, ref_n = wide[:, 8:8 + d_out].cpu().numpy(), orc.l2_normalize(ref)
        if d_out >= 16:
            assert rel_err_inf(got_n, ref_n) < 1e-5
        else:
            # a row of 4 or 8 outputs can have a norm far below the tensor's scale; the normalisation then
            # divides the (asserted) 1e-5-of-scale error of the row by that norm
            row_norm = np.maximum(np.linalg.norm(ref, axis=1, keepdims=True), 1e-12)
            assert np.all(np.abs(got_n - ref_n) <= 1e-5 + 2e-5 * np.abs(ref).max() / row_norm)
        assert torch.all(wide[:, :8] == 9.0) and torch.all(wide[:, 8 + d_out:] == 9.0)
        assert np.all(np.isfinite(wide.cpu().numpy()))
    assert ops.bi_interaction_supported(128, 128) and ops.bi_interaction_supported(8, 8)
    assert not ops.bi_interaction_supported(8, 64) and not ops.bi_interaction_supported(12, 12)


@pytest.mark.parametrize("d_in,d_out", [(64, 64), (64, 32), (32, 16), (128, 128), (16, 128), (8, 8), (16, 8), (4, 32)])
def test_bi_interaction_mul_same_bits_as_the_spmm_epilogue(K, dev, d_in, d_out):
    """kgat_aggregator_f32 with the Bi form (h * h_N formed while the dense kernel loads its rows, ego block copied on
    the way) against the round 1-3 split - the product in the aggregation's epilogue (KGAT_SPMM_MUL_SELF + self_out), then
    kgat_bi_interaction_f32: the same bits in h_out, in the normalised slice and in the ego slice; nothing outside
    the slices touched; row counts around the 16-row tile."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(300 + d_in + d_out)
    for n in (1, 15, 16, 17, 4001):
        e = 12 * n
        src, dst = random_graph(n + d_in, n, e, hub=min(e // 3, 3000), isolated_tail=n // 10)
        X = tf(rng.standard_normal((n, d_in)).astype(np.float32), dev)
        W2 = tf((rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32), dev)
        indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
        w_csr = tf(rng.random(e).astype(np.float32), dev)
        can_copy = d_in % 4 == 0 and d_in >= 16
        ego_a = torch.full((n, d_in + 8), 5.0, device=dev)
        prod = ops.spmm(indptr, col, row_of, X, w_csr, mul_self=True,
                        self_out=ego_a[:, 4:4 + d_in] if can_copy else None)
        wide_a = torch.full((n, d_out + 24), 9.0, device=dev)
        h_a = ops.bi_interaction(prod, W2, 0.01, norm_out=wide_a[:, 8:8 + d_out])
        hn = ops.spmm(indptr, col, row_of, X, w_csr)
        ego_b = torch.full((n, d_in + 8), 5.0, device=dev)
        wide_b = torch.full((n, d_out + 24), 9.0, device=dev)
        h_b = ops.bi_interaction_mul(X, hn, W2, 0.01, norm_out=wide_b[:, 8:8 + d_out],
                                     self_out=ego_b[:, 4:4 + d_in] if can_copy else None)
        assert torch.equal(h_a, h_b) and torch.equal(wide_a, wide_b), (n, float((h_a - h_b).abs().max()))
        if can_copy:
            assert torch.equal(ego_a, ego_b) and torch.equal(ego_b[:, 4:4 + d_in], X)
        assert ops.bi_interaction_mul(X, hn, W2, 0.01, norm_out=wide_b[:, 8:8 + d_out], want_h=False) is None


DEFER_GRAPHS = [  # (n, e, hub, isolated tail)
    (5, 0, 0, 0), (1, 5, 0, 0), (17, 100, 0, 3), (300, 5000, 0, 40), (500, 20000, 9000, 100), (64, 7000, 7000, 0),
    (5000, 60000, 30000, 500), (40000, 2500000, 150000, 1000),
]


@pytest.mark.parametrize("d_in,d_out", [(64, 64), (64, 32), (32, 16), (128, 128), (16, 128), (128, 16)])
def test_bi_interaction_mul_deferred_same_bits_as_two_launch_aggregation(K, dev, d_in, d_out):
    """kgat_spmm_umule_sum_f32(KGAT_SPMM_DEFER_FINISH) + kgat_aggregator_deferred_f32 (Bi form) - the aggregation without
    its second launch, the rows its edge tiles cut (short chains of partials, hub rows spanning tens and hundreds
    of tiles) and the rows without in-edges formed by the dense kernel - against the two-launch aggregation +
    kgat_aggregator_f32: the same bits in h_out, the normalised slice and the ego slice.  The aggregation's
    output is pre-filled with NaN, so a deferred row taken from it would show; all three run lengths (tile sizes)."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(900 + d_in + d_out)
    seen_tiles = set()
    for gi, (n, e, hub, iso) in enumerate(DEFER_GRAPHS):
        src, dst = random_graph(50 + gi, n, e, hub=hub, isolated_tail=iso)
        X = tf(rng.standard_normal((n, d_in)).astype(np.float32), dev)
        W2 = tf((rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32), dev)
        indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
        w_csr = tf(rng.random(e).astype(np.float32), dev)
        hn = ops.spmm(indptr, col, row_of, X, w_csr)
        ego_a = torch.full((n, d_in + 8), 5.0, device=dev)
        wide_a = torch.full((n, d_out + 24), 9.0, device=dev)
        h_a = ops.bi_interaction_mul(X, hn, W2, 0.01, norm_out=wide_a[:, 8:8 + d_out], self_out=ego_a[:, 4:4 + d_in])
        hn_d = torch.full((n, d_in), float("nan"), device=dev)
        hn_d, left = ops.spmm(indptr, col, row_of, X, w_csr, out=hn_d, defer_finish=True)
        seen_tiles.add(left.tile_edges)
        ego_b = torch.full((n, d_in + 8), 5.0, device=dev)
        wide_b = torch.full((n, d_out + 24), 9.0, device=dev)
        h_b = ops.bi_interaction_mul(X, hn_d, W2, 0.01, norm_out=wide_b[:, 8:8 + d_out], self_out=ego_b[:, 4:4 + d_in],
                                     deferred=left)
        assert torch.equal(h_a, h_b), (n, e, float((h_a - h_b).abs().max()))
        assert torch.equal(wide_a, wide_b) and torch.equal(ego_a, ego_b)
        # the rows the aggregation did write are the two-launch rows; the others were left alone
        written = ~torch.isnan(hn_d).any(dim=1)
        assert torch.equal(hn_d[written], hn[written])
        if e > 1000:
            assert int((~written).sum()) > 0
    assert len(seen_tiles) >= 2, seen_tiles


def test_bi_interaction_mul_deferred_on_a_row_range(K, dev):
    """The shard form: rows [row0, row0 + n_rows) of a larger CSR (positions [e0, e1) - tiles counted from e0), the
    deferred pair against the two-launch pair on the same range."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(77)
    n, e, d_in, d_out = 3000, 90000, 64, 32
    src, dst = random_graph(5, n, e, hub=9000, isolated_tail=50)
    X = tf(rng.standard_normal((n, d_in)).astype(np.float32), dev)
    W2 = tf((rng.standard_normal((d_out, d_in)) / 8).astype(np.float32), dev)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    w_csr = tf(rng.random(e).astype(np.float32), dev)
    ip = indptr.cpu().numpy()
    for row0, n_rows in ((0, 1000), (1, 7), (1000, 2000), (2900, 100)):
        e0, e1 = int(ip[row0]), int(ip[row0 + n_rows])
        Xr = X[row0:row0 + n_rows].contiguous()
        hn = ops.spmm(indptr, col, row_of, X, w_csr, rows=(row0, n_rows), e_range=(e0, e1))
        h_a = ops.bi_interaction_mul(Xr, hn, W2, 0.01)
        hn_d = torch.full((n_rows, d_in), float("nan"), device=dev)
        hn_d, left = ops.spmm(indptr, col, row_of, X, w_csr, rows=(row0, n_rows), e_range=(e0, e1), out=hn_d,
                              defer_finish=True)
        h_b = ops.bi_interaction_mul(Xr, hn_d, W2, 0.01, deferred=left)
        assert torch.equal(h_a, h_b), (row0, n_rows, float((h_a - h_b).abs().max()))


def test_deferred_finish_refuses_what_it_cannot_do(K, dev):
    from dgl_kgat_amd import ops
    n, e = 50, 300
    src, dst = random_graph(3, n, e)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    w = torch.rand(e, device=dev)
    with pytest.raises(Exception):   # a width outside the merge kernel's
        ops.spmm(indptr, col, row_of, torch.randn(n, 8, device=dev), w, defer_finish=True)
    with pytest.raises(Exception):   # edge-id-ordered weights
        ops.spmm(indptr, col, row_of, torch.randn(n, 64, device=dev), w, eid=eid, defer_finish=True)
    with pytest.raises(Exception):   # the h * h_N epilogue
        ops.spmm(indptr, col, row_of, torch.randn(n, 64, device=dev), w, mul_self=True, defer_finish=True)
    with pytest.raises(Exception):   # the rows algorithm has no tiles
        ops.spmm(indptr, col, row_of, torch.randn(n, 64, device=dev), w, algo="rows", defer_finish=True)
    X = torch.randn(n, 64, device=dev)
    hn, left = ops.spmm(indptr, col, row_of, X, w, defer_finish=True)
    with pytest.raises(Exception):   # another aggregation's rows
        ops.bi_interaction_mul(torch.randn(n, 32, device=dev), torch.randn(n, 32, device=dev),
                               torch.randn(16, 32, device=dev), deferred=left)
    assert ops.bi_interaction_deferral_supported(64, 32) and not ops.bi_interaction_deferral_supported(8, 8)


def test_gnn_deferred_finish_same_bits(K, dev, monkeypatch):
    """Model.gnn's default (the aggregation's second launch left to the dense kernel) against
    KGAT_GNN_DEFER_FINISH=0 (two launches): the same bits in the whole readout."""
    from dgl_kgat_amd import synth
    n, trip, R = synth.amazon_book_ckg(scale=0.05)
    torch.manual_seed(3)
    model = K.KGATPropagation(n, R, 64, 64, 3, 64, dropout=0.0).to(dev)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
        from dgl_kgat_amd import options
        with options.override(gnn_defer_finish=False):
            two = model.gnn(g)
        with options.override(gnn_defer_finish=True):
            one = model.gnn(g)
    assert torch.equal(one, two), float((one - two).abs().max())


@pytest.mark.parametrize("d_in,d_out", [(64, 64), (64, 32), (32, 16), (128, 128), (16, 128), (128, 16)])
def test_bi_interaction_bwd_input_vs_fp64(K, dev, d_in, d_out):
    """kgat_aggregator_bwd_input_f32 with the Bi form - grad_P = grad_z W2 on the fp32 MFMA, multiplied by H and by HN
    on the way - against the fp64 product: relative to sum |grad_z| |W2| per element (the products' own rounding), row counts around
    the 16-row tile and the wavefronts' tile ranges; every element of both outputs written, nothing else."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(40 + d_in + d_out)
    assert ops.bi_interaction_bwd_input_supported(d_in, d_out) and not ops.bi_interaction_bwd_input_supported(8, 64)
    for n in (1, 15, 16, 17, 4001, 70000):
        gz = rng.standard_normal((n, d_out)).astype(np.float32)
        W2 = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
        H = rng.standard_normal((n, d_in)).astype(np.float32)
        HN = rng.standard_normal((n, d_in)).astype(np.float32)
        t, gb = ops.bi_interaction_bwd_input(tf(gz, dev), tf(W2, dev), tf(H, dev), tf(HN, dev))
        gp = gz.astype(np.float64) @ W2.astype(np.float64)
        bound = np.abs(gz).astype(np.float64) @ np.abs(W2).astype(np.float64)
        for got, factor in ((t, H), (gb, HN)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - gp * factor)
            assert np.all(err <= 4e-7 * bound * np.abs(factor) + 1e-30), (n, float((err / (bound * np.abs(factor) + 1e-30)).max()))
    with pytest.raises(Exception):
        ops.bi_interaction_bwd_input(torch.randn(5, 8, device=dev), torch.randn(8, 64, device=dev),
                                     torch.randn(5, 64, device=dev), torch.randn(5, 64, device=dev))


@pytest.mark.parametrize("d_in,d_out", [(64, 64), (64, 32), (32, 16), (128, 128), (16, 128), (128, 16), (16, 16)])
def test_bi_interaction_bwd_weight_vs_fp64(K, dev, d_in, d_out):
    """kgat_aggregator_bwd_weight_f32 with the Bi form - grad_W2 = grad_z^T (H * HN), reduced over all rows through
    per-workgroup partials - against the fp64 product, relative to sum |grad_z| |H HN| per element; row counts around the 64-row
    slab, one slab per workgroup and many; twice the same bits."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(140 + d_in + d_out)
    for n in (1, 63, 64, 65, 4001, 159251):
        gz = rng.standard_normal((n, d_out)).astype(np.float32)
        H = rng.standard_normal((n, d_in)).astype(np.float32)
        HN = rng.standard_normal((n, d_in)).astype(np.float32)
        gw = ops.bi_interaction_bwd_weight(tf(gz, dev), tf(H, dev), tf(HN, dev))
        assert tuple(gw.shape) == (d_out, d_in)
        P = H.astype(np.float64) * HN.astype(np.float64)
        ref = gz.astype(np.float64).T @ P
        bound = np.abs(gz).astype(np.float64).T @ np.abs(P)
        err = np.abs(gw.cpu().numpy().astype(np.float64) - ref)
        # (fp32 products of fp32 values, fp32 accumulation over n terms in blocks: a few ulp of the absolute sum)
        assert np.all(err <= 2e-6 * bound + 1e-30), (n, float((err / (bound + 1e-30)).max()))
        assert torch.equal(gw, ops.bi_interaction_bwd_weight(tf(gz, dev), tf(H, dev), tf(HN, dev)))


def test_autograd_matches_oracle(K, dev):
    from dgl_kgat_amd import synth
    from dgl_kgat_amd.autograd import edge_softmax, u_mul_e_sum
    n, trip, R = synth.collaborative_kg(30, 40, 30, 3, 900, 400, seed=3)
    src, dst = trip[:, 2], trip[:, 0]
    g = synth.build_graph(n, trip, dev)
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, 32)).astype(np.float32)
    s = rng.standard_normal(len(trip)).astype(np.float32)
    go = rng.standard_normal((n, 32)).astype(np.float32)
    Xd = tf(X, dev).requires_grad_(True)
    sd = tf(s, dev).reshape(-1, 1).requires_grad_(True)
    a = edge_softmax(g, sd)
    out = u_mul_e_sum(g, Xd, a)
    out.backward(tf(go, dev))
    a_ref = orc.edge_softmax(n, dst, s)
    assert rel_err(out.detach().cpu().numpy(), orc.spmm_u_mul_e_sum(n, src, dst, X, a_ref)) < TOL
    assert rel_err(Xd.grad.cpu().numpy(), orc.spmm_backward_x(n, src, dst, go, a_ref)) < TOL
    gw = orc.sddmm_dot(src, dst, X, go)
    gs = orc.edge_softmax_backward(n, dst, a_ref, gw).reshape(-1)
    assert rel_err(sd.grad.cpu().numpy().reshape(-1), gs) < 5e-4


def test_training_step_runs(K, dev):
    """gnn -> BPR loss -> backward -> Adam, the CF step of kgat.py:146-168, over the kernels."""
    from dgl_kgat_amd import synth
    n, trip, R = synth.collaborative_kg(30, 40, 30, 3, 900, 400, seed=5)
    g = synth.build_graph(n, trip, dev)
    torch.manual_seed(0)
    model = K.KGATPropagation(n, R, 16, 16, 2, 16, dropout=0.0).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
    u = torch.randint(0, 30, (64,), device=dev)
    p = torch.randint(30, 70, (64,), device=dev)
    q = torch.randint(30, 70, (64,), device=dev)
    losses = []
    for _ in range(5):
        loss = model.get_loss(model.gnn(g), u, p, q)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_destination_shards_reassemble_to_unsharded(K, dev):
    """Multi-GPU layout on one GPU: the shards of a 3-way destination partition, run one after
    the other, give attention weights and layer outputs whose zero-padded sum (what the RCCL
    all-reduce computes) equals the unsharded result."""
    from dgl_kgat_amd import partition, synth
    n, trip, R = synth.collaborative_kg(60, 80, 60, 4, 3000, 1200, seed=9)
    torch.manual_seed(3)
    model = K.KGATPropagation(n, R, 64, 64, 2, 64, dropout=0.0).to(dev)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        a_full = model.compute_attention(g)
        g.edata["w"] = a_full
        h_full = model.layers[0](g, model.entity_embed.weight, fused=True)
        world = 3
        acc = torch.zeros_like(h_full)
        a_parts = torch.zeros_like(a_full)
        for r in range(world):
            sg, keep = partition.shard_graph(g, r, world)
            assert sg.partition.world == world and sg.number_of_edges() == len(keep)
            a_loc = model.compute_attention(sg)   # no exchange needed: all in-edges are local
            a_parts[torch.as_tensor(keep, device=dev)] = a_loc
            sg.edata["w"] = a_loc
            out_loc = sg.partition.propagate_local(sg, model.entity_embed.weight, model.layers[0].res_fc_2.weight)
            acc += sg.partition.pad(out_loc, out_loc.shape[1])
        assert rel_err_inf(a_parts.cpu().numpy(), a_full.cpu().numpy()) < 1e-6
        assert rel_err_inf(acc.cpu().numpy(), h_full.cpu().numpy()) < 1e-6
        # world = 1: the sharded code paths end to end (exchange without a process group)
        sg, _ = partition.shard_graph(g, 0, 1)
        sg.edata["w"] = model.compute_attention(sg)
        ref = model.gnn(g).cpu().numpy()
        assert rel_err_inf(model.gnn(sg, fused=True).cpu().numpy(), ref) < 1e-6   # bi-interaction kernel + row normalise
        assert rel_err_inf(model.gnn(sg, fused=False).cpu().numpy(), ref) < 1e-6  # torch dense part
        # row normalisation kernel alone, into a column slice, zero rows stay zero
        from dgl_kgat_amd import ops
        x = torch.randn(1000, 48, device=dev)
        x[7] = 0
        wide = torch.full((1000, 60), 3.0, device=dev)
        ops.l2_normalize_rows(x, wide[:, 4:52])
        assert torch.allclose(wide[:, 4:52], torch.nn.functional.normalize(x, dim=1), atol=1e-6)
        assert torch.all(wide[:, :4] == 3.0) and torch.all(wide[:, 52:] == 3.0) and torch.all(wide[7, 4:52] == 0)


def test_att_product_flag_is_validated(K, dev):
    """An unknown flag bit of kgat_att_score_fused_f32 / kgat_att_score_folded_f32 is a bad
    argument (KGAT_E_BADARG, message through kgat_last_error), not silently ignored."""
    from dgl_kgat_amd import _lib, ops
    rng = np.random.default_rng(5)
    n, e, R, d = 200, 3000, 3, 64
    src, dst = rng.integers(0, n, e).astype(np.int32), rng.integers(0, n, e).astype(np.int32)
    et = rng.integers(0, R, e).astype(np.int32)
    rel_ptr, perm, src_g, dst_g, pos_g = _grouped_by_relation_and_destination(ops, n, src, dst, et, R, dev)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    tiles, rel_tptr, part_tptr = ops.fold_tiles(rel_ptr, gid, gptr, n_groups)
    ent, W, rel = torch.randn(n, d, device=dev), torch.randn(R, d, d, device=dev) * 0.1, torch.randn(R, d, device=dev)
    out = torch.empty(e, device=dev)
    lib = _lib.load()
    p = lambda t: t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    for flags, want in ((0, 0), (1, 0), (2, -1), (3, -1), (4, -1), (-1, -1)):   # (2: no longer a flag)
        rec = ops.att_pack_records(rel_ptr, gptr, gid, src_g)
        rc = lib.kgat_att_score_fused_f32(n, e, d, d, R, p(rel_ptr), p(perm), p(rec), p(pos_g), p(gptr),
                                          p(g_node), p(tiles), p(rel_tptr), p(part_tptr), part_tptr.numel() - 1, p(ent),
                                          p(W), p(rel), p(out), None, None, flags, st)
        assert rc == want, (flags, rc, lib.kgat_last_error())
        if want:
            assert b"unknown flag" in lib.kgat_last_error()
    v_tab = torch.empty(max(n_groups, 1), d, device=dev)
    for flags, want in ((0, 0), (1, 0), (4, -1)):
        rc = lib.kgat_att_score_folded_f32(n, e, d, d, R, p(rel_ptr), p(perm), p(src_g), p(pos_g), p(gid), p(gptr),
                                           p(g_node), n_groups, p(ent), p(W), p(rel), p(v_tab), p(out), None, flags, st)
        assert rc == want, (flags, rc, lib.kgat_last_error())
    torch.cuda.synchronize()


def test_f32_products_switch_on_the_surface(K, dev, monkeypatch):
    """KGAT_ATT_F32_PRODUCTS=1 routes compute_attention's kernels to the fp32-MFMA products: same
    weights to rounding, through the same entry points (the flag of the C ABI)."""
    from dgl_kgat_amd import options, synth
    n, trip, R = synth.collaborative_kg(300, 400, 300, 5, 20000, 9000, seed=3)
    torch.manual_seed(0)
    m = K.KGATPropagation(n, R, 64, 64, 1, 64, dropout=0.0).to(dev)
    outs = {}
    try:
        for val in ("", "1"):
            monkeypatch.setenv("KGAT_ATT_F32_PRODUCTS", val)
            options.reload()                # (the environment is read once, at import; a launcher re-reads it like this)
            g = synth.build_graph(n, trip, dev)
            with torch.no_grad():
                outs[val] = torch.as_tensor(m.compute_attention(g)).clone()
    finally:
        monkeypatch.delenv("KGAT_ATT_F32_PRODUCTS")
        options.reload()
    torch.cuda.synchronize()
    assert float((outs[""] - outs["1"]).abs().max()) < 2e-6
    assert not torch.equal(outs[""], outs["1"])  # two different summations


@pytest.mark.parametrize("d", [64, 128])
def test_att_nonfinite_inputs_stay_contained(K, dev, d):
    """An Inf / NaN embedding entry (a diverged model) poisons exactly the softmax rows that hold an
    edge of that node - the bf16-piece cut turns Inf into NaN, nothing else - and every other
    weight keeps its bits; entries near FLT_MAX and subnormals stay finite."""
    from dgl_kgat_amd import synth
    n, trip, R = synth.collaborative_kg(300, 400, 300, 5, 20000, 9000, seed=3)
    torch.manual_seed(0)
    m = K.KGATPropagation(n, R, d, d, 1, d, dropout=0.0).to(dev)
    g = synth.build_graph(n, trip, dev)
    dst = torch.as_tensor(trip[:, 0].astype(np.int64)).to(dev)
    touched = (torch.as_tensor(trip[:, 0] == 7) | torch.as_tensor(trip[:, 2] == 7)).to(dev)
    rows = torch.zeros(n, dtype=torch.bool, device=dev)
    rows[dst[touched]] = True
    clean = ~rows[dst]
    with torch.no_grad():
        a0 = torch.as_tensor(m.compute_attention(g)).clone().reshape(-1)
        assert torch.isfinite(a0).all()
        for val, poisons in ((float("inf"), True), (float("nan"), True), (1e38, False), (1e-45, False)):
            w = m.entity_embed.weight
            old = w[7].clone()
            w[7, 3] = val
            a = torch.as_tensor(m.compute_attention(g)).clone().reshape(-1)
            w[7] = old
            bad = ~torch.isfinite(a)
            assert bool(bad.any()) == poisons, val
            assert not bool((bad & clean).any()), val
            assert torch.equal(a[clean], a0[clean]), val


def test_readout_concat(K, dev):
    """kgat_readout_concat_f32: [h0 | normalize(h1) | ...] (models.py:159-168) from separate blocks."""
    from dgl_kgat_amd import ops
    torch.manual_seed(9)
    for n in (1, 15, 16, 17, 4099):
        blocks = [torch.randn(n, w, device=dev) for w in (64, 128, 32, 16, 4)]
        blocks[2][n // 2] = 0  # an all-zero row normalises to zeros (eps clamp)
        flags = [False, True, True, True, False]
        out = ops.readout_concat(blocks, flags)
        ref = torch.cat([torch.nn.functional.normalize(b, p=2, dim=1) if f else b for b, f in zip(blocks, flags)], 1)
        assert out.shape == ref.shape and torch.allclose(out, ref, atol=1e-6) and torch.isfinite(out).all()
        assert torch.equal(out[:, :64], blocks[0]) and torch.equal(out[:, -4:], blocks[4])
    with pytest.raises(Exception):
        ops.readout_concat([torch.randn(4, 6, device=dev)], [True])  # width not a multiple of 4


def test_full_size_properties(K, dev):
    """amazon-book-sized CKG (BASELINE configs[2]): properties that need no oracle run -
    partition of unity of the attention, merge == rows kernel, linearity, reproducibility -
    plus an oracle spot check on a sample of destination rows."""
    from dgl_kgat_amd import ops, synth
    n, trip, R = synth.amazon_book_ckg()
    src, dst = trip[:, 2], trip[:, 0]
    e = len(trip)
    indptr, col, eid, row_of = ops.csr_from_coo(n, t32(src, dev), t32(dst, dev))
    ip = indptr.cpu().numpy().astype(np.int64)
    assert ip[-1] == e and np.array_equal(np.diff(ip), np.bincount(dst, minlength=n))
    eid_h = eid.cpu().numpy()
    assert np.array_equal(np.sort(eid_h), np.arange(e)) and np.array_equal(dst[eid_h], row_of.cpu().numpy())
    gen = torch.Generator(device="cpu").manual_seed(1)
    s = torch.randn(e, generator=gen).to(dev) * 3
    a, a_csr = ops.edge_softmax(indptr, row_of, eid, s, want_out=True, want_csr=True)
    ones = torch.ones((n, 64), device=dev)
    unity = ops.spmm(indptr, col, row_of, ones, a_csr, algo="merge")
    nonempty = torch.as_tensor(np.diff(ip) > 0, device=dev)
    assert torch.all(unity[~nonempty] == 0)
    assert float((unity[nonempty] - 1).abs().max()) < 1e-4
    X = torch.randn((n, 64), generator=gen).to(dev)
    Y = torch.randn((n, 64), generator=gen).to(dev)
    m = ops.spmm(indptr, col, row_of, X, a_csr, algo="merge")
    r = ops.spmm(indptr, col, row_of, X, a_csr, algo="rows")
    scale = float(r.abs().max())
    assert float((m - r).abs().max()) < 1e-5 * scale
    assert torch.equal(m, ops.spmm(indptr, col, row_of, X, a_csr, algo="merge"))
    lin = ops.spmm(indptr, col, row_of, X + Y, a_csr) - m - ops.spmm(indptr, col, row_of, Y, a_csr)
    assert float(lin.abs().max()) < 1e-4 * scale
    # oracle spot check: 200 rows incl. the heaviest hub
    rows = np.unique(np.concatenate([np.random.default_rng(2).integers(0, n, 199), [int(np.argmax(np.diff(ip)))]]))
    Xh, ah, mh = X.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64), m.cpu().numpy()
    for v in rows:
        seg = eid_h[ip[v]:ip[v + 1]]
        ref = (ah[seg, None] * Xh[src[seg]]).sum(0) if len(seg) else np.zeros(64)
        assert np.max(np.abs(mh[v] - ref)) < 1e-4 * max(np.abs(ref).max(), 1e-3 * scale)


def test_full_size_attention_forms(K, dev):
    """amazon-book-sized CKG: the attention forms against each other (split == one-kernel bit for
    bit; fused, folded and that family within fp32 rounding of each other), an oracle spot check
    on a sample of edges, and the end-to-end attention (all forms) summing to one per destination."""
    from dgl_kgat_amd import ops, synth
    n, trip, R = synth.amazon_book_ckg()
    e, d = len(trip), 64
    g = synth.build_graph(n, trip, dev)
    torch.manual_seed(3)
    m = K.KGATPropagation(n, R, d, d, 3, d, dropout=0.0).to(dev)
    ent, W, rel = m.entity_embed.weight.detach(), m.W_R.detach(), m.relation_embed.weight.detach()
    st = g._st
    groups = st.rel_groups(g.edata["type"], R)
    args = (n, groups.rel_ptr, groups.perm, groups.src_g, groups.pos_g, groups.gid, groups.gptr, groups.g_node)
    tiles, tptr, parts = ops.fold_tiles(groups.rel_ptr, groups.gid, groups.gptr, groups.n_groups)
    assert int(tptr[-1]) <= tiles.shape[0] and int(tptr[-1]) >= (groups.n_groups + 15) // 16
    assert int(parts[0]) == 0 and int(parts[-1]) == int(tptr[-1]) and bool((parts[1:] >= parts[:-1]).all())
    fused, _ = ops.att_score_fused(*args, tiles, tptr, ent, W, rel, want_csr=False, part_tptr=parts)
    assert torch.equal(fused, ops.att_score_fused(*args, tiles, tptr, ent, W, rel, want_csr=False)[0])
    folded, _ = ops.att_score_split(*args, groups.n_groups, ent, W, rel, want_csr=False, folded=True)
    split, _ = ops.att_score_split(*args, groups.n_groups, ent, W, rel, want_csr=False)
    one, _ = ops.att_score(n, groups.rel_ptr, groups.perm, groups.src_g, groups.dst_g, ent, W, rel)
    assert torch.equal(split, one)
    scale = float(one.abs().max())
    assert float((fused - folded).abs().max()) < 2e-6 * scale
    assert float((fused - one).abs().max()) < 1e-5 * scale
    idx = np.random.default_rng(4).choice(e, 5000, replace=False)
    ref = orc.att_score(ent.cpu().numpy(), W.cpu().numpy(), rel.cpu().numpy(), trip[idx, 2], trip[idx, 0], trip[idx, 1])
    assert np.abs(fused.cpu().numpy()[idx] - ref).max() < 1e-5 * scale
    deg = torch.as_tensor(np.bincount(trip[:, 0], minlength=n) > 0, device=dev)
    for form in ("fused", "folded", "split", "one"):
        with torch.no_grad():
            a = g.kgat_attention(ent, W, rel, algo=form)
        sums = torch.zeros(n, device=dev).index_add_(0, torch.as_tensor(trip[:, 0].astype(np.int64), device=dev), a.reshape(-1))
        assert float((sums[deg] - 1).abs().max()) < 1e-4 and torch.all(sums[~deg] == 0), form


def test_attention_forms_degenerate_graphs(K, dev):
    """Every attention form end to end (logits + softmax + propagation) on graphs where a structure
    is empty or trivial: no scored relation at all, a single edge, no edges, one hub group."""
    from dgl_kgat_amd import synth
    rng = np.random.default_rng(0)
    cases = [("all unscored", 50, np.stack([rng.integers(0, 50, 300), np.full(300, 7), rng.integers(0, 50, 300)], 1)),
             ("one edge", 5, np.array([[1, 0, 2]])),
             ("no edges", 5, np.zeros((0, 3), np.int64)),
             ("one hub group", 40, np.stack([np.full(5000, 3), np.zeros(5000, np.int64), rng.integers(0, 40, 5000)], 1))]
    for name, n, trip in cases:
        trip = trip.astype(np.int32)
        g = synth.build_graph(n, trip, dev)
        torch.manual_seed(0)
        m = K.KGATPropagation(n, 3, 16, 16, 2, 16, dropout=0.0).to(dev)
        ref = None
        for form in ("one", "split", "folded", "fused", "auto"):
            with torch.no_grad():
                a = g.kgat_attention(m.entity_embed.weight, m.W_R, m.relation_embed.weight, algo=form)
                g.edata["w"] = a
                out = m.gnn(g)
            assert a.shape == (len(trip), 1) and torch.isfinite(out).all(), (name, form)
            sums = torch.zeros(n, device=dev)
            if len(trip):
                sums.index_add_(0, torch.as_tensor(trip[:, 0].astype(np.int64), device=dev), a.reshape(-1))
            assert bool((((sums - 1).abs() < 1e-5) | (sums == 0)).all()), (name, form)
            if ref is None:
                ref = a
            assert float((a - ref).abs().max()) < 1e-6 if len(trip) else True, (name, form)


def test_training_harness_end_to_end(K, dev):
    """examples/train_kgat.py: reference-format files -> CKGDataset -> KG phase / attention refresh /
    CF phase / recall@20 + ndcg@20, the epoch structure of kgat.py:114-196, on the kernels."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_kgat.py"), "--synthetic", "0.01",
                          "--epochs", "2", "--max_iters", "8", "--lr", "0.01"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if "loss" in l or "recall" in l]
    kge = [float(l.split("loss")[1]) for l in lines if "KGE" in l]
    assert len(kge) == 2 and kge[1] < kge[0] and all(np.isfinite(kge))
    rec = [float(l.split("recall@20")[1].split()[0]) for l in lines if "recall@20" in l]
    assert len(rec) == 4 and all(0.0 <= r <= 1.0 for r in rec)


@pytest.mark.parametrize("d,k,n,R,B", [(64, 64, 3000, 9, 2048), (16, 32, 500, 3, 100), (32, 16, 500, 40, 2730),
                                        (128, 128, 800, 5, 513), (8, 8, 60, 2, 1),
                                        (16, 16, 3_000_000, 4, 2000)])   # entity ids beyond 2^19: the 64-bit sort keys
def test_transr_fused_loss_and_gradients(K, dev, d, k, n, R, B):
    """Fused TransR step (kgat_transr_loss_grad_f32) against the torch restatement of reference
    models.py:114-133 (itself pinned to the reference's own output in the CPU suite): loss and the
    gradients with respect to the entity table, W_R and the relation table; repeated heads
    (duplicate rows in the dense gradient), an unused relation, bitwise reproducibility."""
    torch.manual_seed(5)
    m = K.KGATPropagation(n, R, d, k, 1, d, dropout=0.0).to(dev)
    with torch.no_grad():
        m.relation_embed.weight.mul_(3.0)
    g = torch.Generator().manual_seed(6)
    h = torch.randint(0, max(n // 20, 1), (B,), generator=g).to(dev)      # few distinct heads: many repeats
    if n > (1 << 19):
        h = (h + (n - n // 20 - 1)).clamp_(max=n - 1)                     # ... among the LARGEST ids
    r = torch.randint(0, R, (B,), generator=g)
    if R > 2:
        r[r == 1] = 0                                                     # relation 1 unused
    r = r.to(dev)
    pt, nt = torch.randint(0, n, (B,), generator=g).to(dev), torch.randint(0, n, (B,), generator=g).to(dev)
    params = [m.entity_embed.weight, m.W_R, m.relation_embed.weight]
    ref = m.transR(h, r, pt, nt, fused=False)
    ref_g = torch.autograd.grad(ref, params)
    out = m.transR(h, r, pt, nt, fused=True)
    out_g = torch.autograd.grad(out, params)
    assert abs(float(out.detach()) - float(ref.detach())) < 2e-6 * max(abs(float(ref.detach())), 1.0)
    for a, b_, name in zip(out_g, ref_g, ("entity_embed", "W_R", "relation_embed")):
        assert a.shape == b_.shape
        assert rel_err_inf(a.cpu().numpy(), b_.cpu().numpy()) < 2e-5, name
    touched = torch.zeros(n, dtype=torch.bool, device=dev)
    touched[torch.cat([h, pt, nt])] = True
    assert torch.all(out_g[0][~touched] == 0)
    if R > 2:
        assert torch.all(out_g[1][1] == 0) and torch.all(out_g[2][1] == 0)
    # default dispatch takes the fused path here; upstream gradient scaling; bit-for-bit repeatable
    again = torch.autograd.grad(m.transR(h, r, pt, nt) * 2.5, params)
    for a, b_ in zip(again, out_g):
        assert torch.equal(a, b_ * 2.5)
    with torch.no_grad():
        assert float(m.transR(h, r, pt, nt)) == float(out)


def test_transr_fused_refuses_what_it_cannot_do(K, dev):
    from dgl_kgat_amd import ops
    assert not ops.transr_supported(1000, 64, 64, 5, 4096) and ops.transr_supported(1 << 20, 64, 64, 5, 16)
    assert ops.transr_supported(10_000_000, 64, 64, 64, 2048)   # BASELINE configs[4]'s node count (round 4: 64-bit sort keys)
    m = K.KGATPropagation(100, 3, 16, 16, 1, 16, dropout=0.0).to(dev)
    idx = torch.zeros(4096, dtype=torch.long, device=dev)
    with pytest.raises(Exception):
        m.transR(idx, idx, idx, idx, fused=True)
    assert torch.isfinite(m.transR(idx, idx, idx, idx))  # default dispatch: torch restatement on the device


def _train_graph_and_model(K, dev, d, hidden, p, seed=11):
    from dgl_kgat_amd import synth
    n, e, R = 900, 30000, 5
    src, dst = random_graph(seed, n, e, hub=2500, isolated_tail=15)
    rng = np.random.default_rng(seed + 1)
    trip = np.stack([dst, rng.integers(0, R, e).astype(np.int32), src], 1).astype(np.int32)
    g = synth.build_graph(n, trip, dev)
    torch.manual_seed(seed)
    m = K.KGATPropagation(n, R, d, d, 3, hidden, dropout=p).to(dev)
    with torch.no_grad():
        g.edata["w"] = m.compute_attention(g)
    return g, m, n


@pytest.mark.parametrize("d,hidden", [(64, 64), (32, 64), (16, 64), (128, 128)])
def test_gnn_train_fused_matches_unfused_autograd(K, dev, d, hidden):
    """The fused training stack (one autograd unit: kgat_aggregator_train_f32 /
    _bwd_pre_f32 / kgat_mul2_f32 + the SpMMs) against the operator-by-operator autograd path
    over the drop-in surface, dropout off: readout, gradient of the embeddings and of every W2."""
    g, m, n = _train_graph_and_model(K, dev, d, hidden, 0.0)
    params = [m.entity_embed.weight] + [l.res_fc_2.weight for l in m.layers]
    probe = torch.randn(n, sum([d] + [l.res_fc_2.out_features for l in m.layers]),
                        generator=torch.Generator().manual_seed(3)).to(dev)
    ref = m.gnn(g, fused=False)
    ref_g = torch.autograd.grad((ref * probe).sum(), params)
    out = m.gnn(g)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_GNNTrain")
    out_g = torch.autograd.grad((out * probe).sum(), params)
    assert blocks_rel_err_inf(out.detach().cpu().numpy(), ref.detach().cpu().numpy(),
                              [d] + [l.res_fc_2.out_features for l in m.layers]) < 1e-5
    for a, b_, name in zip(out_g, ref_g, ["entity_embed"] + ["W2_%d" % i for i in range(3)]):
        assert rel_err_inf(a.cpu().numpy(), b_.cpu().numpy()) < 2e-5, name


def test_gnn_train_fused_dropout(K, dev):
    """Dropout on: the kernel's hash mask restated in numpy (ops.dropout_keep_mask) drives a torch
    autograd restatement of the same stack; outputs and gradients must agree, the drop rate must be
    p, and a torch seed must reproduce the run."""
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.autograd import gnn_train, u_mul_e_sum
    d, hidden, p, seed = 32, 64, 0.3, 123456789012
    g, m, n = _train_graph_and_model(K, dev, d, hidden, p)
    weights = [l.res_fc_2.weight for l in m.layers]
    h0 = m.entity_embed.weight
    out = gnn_train(g, h0, weights, 0.01, p, seed)
    h, cache, kept = h0, [h0], []
    for li, w in enumerate(weights):
        mask = torch.as_tensor(ops.dropout_keep_mask(seed + li, n, w.shape[0], p)).to(dev)
        kept.append(float(mask.float().mean()))
        hn = u_mul_e_sum(g, h, g.edata["w"])
        h = torch.nn.functional.leaky_relu(torch.nn.functional.linear(h * hn, w)) * mask / (1 - p)
        cache.append(torch.nn.functional.normalize(h, p=2, dim=1))
    ref = torch.cat(cache, 1)
    assert all(abs(k - (1 - p)) < 0.02 for k in kept)
    widths = [d] + [w.shape[0] for w in weights]
    assert blocks_rel_err_inf(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), widths) < 1e-5
    probe = torch.randn(n, sum(widths), generator=torch.Generator().manual_seed(4)).to(dev)
    params = [h0] + weights
    out_g = torch.autograd.grad((out * probe).sum(), params)
    ref_g = torch.autograd.grad((ref * probe).sum(), params)
    for a, b_ in zip(out_g, ref_g):
        assert rel_err_inf(a.cpu().numpy(), b_.cpu().numpy()) < 2e-5
    # through the module: training mode draws the seed from torch's generator
    m.train()
    torch.manual_seed(77)
    a1 = m.gnn(g).detach()
    torch.manual_seed(77)
    a2 = m.gnn(g).detach()
    a3 = m.gnn(g).detach()
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)


@pytest.mark.parametrize("n,d,wide", [(1000, 64, 176), (77, 16, 48), (4099, 128, 304), (5, 8, 8)])
def test_add3_rows_and_training_ego_block(K, dev, n, d, wide):
    """Round 6's two CF-step helpers: kgat_add3_rows_f32 = (a + b) + c with `a` a column slice of a wider matrix, equal
    bit for bit to the two torch adds it replaces; and the ego block written by the TRAINING dense kernel (self_out of
    kgat_aggregator_train_f32) = the layer's input rows, bit for bit, with the layer's other outputs unchanged."""
    from dgl_kgat_amd import ops
    gen = torch.Generator().manual_seed(n + d)
    big = torch.randn(n, wide, generator=gen).to(dev)
    b, c = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, d, generator=gen).to(dev)
    got = ops.add3_rows(big[:, :d], b, c)
    ref = big[:, :d] + b
    ref += c
    assert torch.equal(got, ref)
    if d in (16, 64, 128):
        H, HN = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, d, generator=gen).to(dev)
        W2 = (torch.randn(d // 2 if d > 16 else 16, d, generator=gen) * 0.1).to(dev)
        out_a = torch.full((n, wide), float("nan"), device=dev)
        out_b = torch.full((n, wide), float("nan"), device=dev)
        do = W2.shape[0]
        h_a = ops.bi_interaction_train(H, HN, W2, 0.01, 0.2, 77, norm_out=out_a[:, d:d + do], self_out=out_a[:, :d])
        h_b = ops.bi_interaction_train(H, HN, W2, 0.01, 0.2, 77, norm_out=out_b[:, d:d + do])
        assert torch.equal(out_a[:, :d], H) and torch.isnan(out_b[:, :d]).all()
        assert torch.equal(h_a, h_b) and torch.equal(out_a[:, d:d + do], out_b[:, d:d + do])


def test_sum_partials_one_launch(K, dev):
    """kgat_sum_partials_f32: several partial sets (the weight gradients of a stack's layers) summed by one launch -
    against a float64 sum, bit for bit the same on a second call, set sizes off every grouping (1 ... 768 partials)."""
    from dgl_kgat_amd import ops
    gen = torch.Generator().manual_seed(9)
    sets = [torch.randn(768, 64, 64, generator=gen).to(dev), torch.randn(768, 32, 64, generator=gen).to(dev),
            torch.randn(129, 16, 32, generator=gen).to(dev), torch.randn(1, 4, 4, generator=gen).to(dev),
            torch.randn(17, 128, 128, generator=gen).to(dev)]
    got = ops.sum_partials(sets)
    again = ops.sum_partials(sets)
    for t, g_, a_ in zip(sets, got, again):
        ref = t.double().sum(0)
        assert g_.shape == t.shape[1:] and torch.equal(g_, a_)
        assert float((g_.double() - ref).abs().max()) <= 1e-6 * float(t.abs().sum(0).max())
