"""The sparse reducers' tile plan and argument checks without a GPU.  kgat_spmm_tile_edges, kgat_spmm_workspace_bytes
and kgat_spmm_max_workspace_bytes are compared with the tile rule restated here (not read from the library) over edge
counts on both sides of every limit; every refusal of the four entries that returns before the first HIP call is
checked with its return code and the exact text of kgat_last_error(), and the order of two refusals wherever one call
triggers both."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dgl_kgat_amd import _lib  # noqa: E402

OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
INT32_MAX = 2 ** 31 - 1

# ---- the rule: width -> edges per tile with short / half-length / full-length runs.  Short runs while they give at
# most 4,096 tiles, else half-length runs while those give at most 16,384, else full-length runs.
TILE = {4: (512, 1024, 1024), 8: (256, 1024, 1024), 16: (256, 512, 1024), 32: (256, 512, 1024), 64: (256, 1024, 1024),
        128: (128, 512, 512), 256: (64, 256, 256)}
SHORT_LIMIT, HALF_LIMIT = 4096, 16384
TILE_WIDTHS = (16, 32, 64, 128)          # kgat_spmm_tile_edges answers for these, the max reducer's fast path too


def _ceil(a, b):
    return -(-a // b)


def _tile_edges(n, D):
    short, half, full = TILE[D]
    if _ceil(n, short) <= SHORT_LIMIT:
        return short
    return half if _ceil(n, half) <= HALF_LIMIT else full


def _rounded(nbytes):
    return _ceil(nbytes, 256) * 256 + 256


def _rule_tile_edges(n, D):
    return _tile_edges(n, D) if n >= 0 and D in TILE_WIDTHS else 0


def _rule_sum_workspace(n, D):           # per tile: its first and its last row, D floats each
    if n <= 0 or D not in TILE:
        return 256
    return _rounded(_ceil(n, _tile_edges(n, D)) * 2 * D * 4)


def _rule_max_workspace(n, D):           # a value and an edge id per column; any other width: D = 64 tiles, 16-column passes
    if n <= 0 or D <= 0:
        return 256
    if D in TILE_WIDTHS:
        return _rounded(_ceil(n, _tile_edges(n, D)) * 2 * D * 8)
    return _rounded(_ceil(n, _tile_edges(n, 64)) * _ceil(D, 16) * 2 * 16 * 8)


def _edge_counts(D):
    geom = TILE[D if D in TILE else 64]
    counts = {-1, 0, 1, 3663302, 5000000, 20000003}
    for te in geom:
        counts |= {te - 1, te, te + 1}
    for te, limit in ((geom[0], SHORT_LIMIT), (geom[1], HALF_LIMIT)):
        counts |= {te * limit - 1, te * limit, te * limit + 1}
    return sorted(counts)


def test_the_limits_named_in_the_rule():
    # both sides of every limit, as edge counts
    for D in (16, 32, 64):
        assert {1048576, 1048577} <= set(_edge_counts(D))
        assert (_rule_tile_edges(1048576, D), _rule_tile_edges(1048577, D)) == (256, TILE[D][1])
    assert {524288, 524289} <= set(_edge_counts(128))
    assert (_rule_tile_edges(524288, 128), _rule_tile_edges(524289, 128)) == (128, 512)
    for D in (16, 32):
        assert {8388608, 8388609} <= set(_edge_counts(D))
        assert (_rule_tile_edges(8388608, D), _rule_tile_edges(8388609, D)) == (512, 1024)


WIDTHS = (4, 8, 16, 32, 64, 128, 256, 1, 20, 65, 100, 0, -4)


@pytest.mark.parametrize("D", WIDTHS)
def test_plan_values(D):
    lib = _lib.load()
    for n in _edge_counts(D):
        assert lib.kgat_spmm_tile_edges(n, D) == _rule_tile_edges(n, D), (n, D)
        assert lib.kgat_spmm_workspace_bytes(n, D) == _rule_sum_workspace(n, D), (n, D)
        assert lib.kgat_spmm_max_workspace_bytes(n, D) == _rule_max_workspace(n, D), (n, D)


def test_tile_edges_is_zero_outside_its_widths():
    lib = _lib.load()
    for D in (4, 8, 256, 20, 65, 0):     # the merge kernels also run at 4, 8 and 256: the deferred consumer does not
        for n in (0, 1, 100000, 5000000):
            assert lib.kgat_spmm_tile_edges(n, D) == 0
            assert lib.kgat_spmm_workspace_bytes(n, D) == _rule_sum_workspace(n, D)
    assert lib.kgat_spmm_workspace_bytes(100000, 20) == 256 and lib.kgat_spmm_workspace_bytes(100000, 8) > 256


# ---- the entries' refusals before the first HIP call
_BUF = C.create_string_buffer(4096)      # a non-null, 16-byte aligned address; no case below gets as far as reading it
P = (C.addressof(_BUF) + 15) & ~15
ODD = P + 4                              # 4-byte aligned only
N, E = 100, 10
MERGE, ROWS, GENERIC, MERGE1 = 1, 2, 3, 4
MUL_SELF, DEFER = 1, 2


def _call(name, args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def _refused(name, args, rc, text):
    got, msg = _call(name, args)
    assert got == rc, (name, got, msg)
    assert msg == text, (name, msg)


def _sum(n_rows=N, row0=0, e0=0, e1=E, D=64, indptr=P, col=P, row_of=P, eid=None, X=P, w=P, out=P, order=None, ws=None,
         ws_bytes=0, flags=0, algo=0, self_out=None, self_stride=0):
    return (n_rows, row0, e0, e1, D, indptr, col, row_of, eid, X, w, out, order, ws, ws_bytes, flags, algo, self_out,
            self_stride, None)


def test_sum_entry_refusals():
    name = "kgat_spmm_umule_sum_f32"
    _refused(name, _sum(n_rows=-1), BADARG, "spmm: bad size (n_rows=-1 row0=0 D=64)")
    _refused(name, _sum(row0=-2), BADARG, "spmm: bad size (n_rows=100 row0=-2 D=64)")
    _refused(name, _sum(D=0), BADARG, "spmm: bad size (n_rows=100 row0=0 D=0)")
    _refused(name, _sum(row0=INT32_MAX - N), BADARG, "spmm: row range exceeds int32")
    _refused(name, _sum(e0=-1), BADARG, "spmm: bad edge range")
    _refused(name, _sum(e0=5, e1=4), BADARG, "spmm: bad edge range")
    _refused(name, _sum(e1=INT32_MAX), BADARG, "spmm: bad edge range")
    assert _call(name, _sum(n_rows=0, indptr=None, X=None, out=None, flags=8, algo=9))[0] == OK
    _refused(name, _sum(indptr=None), BADARG, "spmm: null pointer")
    _refused(name, _sum(X=None), BADARG, "spmm: null pointer")
    _refused(name, _sum(out=None), BADARG, "spmm: null pointer")
    _refused(name, _sum(col=None), BADARG, "spmm: null col/w")
    _refused(name, _sum(w=None), BADARG, "spmm: null col/w")
    _refused(name, _sum(flags=4), BADARG, "spmm: unknown flags 0x4")
    _refused(name, _sum(algo=5), BADARG, "spmm: unknown algo 5")
    _refused(name, _sum(algo=-1), BADARG, "spmm: unknown algo -1")
    _refused(name, _sum(row_of=None, algo=MERGE), BADARG, "spmm: merge algorithm needs row_of")
    _refused(name, _sum(row_of=None, algo=MERGE1), BADARG, "spmm: merge algorithm needs row_of")
    _refused(name, _sum(order=P), BADARG, "spmm: a row order only applies to the rows algorithm")
    _refused(name, _sum(order=P, D=20, algo=ROWS), BADARG, "spmm: a row order only applies to the rows algorithm")
    defer = ("spmm: KGAT_SPMM_DEFER_FINISH goes with the plain operator, CSR-ordered weights, the merge algorithm and D in "
             "{16, 32, 64, 128}")
    _refused(name, _sum(flags=DEFER | MUL_SELF), BADARG, defer)
    _refused(name, _sum(flags=DEFER, eid=P), BADARG, defer)
    _refused(name, _sum(flags=DEFER, algo=ROWS), BADARG, defer)
    for D in (4, 8, 256, 20):
        _refused(name, _sum(flags=DEFER, D=D), BADARG, defer)
    goes = "spmm: self_out goes with KGAT_SPMM_MUL_SELF, CSR-ordered weights and the merge algorithm"
    _refused(name, _sum(self_out=P, self_stride=64), BADARG, goes)
    _refused(name, _sum(self_out=P, self_stride=64, flags=MUL_SELF, eid=P), BADARG, goes)
    _refused(name, _sum(self_out=P, self_stride=64, flags=MUL_SELF, algo=ROWS), BADARG, goes)
    strided = "spmm: self_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= D"
    _refused(name, _sum(self_out=P, self_stride=60, flags=MUL_SELF), BADARG, strided)
    _refused(name, _sum(self_out=P, self_stride=66, flags=MUL_SELF), BADARG, strided)
    _refused(name, _sum(self_out=ODD, self_stride=64, flags=MUL_SELF), BADARG, strided)
    # one tile of two boundary rows of 64 floats; 2,000 edges at D = 16 are eight tiles of 256
    _refused(name, _sum(), WORKSPACE, "spmm: workspace too small (0 < 512)")
    _refused(name, _sum(ws=P, ws_bytes=511, eid=P), WORKSPACE, "spmm: workspace too small (511 < 512)")
    _refused(name, _sum(ws=P, ws_bytes=1023, D=16, e1=2000, algo=MERGE1), WORKSPACE, "spmm: workspace too small (1023 < 1024)")
    _refused(name, _sum(D=256, flags=MUL_SELF), WORKSPACE, "spmm: workspace too small (0 < 2048)")


def test_sum_entry_order_of_refusals():
    name = "kgat_spmm_umule_sum_f32"
    _refused(name, _sum(n_rows=-1, row0=INT32_MAX, e0=-1, X=None), BADARG, "spmm: bad size (n_rows=-1 row0=2147483647 D=64)")
    _refused(name, _sum(row0=INT32_MAX, e0=-1, X=None), BADARG, "spmm: row range exceeds int32")
    _refused(name, _sum(e0=-1, X=None, n_rows=0), BADARG, "spmm: bad edge range")
    _refused(name, _sum(X=None, col=None, flags=4), BADARG, "spmm: null pointer")
    _refused(name, _sum(col=None, flags=4, algo=9), BADARG, "spmm: null col/w")
    _refused(name, _sum(flags=4, algo=9, row_of=None), BADARG, "spmm: unknown flags 0x4")
    _refused(name, _sum(algo=9, row_of=None, order=P), BADARG, "spmm: unknown algo 9")
    _refused(name, _sum(algo=MERGE, row_of=None, order=P), BADARG, "spmm: merge algorithm needs row_of")
    _refused(name, _sum(order=P, flags=DEFER | MUL_SELF), BADARG, "spmm: a row order only applies to the rows algorithm")
    _refused(name, _sum(flags=DEFER | MUL_SELF, self_out=P, self_stride=60, eid=P), BADARG,
             "spmm: KGAT_SPMM_DEFER_FINISH goes with the plain operator, CSR-ordered weights, the merge algorithm and D in "
             "{16, 32, 64, 128}")
    _refused(name, _sum(self_out=ODD, self_stride=60), BADARG,
             "spmm: self_out goes with KGAT_SPMM_MUL_SELF, CSR-ordered weights and the merge algorithm")
    _refused(name, _sum(self_out=ODD, self_stride=64, flags=MUL_SELF), BADARG,
             "spmm: self_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= D")
    # without edges the operands of the edges may be null, and a merge needs no row_of
    got, msg = _call(name, _sum(e1=0, col=None, w=None, row_of=None, algo=MERGE, order=P))
    assert (got, msg) == (BADARG, "spmm: a row order only applies to the rows algorithm")


def _fused(n_rows=N, row0=0, e0=0, e1=E, d_in=64, d_out=64, indptr=P, col=P, row_of=P, X=P, w=P, W2=P, h_out=P,
           norm_out=None, norm_stride=0, scratch=P, ws=None, ws_bytes=0, self_out=None, self_stride=0):
    return (n_rows, row0, e0, e1, d_in, d_out, indptr, col, row_of, X, w, W2, 0.01, h_out, norm_out, norm_stride, scratch,
            ws, ws_bytes, self_out, self_stride, None)


def test_fused_entry_refusals():
    name = "kgat_spmm_bi_fused_f32"
    _refused(name, _fused(n_rows=-1), BADARG, "spmm_bi_fused: bad size (n_rows=-1 row0=0)")
    _refused(name, _fused(row0=-1), BADARG, "spmm_bi_fused: bad size (n_rows=100 row0=-1)")
    _refused(name, _fused(row0=INT32_MAX - N), BADARG, "spmm_bi_fused: row range exceeds int32")
    _refused(name, _fused(e0=5, e1=4), BADARG, "spmm_bi_fused: bad edge range")
    _refused(name, _fused(e1=INT32_MAX), BADARG, "spmm_bi_fused: bad edge range")
    for d_in, d_out in ((64, 128), (128, 64), (32, 64), (16, 32), (8, 8), (0, 0), (64, 48)):
        _refused(name, _fused(d_in=d_in, d_out=d_out), UNSUPPORTED,
                 "spmm_bi_fused: unsupported widths %d -> %d" % (d_in, d_out))
    assert _call(name, _fused(n_rows=0, indptr=None, X=None))[0] == OK
    _refused(name, _fused(n_rows=0, d_in=8, d_out=8), UNSUPPORTED, "spmm_bi_fused: unsupported widths 8 -> 8")
    for null in ("indptr", "X", "W2", "scratch", "h_out"):
        _refused(name, _fused(**{null: None}), BADARG, "spmm_bi_fused: null pointer")
    for null in ("col", "w", "row_of"):
        _refused(name, _fused(**{null: None}), BADARG, "spmm_bi_fused: null col / w / row_of")
    norm = "spmm_bi_fused: norm_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= d_out"
    _refused(name, _fused(norm_out=P, norm_stride=60), BADARG, norm)
    _refused(name, _fused(norm_out=P, norm_stride=66), BADARG, norm)
    _refused(name, _fused(norm_out=ODD, norm_stride=64, h_out=None), BADARG, norm)
    own = "spmm_bi_fused: self_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= d_in"
    _refused(name, _fused(self_out=P, self_stride=32, d_out=32), BADARG, own)
    _refused(name, _fused(self_out=ODD, self_stride=64), BADARG, own)
    # the launcher is the sum operator's and reports under its name
    _refused(name, _fused(), WORKSPACE, "spmm: workspace too small (0 < 512)")
    _refused(name, _fused(d_in=32, d_out=16, ws=P, ws_bytes=255), WORKSPACE, "spmm: workspace too small (255 < 256)")
    # the order
    _refused(name, _fused(n_rows=-1, e0=-1, d_in=8), BADARG, "spmm_bi_fused: bad size (n_rows=-1 row0=0)")
    _refused(name, _fused(row0=INT32_MAX, e0=-1, d_in=8), BADARG, "spmm_bi_fused: row range exceeds int32")
    _refused(name, _fused(e0=-1, d_in=8), BADARG, "spmm_bi_fused: bad edge range")
    _refused(name, _fused(d_in=8, X=None), UNSUPPORTED, "spmm_bi_fused: unsupported widths 8 -> 64")
    _refused(name, _fused(X=None, col=None), BADARG, "spmm_bi_fused: null pointer")
    _refused(name, _fused(col=None, norm_out=ODD, norm_stride=64), BADARG, "spmm_bi_fused: null col / w / row_of")
    _refused(name, _fused(norm_out=ODD, norm_stride=64, self_out=ODD, self_stride=64), BADARG, norm)
    _refused(name, _fused(self_out=ODD, self_stride=64), BADARG, own)


def test_fused_supported_is_its_six_pairs():
    lib = _lib.load()
    pairs = {(64, 64), (64, 32), (64, 16), (32, 32), (32, 16), (16, 16)}
    widths = (0, 4, 8, 16, 20, 32, 48, 64, 128, 256)
    for d_in in widths:
        for d_out in widths:
            assert lib.kgat_spmm_bi_fused_supported(d_in, d_out) == int((d_in, d_out) in pairs), (d_in, d_out)


def _copy(n_rows=N, row0=0, e0=0, e1=E, D=64, indptr=P, col=P, row_of=P, X=P, out=P, reduce=0, ws=None, ws_bytes=0):
    return (n_rows, row0, e0, e1, D, indptr, col, row_of, X, out, reduce, ws, ws_bytes, None)


def test_copy_entry_refusals():
    name = "kgat_copy_reduce_f32"
    _refused(name, _copy(n_rows=-1), BADARG, "copy_reduce: bad size (n_rows=-1 row0=0 D=64)")
    _refused(name, _copy(D=-3), BADARG, "copy_reduce: bad size (n_rows=100 row0=0 D=-3)")
    _refused(name, _copy(row0=INT32_MAX - N), BADARG, "copy_reduce: row range exceeds int32")
    _refused(name, _copy(e0=-1), BADARG, "copy_reduce: bad edge range")
    _refused(name, _copy(e1=INT32_MAX), BADARG, "copy_reduce: bad edge range")
    _refused(name, _copy(reduce=2), BADARG, "copy_reduce: unknown reduce 2")
    _refused(name, _copy(reduce=-1, n_rows=0), BADARG, "copy_reduce: unknown reduce -1")
    assert _call(name, _copy(n_rows=0, indptr=None, X=None, out=None))[0] == OK
    for null in ("indptr", "X", "out"):
        _refused(name, _copy(**{null: None}), BADARG, "copy_reduce: null pointer")
    _refused(name, _copy(col=None), BADARG, "copy_reduce: null col / row_of")
    _refused(name, _copy(row_of=None), BADARG, "copy_reduce: null col / row_of")
    _refused(name, _copy(col=None, D=20), BADARG, "copy_reduce: null col / row_of")
    _refused(name, _copy(X=ODD), BADARG, "copy_reduce: X and out must be 16-byte aligned")
    _refused(name, _copy(out=ODD, reduce=1), BADARG, "copy_reduce: X and out must be 16-byte aligned")
    _refused(name, _copy(), WORKSPACE, "copy_reduce: workspace too small (0 < 512)")
    _refused(name, _copy(D=128, e1=129, reduce=1, ws=P, ws_bytes=2047), WORKSPACE,
             "copy_reduce: workspace too small (2047 < 2048)")
    # the order
    _refused(name, _copy(n_rows=-1, row0=INT32_MAX, e0=-1, reduce=2), BADARG,
             "copy_reduce: bad size (n_rows=-1 row0=2147483647 D=64)")
    _refused(name, _copy(row0=INT32_MAX, e0=-1, reduce=2), BADARG, "copy_reduce: row range exceeds int32")
    _refused(name, _copy(e0=-1, reduce=2), BADARG, "copy_reduce: bad edge range")
    _refused(name, _copy(reduce=2, X=None), BADARG, "copy_reduce: unknown reduce 2")
    _refused(name, _copy(X=None, col=None), BADARG, "copy_reduce: null pointer")
    _refused(name, _copy(col=None, X=ODD), BADARG, "copy_reduce: null col / row_of")
    _refused(name, _copy(X=ODD), BADARG, "copy_reduce: X and out must be 16-byte aligned")


def _max(n_rows=N, row0=0, e0=0, e1=E, D=64, indptr=P, col=P, row_of=P, eid=None, X=P, w=P, out=P, arg=P, ws=None,
         ws_bytes=0):
    return (n_rows, row0, e0, e1, D, indptr, col, row_of, eid, X, w, out, arg, ws, ws_bytes, None)


def test_max_entry_refusals():
    name = "kgat_spmm_umule_max_f32"
    _refused(name, _max(n_rows=-1), BADARG, "spmm_max: bad size (n_rows=-1 row0=0 D=64)")
    _refused(name, _max(D=0), BADARG, "spmm_max: bad size (n_rows=100 row0=0 D=0)")
    _refused(name, _max(row0=INT32_MAX - N), BADARG, "spmm_max: row range exceeds int32")
    _refused(name, _max(e0=3, e1=2), BADARG, "spmm_max: bad edge range")
    _refused(name, _max(e1=INT32_MAX), BADARG, "spmm_max: bad edge range")
    _refused(name, _max(D=16 * 65535 + 1), BADARG, "spmm_max: D = 1048561 is beyond the grid's column passes")
    _refused(name, _max(D=16 * 65535 + 1, n_rows=0), BADARG, "spmm_max: D = 1048561 is beyond the grid's column passes")
    assert _call(name, _max(n_rows=0, indptr=None, X=None, out=None))[0] == OK
    for null in ("indptr", "X", "out"):
        _refused(name, _max(**{null: None}), BADARG, "spmm_max: null pointer")
    _refused(name, _max(col=None), BADARG, "spmm_max: null col/row_of")
    _refused(name, _max(row_of=None, D=20), BADARG, "spmm_max: null col/row_of")
    for odd in ("X", "out", "arg"):
        for D in TILE_WIDTHS:
            _refused(name, _max(**{odd: ODD, "D": D}), BADARG,
                     "spmm_max: X, out and arg must be 16-byte aligned at D = %d" % D)
    # one tile of two boundary rows: a value and an id per column; D = 20: two passes of sixteen columns
    _refused(name, _max(), WORKSPACE, "spmm_max: workspace too small (0 < 1024)")
    _refused(name, _max(arg=None, w=None, ws=P, ws_bytes=1023), WORKSPACE, "spmm_max: workspace too small (1023 < 1024)")
    _refused(name, _max(D=20, X=ODD, out=ODD, arg=ODD), WORKSPACE, "spmm_max: workspace too small (0 < 512)")
    _refused(name, _max(D=256, e1=257), WORKSPACE, "spmm_max: workspace too small (0 < 8192)")
    # the order
    _refused(name, _max(n_rows=-1, row0=INT32_MAX, e0=-1), BADARG, "spmm_max: bad size (n_rows=-1 row0=2147483647 D=64)")
    _refused(name, _max(row0=INT32_MAX, e0=-1), BADARG, "spmm_max: row range exceeds int32")
    _refused(name, _max(e0=-1, D=16 * 65535 + 1), BADARG, "spmm_max: bad edge range")
    _refused(name, _max(D=16 * 65535 + 1, X=None), BADARG, "spmm_max: D = 1048561 is beyond the grid's column passes")
    _refused(name, _max(X=None, col=None), BADARG, "spmm_max: null pointer")
    _refused(name, _max(col=None, out=ODD), BADARG, "spmm_max: null col/row_of")
    _refused(name, _max(out=ODD), BADARG, "spmm_max: X, out and arg must be 16-byte aligned at D = 64")


def test_probe_refusals():
    name = "kgat_gather_probe_f32"
    _refused(name, (-1, 64, P, P, P, None), BADARG, "gather_probe: bad size")
    assert _call(name, (0, 7, None, None, None, None))[0] == OK
    _refused(name, (E, 64, None, P, P, None), BADARG, "gather_probe: null pointer")
    for D in (4, 8, 256, 20):
        _refused(name, (E, D, P, P, P, None), UNSUPPORTED, "gather_probe: D must be 16, 32, 64 or 128 (got %d)" % D)
