"""Graphs, float64 reference and metric for the edge softmax's 1,024-position form (kgat_softmax.hip).

``kgat_edge_softmax_f32`` sweeps 8 positions per lane (512 per wavefront range) while a call covers fewer than
``SWITCH`` = 8,388,608 positions and 16 per lane (1,024 per range) from there on.  The graphs here are just large enough
for the second form and put, inside that one call, what ``test_edge_softmax_lane_structures`` walks for the first: rows
of one length at every alignment against a lane (16 positions), a DPP row (256) and a range (1,024), rows cut once and
rows spanning many ranges, empty rows in between, and hubs whose chains of carries are longer than 64 and longer than
128 ranges, so that ``sm_chain_total`` takes its second and later blocks of 64 followers.

``wide_graph(seed)`` -> (n, dst, lens): destination rows in this order (``wide_layout()`` names the row indices)
    1. a row of 3 positions and a row of 1: indptr starts 0, 3, 4, so position 3 and position 4 are row starts (the
       calls that begin there are unaligned / aligned for 16-byte loads);
    2. for every L in BLOCK_LENGTHS and off in BLOCK_OFFSETS: a prefix row of `off` positions (none for off = 0),
       block_rows(L) rows of length L, one row without in-edges;
    3. the HUBS;
    4. filler rows of min(zipf(1.5), 3000) positions, an empty row before about a tenth of them; the last two filler
       rows are a trimmed one and a row of one position, so that the total comes out as below and both
       e - TAIL and e - TAIL - 1 are row starts;
    5. TAIL rows of one position.
The total is SWITCH + TAIL + 3 = 8,392,707 positions (not a multiple of 4: the last range is ragged), so that
(3, 3 + SWITCH) is a call of exactly SWITCH positions that ends where the tail begins.  `dst` is in edge-id order and
edge ids are a random permutation of the CSR positions.

``const_graph(seed)`` -> (n, dst, lens): every non-empty row is a power of two long, 2^0 .. 2^18, each length at
offsets CONST_OFFSETS past a multiple of 1,024 (the padding and the offsets are themselves power-of-two rows), an empty
row after each, power-of-two filler, TAIL rows of one position, the same total.  With one constant logit per row every
weight is exactly 1 / L.

``segment_softmax`` is the reference (float64) and, with dtype=np.float32, its restatement; ``metric`` is the one of
``test_edge_softmax_lane_structures``: |got - ref| / max(ref, 1e-3), under the same bar of 2e-6."""
import numpy as np

SWITCH = 8 << 20          # kSmSmallEdges
RANGE = 1024              # positions per wavefront range at 16 per lane
LANE = 16
TAIL = 4096
TOTAL = SWITCH + TAIL + 3
BAR = 2e-6

BLOCK_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 240, 255, 256, 257, 272, 511, 512, 513, 1008, 1023, 1024, 1025, 1040,
                 2047, 2048, 2049, 3000, 5000)
BLOCK_OFFSETS = (0, 1, 5, 8, 13, 15, 16, 17)
HUBS = (70000, 200000, 66560, 65537)
CONST_OFFSETS = (0, 1, 5, 15, 16, 17)
CONST_MAX_LOG2 = 18


def block_rows(L):
    return max(3, 4096 // L + 2)


def wide_layout():
    """({(L, off): index of the block's first row of length L}, [the hubs' row indices], first filler row)."""
    blocks, r = {}, 2
    for L in BLOCK_LENGTHS:
        for off in BLOCK_OFFSETS:
            r += 1 if off else 0
            blocks[(L, off)] = r
            r += block_rows(L) + 1
    return blocks, list(range(r, r + len(HUBS))), r + len(HUBS)


def _powers_of_two(v):
    """v as a descending list of powers of two."""
    return [1 << b for b in range(int(v).bit_length() - 1, -1, -1) if (int(v) >> b) & 1]


def _dst_in_edge_id_order(lens, rng):
    e = int(lens.sum())
    row_csr = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
    dst = np.empty(e, np.int32)
    dst[rng.permutation(e)] = row_csr
    return dst


def _draw_until(room, draw):
    """Lengths from draw(k), as many as fit into `room` positions."""
    got, left = [], room
    while True:
        ln = draw(1 << 16)
        k = int(np.searchsorted(np.cumsum(ln), left, side="right"))
        got.append(ln[:k])
        left -= int(ln[:k].sum())
        if k < len(ln):
            return np.concatenate(got), left


def wide_graph(seed):
    rng = np.random.default_rng(seed)
    head = [3, 1]
    for L in BLOCK_LENGTHS:
        for off in BLOCK_OFFSETS:
            head += ([off] if off else []) + [L] * block_rows(L) + [0]
    head += list(HUBS)
    head = np.asarray(head, np.int64)
    room = TOTAL - TAIL - int(head.sum()) - 1          # (- 1: the filler's closing row of one position)
    fill, left = _draw_until(room, lambda k: np.minimum(rng.zipf(1.5, k), 3000).astype(np.int64))
    fill = np.insert(fill, np.flatnonzero(rng.random(len(fill)) < 0.1), 0)
    lens = np.concatenate([head, fill, np.asarray(([left] if left else []) + [1], np.int64), np.ones(TAIL, np.int64)])
    assert int(lens.sum()) == TOTAL
    return len(lens), _dst_in_edge_id_order(lens, rng), lens


def const_graph(seed):
    rng = np.random.default_rng(seed)
    head, pos = [2, 1, 1], 4
    for k in range(CONST_MAX_LOG2 + 1):
        for off in CONST_OFFSETS:
            pad = _powers_of_two(-pos % RANGE) + _powers_of_two(off)
            head += pad + [1 << k, 0]
            pos += sum(pad) + (1 << k)
    head = np.asarray(head, np.int64)
    room = TOTAL - TAIL - int(head.sum())
    fill, left = _draw_until(room, lambda k: np.int64(1) << rng.integers(0, 13, k))
    lens = np.concatenate([head, fill, np.asarray(_powers_of_two(left), np.int64), np.ones(TAIL, np.int64)])
    assert int(lens.sum()) == TOTAL
    return len(lens), _dst_in_edge_id_order(lens, rng), lens


def indptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def segment_softmax(x_csr, indptr, e0=0, e1=None, dtype=np.float64, with_rows=False):
    """Softmax of x_csr[e0:e1] over each row's positions inside [e0, e1) (what a call with that e_range computes),
    with np.maximum.reduceat / np.add.reduceat in `dtype`.  with_rows=True: also the maxima and the sums of
    exp(x - max) per row (NaN / 0 for rows without a position in the range)."""
    e1 = len(x_csr) if e1 is None else e1
    ip = np.clip(np.asarray(indptr, np.int64), e0, e1) - e0
    ln_all = np.diff(ip)
    starts, ln = ip[:-1][ln_all > 0], ln_all[ln_all > 0]
    x = np.asarray(x_csr[e0:e1], dtype)
    m = np.maximum.reduceat(x, starts)
    ex = np.exp(x - np.repeat(m, ln))
    z = np.add.reduceat(ex, starts)
    assert ex.dtype == dtype and z.dtype == dtype
    a = ex / np.repeat(z, ln)
    if not with_rows:
        return a
    m_rows, z_rows = np.full(len(ln_all), np.nan), np.zeros(len(ln_all))
    m_rows[ln_all > 0], z_rows[ln_all > 0] = m, z
    return a, m_rows, z_rows


def metric(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(ref, 1e-3)


def position_classes(lens, e0, e1, epw):
    """Boolean masks over the positions [e0, e1) of a call with ranges of `epw` positions: rows that lie inside one
    range ("uncut"; all of them are at most 5,000 long), rows a range edge cuts ("cut", the hubs apart), and each hub
    ("hub L").  A row is taken as far as it lies inside [e0, e1)."""
    indptr = indptr_of(lens)
    beg, end = np.clip(indptr[:-1], e0, e1), np.clip(indptr[1:], e0, e1)
    cut_row = (end > beg) & ((beg - e0) // epw != (np.maximum(end, beg + 1) - 1 - e0) // epw)
    hub_row = lens > 5000
    row_of = np.repeat(np.arange(len(lens)), end - beg)
    out = {"uncut": ~cut_row[row_of], "cut": (cut_row & ~hub_row)[row_of]}
    for r in np.flatnonzero(hub_row):
        out["hub %d" % lens[r]] = row_of == r
    return out


def range_cuts(lens, e0, e1, epw):
    """How the ranges of a call over [e0, e1) meet the rows, as the sweep decides it (cut_start: the range's first row
    began before it; cut_end: its last row goes on after it): the numbers of ranges cut at the start only, at the end
    only, at both ends by two rows, filled by one row that goes on at both ends, and every row's number of ranges."""
    indptr = indptr_of(lens)
    base = np.arange(e0, e1, epw, dtype=np.int64)
    end = np.minimum(base + epw, e1)
    first = np.searchsorted(indptr, base, side="right") - 1       # the row holding position base
    last = np.searchsorted(indptr, end - 1, side="right") - 1     # the row holding position end - 1
    cs = (base > e0) & (indptr[first] < base)
    ce = (end < e1) & (indptr[last + 1] > end)
    beg_r, end_r = np.clip(indptr[:-1], e0, e1), np.clip(indptr[1:], e0, e1)
    chain = np.where(end_r > beg_r, (np.maximum(end_r, beg_r + 1) - 1 - e0) // epw - (beg_r - e0) // epw + 1, 0)
    return {"start_only": int((cs & ~ce).sum()), "end_only": int((ce & ~cs).sum()),
            "both_two_rows": int((cs & ce & (first != last)).sum()), "whole_range": int((cs & ce & (first == last)).sum()),
            "chain": chain}
