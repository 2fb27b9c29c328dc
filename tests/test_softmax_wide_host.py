"""tests/_softmax_wide_ref.py checked where no GPU is needed: the graphs hold what they claim, the float32 restatement of
the reference stays inside the bar the device is held to, and two ways in which the 1,024-position form could go
wrong - a lane normalised with its neighbour row's sum, a cut row's positions left scaled with a range's partial
maximum - miss that bar."""
import numpy as np
import pytest

import _softmax_wide_ref as W


@pytest.fixture(scope="module")
def wide():
    n, dst, lens = W.wide_graph(0)
    indptr = W.indptr_of(lens)
    eid = np.argsort(dst, kind="stable")
    x = (np.random.default_rng(1).standard_normal(len(dst)) * 4).astype(np.float32)[eid]   # logits in CSR order
    ref, m, z = W.segment_softmax(x, indptr, with_rows=True)
    return dict(n=n, dst=dst, lens=lens, indptr=indptr, eid=eid, x=x, ref=ref, m=m, z=z)


def test_wide_graph_is_what_it_claims(wide):
    n, dst, lens, indptr = wide["n"], wide["dst"], wide["lens"], wide["indptr"]
    e = len(dst)
    assert n == len(lens) and e == W.TOTAL == 8_392_707 and e % 4 != 0
    assert np.array_equal(np.bincount(dst, minlength=n), lens)
    assert np.array_equal(indptr[:3], [0, 3, 4])
    assert np.all(lens[-W.TAIL:] == 1) and e - W.TAIL >= 3 + W.SWITCH
    assert np.isin([3, 4, 3 + W.SWITCH, 3 + W.SWITCH - 1], indptr).all()   # the calls' ranges begin and end with rows
    eid = wide["eid"]
    assert not np.array_equal(eid, np.arange(e)) and np.mean(eid == np.arange(e)) < 1e-3
    # every (L, off) block, walked from the lengths alone, sits where wide_layout() says
    blocks, hubs, first_filler = W.wide_layout()
    i = 2
    for L in W.BLOCK_LENGTHS:
        for off in W.BLOCK_OFFSETS:
            if off:
                assert lens[i] == off, (L, off)
                i += 1
            k = max(3, 4096 // L + 2)
            assert blocks[(L, off)] == i and np.all(lens[i:i + k] == L) and lens[i + k] == 0, (L, off)
            i += k + 1
    assert hubs == list(range(i, i + 4)) and list(lens[i:i + 4]) == [70000, 200000, 66560, 65537]
    assert first_filler == i + 4
    filler = lens[first_filler:-W.TAIL]
    assert filler.max() == 3000 and 0.05 < np.mean(filler == 0) < 0.15
    assert np.all(lens[np.setdiff1d(np.arange(n), hubs)] <= 5000)
    # rows against the 1,024-position ranges of the calls that start at 0 and at 3
    for e0, e1 in ((0, e), (3, 3 + W.SWITCH), (4, e)):
        c = W.range_cuts(lens, e0, e1, W.RANGE)
        assert min(c["start_only"], c["end_only"], c["both_two_rows"], c["whole_range"]) > 0, (e0, c)
        chain = c["chain"][hubs]
        assert np.all(chain > 64) and chain[1] > 128, (e0, chain)
        assert c["chain"][np.setdiff1d(np.arange(n), hubs)].max() <= 6
        # followers of a chain's head are walked in blocks of 64: one block exactly, a second, a third and a fourth
        blocks_of_64 = -(-(chain - 1) // 64)
        assert blocks_of_64.min() <= 2 <= blocks_of_64.max() and blocks_of_64[1] >= 3, (e0, chain)
    # the 512-position form on the same rows (e_range = (3, 3 + SWITCH - 1))
    c = W.range_cuts(lens, 3, 3 + W.SWITCH - 1, 512)
    assert min(c["start_only"], c["end_only"], c["both_two_rows"], c["whole_range"]) > 0


def test_const_graph_is_what_it_claims():
    n, dst, lens = W.const_graph(0)
    indptr = W.indptr_of(lens)
    assert len(dst) == W.TOTAL >= W.SWITCH + 4099 and np.array_equal(np.bincount(dst, minlength=n), lens)
    nz = lens[lens > 0]
    assert np.all(nz & (nz - 1) == 0) and nz.max() == 1 << W.CONST_MAX_LOG2 and np.all(lens[-W.TAIL:] == 1)
    at = {(int(L), int(o)) for L, o in zip(lens[lens > 0], indptr[:-1][lens > 0] % W.RANGE)}
    for k in range(W.CONST_MAX_LOG2 + 1):
        for off in W.CONST_OFFSETS:
            assert (1 << k, off) in at, (k, off)
    assert np.any(lens == 0)
    c = W.range_cuts(lens, 0, W.TOTAL, W.RANGE)
    assert min(c["start_only"], c["end_only"], c["both_two_rows"], c["whole_range"]) > 0 and c["chain"].max() > 256


def test_fp32_restatement_is_inside_the_bar(wide):
    x, indptr, ref, lens = wide["x"], wide["indptr"], wide["ref"], wide["lens"]
    assert np.allclose(np.add.reduceat(ref, indptr[:-1][lens > 0]), 1.0, atol=1e-12)
    err = W.metric(W.segment_softmax(x, indptr, dtype=np.float32), ref)
    for name, mask in W.position_classes(lens, 0, len(x), W.RANGE).items():
        print("fp32 restatement, %-10s %.2e" % (name, err[mask].max()))
    assert err.max() < W.BAR
    # a sub-range is the same rows' softmax: (3, 3 + SWITCH) begins and ends with a row
    part = W.segment_softmax(x, indptr, 3, 3 + W.SWITCH)
    assert np.array_equal(part, ref[3:3 + W.SWITCH])
    # and one that ends inside a row normalises what lies inside it
    cut = int(indptr[5]) + 1
    part = W.segment_softmax(x, indptr, 0, cut)
    assert abs(part[indptr[5]:].sum() - 1.0) < 1e-12 and np.array_equal(part[:indptr[5]], ref[:indptr[5]])


def test_corruptions_miss_the_bar(wide):
    x, indptr, ref, m, z = wide["x"].astype(np.float64), wide["indptr"], wide["ref"], wide["m"], wide["z"]
    blocks, hubs, _ = W.wide_layout()
    # (a) one 16-position lane of a row normalised with the previous row's sum
    for L in (17, 33, 257, 1025, 5000):
        for off in (0, 13):
            r = blocks[(L, off)] + 1
            beg, end = int(indptr[r]), int(indptr[r + 1])
            lane = (beg + int(np.argmax(x[beg:end]))) // W.LANE
            lo, hi = max(beg, lane * W.LANE), min(end, (lane + 1) * W.LANE)
            bad = ref.copy()
            bad[lo:hi] *= z[r] / z[r - 1]
            err = W.metric(bad, ref)
            assert 0 < np.count_nonzero(err) <= W.LANE and err.max() > 10 * W.BAR, (L, off, err.max())
    # (b) a cut row's positions inside one range scaled with that range's partial maximum instead of the row's
    for r in hubs + [blocks[(1025, 0)] + 1, blocks[(2049, 5)] + 2, blocks[(5000, 17)]]:
        beg, end = int(indptr[r]), int(indptr[r + 1])
        top = beg + int(np.argmax(x[beg:end]))
        spans = [(max(beg, b), min(end, b + W.RANGE)) for b in range(beg - beg % W.RANGE, end, W.RANGE)]
        spans = [s for s in spans if not s[0] <= top < s[1]]
        assert spans, r
        lo, hi = max(spans, key=lambda s: s[1] - s[0])
        bad = ref.copy()
        bad[lo:hi] = np.exp(x[lo:hi] - x[lo:hi].max()) / z[r]
        err = W.metric(bad, ref)
        assert np.count_nonzero(err) <= W.RANGE and err.max() > 10 * W.BAR, (r, err.max())
