"""The edge softmax's 16-positions-per-lane form (1,024-position ranges) against float64, on graphs built for it.

``kgat_edge_softmax_f32`` launches ``softmax_local_kernel<IN_CSR, 16>`` + ``softmax_cut_rows_kernel<16>`` from 8,388,608
positions on, and the <.., 8> instances below; inside the sweep a range takes the 16-byte path (FAST) when it is full and
the call's first position is a multiple of 4.  Graphs, reference, metric and classes: tests/_softmax_wide_ref.py (checked
without a GPU by tests/test_softmax_wide_host.py).  Which instance each call reaches:

    call on wide_graph                        input     instance of the sweep
    (0, e)                                    edge id   <false, 16>, FAST; its ragged last range (3 positions) not FAST
    (0, e)                                    CSR       <true, 16>, FAST; the last range not FAST
    (3, 3 + 8,388,608)                        CSR       <true, 16>, not FAST, every range - exactly at the switch
    (3, 3 + 8,388,608)                        edge id   <false, 16>, not FAST, every range
    (4, e)                                    both      <true, 16> / <false, 16>, FAST with e0 > 0
    (3, 3 + 8,388,607)                        CSR       <true, 8>, not FAST: the 512-position form on the same rows

Every element must be finite and within 2e-6 under |got - ref| / max(ref, 1e-3), the bar and the metric of
test_edge_softmax_lane_structures; the float32 numpy restatement of the reference reaches 6.2e-7 (rows inside one range),
5.4e-7 (cut rows) and 1.3e-7 .. 2.5e-7 (hubs) on the same logits.

Measured on an MI355X when the test was written (worst value of the metric per class of row):

    call (both input orders: same bits)   rows in one range   cut rows   hub 70,000   hub 200,000   hub 66,560   hub 65,537
    (0, e)                                6.34e-07            5.34e-07   1.49e-07     1.57e-07      2.02e-07     2.10e-07
    (3, 3 + 8,388,608)                    7.28e-07            5.44e-07   2.85e-07     1.51e-07      2.26e-07     1.39e-07
    (4, e)                                6.39e-07            5.06e-07   1.49e-07     1.51e-07      1.38e-07     1.39e-07
    (3, 3 + 8,388,607), 512 positions     7.28e-07            6.69e-07   2.49e-07     1.51e-07      3.24e-07     1.45e-07
    512- against 1,024-position form on the common positions: 7.12e-07 (bar 4e-6: two results, each within 2e-6)

The device sits where the restatement sits, about a third of the bar, in every class and every instance; nothing had
to be fixed.

const_graph: with one constant logit per row every weight is float32(1 / L) bit for bit - exp(0) is 1 in sm_exp, sums of
ones are exact, the rows a range cuts divide by an exact power of two and the others take the hardware reciprocal of
their length.  That reciprocal proved exact at every power of two a row inside one range can have (2^0 .. 2^10), in
the 1,024- and in the 512-position form, so the comparison is equality for all rows.
"""
import numpy as np
import pytest
import torch

import _softmax_wide_ref as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _csr_on_device(n, dst, lens, dev):
    """The device's CSR of the graph, checked as far as the softmax depends on it: the row offsets and row ids are the
    graph's, and eid is a permutation that puts every edge into its destination's row."""
    from dgl_kgat_amd import ops
    e = len(dst)
    src = torch.zeros(e, dtype=torch.int32, device=dev)
    indptr, _, eid, row_of = ops.csr_from_coo(n, src, torch.as_tensor(dst, device=dev))
    eid_h = eid.cpu().numpy()
    assert np.array_equal(indptr.cpu().numpy(), W.indptr_of(lens))
    assert np.array_equal(row_of.cpu().numpy(), np.repeat(np.arange(n, dtype=np.int32), lens))
    assert np.array_equal(np.bincount(eid_h, minlength=e), np.ones(e, np.int64))
    assert np.array_equal(dst[eid_h], row_of.cpu().numpy()) and not np.array_equal(eid_h, np.arange(e))
    return indptr, eid, row_of, eid_h


@pytest.fixture(scope="module")
def wide(dev):
    n, dst, lens = W.wide_graph(0)
    indptr, eid, row_of, eid_h = _csr_on_device(n, dst, lens, dev)
    s = (np.random.default_rng(1).standard_normal(len(dst)) * 4).astype(np.float32)   # edge-id order
    x = s[eid_h]                                                                     # CSR order
    ref = W.segment_softmax(x, W.indptr_of(lens))
    ref.setflags(write=False)
    return dict(lens=lens, e=len(dst), indptr=indptr, eid=eid, row_of=row_of, eid_h=eid_h, ref=ref,
                s=torch.as_tensor(s, device=dev), x=torch.as_tensor(x, device=dev), x_h=x)


def _softmax(g, e_range, in_csr, want_out, want_csr):
    from dgl_kgat_amd import ops
    return ops.edge_softmax(g["indptr"], g["row_of"], g["eid"], g["x"] if in_csr else g["s"], in_csr_order=in_csr,
                            e_range=e_range, want_out=want_out, want_csr=want_csr)


def _ref(g, e0, e1):
    ip = W.indptr_of(g["lens"])
    if np.isin([e0, e1], ip).all():     # the range begins and ends with a row: the rows' own softmax
        return g["ref"][e0:e1]
    return W.segment_softmax(g["x_h"], ip, e0, e1)


def _check(g, name, got_csr, e0, e1, epw):
    got, ref = got_csr[e0:e1].cpu().numpy(), _ref(g, e0, e1)
    err = W.metric(got, ref)
    for cls, mask in W.position_classes(g["lens"], e0, e1, epw).items():
        print("    %-34s %-11s %.2e" % (name, cls, err[mask].max()))
    assert np.all(np.isfinite(got)), name
    assert err.max() < W.BAR, (name, err.max(), int(np.argmax(err)) + e0)
    return got


def test_wide_full_range_both_input_orders(wide):
    g, e = wide, wide["e"]
    out, out_csr = _softmax(g, (0, e), False, True, True)
    _check(g, "(0, e) edge-id input", out_csr, 0, e, W.RANGE)
    assert torch.equal(out_csr, out[g["eid"].long()])
    out2, out2_csr = _softmax(g, (0, e), True, True, True)
    _check(g, "(0, e) CSR input", out2_csr, 0, e, W.RANGE)
    assert torch.equal(out2_csr, out_csr) and torch.equal(out2, out)
    out3, out3_csr = _softmax(g, (0, e), False, True, True)
    assert torch.equal(out3_csr, out_csr) and torch.equal(out3, out)


def test_wide_unaligned_at_the_switch_and_the_512_form_on_the_same_rows(wide):
    g, e0 = wide, 3
    e1 = e0 + W.SWITCH
    _, a16 = _softmax(g, (e0, e1), True, False, True)
    got16 = _check(g, "(3, 3 + 8388608) CSR input", a16, e0, e1, W.RANGE)
    _, b16 = _softmax(g, (e0, e1), False, False, True)
    _check(g, "(3, 3 + 8388608) edge-id input", b16, e0, e1, W.RANGE)
    assert torch.equal(b16[e0:e1], a16[e0:e1])
    out, _ = _softmax(g, (e0, e1), False, True, False)      # edge-id ordered result of a sub-range: positions eid[e0:e1]
    assert torch.equal(out[g["eid"][e0:e1].long()], a16[e0:e1])
    # one position fewer: the 8-per-lane form on the same rows
    _, a8 = _softmax(g, (e0, e1 - 1), True, False, True)
    got8 = _check(g, "(3, 3 + 8388607) CSR input", a8, e0, e1 - 1, 512)
    both = np.abs(got8.astype(np.float64) - got16[:-1]) / np.maximum(g["ref"][e0:e1 - 1], 1e-3)
    print("    512-position against 1,024-position form: %.2e" % both.max())
    assert both.max() < 2 * W.BAR


def test_wide_aligned_with_a_first_position_above_zero(wide):
    g, e = wide, wide["e"]
    out, a = _softmax(g, (4, e), False, True, True)
    _check(g, "(4, e) edge-id input", a, 4, e, W.RANGE)
    assert torch.equal(out[g["eid"][4:].long()], a[4:])
    _, b = _softmax(g, (4, e), True, False, True)
    _check(g, "(4, e) CSR input", b, 4, e, W.RANGE)
    assert torch.equal(b[4:], a[4:])


@pytest.fixture(scope="module")
def const(dev):
    n, dst, lens = W.const_graph(0)
    indptr, eid, row_of, eid_h = _csr_on_device(n, dst, lens, dev)
    c = (np.arange(n) % 7 - 3).astype(np.float32)      # neighbouring rows differ
    row_csr = np.repeat(np.arange(n), lens)
    want = (np.float32(1.0) / lens[row_csr].astype(np.float32)).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), 1.0 / lens[row_csr])
    return dict(lens=lens, e=len(dst), indptr=indptr, eid=eid, row_of=row_of, want=want, row_csr=row_csr, s=torch.as_tensor(c[dst], device=dev), x=torch.as_tensor(c[row_csr], device=dev))


def _exact(g, name, got, want, rows):
    got = got.cpu().numpy()
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        L = g["lens"][rows[bad]]
        print("    %s: %d weights differ from 1 / L, at row lengths %s; largest |got * L - 1| = %.2e"
              % (name, int(bad.sum()), sorted(set(L.tolist())), float(np.abs(got[bad].astype(np.float64) * L - 1).max())))
    assert not bad.any(), name


def test_const_rows_give_one_over_their_length_exactly(const):
    g, e = const, const["e"]
    for in_csr in (False, True):
        out, out_csr = _softmax(g, (0, e), in_csr, True, True)
        _exact(g, "(0, e) %s input, CSR order" % ("CSR" if in_csr else "edge-id"), out_csr, g["want"], g["row_csr"])
        assert torch.equal(out_csr, out[g["eid"].long()])
    # a call below the switch that begins and ends with a row: up to the tail, at most 8,388,607 positions
    ip = W.indptr_of(g["lens"])
    e1 = e - W.TAIL
    e0 = int(ip[np.searchsorted(ip, e1 - (W.SWITCH - 1))])
    assert 0 < e1 - e0 < W.SWITCH and e1 - e0 > W.SWITCH - (1 << 13)
    _, part = _softmax(g, (e0, e1), True, False, True)
    _exact(g, "(%d, %d) CSR input" % (e0, e1), part[e0:e1], g["want"][e0:e1], g["row_csr"][e0:e1])
