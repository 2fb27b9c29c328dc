"""``kgat_edge_softmax_permuted_f32`` - the sweep, the permutation's bin pass with the cut-row rescale folded in, the
place pass - against the two calls it stands for: ``ops.edge_softmax(..., want_csr=True)`` followed by ``ops.permute``
on the same inputs.  Both results, the CSR-ordered weights and their edge-id-ordered copy, must be the same BITS
(``torch.equal`` on int32 views), and every non-empty row must sum to one at the tolerance of
``test_edge_softmax_vs_oracle`` (``allclose(sums, 1, atol=1e-5)``).

T = ``kgat_permute_tile()`` = 16,384 positions: a chunk of the bin pass, 32 ranges of the sweep's 512-position form, 16
of its 1,024-position form.  The graphs are CSRs built from a list of row lengths, edge ids a seeded permutation:

    boundaries        E = 3 T + 777 (last range 265 positions, last chunk ragged, a last thread with 1 of 8 items):
                      a hub of 40,000 positions from position 300 (two chunk boundaries, 78 followers: two blocks of
                      sm_chain_total), rows of 511 / 512 / 513 across range boundaries, a row that is exactly one
                      range (never cut), one that is exactly two (cut in the middle only), a row that ends on a chunk
                      boundary, single-edge rows, rows without edges
    no cut rows       E = 200, one partial range
    single-edge rows  E = T, every row one edge: no factor is ever applied
    EPL = 16          E = (8 << 20) + 4,133 with Zipf row lengths: 1,024-position ranges, 16 per chunk

each with logits N(0, 1) and 30 N(0, 1) (maxima far apart between ranges, terms flushed to zero), fed in CSR order
and through a random position map (the grouped-order input of compute_attention).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _boundaries_lens(T):
    """Row lengths of the "boundaries" case; the positions named in the module docstring are asserted."""
    rng = np.random.default_rng(11)
    lens = []
    for i in range(100):                       # single-edge rows and rows without edges: positions 0 .. 100
        lens += [1, 0] if i % 3 == 0 else [1]
    lens += [200]                              # .. 300
    hub = len(lens)
    lens += [40000]                            # 300 .. 40,300
    lens += [148]                              # .. 40,448 = 79 * 512: ends on a range boundary
    one_range = len(lens)
    lens += [512]                              # 40,448 .. 40,960: exactly one range, never cut
    lens += [1024]                             # .. 41,984: exactly two ranges
    lens += [100, 511, 512, 513]               # 42,084 .. 42,595 .. 43,107 .. 43,620: across 83 * 512, 84 * 512, 85 * 512
    lens += [1, 0, 0, 1] * 25                  # .. 43,670
    fill = 48000 - 43670
    small = []
    while sum(small) < fill:
        small.append(int(rng.integers(1, 41)))
    small[-1] -= sum(small) - fill
    lens += [x for x in small if x > 0]        # .. 48,000
    to_chunk = len(lens)
    lens += [3 * T - 48000]                    # .. 3 T: ends on a chunk boundary, across two range boundaries
    lens += [600, 0, 100] + [1, 0] * 77        # .. 3 T + 777: the row of 600 across 97 * 512
    lens = np.asarray(lens, dtype=np.int64)
    ip = np.concatenate([[0], np.cumsum(lens)])
    assert T == 16384 and ip[-1] == 3 * T + 777 and (3 * T + 777) % 512 == 265
    assert ip[hub] == 300 and ip[hub + 1] == 40300 and (40300 - 1) // 512 - 300 // 512 == 78
    assert ip[one_range] == 79 * 512 and ip[one_range + 1] == 80 * 512 and ip[one_range + 2] == 82 * 512
    assert ip[to_chunk + 1] == 3 * T and ip[to_chunk] % 512 != 0
    for k, L in ((83, 511), (84, 512), (85, 513)):
        r = int(np.searchsorted(ip, k * 512, side="right")) - 1
        assert lens[r] == L and ip[r] < k * 512 < ip[r + 1]
    return lens


def _zipf_lens(e):
    rng = np.random.default_rng(12)
    lens = np.minimum(rng.zipf(1.3, size=e // 4), 300000).astype(np.int64)
    lens = lens[: int(np.searchsorted(np.cumsum(lens), e)) + 1]
    lens[-1] -= lens.sum() - e
    assert lens.sum() == e and lens.min() >= 1 and lens.max() > 65536
    return lens


def _lens(case, T):
    if case == "boundaries":
        return _boundaries_lens(T)
    if case == "no cut rows":
        return np.asarray([50, 0, 1, 149], dtype=np.int64)
    if case == "single-edge rows":
        return np.ones(T, dtype=np.int64)
    return _zipf_lens((8 << 20) + 4133)


class Graph:
    """CSR arrays on the device, the plan of CSR position -> edge id, and the logits of both scales in both orders."""

    def __init__(self, case, dev):
        from dgl_kgat_amd import ops
        lens = _lens(case, ops.permute_tile())
        e, n = int(lens.sum()), len(lens)
        rng = np.random.default_rng(13)
        eid = rng.permutation(e).astype(np.int32)                 # edge id of every CSR position
        csr_pos = np.empty(e, dtype=np.int32)
        csr_pos[eid] = np.arange(e, dtype=np.int32)               # out[i] = in[csr_pos[i]]
        gmap = rng.permutation(e).astype(np.int32)                # grouped position of every CSR position
        self.e, self.n = e, n
        self.nonempty = torch.as_tensor(lens > 0, device=dev)
        self.indptr = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=dev)
        self.row_of = torch.as_tensor(np.repeat(np.arange(n, dtype=np.int32), lens), device=dev)
        self.eid = torch.as_tensor(eid, device=dev)
        self.gmap = torch.as_tensor(gmap, device=dev)
        self.plan = ops.permute_plan(torch.as_tensor(csr_pos, device=dev))
        self.logits = {}
        for scale in (1.0, 30.0):
            x = (rng.standard_normal(e) * scale).astype(np.float32)   # CSR order
            xg = np.empty_like(x)
            xg[gmap] = x
            self.logits[scale] = (torch.as_tensor(x, device=dev), torch.as_tensor(xg, device=dev))


@pytest.fixture(scope="module", params=["boundaries", "no cut rows", "single-edge rows", "EPL = 16"])
def graph(request, dev):
    return Graph(request.param, dev)


@pytest.mark.parametrize("order", ["csr", "grouped"])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_same_bits_as_softmax_then_permute(graph, scale, order):
    from dgl_kgat_amd import ops
    g = graph
    assert ops.edge_softmax_permuted_supported(g.e)
    x, xg = g.logits[scale]
    logits, index, in_csr = (x, g.eid, True) if order == "csr" else (xg, g.gmap, False)
    _, ref_csr = ops.edge_softmax(g.indptr, g.row_of, index, logits, in_csr_order=in_csr, want_out=False, want_csr=True)
    ref = ops.permute(g.plan, ref_csr)
    assert torch.equal(ref[g.eid.long()], ref_csr)                # (the plan is the permutation CSR position -> edge id)
    got, got_csr = ops.edge_softmax_permuted(g.indptr, g.row_of, index, logits, g.plan, in_csr_order=in_csr)
    torch.cuda.synchronize()
    diff = int((got_csr.view(torch.int32) != ref_csr.view(torch.int32)).sum())
    print("    E = %d, %d CSR-ordered weights differ" % (g.e, diff))
    assert torch.equal(got_csr.view(torch.int32), ref_csr.view(torch.int32))
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # row sums from fp64 prefix sums over the CSR order (8.4e6 terms below one: ~1e-9 per difference)
    cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=x.device), got_csr.double().cumsum(0)])
    sums = (cs[g.indptr[1:].long()] - cs[g.indptr[:-1].long()])[g.nonempty].cpu().numpy()
    print("    largest |row sum - 1| = %.2e" % np.abs(sums - 1.0).max())
    assert np.allclose(sums, 1.0, atol=1e-5)


def _call(lib, g, e0, e1, logits, out, out_csr, tmp, ws):
    from dgl_kgat_amd.ops import _stream
    return lib.kgat_edge_softmax_permuted_f32(g.n, e0, e1, g.indptr.data_ptr(), g.row_of.data_ptr(), g.eid.data_ptr(),
                                              logits.data_ptr(), 1, g.plan.slot_a.data_ptr(), g.plan.dst_a.data_ptr(),
                                              g.plan.slot_b.data_ptr(), out.data_ptr(), out_csr.data_ptr(), tmp.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream(logits))


def test_refusals_launch_nothing(dev):
    """A misaligned array, a first position above zero and a size beyond the permutation's limit: the unsupported code,
    and the outputs as they were."""
    from dgl_kgat_amd import _lib, ops
    lib = _lib.load()
    g = Graph("no cut rows", dev)
    e, T = g.e, ops.permute_tile()
    x = g.logits[1.0][0]
    ws = torch.empty(int(lib.kgat_edge_softmax_workspace_bytes(g.n, e)) + 256, dtype=torch.uint8, device=dev)
    bufs = [torch.full((e + 4,), -7.0, device=dev) for _ in range(3)]
    out, out_csr, tmp = (b[:e] for b in bufs)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((b == -7.0).all()) for b in bufs)

    assert _call(lib, g, 0, e, x, bufs[0][1:e + 1], out_csr, tmp, ws) == UNSUPPORTED and untouched()
    assert _call(lib, g, 0, e, x, out, bufs[1][1:e + 1], tmp, ws) == UNSUPPORTED and untouched()
    assert _call(lib, g, 0, e, x, out, out_csr, bufs[2][1:e + 1], ws) == UNSUPPORTED and untouched()
    assert _call(lib, g, 0, e, x, out, out_csr, tmp, ws[4:]) == UNSUPPORTED and untouched()
    assert b"aligned" in lib.kgat_last_error()
    assert lib.kgat_edge_softmax_permuted_supported(4, e) == 0
    assert _call(lib, g, 4, e, x, out, out_csr, tmp, ws) == UNSUPPORTED and untouched()
    beyond = T * T // 16 + 1
    assert lib.kgat_permute_supported(beyond - 1) == 1 and lib.kgat_permute_supported(beyond) == 0
    assert lib.kgat_edge_softmax_permuted_supported(0, beyond - 1) == 1
    assert lib.kgat_edge_softmax_permuted_supported(0, beyond) == 0
    assert _call(lib, g, 0, beyond, x, out, out_csr, tmp, ws) == UNSUPPORTED and untouched()
    # and the same buffers, taken as they are, are written
    assert _call(lib, g, 0, e, x, out, out_csr, tmp, ws) == 0
    _, ref_csr = ops.edge_softmax(g.indptr, g.row_of, g.eid, x, in_csr_order=True, want_out=False, want_csr=True)
    assert torch.equal(out_csr, ref_csr) and torch.equal(out, ops.permute(g.plan, ref_csr))


def test_model_step_same_bits_with_the_switch_on_and_off(dev):
    """compute_attention then gnn on a small amazon-book-shaped CKG: the attention and the readout are the same bits
    whether the eager branch takes the fused entry or the two calls - and each arm takes the one it should.  (Eager
    weights are asked for by switch: a process that opted into the deferred form keeps the two calls, by design.)"""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops, synth
    from dgl_kgat_amd.options import override
    n, trip, n_rel = synth.amazon_book_ckg(scale=0.02)
    torch.manual_seed(3)
    model = K.KGATPropagation(n, n_rel, input_node_dim=64, relation_dim=64, num_gnn_layers=3, n_hidden=64,
                              dropout=0.0).to(dev)
    res = {}
    for on in (True, False):
        g = synth.build_graph(n, trip, dev)
        with override(softmax_permuted=on, eager_edge_weights=True), torch.no_grad(), ops.KernelTimer() as timer:
            a = model.compute_attention(g)
            g.edata["w"] = a
            out = model.gnn(g)
        torch.cuda.synchronize()
        names = {rec[0] for rec in timer.records}
        assert ("edge_softmax_permuted" in names) == on and ("edge_softmax" in names) == (not on), names
        res[on] = (a.clone(), out.clone())
    assert res[True][0].shape == (len(trip), 1)
    assert torch.equal(res[True][0].view(torch.int32), res[False][0].view(torch.int32))
    assert torch.equal(res[True][1].view(torch.int32), res[False][1].view(torch.int32))
