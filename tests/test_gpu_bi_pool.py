"""The Bi-Interaction pooling kernels (csrc/kgat_bi_pool.hip) on the device: bit-for-bit against the float64 restatement
on inputs whose every intermediate is exact in fp32, within rounding bounds on real-valued inputs, the memory contract
(poisoned outputs, exact-size scratch between guard bands, two calls alike) and the autograd function.

Worst fractions of the bounds measured on MI355X (the printed lines of a run; 1 = the bound): see DESIGN section 27."""
import numpy as np
import pytest
import torch

import _arena
import _bi_pool_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (16, 32, 64, 128)
POISON = 0x7FC0DEAD        # a NaN word


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x if dtype is None else np.asarray(x, dtype)), device=DEV)


_feats = {}


def feats_of(d, hub=False):
    from dgl_kgat_amd.fm_models import FeatureSets
    if (d, hub) not in _feats:
        indptr, ids, _ = R.world(d, hub)
        _feats[(d, hub)] = FeatureSets(indptr, ids, R.N_NODES, device=DEV)
    return _feats[(d, hub)]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def _assert_bits(what, got, want):
    """`got` (a device tensor) has the bits of `want` as float32; a failure names the first elements that differ."""
    a, b = np.ascontiguousarray(got.cpu().numpy(), np.float32), np.ascontiguousarray(want, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a.view(np.int32) != b.view(np.int32))
    assert len(bad) == 0, "%s: %d of %d elements differ; first %s: got %r, want %r" % (
        what, len(bad), a.size, [tuple(i) for i in bad[:4]], [float(a[tuple(i)]) for i in bad[:4]], [float(b[tuple(i)]) for i in bad[:4]])


def _run(d, hub, items, extra, V, w, grads):
    from dgl_kgat_amd import ops
    f = feats_of(d, hub)
    it, ex = dev(items, np.int32), (None if extra is None else dev(extra, np.int32))
    S, bi, lin, sq = ops.bi_pool_fwd(dev(V), None if w is None else dev(w), f, it, ex)
    gV, gw = ops.bi_pool_bwd(dev(V), f, it, ex, S, *[None if g is None else dev(g) for g in grads])
    torch.cuda.synchronize()
    return {"S": S, "bi": bi, "lin": lin, "sq": sq, "grad_V": gV, "grad_w": gw}


def _exact_case(d, n_sets, hub):
    rng = np.random.default_rng(5 * d + n_sets)
    items, extra = R.batch(d, n_sets, hub)
    V, w = R.exact_values(rng, d)
    grads = R.exact_grads(rng, n_sets, d)
    indptr, ids, _ = R.world(d, hub)
    f, ptr = R.set_lists(indptr, ids, items, extra)
    ref = dict(zip(("S", "bi", "lin", "sq"), R.forward(V, w, f, ptr)))
    ref["grad_V"], ref["grad_w"] = R.backward(V, f, ptr, ref["S"], *grads)
    # every intermediate is exact in fp32: the fp32 restatement has the float64 one's bits, and no sum of absolute
    # values comes near 2^24 units of the inputs' grid (1/16 for products of two multiples of 1/4)
    r32 = dict(zip(("S", "bi", "lin", "sq"), R.forward(V, w, f, ptr, np.float32)))
    r32["grad_V"], r32["grad_w"] = R.backward(V, f, ptr, r32["S"], *grads, dtype=np.float32)
    for k in ref:
        assert r32[k].dtype == np.float32 and _bits(r32[k], ref[k].astype(np.float32)) and np.array_equal(r32[k].astype(np.float64), ref[k]), k
    rows = np.abs(V.astype(np.float64))[f]
    A, Q = R._segment_sum(rows, ptr), R._segment_sum(rows * rows, ptr)
    assert (A * A + Q).max() * 16 < 2 ** 24 and Q.sum(1).max() * 16 < 2 ** 24
    assert R.backward_bounds(V, f, ptr, *grads)["abs_terms"].max() * 16 < 2 ** 24
    return items, extra, V, w, grads, ref, (f, ptr)


@pytest.mark.parametrize("n_sets", [1, 3, 257, 2048])
@pytest.mark.parametrize("d", WIDTHS)
def test_exact_inputs_bit_for_bit(d, n_sets):
    """Every list length of _bi_pool_ref.list_lengths(d) with and without an extra, an extra that is in the item's list,
    a multiset item, one item five times across the two halves, a repeated user, extra = -1: S, bi, lin, sq, grad_V and
    grad_w equal the float64 restatement bit for bit, rows no set touches are exactly 0."""
    items, extra, V, w, grads, ref, (f, ptr) = _exact_case(d, n_sets, False)
    if n_sets >= 257:
        lens = set(np.diff(ptr).tolist())
        assert set(R.list_lengths(d)) <= lens, sorted(set(R.list_lengths(d)) - lens)
    got = _run(d, False, items, extra, V, w, grads)
    for k, want in ref.items():
        _assert_bits("%s d=%d n_sets=%d" % (k, d, n_sets), got[k], want)
    untouched = np.bincount(f, minlength=R.N_NODES) == 0      # (2,048 sets reach every feature)
    assert untouched.any() == (n_sets <= 257)
    assert not got["grad_V"].cpu().numpy()[untouched].any() and not got["grad_w"].cpu().numpy()[untouched].any()


@pytest.mark.parametrize("d", WIDTHS)
def test_hub_feature_in_every_item(d):
    """One feature in every item's list, 2,048 sets: its gradient row sums more than 2,048 hits, dealt over the lane
    groups of the 16 wavefronts that share a row of more than 256 sources - bit for bit; the two features at that
    threshold (255 and 256 list entries: one wavefront, sixteen) alike; and optional inputs left out (no extra, no
    w_lin, g_lin and g_sq None) give the same bits as zeros."""
    items, extra, V, w, grads, ref, (f, ptr) = _exact_case(d, 2048, True)
    hits = np.bincount(f, minlength=R.N_NODES)
    assert hits[R.HUB] >= 2048 and hits[R.AT_255] > 100 and hits[R.AT_256] > 100
    rev = np.diff(feats_of(d, True).rev_indptr.cpu().numpy())
    assert rev[R.HUB] > 1024 and rev[R.AT_255] == 255 and rev[R.AT_256] == 256
    got = _run(d, True, items, extra, V, w, grads)
    for k, want in ref.items():
        _assert_bits("%s d=%d hub" % (k, d), got[k], want)
    # the optional pointers
    f0, ptr0 = R.set_lists(*R.world(d, True)[:2], items, None)
    S0, bi0, _, sq0 = R.forward(V, None, f0, ptr0)
    gV0, _ = R.backward(V, f0, ptr0, S0, grads[0], None, None)
    got0 = _run(d, True, items, None, V, None, (grads[0], None, None))
    assert got0["lin"] is None
    for k, want in (("S", S0), ("bi", bi0), ("sq", sq0), ("grad_V", gV0)):
        _assert_bits("%s d=%d hub, optional inputs left out" % (k, d), got0[k], want)
    assert not got0["grad_w"].any()


@pytest.mark.parametrize("d", WIDTHS)
def test_real_valued_inputs_within_rounding_bounds(d):
    """N(0, 1) rows, some scaled by 1e-2 and by 30, 257 sets: per element |bi - bi64| <= (n + 4) 2^-24 ((sum |v|)^2 +
    sum v^2); S, lin, sq within (n + 4) 2^-24 sum |term|; grad_V within (h + n + 4) 2^-24 x the sum of the absolute
    values of its terms (h hits, n the longest set among them).  Prints the worst fraction of each bound."""
    rng = np.random.default_rng(40 + d)
    n_sets = 257
    items, extra = R.batch(d, n_sets)
    V, w = R.real_values(rng, d)
    grads = (rng.standard_normal((n_sets, d)).astype(np.float32), rng.standard_normal(n_sets).astype(np.float32),
             rng.standard_normal(n_sets).astype(np.float32))
    indptr, ids, _ = R.world(d)
    f, ptr = R.set_lists(indptr, ids, items, extra)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in _run(d, False, items, extra, V, w, grads).items()}
    ref = dict(zip(("S", "bi", "lin", "sq"), R.forward(V, w, f, ptr)))
    # the backward is handed the DEVICE's S (as autograd hands it): its bound covers the backward's own rounding
    ref["grad_V"], ref["grad_w"] = R.backward(V, f, ptr, got["S"], *grads)
    bounds = R.forward_bounds(V, w, f, ptr)
    bounds.update(R.backward_bounds(V, f, ptr, *grads))
    worst = {}
    for k in ("S", "bi", "lin", "sq", "grad_V", "grad_w"):
        err, bar = np.abs(got[k] - ref[k]), bounds[k]
        assert np.all(err[bar == 0] == 0), k
        worst[k] = float((err[bar > 0] / bar[bar > 0]).max())
    print("bi_pool d=%d worst fraction of the bound: %s" % (d, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("d, n_sets", [(16, 257), (64, 2048), (128, 3)])
def test_memory_contract(d, n_sets):
    """Outputs poisoned beforehand, the scratch exactly the size asked for between guard bands and poisoned too: the
    bands stay intact, no output word keeps the poison, every row of grad_V and grad_w is written, and the bits are the
    clean pass's - which a second clean pass repeats."""
    from dgl_kgat_amd import ops
    items, extra, V, w, grads, ref, _ = _exact_case(d, n_sets, n_sets == 2048)
    hub = n_sets == 2048
    clean = _run(d, hub, items, extra, V, w, grads)
    again = _run(d, hub, items, extra, V, w, grads)
    for k in clean:
        assert torch.equal(clean[k].view(torch.int32), again[k].view(torch.int32)), k
    for poison in (POISON, 0xC2280000):
        with _arena.patched(ops, poison) as ar:
            got = _run(d, hub, items, extra, V, w, grads)
        torch.cuda.synchronize()
        assert "kgat_bi_pool_fwd_f32" in ar.calls and "kgat_bi_pool_bwd_f32" in ar.calls
        need = ops._lib.load().kgat_bi_pool_scratch_bytes(n_sets, feats_of(d, hub).n_items, R.N_NODES, feats_of(d, hub).n_pairs)
        assert any(g.nbytes == need and g.what.startswith("workspace") for g in ar.guards)
        assert not ar.broken_bands(), ar.broken_bands()
        for k in clean:
            assert torch.equal(clean[k].view(torch.int32), got[k].view(torch.int32)), (k, hex(poison))
            if poison == POISON:
                assert not _arena.poison_words(got[k], poison).any(), k


@pytest.mark.parametrize("d", [16, 64])
def test_autograd_function(d):
    """autograd.bi_pool: outputs and gradients have the bits of the two raw entries, and agree with the torch
    restatement under autograd within the bounds above; CPU tensors and a width outside the envelope take the
    restatement."""
    from dgl_kgat_amd import autograd, fm_models
    rng = np.random.default_rng(90 + d)
    n_sets = 257
    items, extra = R.batch(d, n_sets)
    Vh, wh = R.real_values(rng, d)
    grads = (rng.standard_normal((n_sets, d)).astype(np.float32), rng.standard_normal(n_sets).astype(np.float32),
             rng.standard_normal(n_sets).astype(np.float32))
    raw = _run(d, False, items, extra, Vh, wh, grads)
    f = feats_of(d)
    out = {}
    for name, fn in (("fused", autograd.bi_pool), ("torch", fm_models.bi_pool_torch)):
        V, w = dev(Vh).requires_grad_(), dev(wh).requires_grad_()
        bi, lin, sq = fn(V, w, f, dev(items).long(), dev(extra).long())
        (bi * dev(grads[0])).sum().add((lin * dev(grads[1])).sum()).add((sq * dev(grads[2])).sum()).backward()
        out[name] = {"bi": bi.detach(), "lin": lin.detach(), "sq": sq.detach(), "grad_V": V.grad, "grad_w": w.grad}
    for k, v in out["fused"].items():
        assert torch.equal(v.view(torch.int32), raw[k].view(torch.int32)), k
    indptr, ids, _ = R.world(d)
    fl, ptr = R.set_lists(indptr, ids, items, extra)
    bounds = R.forward_bounds(Vh, wh, fl, ptr)
    bounds.update(R.backward_bounds(Vh, fl, ptr, *grads))
    for k in out["fused"]:
        a, b = out["fused"][k].cpu().numpy().astype(np.float64), out["torch"][k].cpu().numpy().astype(np.float64)
        # (each side is within its bound of float64; the backward's S differs between them by the forward's bound)
        slack = 3.0 if k.startswith("grad") else 2.0
        assert np.all(np.abs(a - b) <= slack * bounds[k] + 1e-30), k
    # a loss that uses bi alone: the unused outputs' gradients arrive as None and take the entry's NULL paths
    only = _run(d, False, items, extra, Vh, wh, (grads[0], None, None))
    V, w = dev(Vh).requires_grad_(), dev(wh).requires_grad_()
    (autograd.bi_pool(V, w, f, dev(items), dev(extra))[0] * dev(grads[0])).sum().backward()
    assert torch.equal(V.grad.view(torch.int32), only["grad_V"].view(torch.int32)) and not w.grad.any()
    # outside the envelope: the restatement, on any device
    f24 = fm_models.FeatureSets([0, 2, 3], [0, 1, 2], 4, device=DEV)
    V24 = torch.randn(4, 24, device=DEV, requires_grad=True)
    bi, lin, sq = autograd.bi_pool(V24, None, f24, torch.tensor([0, 1], device=DEV))
    assert bi.shape == (2, 24) and bi.grad_fn is not None and not lin.any()
    assert torch.allclose(bi[0], V24[0] * V24[1]) and not bi[1].any()
