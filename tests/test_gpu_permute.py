"""The planned permutation (kgat_permute_f32: out[i] = in[src_of[i]] as a bin pass and a place pass through LDS over a
static plan) on the MI355X.  The result is a permutation of 32-bit words, so every comparison is bit equality with
torch indexing, ``in[src_of]``, on int32 views.  T = kgat_permute_tile() is the chunk (sources) and block
(destinations) length; the lengths are the smallest that give a partial last chunk / block and more than one of each,
the permutations the ones with the longest and the shortest (chunk, block) runs.  Then the size rule
(kgat_permute_supported), the graph-level caller with its gather fallback, and a small CKG end to end: the attention,
the propagation that follows and the lazy tensor, against the gather they replace."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# NaN with payloads (quiet, signalling, negative), +-inf, -0.0, +0.0, smallest / largest denormal of either sign
SPECIAL_BITS = [0x7FC12345, 0x7F800001, 0xFFC00001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                0x00000001, 0x807FFFFF, 0x007FFFFF, 0x80000001]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from dgl_kgat_amd import ops
    return ops


@pytest.fixture(scope="module")
def T(ops):
    return ops.permute_tile()


def _values(n, dev, seed=5):
    """n floats whose bit patterns are uniformly random words (every class of fp32 occurs), the special ones first."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    k = min(n, len(SPECIAL_BITS))
    bits[:k] = np.array(SPECIAL_BITS[:k], np.uint32)
    return torch.from_numpy(bits.view(np.int32)).to(dev).view(torch.float32)


def _permutation(kind, n, T, dev):
    """src_of (int32, device) of the named permutation, or None where the length does not allow it."""
    i = torch.arange(n, dtype=torch.int64, device=dev)
    if kind == "identity":
        p = i
    elif kind == "reversal":
        p = n - 1 - i
    elif kind == "random":
        g = torch.Generator(device="cpu")
        g.manual_seed(1000 + n)
        p = torch.randperm(n, generator=g).to(dev)
    elif kind == "stride":
        # destinations ordered by (source position mod number of blocks): neighbouring sources of a chunk land in
        # different blocks - the shortest runs the length allows
        n_blk = max((n + T - 1) // T, 1)
        p = torch.argsort(i % n_blk, stable=True)
    elif kind == "chunk_to_block":
        # cyclic shift by T: chunk c + 1 goes whole to block c (the longest run); needs a second chunk
        if n <= T:
            return None
        p = (i + T) % n
    elif kind == "half_shift":
        # cyclic shift by T / 2: every chunk splits half and half between two blocks, every block has two sources
        if n < 4 * T:
            return None
        p = (i + T // 2) % n
    else:
        raise AssertionError(kind)
    return p.to(torch.int32).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lengths(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


KINDS = ("identity", "reversal", "random", "stride", "chunk_to_block")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", range(9))
def test_permute_is_bit_exact(ops, dev, T, which, kind):
    n = _lengths(T)[which]
    src_of = _permutation(kind, n, T, dev)
    if src_of is None:   # chunk_to_block at one chunk is the identity case
        src_of = _permutation("identity", n, T, dev)
    vals = _values(n, dev)
    plan = ops.permute_plan(src_of)
    assert plan.n == n and plan.slot_a.numel() == n and plan.dst_a.numel() == n and plan.slot_b.numel() == n
    out = ops.permute(plan, vals)
    want = _bits(vals)[src_of.long()]
    assert torch.equal(_bits(out), want), (n, kind)
    # determinism, and the caller's own output / scratch buffers
    out2, tmp = torch.full_like(vals, 7.0), torch.empty_like(vals)
    assert ops.permute(plan, vals, out=out2, tmp=tmp) is out2
    assert torch.equal(_bits(out2), _bits(out)), (n, kind, "second call")


@pytest.mark.parametrize("extra", [0, 5])
def test_half_shift_splits_every_chunk_between_two_blocks(ops, dev, T, extra):
    n = 4 * T + extra
    vals = _values(n, dev, seed=9)
    for kind in ("half_shift", "chunk_to_block", "stride"):
        src_of = _permutation(kind, n, T, dev)
        out = ops.permute(ops.permute_plan(src_of), vals)
        assert torch.equal(_bits(out), _bits(vals)[src_of.long()]), (n, kind)


def test_plan_refuses_what_is_no_permutation(ops, dev, T):
    with pytest.raises(ValueError):
        ops.permute_plan(torch.tensor([0, 1, 5], dtype=torch.int32, device=dev))
    with pytest.raises(ops.KGATLibraryError):   # a repeated source: the plan cannot reproduce it
        ops.permute_plan(torch.tensor([0, 1, 1, 3], dtype=torch.int32, device=dev))
    plan = ops.permute_plan(_permutation("random", 100, T, dev))
    with pytest.raises(ValueError):
        ops.permute(plan, torch.zeros(99, device=dev))
    v = torch.zeros(104, device=dev)
    with pytest.raises(ops.KGATLibraryError):   # in off a 16-byte boundary: the entry refuses, the caller below gathers
        ops.permute(plan, v[1:101])


def test_size_rule_and_the_callers_fallback(ops, dev, T):
    from dgl_kgat_amd import _lib
    from dgl_kgat_amd.graph import _Structure
    lib = _lib.load()
    limit = T * T // 16
    if T == 16384:
        assert limit == 16_777_216
    assert ops.permute_supported(0) and ops.permute_supported(1) and ops.permute_supported(limit)
    assert not ops.permute_supported(limit + 1) and not ops.permute_supported(200_000_000) and not ops.permute_supported(-1)
    assert lib.kgat_permute_f32(limit + 1, None, None, None, None, None, None, None) == -2     # KGAT_E_UNSUPPORTED
    assert b"kgat_gather_f32" in lib.kgat_last_error()
    with pytest.raises(ops.KGATLibraryError):
        ops.permute_plan(torch.zeros(limit + 1, dtype=torch.int32, device=dev))
    # the graph-level caller above the rule: the gather's result, and no plan is built
    n = limit + 1
    st = _Structure()
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    src_of = torch.randperm(n, generator=g, device=dev).to(torch.int32)
    vals = torch.arange(n, dtype=torch.int32, device=dev).view(torch.float32)
    out = st.permuted("probe", src_of, vals)
    assert torch.equal(_bits(out), src_of) and torch.equal(_bits(out), _bits(ops.gather(src_of, vals)))
    assert not any(isinstance(k, tuple) and k[0] == "permute_plan" for k in st._cache(dev))


def test_caller_plans_once_and_gathers_unaligned_values(ops, dev, T):
    from dgl_kgat_amd.graph import _Structure
    st, n = _Structure(), 2 * T + 3
    src_of = _permutation("random", n, T, dev)
    vals = _values(n, dev, seed=11)
    want = _bits(vals)[src_of.long()]
    out = st.permuted("probe", src_of, vals)
    c = st._cache(dev)
    plan, tmp = c[("permute_plan", "probe")], c["permute_tmp"]
    assert torch.equal(_bits(out), want)
    out2 = torch.empty_like(vals)
    assert st.permuted("probe", src_of, vals, out=out2) is out2 and torch.equal(_bits(out2), want)
    assert c[("permute_plan", "probe")] is plan and c["permute_tmp"] is tmp          # built once, kept
    # values off a 16-byte boundary, and int32 values: the gather, same result
    shifted = torch.empty(n + 1, dtype=torch.float32, device=dev)[1:]
    shifted.copy_(vals)
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(_bits(st.permuted("probe", src_of, shifted)), want)
    assert torch.equal(st.permuted("probe", src_of, _bits(vals)), want)


@pytest.fixture(scope="module")
def ckg(dev):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth
    n, trip, n_rel = synth.collaborative_kg(100, 150, 120, 4, 12000, 4500, seed=5)   # E = 21,000: two chunks at T = 16,384
    torch.manual_seed(7)
    model = K.KGATPropagation(n, n_rel, input_node_dim=64, relation_dim=64, num_gnn_layers=3, n_hidden=64,
                              dropout=0.0).to(dev)
    return K, model, synth.build_graph(n, trip, dev)


def test_attention_propagation_and_lazy_tensor_on_a_small_ckg(ops, dev, ckg):
    from dgl_kgat_amd import lazy as lazy_mod
    K, model, g = ckg
    st = g._st
    try:
        _check_small_ckg(ops, dev, model, g, st)
    finally:
        lazy_mod._guard_legacy_to_dlpack(install=False)   # (an explicit lazy=True installs the export guard)


def _check_small_ckg(ops, dev, model, g, st):
    with torch.no_grad():
        a = model.compute_attention(g)
        assert ("permute_plan", "csr_pos") in st._cache(dev)            # the planned form ran
        a_csr = st.csr_weights(a)                                      # the CSR-ordered copy kept with the graph
        csr_pos = st.csr_pos(dev)
        want = _bits(a_csr)[csr_pos.long()]
        assert torch.equal(_bits(a).view(-1), want)
        assert torch.equal(_bits(a).view(-1), _bits(ops.gather(csr_pos, a_csr)))
        g.edata["w"] = a
        out = model.gnn(g)
        # the same propagation from weights the gather put into edge-id order: the CSR copy now comes from the
        # edge-id-ordered tensor through the planned csr.eid permutation
        g.edata["w"] = ops.gather(csr_pos, a_csr).view(-1, 1)
        assert torch.equal(_bits(st.csr_weights(g.edata["w"])), _bits(a_csr))
        assert ("permute_plan", "csr_eid") in st._cache(dev)
        assert torch.equal(_bits(model.gnn(g)), _bits(out))
        # the reversed-CSR stream of the SpMM backward through its composed map
        lazy = g.kgat_attention(model._node_embeddings(g), model.W_R, model.relation_embed.weight, lazy=True)
        assert lazy.pending
        rev = st.rev_weights(lazy)
        assert lazy.pending and ("permute_plan", "rev_from_csr") in st._cache(dev)
        rev_eid = st.csr_rev(dev).eid
        assert torch.equal(_bits(rev), want[rev_eid.long()])
        # the lazy tensor materialises to the same bits
        g.edata["w"] = lazy
        assert torch.equal(_bits(model.gnn(g)), _bits(out)) and lazy.pending
        assert torch.equal(_bits(lazy.clone()).view(-1), want) and not lazy.pending
