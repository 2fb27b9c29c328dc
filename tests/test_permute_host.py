"""The planned permutation without a GPU: the plan arithmetic (ops.permute_plan_arrays, plain torch) replayed by a
numpy restatement of the two passes of csrc/kgat_permute.hip, the layout the header promises (tmp ordered by
destination block, then source position; ranks below the tile), and the host-only part of the C ABI (tile, size rule,
argument refusals, which happen before any device work)."""
import numpy as np
import pytest
import torch

from dgl_kgat_amd import _lib, ops


def _two_passes(slot_a, dst_a, slot_b, vals, tile):
    """What the bin pass and the place pass do with a plan, one chunk / block at a time."""
    n = len(vals)
    tmp = np.full(n, -1, np.int64)
    for base in range(0, n, tile):
        cnt = min(tile, n - base)
        lds = np.full(tile, -1, np.int64)
        lds[slot_a[base:base + cnt]] = vals[base:base + cnt]
        tmp[dst_a[base:base + cnt]] = lds[:cnt]
    out = np.full(n, -1, np.int64)
    for base in range(0, n, tile):
        cnt = min(tile, n - base)
        lds = np.full(tile, -1, np.int64)
        lds[slot_b[base:base + cnt]] = tmp[base:base + cnt]
        out[base:base + cnt] = lds[:cnt]
    return tmp, out


def _perms(n, tile):
    i = np.arange(n)
    rng = np.random.default_rng(n + tile)
    yield "identity", i
    yield "reversal", n - 1 - i
    yield "random", rng.permutation(n)
    yield "stride", np.argsort(i % max(-(-n // tile), 1), kind="stable")
    if n > tile:
        yield "shift by a tile", (i + tile) % n
        yield "shift by half a tile", (i + tile // 2) % n


@pytest.mark.parametrize("tile", [8, 64])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 3 * 64 + 17, 4 * 64])
def test_plan_arrays_replayed_on_the_host(n, tile):
    vals = np.arange(n) + 1000
    for name, src_of in _perms(n, tile):
        slot_a, dst_a, slot_b = (t.numpy().astype(np.int64) for t in
                                 ops.permute_plan_arrays(torch.as_tensor(src_of, dtype=torch.int32), tile))
        for a in (slot_a, slot_b):
            assert a.shape == (n,) and (n == 0 or (a.min() >= 0 and a.max() < tile)), name
        assert sorted(dst_a) == list(range(n)), name
        tmp, out = _two_passes(slot_a, dst_a, slot_b, vals, tile)
        assert np.array_equal(out, vals[src_of]), (name, n, tile)
        # tmp is ordered by (destination block, source position); block b owns tmp[b * tile, ...)
        dst_of = np.empty(n, np.int64)
        dst_of[src_of] = np.arange(n)
        src_at = tmp - 1000
        key = (dst_of[src_at] // tile) * n + src_at
        assert np.all(np.diff(key) > 0), name
        assert np.array_equal(dst_of[src_at] // tile, np.arange(n) // tile), name
        # ranks inside a chunk ascend with (destination block, source position) as well
        for base in range(0, n, tile):
            p = np.arange(base, min(base + tile, n))
            k = (dst_of[p] // tile) * n + p
            assert np.array_equal(np.argsort(k), np.argsort(slot_a[p])), name


def test_host_side_of_the_abi():
    lib = _lib.load()
    T = lib.kgat_permute_tile()
    assert T == ops.permute_tile() == 16384                      # one 64 KB LDS image of 32-bit words
    limit = T * T // 16                                          # mean run of one 64-byte sector
    assert lib.kgat_permute_supported(limit) == 1 and lib.kgat_permute_supported(limit + 1) == 0
    assert lib.kgat_permute_supported(3663302) == 1 and lib.kgat_permute_supported(200_000_000) == 0
    assert lib.kgat_permute_supported(0) == 1 and lib.kgat_permute_supported(-1) == 0
    assert lib.kgat_permute_f32(0, None, None, None, None, None, None, None) == 0
    assert lib.kgat_permute_f32(-1, None, None, None, None, None, None, None) == -1 and b"permute" in lib.kgat_last_error()
    assert lib.kgat_permute_f32(5, None, None, None, None, None, None, None) == -1 and b"null" in lib.kgat_last_error()
    P = 1 << 20
    assert lib.kgat_permute_f32(5, P, P, P, P + 4, P + 64, P + 128, None) == -1 and b"aligned" in lib.kgat_last_error()
    assert lib.kgat_permute_f32(5, P, P, P, P + 64, P + 64, P + 128, None) == -1 and b"three buffers" in lib.kgat_last_error()
    assert lib.kgat_permute_f32(limit + 1, P, P, P, P, P + 64, P + 128, None) == -2
    with pytest.raises(ops.KGATLibraryError):                    # no CPU form: the op layer refuses host tensors
        ops.permute(ops.PermutePlan(4, *ops.permute_plan_arrays(torch.arange(4, dtype=torch.int32), T)), torch.zeros(4))
