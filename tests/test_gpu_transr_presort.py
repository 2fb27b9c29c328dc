"""The KG phase's presort (kgat_transr_presort_f32: the one-workgroup LDS sort of kgat_lds_sort.h under
small_sort_body's key load and epilogue) against numpy, exactly: a stable sort's output is unique, so every array of a
batch's block has one right value.  Each case is ONE launch over two different batches (the per-batch block stride is
exercised too); the blocks are decoded with the layout restated in tests/_transr_ref.py.

The shapes are the smallest at which the sort takes another path: one key; either side of one 64-key ballot step and of
the per-wavefront slice growing from 64 to 128 keys; the capacity (8,190 ids) with two and three 9-bit passes of the
32-bit packing, the first id width of the 64-bit packing (8-bit digits), and 31-bit ids (four passes) with 4,096
relations - the chunk table in which no thread owns key n_rel."""
import numpy as np
import pytest
import torch

import _transr_ref as T

CASES = [(50, 1, 1), (1000, 7, 21), (1000, 7, 22), (5000, 41, 341), (5000, 41, 342), (1 << 18, 300, 2730),
         (1 << 19, 300, 2730), ((1 << 19) + 1, 300, 2730), ((1 << 31) - 2, 4096, 2730)]
PLANTED_RUNS = (64, 65, 128, 129)   # relations with exactly these many samples: the chunk boundaries


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def presort_batch(n_nodes, n_rel, batch, seed):
    """h, r, pos_t, neg_t (int64 numpy) of one batch.  Ids: drawn over all of [0, n_nodes) (the high bits are used) from
    a pool of half as many ids as places (runs of equal ids), with 0 and n_nodes - 1 among them and one hub id of up to
    400 occurrences across the three roles.  Relations: as many of PLANTED_RUNS as the batch and n_rel allow, on relations
    spread over the range, with exactly that many samples; the other samples on the other relations, the first and the
    last among them."""
    rng = np.random.default_rng(seed)
    n_ids = 3 * batch
    pool = rng.integers(0, n_nodes, max(1, n_ids // 2))
    ids = rng.choice(pool, n_ids)
    places = rng.permutation(n_ids)
    ids[places[:2]] = (0, n_nodes - 1)
    ids[places[2:2 + min(400, n_ids // 5)]] = int(rng.integers(n_nodes // 2, n_nodes))
    ids = ids.reshape(batch, 3)

    planted = {}
    spread = np.unique(np.linspace(1, n_rel - 2, len(PLANTED_RUNS)).astype(np.int64)) if n_rel >= 6 else []
    for rel, run in zip(spread, PLANTED_RUNS):
        if sum(planted.values()) + run <= batch:
            planted[int(rel)] = run
    others = np.setdiff1d(np.arange(n_rel), list(planted))
    rest = batch - sum(planted.values())
    r = rng.choice(others, rest)
    if rest >= 2:
        r[:2] = (0, n_rel - 1)
    r = rng.permutation(np.concatenate([r] + [np.full(run, rel) for rel, run in planted.items()]))
    for rel, run in planted.items():
        assert int((r == rel).sum()) == run
    return ids[:, 0].copy(), r.astype(np.int64), ids[:, 1].copy(), ids[:, 2].copy()


def test_the_builder_plants_what_the_cases_are_for():
    for n_nodes, n_rel, batch in CASES:
        for seed in (1, 2):
            h, r, p, n = presort_batch(n_nodes, n_rel, batch, seed)
            ids = np.stack([h, p, n], 1).reshape(-1)
            assert r.size == batch and r.min() >= 0 and r.max() < n_rel
            assert ids.min() == 0 and ids.max() == n_nodes - 1
            if batch >= 2:
                assert r.min() == 0 and r.max() == n_rel - 1
            if batch == 2730:
                counts = np.bincount(r, minlength=n_rel)
                assert sorted(c for c in counts if c in PLANTED_RUNS) == list(PLANTED_RUNS)
                hub, runs = np.unique(ids, return_counts=True)
                assert runs.max() >= 400 and all((col == hub[runs.argmax()]).any() for col in (h, p, n))
    assert np.bincount(presort_batch(5000, 41, 342, 1)[1]).tolist().count(128) >= 1   # 64 + 65 + 128 fit in 342


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,n_rel,batch", CASES)
def test_presort_blocks_equal_numpy(dev, n_nodes, n_rel, batch):
    from dgl_kgat_amd import ops
    batches = [presort_batch(n_nodes, n_rel, batch, seed) for seed in (1, 2)]
    assert any(not np.array_equal(a, b) for a, b in zip(*batches))
    h, r, pos_t, neg_t = (torch.as_tensor(np.stack([b[i] for b in batches]), dtype=torch.int32, device=dev)
                          for i in range(4))
    out, stride = ops.transr_presort(h, r, pos_t, neg_t, n_nodes, n_rel)
    blocks = out.cpu().numpy()
    assert stride == T.sorted_block_layout(batch, n_rel)[1] and blocks.size == 2 * stride
    for j, b in enumerate(batches):
        got = T.decode_sorted_block(blocks[j * stride:(j + 1) * stride], batch, n_rel)
        want = T.presort_expected(*b, n_rel)
        total = int(want.chunk_ptr[n_rel])
        assert total <= T.max_chunks(batch, n_rel)
        for name, g, w in (("order", got.order, want.order), ("seg", got.seg[:n_rel + 1], want.seg),
                           ("chunk_ptr", got.chunk_ptr[:n_rel + 1], want.chunk_ptr),
                           ("chunks", got.chunks[:total], want.chunks), ("sorted_ids", got.sorted_ids, want.sorted_ids),
                           ("row_order", got.row_order, want.row_order), ("inv_pos", got.inv_pos, want.inv_pos),
                           ("run_len", got.run_len, want.run_len)):
            assert np.array_equal(g, w), (name, "batch %d" % j, n_nodes, n_rel, batch)
