"""TransR link prediction, the host side (no GPU): the ABI, the argument refusals, KnownTriples, the metric arithmetic,
the harness flags and the reference module of the device tests against a literal loop."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _kg_rank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("kgat_transr_project_supported", "kgat_transr_project_f32", "kgat_transr_rank_supported",
               "kgat_transr_rank_f32")


def _lib():
    from dgl_kgat_amd import _lib
    return _lib


def test_header_declares_the_entries_at_abi_16_and_the_library_exports_them():
    lib = _lib()
    with open(lib.HEADER) as fh:
        text = fh.read()
    assert re.search(r"#define\s+KGAT_ABI_VERSION\s+16\b", text)
    assert lib.ABI_VERSION == 16
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES, name
    assert "kgat_transr_rank.hip" in lib.SOURCES
    lib.build()
    so = ctypes.CDLL(lib.SO_PATH)       # (symbol lookup only: nothing is called)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name


def test_supported_widths():
    so = ctypes.CDLL(_lib().build())
    for d in (8, 16, 24, 32, 64, 100, 128, 256):
        for k in (16, 48, 128):
            want = int(d in (16, 32, 64, 128) and k in (16, 32, 64, 128))
            assert so.kgat_transr_project_supported(d, k) == want, (d, k)
        assert so.kgat_transr_rank_supported(d) == int(d in (16, 32, 64, 128)), d


def _rank_args(n_q=3, n_c=10, k=16, c0=0):
    Q, P = torch.zeros(n_q, k), torch.zeros(n_c, k)
    return dict(Q=Q, t=torch.full((n_q,), c0, dtype=torch.int32), P=P, n2=torch.zeros(n_c), c0=c0,
                filter_ptr=torch.zeros(n_q + 1, dtype=torch.int32), filter_ids=torch.zeros(0, dtype=torch.int32))


def test_transr_rank_refusals():
    from dgl_kgat_amd import ops
    ok = _rank_args()
    with pytest.raises(ops.KGATLibraryError):       # everything in order but the device: no CPU implementation
        ops.transr_rank(**ok)
    for name, dtype in (("Q", torch.float64), ("P", torch.float16), ("n2", torch.float64), ("t", torch.int64),
                        ("filter_ptr", torch.int64), ("filter_ids", torch.int64)):
        with pytest.raises(TypeError, match=name):
            ops.transr_rank(**{**ok, name: ok[name].to(dtype)})
    with pytest.raises(TypeError):
        ops.transr_rank(**{**ok, "Q": np.zeros((3, 16), np.float32)})
    for bad in ({"P": torch.zeros(10, 32)}, {"n2": torch.zeros(9)}, {"t": torch.zeros(4, dtype=torch.int32)},
                {"Q": torch.zeros(3 * 16)}, {"filter_ptr": torch.zeros(3, dtype=torch.int32)},
                {"Q": torch.zeros(0, 16), "t": torch.zeros(0, dtype=torch.int32), "filter_ptr": torch.zeros(1, dtype=torch.int32)},
                {"c0": -1}):
        with pytest.raises(ValueError):
            ops.transr_rank(**{**ok, **bad})
    # t outside the candidate range, on either end and with c0 > 0
    for t, c0 in (([0, 10, 0], 0), ([0, -1, 0], 0), ([5, 4, 6], 5), ([5, 15, 6], 5)):
        with pytest.raises(IndexError, match="outside the candidate range"):
            ops.transr_rank(**{**_rank_args(c0=c0), "t": torch.tensor(t, dtype=torch.int32)})
    # filters: unsorted inside a query, a repeat, a pointer that decreases, one that does not end at the length
    ids = lambda *x: torch.tensor(x, dtype=torch.int32)     # noqa: E731
    with pytest.raises(ValueError, match="sorted"):
        ops.transr_rank(**{**ok, "filter_ptr": ids(0, 3, 3, 4), "filter_ids": ids(1, 5, 2, 0)})
    with pytest.raises(ValueError, match="sorted"):
        ops.transr_rank(**{**ok, "filter_ptr": ids(0, 2, 2, 2), "filter_ids": ids(4, 4)})
    with pytest.raises(ValueError, match="filter_ptr"):
        ops.transr_rank(**{**ok, "filter_ptr": ids(0, 2, 1, 3), "filter_ids": ids(1, 2, 3)})
    with pytest.raises(ValueError, match="filter_ptr"):
        ops.transr_rank(**{**ok, "filter_ptr": ids(0, 1, 1, 2), "filter_ids": ids(1, 2, 3)})
    # a descent where a new query's list begins is in order: only the device is missing
    with pytest.raises(ops.KGATLibraryError):
        ops.transr_rank(**{**ok, "filter_ptr": ids(0, 2, 2, 4), "filter_ids": ids(3, 7, 1, 2)})


def test_transr_project_refusals():
    from dgl_kgat_amd import ops
    ent, W = torch.zeros(10, 16), torch.zeros(16, 32)
    with pytest.raises(ops.KGATLibraryError):
        ops.transr_project(ent, W)
    with pytest.raises(ValueError):
        ops.transr_project(ent, torch.zeros(8, 32))
    with pytest.raises(ValueError):
        ops.transr_project(ent, W, sign=0.5)
    with pytest.raises(ValueError):
        ops.transr_project(ent, W, ids=torch.zeros(2, dtype=torch.int32), rows=(0, 2))
    with pytest.raises(TypeError):
        ops.transr_project(ent, W, ids=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(IndexError):
        ops.transr_project(ent, W, ids=torch.tensor([0, 10], dtype=torch.int32))
    with pytest.raises(IndexError):
        ops.transr_project(ent, W, rows=(3, 11))
    with pytest.raises(TypeError):
        ops.transr_project(ent.double(), W.double())


def _cpu_model(N=60, d=8, k=8, seed=0):
    import dgl_kgat_amd as K
    torch.manual_seed(seed)
    return K.KGATPropagation(N, R.N_REL, input_node_dim=d, relation_dim=k, num_gnn_layers=1, n_hidden=8, dropout=0.0)


def test_kg_eval_refusals():
    import dgl_kgat_amd as K
    model = _cpu_model()
    h, r, t = [1, 2], [0, 1], [3, 4]
    for fn in (model.kg_rank, model.kg_metrics):
        with pytest.raises(ValueError, match="side"):
            fn(h, r, t, side="left")
    with pytest.raises(ValueError):
        model.kg_rank(h, r, [3])
    with pytest.raises(IndexError):
        model.kg_rank(h, r, [3, 60])
    with pytest.raises(IndexError, match="candidate range"):
        model.kg_rank(h, r, t, candidates=(4, 20))
    with pytest.raises(ValueError):
        model.kg_rank(h, r, t, candidates=(20, 20))
    with pytest.raises(K.KGATLibraryError, match="128"):
        model.kg_complete(h, r, 129)
    with pytest.raises(K.KGATLibraryError):
        model.kg_complete(h, r, 0)
    with pytest.raises(K.KGATLibraryError, match="HIP"):     # the top-K sweep has no CPU form
        model.kg_complete(h, r, 5)
    known = K.KnownTriples(h, r, t, 60, R.N_REL)
    with pytest.raises(ValueError, match="side"):
        known.lists((h, r), "both")
    with pytest.raises(IndexError):
        K.KnownTriples([60], [0], [1], 60, R.N_REL)


def test_known_triples_against_a_dict():
    import dgl_kgat_amd as K
    rng = np.random.default_rng(1)
    N, n_rel = 40, 3
    trip = np.stack([rng.integers(0, N, 400), rng.integers(0, n_rel, 400), rng.integers(0, N, 400)], 1)
    trip = np.concatenate([trip, trip[:50]])                       # duplicates
    known = K.KnownTriples(trip[:, 0], trip[:, 1], trip[:, 2], N, n_rel)
    assert known.n_triples == len(np.unique(trip, axis=0))
    tails, heads = {}, {}
    for h, r, t in trip:
        tails.setdefault((h, r), set()).add(t)
        heads.setdefault((t, r), set()).add(h)
    e = np.concatenate([rng.integers(0, N, 64), [0, N - 1]])
    r = np.concatenate([rng.integers(0, n_rel, 64), [n_rel - 1, 0]])
    for side, want in (("tail", tails), ("head", heads)):
        for rng_ in (None, (10, 25)):
            ptr, ids = known.lists((e, r), side, id_range=rng_)
            assert ptr.dtype == torch.int32 and ids.dtype == torch.int32 and ptr[0] == 0 and ptr[-1] == len(ids)
            for j, key in enumerate(zip(e, r)):
                exp = sorted(x for x in want.get(key, ()) if rng_ is None or rng_[0] <= x < rng_[1])
                assert ids[ptr[j]:ptr[j + 1]].tolist() == exp, (side, key)
    ptr, ids = known.lists(([], []), "tail")
    assert ptr.tolist() == [0] and ids.numel() == 0


def test_metric_arithmetic():
    from dgl_kgat_amd import kg_eval
    lt, eq = [0, 2, 0, 9, 30], [0, 0, 2, 1, 0]
    ranks = [1.0, 3.0, 2.0, 10.5, 31.0]
    m = kg_eval.metrics_from_counts(lt, eq, hits=(1, 3, 10))
    want = R.metrics_ref(ranks, (1, 3, 10))
    assert m.keys() == want.keys() == {"mr", "mrr", "hits@1", "hits@3", "hits@10", "n"}
    for key in want:
        assert m[key] == pytest.approx(want[key], rel=1e-15), key
    assert m["hits@1"] == 0.2 and m["hits@3"] == 0.6 and m["hits@10"] == 0.6 and m["n"] == 5
    with pytest.raises(ZeroDivisionError):
        kg_eval.metrics_from_ranks([])


def test_both_sides_average_and_ranks_follow_the_loop():
    """kg_rank's torch form (the CPU / odd-width path) against the literal loop, and "both" = the two sides pooled."""
    import dgl_kgat_amd as K
    model = _cpu_model().double()        # float64: the counts are the loop's, exactly
    rng = np.random.default_rng(2)
    N = 60
    trip = np.stack([rng.integers(0, N, 150), rng.integers(0, R.N_REL, 150), rng.integers(0, N, 150)], 1)
    trip[trip[:, 1] == 3, 1] = 2                                    # relation 3: no triple at all
    known = K.KnownTriples(trip[:, 0], trip[:, 1], trip[:, 2], N, R.N_REL)
    q = trip[rng.choice(len(trip), 24, replace=False)]
    kset = {tuple(x) for x in trip.tolist()}
    p = [x.detach().numpy() for x in (model.entity_embed.weight, model.W_R, model.relation_embed.weight)]
    pooled = []
    for side in ("tail", "head"):
        for cand in (None, (0, N), (5, N)):
            lo, hi = cand or (0, N)
            ans = q[:, 2] if side == "tail" else q[:, 0]
            sel = q[(ans >= lo) & (ans < hi)]
            got = model.kg_rank(sel[:, 0], sel[:, 1], sel[:, 2], known=known, side=side, candidates=cand)
            lt, eq = R.loop_counts(*p, sel.tolist(), kset, side, lo, hi)
            assert got.lt.tolist() == lt and got.eq.tolist() == eq, (side, cand)
            assert got.rank.dtype == torch.float64
            assert got.rank.tolist() == [1 + a + b / 2 for a, b in zip(lt, eq)]
            if cand is None:
                pooled += got.rank.tolist()
        unfiltered = model.kg_rank(q[:, 0], q[:, 1], q[:, 2], side=side)
        assert (unfiltered.lt >= model.kg_rank(q[:, 0], q[:, 1], q[:, 2], known=known, side=side).lt).all()
    both = model.kg_metrics(q[:, 0], q[:, 1], q[:, 2], known=known, side="both", hits=(1, 5), batch=7)
    want = R.metrics_ref(pooled, (1, 5))
    assert both["n"] == 48
    for key in want:
        assert both[key] == pytest.approx(want[key], rel=1e-12), key
    # read, not differentiated
    out = model.kg_rank(q[:, 0], q[:, 1], q[:, 2])
    assert not out.rank.requires_grad and model.entity_embed.weight.grad is None


def test_reference_module_against_the_loop():
    """(Exercises tests/_kg_rank_ref.py alone - the reference the device tests lean on - so unlike the other tests of this
    file it does not depend on the package's new entry points.)"""
    rng = np.random.default_rng(4)
    N, d, k = 30, 6, 5
    ent, W_R, rel = rng.normal(size=(N, d)), rng.normal(size=(2, d, k)), rng.normal(size=(2, k))
    ent[7] = 0.0                                                    # a zero row: norm clamp
    trip = [(1, 0, 2), (7, 1, 3), (4, 0, 7), (5, 1, 5)]
    kset = {(1, 0, 9), (1, 0, 2), (8, 1, 3), (4, 0, 6)}
    for side in ("tail", "head"):
        for lo, hi in ((0, N), (2, 20)):
            lts, eqs = R.loop_counts(ent, W_R, rel, trip, kset, side, lo, hi)
            for j, (h, r, t) in enumerate(trip):
                anchor, ans = (h, t) if side == "tail" else (t, h)
                if not lo <= ans < hi:          # (the answer must be a candidate)
                    continue
                S = R.direct_scores(ent, W_R[r], rel[r], [anchor], side, lo, hi)
                exc = np.zeros(S.shape, bool)
                for c in range(lo, hi):
                    exc[0, c - lo] = ((h, r, c) if side == "tail" else (c, r, t)) in kset
                lt, eq = R.brute_counts(S, np.array([ans - lo]), exc)
                assert (int(lt[0]), int(eq[0])) == (lts[j], eqs[j]), (side, lo, hi, j)
                b_lo, b_hi = R.band(S, np.array([ans - lo]), exc, 0.0)
                assert b_lo[0] == lt[0] and b_hi[0] == lt[0] + eq[0]
                w_lo, w_hi = R.band(S, np.array([ans - lo]), exc, 100.0)
                assert w_lo[0] == 0 and w_hi[0] == (~exc[0]).sum() - (0 if exc[0, ans - lo] else 1)
    # the projection: against the definition, the zero row, the kernel's identity against the direct form
    out, n2, S = R.project_ref(ent, W_R[0], rel[0], -1.0, ids=[7, 3])
    ur = rel[0] / np.linalg.norm(rel[0])
    a = ent[3] @ W_R[0]
    assert np.array_equal(out[0], -ur) and n2[0] == 0.0 and S[0] == 1.0
    assert np.allclose(out[1], a / np.linalg.norm(a) - ur, rtol=0, atol=1e-15) and abs(n2[1] - 1) < 1e-15 and S[1] >= 1
    q, _, _ = R.project_ref(ent, W_R[1], rel[1], 1.0, ids=[4])
    p, pn2, _ = R.project_ref(ent, W_R[1], rows=(2, 20))
    direct = R.direct_scores(ent, W_R[1], rel[1], [4], "tail", 2, 20)
    assert np.allclose(pn2 - 2 * p @ q[0] + (q[0] ** 2).sum(), direct[0], rtol=0, atol=1e-13)


@pytest.mark.parametrize("N", R.E2E_SIZES)
def test_the_band_is_narrow_and_holds_the_fp32_torch_form(N):
    """The cap of the device test, checked here first: on these graphs the band is open for at most 2 % of the queries,
    and kg_rank's fp32 torch form (the identity n2 - 2 q.p, as the kernel) lies inside it."""
    import dgl_kgat_amd as K
    d, k = (64, 32) if N == 300 else (16, 16)
    trip, items = R.random_ckg(N, d, k)
    model = R.make_model(K, N, d, k, "cpu")
    known = K.KnownTriples(trip[:, 0], trip[:, 1], trip[:, 2], N, R.N_REL)
    for side in ("tail", "head"):
        for items_only in (False, True):
            case = R.e2e_case(N, d, k, side, items_only)
            print("N %d %s items_only %d: tau %.3e (restatement %.3e), band open for %.2f %% of %d queries"
                  % (N, side, items_only, case.tau, case.restatement_err, 100 * case.open_share, len(case.triples)))
            assert case.open_share <= R.BAND_CAP
            assert R.TAU_FLOOR <= case.tau < 1e-4
            assert (case.triples[:, 1] < R.N_REL - 1).all() and len(np.unique(case.triples[:, 1])) == R.N_REL - 1 - \
                (0 if not items_only else (1 if side == "tail" else 2))
            q = case.triples
            got = model.kg_rank(q[:, 0], q[:, 1], q[:, 2], known=known, side=side,
                                candidates=(case.lo, case.hi) if items_only else None)
            R.check_band(case, got.lt.numpy(), got.eq.numpy())
            if N == 300:    # true answers placed at random: the cap holds at this size too
                rnd = R.e2e_case(N, d, k, side, items_only, False)
                trip_r, _ = R.random_ckg(N, d, k, False)
                known_r = K.KnownTriples(trip_r[:, 0], trip_r[:, 1], trip_r[:, 2], N, R.N_REL)
                q = rnd.triples
                got = model.kg_rank(q[:, 0], q[:, 1], q[:, 2], known=known_r, side=side,
                                    candidates=(rnd.lo, rnd.hi) if items_only else None)
                assert rnd.open_share <= R.BAND_CAP and np.median(rnd.lt_lo) > (rnd.hi - rnd.lo) / 5
                R.check_band(rnd, got.lt.numpy(), got.eq.numpy())


def _harness():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    return train_kgat


def test_harness_flags_parse():
    tk = _harness()
    args = tk.parse_args([])
    assert args.kg_eval == 0 and args.kg_holdout == 0.0
    args = tk.parse_args(["--kg_eval", "500", "--kg_holdout", "0.1"])
    assert args.kg_eval == 500 and args.kg_holdout == 0.1
    for bad in (["--kg_eval", "-1"], ["--kg_holdout", "1.0"], ["--kg_holdout", "-0.1"], ["--kg_holdout", "0.1"],
                ["--kg_eval", "10", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            tk.parse_args(bad)


def test_kg_holdout_takes_reverse_twins_and_no_interaction():
    tk = _harness()
    rng = np.random.default_rng(0)
    n_users, n_ent = 10, 50
    kg = np.stack([rng.integers(n_users, n_ent, 300), rng.integers(0, 2, 300), rng.integers(n_users, n_ent, 300)], 1)
    kg = np.unique(kg, axis=0)
    inverse = kg[:, [2, 1, 0]].copy()
    inverse[:, 1] += 2                                  # relations 2, 3: the inverses of 0, 1
    inter = np.stack([rng.integers(0, n_users, 80), np.full(80, 4), rng.integers(n_users, 30, 80)], 1)
    inter_inv = inter[:, [2, 1, 0]].copy()
    inter_inv[:, 1] = 5
    trip = np.concatenate([kg, inverse, inter, inter_inv])
    trip = trip[rng.permutation(len(trip))]
    is_inter = np.isin(trip[:, 1], (4, 5))
    keep = tk.kg_holdout_mask(trip, is_inter, 0.25, seed=3)
    assert keep.dtype == bool and keep.shape == (len(trip),)
    assert keep[is_inter].all()                                         # never an interaction triple
    held = trip[~keep]
    assert 0.2 * (~is_inter).sum() <= len(held) <= 0.3 * (~is_inter).sum() + 2
    for h, r, t in held:                                                # no twin (t, ., h) left behind
        twin = (trip[:, 0] == t) & (trip[:, 2] == h) & ~is_inter
        assert not keep[twin].any(), (h, r, t)
    assert np.array_equal(keep, tk.kg_holdout_mask(trip, is_inter, 0.25, seed=3))       # fixed by the seed
    assert tk.kg_holdout_mask(trip, is_inter, 0.0, seed=3).all()
