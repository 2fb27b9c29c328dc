"""Exact ranks of the held-out items, the host side (no GPU): the ABI, the refusals that need no device, and the numpy
restatement the device tests compare with (_rank_ref) against brute force - a stable descending argsort per user, the
places looked up in it and every metric computed straight from its definition."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _rank_ref as R

NEW_SYMBOLS = ("kgat_eval_rank_supported", "kgat_eval_rank_workspace_bytes", "kgat_eval_rank_f32",
               "kgat_eval_rank_metrics_workspace_bytes", "kgat_eval_rank_metrics")
KS = (1, 3, 10, 29, 30)


def _lib():
    from dgl_kgat_amd import _lib
    return _lib


def test_header_declares_the_entries_and_the_library_exports_them():
    lib = _lib()
    with open(lib.HEADER) as fh:
        text = fh.read()
    assert re.search(r"#define\s+KGAT_ABI_VERSION\s+16\b", text) and lib.ABI_VERSION == 16   # additive
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES, name
    assert "kgat_eval_rank.hip" in lib.SOURCES
    so = ctypes.CDLL(lib.build())       # (symbol lookup and host-only predicates: no device work)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name
    # the widths of kgat_eval_topk_supported at K = 32
    for F in (0, 1, 7, 40, 41, 96, 176, 177, 256, 352, 353, 1000, 1100, 1200, 5000):
        assert so.kgat_eval_rank_supported(F) == so.kgat_eval_topk_supported(F, 32), F


def _case():
    """8 users x 30 items of small integers: ties everywhere, masked zeros, a duplicated test entry, an empty test list,
    an empty train list, test items that are training items, every item in train, every item in test."""
    rng = np.random.default_rng(5)
    n_u, n_i = 8, 30
    score = rng.integers(-3, 4, (n_u, n_i)).astype(np.float64)
    score[3, 10:20] = -0.0                                    # -0 ties with the masked +0
    train = [rng.choice(n_i, int(rng.integers(1, 12)), replace=False) for _ in range(n_u)]
    test = [rng.choice(n_i, int(rng.integers(1, 7)), replace=False) for _ in range(n_u)]
    test[1] = np.array([7, 2, 7, 19])                         # a duplicate, unsorted
    test[2] = np.zeros(0, np.int64)                           # no test item
    train[3] = np.zeros(0, np.int64)                          # no training item
    train[4] = np.array([3, 11, 20, 28])
    test[4] = np.concatenate([train[4][:2], [int(np.setdiff1d(np.arange(n_i), train[4])[0])]])   # test items in train
    train[5] = np.arange(n_i)                                 # every item a training item
    test[6] = np.arange(n_i)                                  # every item held out: C == T under `mask`
    return score, train, test


def _brute(score, train, test, mode, ks):
    """Per user: the candidates in a stable descending argsort of s', each test entry's place in it, the metrics from
    their definitions over the ranking's binary relevance vector."""
    n_u, n_i = score.shape
    above, at_k, scalar, n_cand = [], np.zeros((n_u, len(ks), 4)), np.zeros((n_u, 4)), []
    for r in range(n_u):
        s = score[r].copy()
        tr = np.asarray(train[r], dtype=np.int64)
        if mode == "mask":
            s[tr] = 0.0
            cand = np.arange(n_i)
        else:
            cand = np.setdiff1d(np.arange(n_i), tr)
        order = cand[np.argsort(-s[cand], kind="stable")]    # (-(-0.0) == 0.0 == -(0.0): equal, the position decides)
        place = {int(p): x for x, p in enumerate(order)}
        te = sorted(int(t) for t in test[r])
        above.append(np.array([place.get(t, -1) for t in te], dtype=np.int64))
        n_cand.append(len(cand))
        rel = np.isin(order, te).astype(np.float64)
        C, T = len(order), int(rel.sum())
        for j, k in enumerate(ks):
            head = rel[:k]
            disc = 1.0 / np.log2(np.arange(2, len(head) + 2))
            ideal = float((np.sort(head)[::-1] * disc).sum())
            at_k[r, j] = (head.sum() / len(te) if te else 0.0, float((head * disc).sum()) / ideal if ideal > 0 else 0.0,
                          head.sum() / k, float(head.any()))
        if T:
            where = np.flatnonzero(rel)
            neg = np.flatnonzero(rel == 0)
            right = sum(int((neg > p).sum()) for p in where)            # (held-out, other) pairs in the right order
            scalar[r] = (1.0 / (where[0] + 1), np.mean([rel[:p + 1].sum() / (p + 1) for p in where]),
                         right / (T * (C - T)) if C > T else 0.0, np.mean(where + 1.0))
    return above, at_k, scalar, n_cand


@pytest.mark.parametrize("mode", ["mask", "drop"])
def test_rank_ref_against_brute_force(mode):
    score, train, test = _case()
    above, at_k, scalar, n_cand = _brute(score, train, test, mode, KS)
    got = R.rank_items(score, train, test, mode)
    for r in range(len(test)):
        assert np.array_equal(got[r], above[r]), (r, got[r], above[r])
    assert np.array_equal(got[1][[1, 2]], got[1][[2, 1]])               # the duplicated entry: the same value twice
    if mode == "drop":
        assert list(got[4][np.isin(np.sort(test[4]), train[4])]) == [-1, -1] and (got[5] == -1).all()
        assert (got[3] >= 0).all()
    else:
        assert all((g >= 0).all() for g in got)
    m_at_k, m_scalar = R.rank_metrics(got, test, n_cand, KS)
    assert np.allclose(m_at_k, at_k, rtol=0, atol=1e-12), np.argwhere(np.abs(m_at_k - at_k) > 1e-12)
    assert np.allclose(m_scalar, scalar, rtol=0, atol=1e-12), (m_scalar, scalar)
    assert not m_at_k[2].any() and not m_scalar[2].any()                # no test item: zeros
    if mode == "mask":
        assert m_scalar[6, 2] == 0.0 and m_scalar[6, 0] == 1.0 and m_scalar[6, 3] == 15.5    # C == T
        assert m_at_k[1, -1, 0] == 0.75                                 # 3 distinct hits over a list of 4
    assert 0.0 < m_scalar[0, 2] <= 1.0 and 0.0 < m_scalar[0, 1] <= 1.0


def test_python_refusals_without_a_device():
    from dgl_kgat_amd import metrics, ops
    emb = torch.zeros((80, 8))
    train, test, items = {0: np.array([1])}, {0: np.array([2])}, np.arange(4, 64)
    with pytest.raises(ops.KGATLibraryError):                           # no CPU implementation
        metrics.calc_rank_metrics(emb, train, test, items, Ks=(20,))
    with pytest.raises(ops.KGATLibraryError):
        metrics.rank_items(emb, train, test, items)
    for Ks in ((40, 20), (20, 20), (0, 5), (), (20, 61), tuple(range(1, 70))):   # (61 > the 60 items)
        with pytest.raises(ValueError):
            metrics.calc_rank_metrics(emb, train, test, items, Ks=Ks)
    with pytest.raises(ValueError):
        metrics.calc_rank_metrics(emb, train, test, items, mode="filter")
    z = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(ops.KGATLibraryError):
        ops.eval_rank(emb, z, z, torch.zeros(1, dtype=torch.int32), z, torch.zeros(1, dtype=torch.int32), z)
    with pytest.raises(ops.KGATLibraryError):
        ops.eval_rank_metrics(z, torch.zeros(1, dtype=torch.int32), z, 10, (1,))
