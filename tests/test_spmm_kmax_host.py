"""Host-side checks of the top-4 reducer and the ranked attention paths (no GPU): the two ABI entries and their
argument validation, attention_paths' `top` argument, and a self-check of the numpy restatement the GPU tests compare
against (tests/_kmax_ref.py) by enumeration of every walk of small random graphs."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, explain  # noqa: E402

import _kmax_ref  # noqa: E402
import _max_ref  # noqa: E402

NAMES = ("kgat_spmm_max4_workspace_bytes", "kgat_spmm_umule_max4_f32")
E_FULL = 3663302


def test_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "kgat_spmm_kmax.hip" in _lib.SOURCES
    assert lib.kgat_version() == 16 and _lib.ABI_VERSION == 16
    assert _lib.SIGNATURES[NAMES[0]] == _lib.SIGNATURES["kgat_spmm_max_workspace_bytes"]
    res, args = _lib.SIGNATURES[NAMES[1]]
    assert res is ctypes.c_int32 and len(args) == 17          # the max entry's arguments and one more output
    assert len(_lib.SIGNATURES["kgat_spmm_umule_max_f32"][1]) == 16
    # per tile two slots of Q lists: four values, four ids and a word of slots each, on the sum kernel's tiles
    for q in (4, 8, 16, 32):
        te = lib.kgat_spmm_tile_edges(E_FULL, 4 * q)
        assert lib.kgat_spmm_max4_workspace_bytes(E_FULL, q) >= -(-E_FULL // te) * 2 * q * 36
    assert lib.kgat_spmm_max4_workspace_bytes(0, 16) > 0


def test_argument_validation_before_device_work():
    """Host buffers stand in for device memory: every call is refused before anything is launched or read."""
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    nothing = [None] * 10

    def call(n_rows, row0, e0, e1, q, ptrs, ws_bytes):
        return lib.kgat_spmm_umule_max4_f32(n_rows, row0, e0, e1, q, *ptrs, ws_bytes, None)

    def refused(rc, word):
        msg = lib.kgat_last_error()
        assert rc == -1 and b"spmm_max4" in msg and word in msg, (rc, msg)

    refused(call(-1, 0, 0, 0, 16, nothing, 0), b"bad size")                    # negative sizes
    refused(call(4, -1, 0, 0, 16, nothing, 0), b"bad size")
    refused(call(4, 0, 0, -1, 16, nothing, 0), b"bad edge range")
    for q in (5, 0, -4, 1, 64, 2 ** 30):                                        # Q outside {4, 8, 16, 32}
        assert call(4, 0, 0, 0, q, [p] * 10, 4096) == -1 and b"spmm_max4" in lib.kgat_last_error(), q
    refused(call(4, 0, 0, 0, 5, [p] * 10, 4096), b"Q = 5")
    refused(call(4, 0, 0, 0, 16, nothing, 0), b"null pointer")
    # a workspace that is too small: 1,000 edges need more than 64 bytes at every width, and a null one is too small
    for q in (4, 8, 16, 32):
        assert lib.kgat_spmm_max4_workspace_bytes(1000, q) > 64
        refused(call(4, 0, 0, 1000, q, [p] * 10, 64), b"workspace too small")
        refused(call(4, 0, 0, 1000, q, [p] * 9 + [None], 1 << 20), b"workspace too small")
    assert call(0, 0, 0, 0, 16, nothing, 0) == 0                                # no rows: nothing to do


def test_top_argument():
    g = K.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
    g.edata["w"] = torch.rand(5, 1)
    for top in (0, 5, -1):
        with pytest.raises(ValueError, match="top"):
            explain.attention_paths(g, g.edata["w"], [0], [1], top=top)
    # top=1 is the old call: a CPU weight reaches the same refusal, as does every top in range
    for top in (1, 2, 4):
        with pytest.raises(K.KGATLibraryError):
            explain.attention_paths(g, g.edata["w"], [0], [1], top=top)
    with pytest.raises(K.KGATLibraryError):
        explain.attention_paths(g, g.edata["w"], [0], [1])
    with pytest.raises(ValueError):
        explain.attention_paths(g, g.edata["w"], [0], [1], max_len=0, top=2)
    sharded = g.local_var()
    sharded.partition = object()
    with pytest.raises(K.DGLError):
        explain.attention_paths(sharded, g.edata["w"], [0], [1], top=3)
    import inspect
    assert inspect.signature(K.KGATPropagation.explain).parameters["top"].default == 1
    assert inspect.signature(explain.attention_paths).parameters["top"].default == 1


def _random_graph(seed):
    """9 nodes, 14-30 edges with parallel edges and self-loops allowed; every other graph draws its weights from
    {0.25, 0.5, 1}, so that different walks tie."""
    rng = np.random.default_rng(seed)
    n, e = 9, int(rng.integers(14, 31))
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    if seed % 2:
        w = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), e)
    else:
        w = (rng.random(e) * 0.9 + 0.05).astype(np.float32)
    return n, src, dst, w.astype(np.float32)


def _all_walks(n, src, dst, w, L):
    """walks[item][user][l - 1]: the list of (fp32 product formed in flow order, edge tuple) of every walk."""
    out_edges = [np.nonzero(src == v)[0] for v in range(n)]
    walks = [[[[] for _ in range(L)] for _ in range(n)] for _ in range(n)]
    for start in range(n):
        frontier = [(start, np.float32(1.0), ())]
        for hop in range(L):
            nxt = []
            for at, p, ee in frontier:
                for e in out_edges[at]:
                    nxt.append((int(dst[e]), np.float32(p * w[e]), ee + (int(e),)))
            for at, p, ee in nxt:
                walks[start][at][hop].append((p, ee))
            frontier = nxt
    return walks


def test_restatement_against_enumeration():
    """120 random 9-node graphs, L = 3, K = 4, all 81 (user, item) pairs: the four scores per length have the bits of
    the four largest products over every walk; every returned walk is a real walk whose flow-order product gives its
    score; the walks of one (pair, length) are distinct; slot 0 is _max_ref.attention_paths."""
    L, top = 3, 4
    n_walks = n_tied = n_short = 0
    for seed in range(120):
        n, src, dst, w = _random_graph(seed)
        pairs = [(u, i) for u in range(n) for i in range(n)]
        users, items = [p[0] for p in pairs], [p[1] for p in pairs]
        score, edges, nodes, r_score, r_len, r_slot = _kmax_ref.attention_paths_top(n, src, dst, w, users, items, L, top)
        s1, e1, n1, _ = _max_ref.attention_paths(n, src, dst, w, users, items, L)
        assert np.array_equal(score[:, :, 0].view(np.int32), s1.view(np.int32))
        assert np.array_equal(edges[:, :, 0], e1) and np.array_equal(nodes[:, :, 0], n1)
        walks = _all_walks(n, src, dst, w, L)
        for q, (u, i) in enumerate(pairs):
            for hop in range(L):
                ln = hop + 1
                prods = sorted((p for p, _ in walks[i][u][hop] if p > 0), reverse=True)[:top]
                want = np.array(prods + [0.0] * (top - len(prods)), np.float32)
                assert np.array_equal(score[q, hop].view(np.int32), want.view(np.int32)), (seed, u, i, hop)
                n_short += 0 < len(prods) < top
                n_tied += len(prods) > 1 and prods[0] == prods[1]
                seen = set()
                for r in range(top):
                    ee, nn = edges[q, hop, r], nodes[q, hop, r]
                    if score[q, hop, r] == 0:
                        assert (ee == -1).all() and (nn == -1).all()
                        continue
                    n_walks += 1
                    assert (ee[:ln] >= 0).all() and (ee[ln:] == -1).all() and (nn[ln + 1:] == -1).all()
                    assert nn[0] == i and nn[ln] == u
                    p = np.float32(1.0)
                    for j in range(ln):
                        assert src[ee[j]] == nn[j] and dst[ee[j]] == nn[j + 1]
                        p = np.float32(p * w[ee[j]])
                    assert p.view(np.int32) == score[q, hop, r].view(np.int32)
                    seen.add(tuple(ee[:ln].tolist()))
                assert len(seen) == int((score[q, hop] != 0).sum())             # distinct walks
            # the ranking over all lengths
            cand = sorted(((-float(score[q, l, r]), l + 1, r) for l in range(L) for r in range(top) if score[q, l, r] > 0))[:top]
            for r in range(top):
                if r < len(cand):
                    assert (r_score[q, r], r_len[q, r], r_slot[q, r]) == (np.float32(-cand[r][0]), cand[r][1], cand[r][2])
                else:
                    assert (r_score[q, r], r_len[q, r], r_slot[q, r]) == (0, 0, -1)
    # the graphs exercise what they are meant to: walks by the ten thousand, tied leaders, lists shorter than four
    assert n_walks > 10000 and n_tied > 1000 and n_short > 1000, (n_walks, n_tied, n_short)


def test_restatement_reducer_rules():
    """Identity -inf (negative winners survive), unsorted source slots, zero-degree rows, -0.0 ties with 0.0, the
    smallest id and then the smallest slot win."""
    src = np.array([0, 1, 2, 0, 1])
    dst = np.array([3, 3, 3, 4, 4])
    X = np.zeros((5, 1, 4), np.float32)
    X[0, 0] = [-1.0, 2.0, -3.0, 2.0]
    X[1, 0] = [2.0, -0.0, 0.0, -5.0]
    X[2, 0] = [1.0, 1.0, 4.0, -7.0]
    w = np.array([1.0, 1.0, 0.5, 1.0, 1.0], np.float32)
    out, eid, pos, slot = _kmax_ref.spmm_max4(5, src, dst, X, w)
    # row 3: candidates 2 (e0 s1), 2 (e0 s3), 2 (e1 s0), 2 (e2 s2) - a four-way tie, ordered by (id, slot)
    assert out[3, 0].tolist() == [2.0] * 4 and eid[3, 0].tolist() == [0, 0, 1, 2] and slot[3, 0].tolist() == [1, 3, 0, 2]
    # row 4 (edges 3, 4 from nodes 0, 1): 2 (e3 s1), 2 (e3 s3), 2 (e4 s0), then -0.0 (e4 s1) before 0.0 (e4 s2)
    assert out[4, 0].tolist() == [2.0, 2.0, 2.0, 0.0] and np.signbit(out[4, 0, 3])
    assert eid[4, 0].tolist() == [3, 3, 4, 4] and slot[4, 0].tolist() == [1, 3, 0, 1]
    assert (out[:3] == 0).all() and (eid[:3] == -1).all() and (pos[:3] == -1).all() and (slot[:3] == 255).all()
    neg, eid2, _, slot2 = _kmax_ref.spmm_max4(5, src[:1], dst[:1], -np.abs(X) - 1)      # one edge, all negative
    assert neg[3, 0].tolist() == [-2.0, -3.0, -3.0, -4.0] and slot2[3, 0].tolist() == [0, 1, 3, 2]
    assert eid2[3, 0].tolist() == [0] * 4
