"""Host-side checks of the max reducer (no GPU): the two ABI entries, the fn.max descriptor and update_all's refusals,
and a self-check of the numpy restatement the GPU tests compare against (tests/_max_ref.py) by brute force over every
walk of a small graph."""
import itertools
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
from dgl_kgat_amd import _lib, function as fn  # noqa: E402

import _max_ref  # noqa: E402

NAMES = ("kgat_spmm_max_workspace_bytes", "kgat_spmm_umule_max_f32")


def test_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "kgat_spmm_max.hip" in _lib.SOURCES
    assert lib.kgat_version() == 16 and _lib.ABI_VERSION == 16
    # argument validation comes before any device work
    rc = lib.kgat_spmm_umule_max_f32(-1, 0, 0, 0, 64, None, None, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"spmm_max" in lib.kgat_last_error()
    assert lib.kgat_spmm_umule_max_f32(4, 0, 0, 0, 64, None, None, None, None, None, None, None, None, None, 0, None) == -1
    for d in (16, 32, 64, 128, 1, 20):
        assert lib.kgat_spmm_max_workspace_bytes(3663302, d) > 0
    # two slots of (value, id) per tile and column
    te = lib.kgat_spmm_tile_edges(3663302, 64)
    assert lib.kgat_spmm_max_workspace_bytes(3663302, 64) >= -(-3663302 // te) * 2 * 64 * 8
    assert lib.kgat_spmm_max_workspace_bytes(0, 64) > 0


def test_fn_max_surface():
    r = fn.max("m", "h")
    assert isinstance(r, fn.BuiltinReduce) and repr(r) == "fn.max('m', 'h')"
    assert (r.name, r.msg_field, r.out_field) == ("max", "m", "h")
    g = K.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
    g.ndata["h"] = torch.randn(5, 8)
    g.edata["w"] = torch.rand(5, 1)
    with pytest.raises(NotImplementedError) as ei:
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.mean("m", "o"))
    msg = str(ei.value)
    assert "fn.sum | fn.max" in msg and "fn.sum | fn.mean | fn.max" in msg
    # the pairs are accepted and reach the kernel wrapper, which has no CPU implementation
    with pytest.raises(K.KGATLibraryError):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "o"))
    with pytest.raises(K.KGATLibraryError):
        g.update_all(fn.copy_src("h", "m"), fn.max("m", "o"))
    # no backward: refused, not detached
    g.ndata["h"] = torch.randn(5, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="no backward"):
        g.update_all(fn.copy_src("h", "m"), fn.max("m", "o"))
    with torch.no_grad(), pytest.raises(K.KGATLibraryError):
        g.update_all(fn.copy_src("h", "m"), fn.max("m", "o"))
    from dgl_kgat_amd import explain
    with pytest.raises(K.KGATLibraryError):
        explain.attention_paths(g, g.edata["w"], [0], [1])
    with pytest.raises(ValueError):
        explain.attention_paths(g, g.edata["w"], [0], [1], max_len=0)


def _small_graph():
    """12 nodes, 40 edges: parallel edges of equal weight, weights from a small dyadic set (ties between different
    walks), node 11 without in-edges, node 10 without out-edges."""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 12, 34)
    dst = rng.integers(0, 11, 34)
    src[src == 10] = 11
    w = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), 34)
    w[::3] = rng.random(12).astype(np.float32)[:len(w[::3])] * 0.9 + 0.05
    par = np.array([0, 3, 3, 7, 12, 20])              # parallel copies (edge 3 twice): same endpoints, same weight
    src, dst, w = np.concatenate([src, src[par]]), np.concatenate([dst, dst[par]]), np.concatenate([w, w[par]])
    perm = rng.permutation(len(src))
    return 12, src[perm], dst[perm], w[perm].astype(np.float32)


def test_restatement_against_brute_force():
    n, src, dst, w = _small_graph()
    assert len(src) == 40 and 11 not in dst and 10 not in src
    L = 3
    pairs = [(u, i) for u in range(n) for i in range(n)]
    users, items = [p[0] for p in pairs], [p[1] for p in pairs]
    score, edges, nodes, best_len = _max_ref.attention_paths(n, src, dst, w, users, items, L)
    out_edges = [np.nonzero(src == v)[0] for v in range(n)]
    # every walk of 1..L edges from every start node, its fp32 product formed in flow order
    best = np.zeros((n, n, L), np.float32)  # [item, user, l - 1]
    for start in range(n):
        frontier = [(start, np.float32(1.0))]
        for hop in range(L):
            nxt = []
            for at, p in frontier:
                for e in out_edges[at]:
                    nxt.append((int(dst[e]), np.float32(p * w[e])))
            for at, p in nxt:
                best[start, at, hop] = max(best[start, at, hop], p)
            frontier = nxt
    n_walks = n_ties = 0
    for q, (u, i) in enumerate(pairs):
        for hop in range(L):
            assert score[q, hop].view(np.int32) == best[i, u, hop].view(np.int32), (u, i, hop)
            if score[q, hop] == 0:
                assert (edges[q, hop] == -1).all() and (nodes[q, hop] == -1).all()
                continue
            n_walks += 1
            ln = hop + 1
            ee, nn = edges[q, hop], nodes[q, hop]
            assert (ee[ln:] == -1).all() and (nn[ln + 1:] == -1).all()
            assert nn[0] == i and nn[ln] == u
            p = np.float32(1.0)
            for j in range(ln):
                assert src[ee[j]] == nn[j] and dst[ee[j]] == nn[j + 1]
                p = np.float32(p * w[ee[j]])
            assert p.view(np.int32) == score[q, hop].view(np.int32)
            # the last hop: the smallest edge id among the in-edges of the user that attain the score
            if ln == 1:
                prev = np.where(np.arange(n) == i, np.float32(1), np.float32(0)).astype(np.float32)
            else:
                prev = best[i, :, hop - 1]
            into = np.nonzero(dst == u)[0]
            attain = into[(w[into] * prev[src[into]]).astype(np.float32) == score[q, hop]]
            assert ee[ln - 1] == attain.min()
            n_ties += len(attain) > 1
        top = score[q].max()
        assert best_len[q] == (0 if top == 0 else int(np.argmax(score[q])) + 1)
    assert n_walks > 100 and n_ties > 10, (n_walks, n_ties)   # the graph exercises what it is meant to


def test_restatement_reducer_rules():
    """Identity -inf (a negative maximum survives), zero-degree rows, -0.0 ties with 0.0 and the smallest id wins."""
    src = np.array([0, 1, 2, 0, 1])
    dst = np.array([3, 3, 3, 4, 4])
    X = np.array([[-1.0, 0.0], [-2.0, -0.0], [-0.5, 5.0], [9.0, 9.0], [9.0, 9.0]], np.float32)
    w = np.array([1.0, 1.0, 2.0, 1.0, 1.0], np.float32)
    out, arg, pos = _max_ref.spmm_max(5, src, dst, X, w)
    assert out[3].tolist() == [-1.0, 10.0] and arg[3].tolist() == [0, 2]
    assert out[4, 1] == 0 and not np.signbit(out[4, 1]) and arg[4].tolist() == [3, 3]   # 0.0 (edge 3) ties with -0.0 (edge 4)
    assert (out[:3] == 0).all() and (arg[:3] == -1).all() and (pos[:3] == -1).all()
    out2, arg2, _ = _max_ref.spmm_max(5, src, dst, X, None)
    assert out2[3].tolist() == [-0.5, 5.0] and arg2[3].tolist() == [2, 2]
    for a, b in itertools.product(range(5), range(2)):
        if arg[a, b] >= 0:
            assert dst[arg[a, b]] == a
