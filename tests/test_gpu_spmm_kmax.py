"""The top-4 reducer (kgat_spmm_umule_max4_f32) and the ranked attention-path explanations on the MI355X, against the
numpy restatement of tests/_kmax_ref.py.  Every candidate is one fp32 multiply and a selection never rounds: all
comparisons are for bit equality, there is no tolerance in this file."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _kmax_ref  # noqa: E402
import _max_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N, HUB, N_HUB, N_DUP = 3000, 1500, 5000, 500
SUB = (HUB - 3, 7)   # rows of the sub-range call: the hub and its neighbours; its tiles start at another offset


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graph(dev):
    """The graph of tests/test_gpu_spmm_max.py: N = 3,000, E = 60,000 in shuffled edge-id order, one hub row of 5,000
    in-edges, 5 % of the rows without in-edges, a power-law remainder, 500 duplicated (src, dst) pairs that share their
    original's weight."""
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(11)
    near_hub = np.arange(SUB[0], SUB[0] + SUB[1])
    empty = rng.choice(np.setdiff1d(np.arange(N), near_hub), N // 20, replace=False)
    allowed = np.setdiff1d(np.arange(N), empty)
    p = 1.0 / np.power(1.0 + rng.permutation(len(allowed)), 0.9)
    n_pl = 60000 - N_HUB - N_DUP - len(allowed)   # every other row has at least one in-edge
    dst = np.concatenate([allowed, rng.choice(allowed, n_pl, p=p / p.sum()), np.full(N_HUB, HUB)])
    src = rng.integers(0, N, len(dst))
    m = len(dst)
    dup = rng.choice(m, N_DUP, replace=False)
    src, dst, key = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]]), np.concatenate([np.arange(m), dup])
    perm = rng.permutation(len(src))
    src, dst, key = src[perm], dst[perm], key[perm]
    indptr, col, eid, row_of = ops.csr_from_coo(N, torch.as_tensor(src, dtype=torch.int32, device=dev),
                                                torch.as_tensor(dst, dtype=torch.int32, device=dev))
    deg = np.bincount(dst, minlength=N)
    assert len(src) == 60000 and deg[HUB] >= N_HUB and (deg == 0).sum() == N // 20
    assert not np.array_equal(eid.cpu().numpy(), np.arange(len(src)))      # edge id differs from CSR position
    for d in (16, 32, 64, 128):
        assert N_HUB >= 10 * ops._lib.load().kgat_spmm_tile_edges(len(src), d)  # the hub spans >= 10 tiles
    return dict(src=src, dst=dst, key=key, m=m, deg=deg, indptr=indptr, col=col, eid=eid, row_of=row_of)


def _inputs(kind, graph, Q):
    """(X of (N, Q, 4), w in edge-id order or None)."""
    rng = np.random.default_rng({"tie-heavy": 1, "signed": 2, "copy_src": 3}[kind] * 1000 + Q)
    if kind == "tie-heavy":   # few distinct products: ties between edges and between the slots of one edge
        X = rng.integers(0, 4, (N, Q, 4)).astype(np.float32)
        w = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), graph["m"])[graph["key"]]
        return X, w
    X = rng.standard_normal((N, Q, 4)).astype(np.float32)   # slots in no order
    if kind == "copy_src":
        return X, None
    w = (rng.random(graph["m"]).astype(np.float32) * np.float32(0.9) + np.float32(0.1))[graph["key"]]
    rows = rng.choice(np.nonzero((graph["deg"] > 0) & (graph["deg"] < 200))[0], 50, replace=False)  # all-negative rows
    srcs = np.unique(graph["src"][np.isin(graph["dst"], rows)])
    X[srcs] = -np.abs(X[srcs])
    return X, w


def _bits(t):
    return t.view(torch.int32) if isinstance(t, torch.Tensor) else np.asarray(t, np.float32).view(np.int32)


def _same(got, ref_out, ref_edge, ref_slot, what):
    out, edge, slot = got
    o = _bits(out).cpu().numpy()
    assert o.shape == ref_out.shape
    assert np.array_equal(o, _bits(ref_out)), "%s: out differs in %d elements" % (what, (o != _bits(ref_out)).sum())
    if ref_edge is None:
        assert edge is None and slot is None
        return
    assert edge.dtype == torch.int32 and slot.dtype == torch.uint8
    e, s = edge.cpu().numpy(), slot.cpu().numpy()
    assert np.array_equal(e, ref_edge), "%s: arg_edge differs in %d elements" % (what, (e != ref_edge).sum())
    assert np.array_equal(s, ref_slot), "%s: arg_slot differs in %d elements" % (what, (s != ref_slot).sum())


@pytest.mark.parametrize("Q", [4, 8, 16, 32])
@pytest.mark.parametrize("kind", ["tie-heavy", "signed", "copy_src"])
def test_kernel_parity(dev, graph, kind, Q):
    from dgl_kgat_amd import ops
    X, w = _inputs(kind, graph, Q)
    ref_out, ref_eid, ref_pos, ref_slot = _kmax_ref.spmm_max4(N, graph["src"], graph["dst"], X, w)
    has_in = graph["deg"] > 0
    if kind == "signed":
        assert ((ref_out < 0).all((1, 2))).sum() >= 50     # the identity is -inf, not 0
    if kind == "tie-heavy":                                # ties down to the slot level: equal value and equal edge
        tied = (ref_out[:, :, 1:] == ref_out[:, :, :-1]) & (ref_eid[:, :, 1:] == ref_eid[:, :, :-1]) & has_in[:, None, None]
        assert tied.sum() > 1000
    assert ((ref_eid == -1).all((1, 2))).sum() == N // 20 and (ref_out[~has_in] == 0).all() and (ref_slot[~has_in] == 255).all()
    assert (ref_slot[has_in] < 4).all() and (ref_eid[has_in] >= 0).all()
    Xd = torch.as_tensor(X, device=dev)
    g = graph
    w_csr = None if w is None else torch.as_tensor(w, device=dev)[g["eid"].long()].contiguous()
    got = ops.spmm_max4(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"])
    _same(got, ref_out, ref_eid, ref_slot, "eid")
    again = ops.spmm_max4(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"])
    assert all(torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
               for a, b in zip(got, again))                                       # reproducible
    got = ops.spmm_max4(g["indptr"], g["col"], g["row_of"], Xd.reshape(N, 4 * Q), w_csr)   # (N, 4 Q) is the same operand
    _same(got, ref_out, ref_pos, ref_slot, "position")
    got = ops.spmm_max4(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"], want_arg=False)
    _same(got, ref_out, None, None, "no arg")
    row0, n_rows = SUB
    ip = g["indptr"][row0:row0 + n_rows + 1].tolist()
    got = ops.spmm_max4(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"], rows=SUB, e_range=(ip[0], ip[-1]))
    assert got[0].shape == (n_rows, Q, 4)
    _same(got, ref_out[row0:row0 + n_rows], ref_eid[row0:row0 + n_rows], ref_slot[row0:row0 + n_rows], "sub-range")


def test_other_widths_are_refused(dev, graph):
    from dgl_kgat_amd import ops
    import dgl_kgat_amd as K
    g = graph
    for q in (1, 5, 64):
        with pytest.raises(K.KGATLibraryError):
            ops.spmm_max4(g["indptr"], g["col"], g["row_of"], torch.zeros(N, q, 4, device=dev))
    with pytest.raises(ValueError):
        ops.spmm_max4(g["indptr"], g["col"], g["row_of"], torch.zeros(N, 18, device=dev))


@pytest.mark.parametrize("Q", [4, 16])
def test_kernel_parity_production_tiles(dev, Q):
    """The small graph above only reaches the quarter-length runs.  At E = 1.05 M the launch takes the tiles of the
    full-size graphs - 512 edges at Q = 4, 1,024 at Q = 16 - with a hub row of 20,000 in-edges across them.  At Q = 16
    four query columns chosen by seed are compared: columns are independent."""
    from dgl_kgat_amd import ops
    n, e, n_hub = 20000, 1050000, 20000
    rng = np.random.default_rng(77 + Q)
    dst = np.concatenate([rng.integers(n // 20, n, e - n_hub), np.full(n_hub, n // 2)])   # the first 5 %: no in-edges
    src = rng.integers(0, n, e)
    perm = rng.permutation(e)
    src, dst = src[perm], dst[perm]
    X = rng.standard_normal((n, Q, 4)).astype(np.float32)
    w = rng.random(e).astype(np.float32) * np.float32(0.9) + np.float32(0.1)
    assert ops._lib.load().kgat_spmm_tile_edges(e, 4 * Q) == {4: 512, 16: 1024}[Q]
    indptr, col, eid, row_of = ops.csr_from_coo(n, torch.as_tensor(src, dtype=torch.int32, device=dev),
                                                torch.as_tensor(dst, dtype=torch.int32, device=dev))
    w_csr = torch.as_tensor(w, device=dev)[eid.long()].contiguous()
    out, edge, slot = ops.spmm_max4(indptr, col, row_of, torch.as_tensor(X, device=dev), w_csr, eid=eid)
    cols = np.arange(Q) if Q == 4 else np.sort(rng.choice(Q, 4, replace=False))
    ref_out, ref_eid, _, ref_slot = _kmax_ref.spmm_max4(n, src, dst, X[:, cols], w)
    ct = torch.as_tensor(cols, device=dev)
    _same((out[:, ct].contiguous(), edge[:, ct].contiguous(), slot[:, ct].contiguous()), ref_out, ref_eid, ref_slot,
          "production tiles")


# ------------------------------------------------------------------------------------------------ paths
@pytest.fixture(scope="module")
def ckg(dev):
    """The synth CKG of tests/test_gpu_spmm_max.py: 2,000 nodes with the model's softmax attention; user 0 is isolated
    (its triplets are dropped)."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import synth
    n_users = 600
    n, trip, n_rel = synth.collaborative_kg(n_users, 800, 600, 4, 12000, 6000, seed=3)
    trip = trip[(trip[:, 0] != 0) & (trip[:, 2] != 0)]
    torch.manual_seed(5)
    model = K.KGATPropagation(n, n_rel, input_node_dim=64, relation_dim=64, num_gnn_layers=3, n_hidden=64, dropout=0.0).to(dev)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
    src, dst = trip[:, 2].astype(np.int64), trip[:, 0].astype(np.int64)
    w = g.edata["w"].detach().cpu().numpy().reshape(-1).astype(np.float32)
    rng = np.random.default_rng(9)
    direct = np.nonzero((dst < n_users) & (src >= n_users))[0][:12]            # item -> user edges
    users = np.concatenate([dst[direct], np.zeros(4, np.int64), np.full(6, dst[direct[0]]), rng.integers(1, n_users, 18)])
    items = np.concatenate([src[direct], rng.integers(n_users, n_users + 800, 4), rng.integers(n_users, n_users + 800, 6),
                            rng.integers(n_users, n_users + 800, 18)])
    order = np.concatenate([[0, 12, 16], np.setdiff1d(np.arange(len(users)), [0, 12, 16])])  # direct, isolated, repeated first
    users, items = users[order], items[order]
    L = 3
    # computed once: four slots are always formed and `top` slices them, in the restatement as in the library
    four = _kmax_ref.attention_paths_top(n, src, dst, w, users, items, L, 4)
    two = tuple(a[:, :, :2] for a in four[:3])
    ref = {4: four, 2: two + _kmax_ref.rank_walks(two[0])}
    return dict(n=n, g=g, model=model, src=src, dst=dst, w=w, et=trip[:, 1].astype(np.int64), users=users, items=items,
                L=L, ref=ref)


@pytest.mark.parametrize("Q", [1, 5, 40])
@pytest.mark.parametrize("top", [2, 4])
def test_attention_paths_top(dev, ckg, top, Q):
    from dgl_kgat_amd import explain
    c = ckg
    assert len(c["users"]) == 40
    users, items = c["users"][:Q].tolist(), c["items"][:Q].tolist()
    L = c["L"]
    res = explain.attention_paths(c["g"], c["g"].edata["w"], users, items, max_len=L, top=top)
    assert isinstance(res, explain.TopAttentionPaths)
    score, edges, nodes = res.score.cpu().numpy(), res.edges.cpu().numpy(), res.nodes.cpu().numpy()
    assert score.shape == (Q, L, top) and score.dtype == np.float32
    assert edges.shape == (Q, L, top, L) and edges.dtype == np.int64
    assert nodes.shape == (Q, L, top, L + 1) and nodes.dtype == np.int64
    # queries are independent columns: the restatement of all 40 holds every prefix
    r_score, r_edges, r_nodes, r_rs, r_rl, r_rt = (a[:Q] for a in c["ref"][top])
    assert np.array_equal(_bits(score), _bits(r_score))
    assert np.array_equal(edges, r_edges) and np.array_equal(nodes, r_nodes)
    rel = res.relations.cpu().numpy()
    assert np.array_equal(rel, np.where(edges >= 0, c["et"][np.maximum(edges, 0)], -1))
    # every returned walk on its own; the walks of one (query, length) are distinct
    n_found = 0
    for q in range(Q):
        for hop in range(L):
            ln = hop + 1
            seen = set()
            assert (np.diff(score[q, hop]) <= 0).all()
            for r in range(top):
                ee, nn = edges[q, hop, r], nodes[q, hop, r]
                if score[q, hop, r] == 0:
                    assert (ee == -1).all() and (nn == -1).all()
                    continue
                n_found += 1
                assert (ee[:ln] >= 0).all() and (ee[ln:] == -1).all() and (nn[ln + 1:] == -1).all()
                assert nn[0] == items[q] and nn[ln] == users[q]
                p = np.float32(1.0)
                for j in range(ln):
                    assert c["src"][ee[j]] == nn[j] and c["dst"][ee[j]] == nn[j + 1]
                    p = np.float32(p * c["w"][ee[j]])
                assert p.view(np.int32) == score[q, hop, r].view(np.int32)
                seen.add(tuple(ee[:ln].tolist()))
            assert len(seen) == int((score[q, hop] != 0).sum())
    # slot 0 and first() are the top=1 call, bit for bit
    one = explain.attention_paths(c["g"], c["g"].edata["w"], users, items, max_len=L)
    assert isinstance(one, explain.AttentionPaths)
    r1 = _max_ref.attention_paths(c["n"], c["src"], c["dst"], c["w"], users, items, L)
    assert np.array_equal(_bits(one.score.cpu().numpy()), _bits(r1[0])) and np.array_equal(one.edges.cpu().numpy(), r1[1])
    assert torch.equal(_bits(res.score[:, :, 0]), _bits(one.score))
    assert torch.equal(res.edges[:, :, 0], one.edges) and torch.equal(res.nodes[:, :, 0], one.nodes)
    first = res.first()
    assert isinstance(first, explain.AttentionPaths) and torch.equal(_bits(first.score), _bits(one.score))
    for f in ("edges", "nodes", "relations", "best_len"):
        assert torch.equal(getattr(first, f), getattr(one, f)), f
    # the ranking over all lengths: (score descending, length ascending, slot ascending)
    rs, rl, rt = res.ranked_score.cpu().numpy(), res.ranked_len.cpu().numpy(), res.ranked_slot.cpu().numpy()
    assert rs.shape == rl.shape == rt.shape == (Q, top) and rl.dtype == np.int64 and rt.dtype == np.int64
    assert np.array_equal(_bits(rs), _bits(r_rs)) and np.array_equal(rl, r_rl) and np.array_equal(rt, r_rt)
    for q in range(Q):
        cand = sorted((-float(score[q, l, r]), l + 1, r) for l in range(L) for r in range(top) if score[q, l, r] > 0)[:top]
        for r in range(top):
            nodes_r, rel_r, s_r = res.walk(q, r)
            if r >= len(cand):
                assert (rs[q, r], rl[q, r], rt[q, r]) == (0, 0, -1) and nodes_r == [] and res.describe(q, r) == "(no walk)"
                continue
            assert (rs[q, r], rl[q, r], rt[q, r]) == (np.float32(-cand[r][0]), cand[r][1], cand[r][2])
            assert nodes_r == nodes[q, rl[q, r] - 1, rt[q, r], :rl[q, r] + 1].tolist() and s_r == float(rs[q, r])
            assert rel_r == rel[q, rl[q, r] - 1, rt[q, r], :rl[q, r]].tolist()
            toks = res.describe(q, r).split()
            assert [int(t) for t in toks[0::2]] == nodes_r and toks[1::2] == ["-%d->" % x for x in rel_r]
        assert rl[q, 0] == int(one.best_len[q]) and res.describe(q, 0) == one.describe(q)
    assert score[0, 0, 0] > 0                                # a pair with a direct edge
    if Q >= 5:
        assert users[1] == 0 and (score[1] == 0).all() and (rl[1] == 0).all() and (edges[1] == -1).all()  # the isolated user
        assert n_found > Q
    if Q == 40:
        assert len(set(users)) < Q - 4                       # repeated users


def test_explain_method_and_empty_graph(dev, ckg):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import explain
    c = ckg
    users, items = c["users"][:7].tolist(), c["items"][:7].tolist()
    a = c["model"].explain(c["g"], users, items, top=3)
    b = explain.attention_paths(c["g"], c["g"].edata["w"], users, items, max_len=len(c["model"].layers), top=3)
    assert isinstance(a, explain.TopAttentionPaths) and a.score.shape == (7, 3, 3)
    for f in ("score", "edges", "nodes", "relations", "ranked_score", "ranked_len", "ranked_slot"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    four = c["ref"][4]
    assert np.array_equal(_bits(a.score.cpu().numpy()), _bits(four[0][:7, :, :3]))     # top slices the four slots
    assert np.array_equal(a.edges.cpu().numpy(), four[1][:7, :, :3])
    short = c["model"].explain(c["g"], users, items, max_len=2, top=3)
    assert torch.equal(short.score, a.score[:, :2]) and torch.equal(short.edges, a.edges[:, :2, :, :2])
    with pytest.raises(ValueError):
        c["model"].explain(c["g"], users, items, top=5)
    with pytest.raises(ValueError):
        explain.attention_paths(c["g"], c["g"].edata["w"], [c["n"]], [1], top=2)
    with pytest.raises(NotImplementedError, match="no backward"):
        explain.attention_paths(c["g"], c["g"].edata["w"].clone().requires_grad_(True), [1], [2], top=2)
    empty = K.DGLGraph()                                  # no edges at all: every query comes back padded
    empty.add_nodes(4)
    res = explain.attention_paths(empty, torch.zeros(0, 1, device=dev), [1, 2], [3, 0], max_len=2, top=4)
    assert res.score.shape == (2, 2, 4) and res.edges.shape == (2, 2, 4, 2) and res.nodes.shape == (2, 2, 4, 3)
    assert (res.score == 0).all() and (res.edges == -1).all() and (res.nodes == -1).all() and res.relations is None
    assert (res.ranked_score == 0).all() and (res.ranked_len == 0).all() and (res.ranked_slot == -1).all()
    assert res.walk(0, 0) == ([], None, 0.0) and (res.first().best_len == 0).all()
    none = explain.attention_paths(c["g"], c["g"].edata["w"], [], [], top=2)
    assert none.score.shape == (0, 3, 2) and none.ranked_len.shape == (0, 2)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %(examples)r)
import train_kgat
import dgl_kgat_amd as K

explain = K.KGATPropagation.explain
def explained(self, g, users, items, max_len=None, top=1):   # the graph the walks are searched in
    src, dst = g._st._host_edges()
    np.savez(%(dump)r, src=src, dst=dst, type=g.edata["type"].cpu().numpy(), top=top)
    return explain(self, g, users, items, max_len, top)
K.KGATPropagation.explain = explained

train_kgat.main(["--planted", "--epochs", "1", "--max_iters", "2", "--explain", "2", "--explain_top", "3"])
"""


def test_example_ranks_three_walks(dev, tmp_path):
    """examples/train_kgat.py --explain 2 --explain_top 3, in a child process (main() alters process-wide state): two
    `explain |` lines, each followed by up to three `explain+ |` lines in rank order whose first repeats it, and every
    hop of every printed walk is a typed edge of the graph the harness handed to explain."""
    dump = str(tmp_path / "explain_graph.npz")
    code = _CHILD % dict(examples=os.path.join(ROOT, "examples"), dump=dump)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    graph = np.load(dump)
    assert int(graph["top"]) == 3
    typed_edges = set(zip(graph["src"].tolist(), graph["type"].tolist(), graph["dst"].tolist()))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("explain")]
    heads = [k for k, ln in enumerate(lines) if ln.startswith("explain |")]
    assert len(heads) == 2 and heads[0] == 0, r.stdout[-2000:]
    n_plus = 0
    for h, end in zip(heads, heads[1:] + [len(lines)]):
        m = re.match(r"explain \| user (\d+) item (\d+) \| score (\S+) \| (.*)$", lines[h])
        assert m, lines[h]
        user, item = int(m.group(1)), int(m.group(2))
        more = lines[h + 1:end]
        assert 1 <= len(more) <= 3, lines[h:end]
        last = None
        for rank, ln in enumerate(more, 1):
            p = re.match(r"explain\+ \| user (\d+) item (\d+) \| rank (\d+) \| len (\d+) \| score (\S+) \| (.*)$", ln)
            assert p, ln
            n_plus += 1
            assert (int(p.group(1)), int(p.group(2)), int(p.group(3))) == (user, item, rank), ln
            ln_, sc, toks = int(p.group(4)), float(p.group(5)), p.group(6).split()
            assert sc > 0 and 1 <= ln_ <= 3 and len(toks) == 2 * ln_ + 1, ln
            assert last is None or sc <= last, (ln, last)                 # score descending
            last = sc
            assert int(toks[0]) == item and int(toks[-1]) == user, ln
            for j in range(0, len(toks) - 2, 2):                          # every hop is a typed edge, in flow order
                rel = re.fullmatch(r"-(\d+)->", toks[j + 1])
                assert rel and (int(toks[j]), int(rel.group(1)), int(toks[j + 2])) in typed_edges, (ln, j)
            if rank == 1:
                assert p.group(5) == m.group(3) and p.group(6) == m.group(4), (lines[h], ln)   # the best walk again
    assert n_plus > 2                                                     # some pair has more than one walk
