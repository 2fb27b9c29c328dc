"""The max reducer (kgat_spmm_umule_max_f32) and the attention-path explanations on the MI355X, against the numpy
restatement of tests/_max_ref.py.  Every message is one fp32 multiply and max never rounds: all comparisons are for
bit equality, there is no tolerance in this file."""
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
    """N = 3,000, E = 60,000 in shuffled edge-id order: one hub row of 5,000 in-edges, 5 % of the rows without
    in-edges, a power-law remainder, 500 duplicated (src, dst) pairs that share their original's weight."""
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


def _inputs(kind, graph, D):
    """(X, w in edge-id order or None)."""
    rng = np.random.default_rng({"tie-heavy": 1, "signed": 2, "copy_src": 3}[kind] * 1000 + D)
    if kind == "tie-heavy":
        X = rng.integers(0, 4, (N, D)).astype(np.float32)
        w = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), graph["m"])[graph["key"]]
        return X, w
    X = rng.standard_normal((N, D)).astype(np.float32)
    if kind == "copy_src":
        return X, None
    w = (rng.random(graph["m"]).astype(np.float32) * np.float32(0.9) + np.float32(0.1))[graph["key"]]
    rows = rng.choice(np.nonzero((graph["deg"] > 0) & (graph["deg"] < 200))[0], 50, replace=False)  # all-negative rows
    srcs = np.unique(graph["src"][np.isin(graph["dst"], rows)])
    X[srcs] = -np.abs(X[srcs])
    return X, w


def _bits(t):
    return t.view(torch.int32) if isinstance(t, torch.Tensor) else np.asarray(t, np.float32).view(np.int32)


def _same(out, arg, ref_out, ref_arg, what):
    got = _bits(out).cpu().numpy()
    assert np.array_equal(got, _bits(ref_out)), "%s: out differs in %d elements" % (what, (got != _bits(ref_out)).sum())
    if ref_arg is not None:
        assert arg.dtype == torch.int32
        a = arg.cpu().numpy()
        assert np.array_equal(a, ref_arg), "%s: arg differs in %d elements" % (what, (a != ref_arg).sum())


@pytest.mark.parametrize("D", [16, 32, 64, 128, 1, 20])
@pytest.mark.parametrize("kind", ["tie-heavy", "signed", "copy_src"])
def test_kernel_parity(dev, graph, kind, D):
    from dgl_kgat_amd import ops
    X, w = _inputs(kind, graph, D)
    ref_out, ref_eid, ref_pos = _max_ref.spmm_max(N, graph["src"], graph["dst"], X, w)
    if kind == "signed":
        assert ((ref_out < 0).all(1)).sum() >= 50          # the identity is -inf, not 0
    assert ((ref_eid == -1).all(1)).sum() == N // 20 and (ref_out[graph["deg"] == 0] == 0).all()
    Xd = torch.as_tensor(X, device=dev)
    g = graph
    w_csr = None if w is None else torch.as_tensor(w, device=dev)[g["eid"].long()].contiguous()
    out, arg = ops.spmm_max(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"])
    _same(out, arg, ref_out, ref_eid, "eid")
    out2, arg2 = ops.spmm_max(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"])
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(arg, arg2)       # reproducible
    out, arg = ops.spmm_max(g["indptr"], g["col"], g["row_of"], Xd, w_csr)
    _same(out, arg, ref_out, ref_pos, "position")
    out, arg = ops.spmm_max(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"], want_arg=False)
    assert arg is None
    _same(out, None, ref_out, None, "no arg")
    row0, n_rows = SUB
    ip = g["indptr"][row0:row0 + n_rows + 1].tolist()
    out, arg = ops.spmm_max(g["indptr"], g["col"], g["row_of"], Xd, w_csr, eid=g["eid"], rows=SUB, e_range=(ip[0], ip[-1]))
    assert out.shape == (n_rows, D)
    _same(out, arg, ref_out[row0:row0 + n_rows], ref_eid[row0:row0 + n_rows], "sub-range")


def test_update_all_surface(dev, graph):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import function as fn, ops
    X, w = _inputs("signed", graph, 64)
    g = K.DGLGraph()
    g.add_nodes(N)
    g.add_edges(graph["src"].astype(np.int64), graph["dst"].astype(np.int64))
    g.readonly()
    Xd, wd = torch.as_tensor(X, device=dev), torch.as_tensor(w, device=dev).reshape(-1, 1)
    g.ndata["h"], g.edata["w"] = Xd, wd
    csr = g._st.csr(dev)
    with torch.no_grad():
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "o"))
        g.update_all(fn.copy_src("h", "m"), fn.max("m", "c"))
    want, _ = ops.spmm_max(csr.indptr, csr.col, csr.row_of, Xd, wd.reshape(-1)[csr.eid.long()].contiguous(), want_arg=False)
    assert torch.equal(_bits(g.ndata["o"]), _bits(want))
    _same(g.ndata["o"], None, _max_ref.spmm_max(N, graph["src"], graph["dst"], X, w)[0], None, "update_all")
    want, _ = ops.spmm_max(csr.indptr, csr.col, csr.row_of, Xd, None, want_arg=False)
    assert torch.equal(_bits(g.ndata["c"]), _bits(want))
    # grad mode without a gradient to carry: runs; with one: refused (no backward, no silent detach)
    g.update_all(fn.copy_src("h", "m"), fn.max("m", "c2"))
    assert torch.equal(_bits(g.ndata["c2"]), _bits(want)) and not g.ndata["c2"].requires_grad
    g.ndata["h"] = Xd.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="no backward"):
        g.update_all(fn.copy_src("h", "m"), fn.max("m", "o"))
    g.ndata["h"], g.edata["w"] = Xd, wd.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="no backward"):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "o"))


# ------------------------------------------------------------------------------------------------ paths
@pytest.fixture(scope="module")
def ckg(dev):
    """A synth CKG of 2,000 nodes with the model's softmax attention; user 0 is isolated (its triplets are dropped)."""
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
    direct = np.nonzero((dst < n_users) & (src >= n_users))[0][:40]            # item -> user edges
    users = np.concatenate([dst[direct], np.zeros(10, np.int64), np.full(20, dst[direct[0]]), rng.integers(1, n_users, 60)])
    items = np.concatenate([src[direct], rng.integers(n_users, n_users + 800, 10), rng.integers(n_users, n_users + 800, 20),
                            rng.integers(n_users, n_users + 800, 60)])
    order = np.concatenate([[0, 40, 50], np.setdiff1d(np.arange(len(users)), [0, 40, 50])])  # direct, isolated, repeated first
    return dict(n=n, g=g, model=model, src=src, dst=dst, w=w, et=trip[:, 1].astype(np.int64), users=users[order],
                items=items[order])


@pytest.mark.parametrize("Q", [1, 5, 130])
def test_attention_paths(dev, ckg, Q):
    from dgl_kgat_amd import explain
    c = ckg
    assert len(c["users"]) == 130
    users, items = c["users"][:Q].tolist(), c["items"][:Q].tolist()
    L = 3
    res = explain.attention_paths(c["g"], c["g"].edata["w"], users, items, max_len=L)
    score, edges, nodes = res.score.cpu().numpy(), res.edges.cpu().numpy(), res.nodes.cpu().numpy()
    assert score.shape == (Q, L) and score.dtype == np.float32
    assert edges.shape == (Q, L, L) and edges.dtype == np.int64 and nodes.shape == (Q, L, L + 1) and nodes.dtype == np.int64
    r_score, r_edges, r_nodes, r_best = _max_ref.attention_paths(c["n"], c["src"], c["dst"], c["w"], users, items, L)
    assert np.array_equal(_bits(score), _bits(r_score))
    assert np.array_equal(edges, r_edges) and np.array_equal(nodes, r_nodes)
    assert np.array_equal(res.best_len.cpu().numpy(), r_best)
    rel = res.relations.cpu().numpy()
    assert np.array_equal(rel, np.where(edges >= 0, c["et"][np.maximum(edges, 0)], -1))
    # every returned walk on its own
    n_found = 0
    for q in range(Q):
        for hop in range(L):
            ln = hop + 1
            if score[q, hop] == 0:
                assert (edges[q, hop] == -1).all() and (nodes[q, hop] == -1).all()
                continue
            n_found += 1
            ee, nn = edges[q, hop], nodes[q, hop]
            assert (ee[:ln] >= 0).all() and (ee[ln:] == -1).all() and (nn[ln + 1:] == -1).all()
            assert nn[0] == items[q] and nn[ln] == users[q]
            p = np.float32(1.0)
            for j in range(ln):
                assert c["src"][ee[j]] == nn[j] and c["dst"][ee[j]] == nn[j + 1]
                p = np.float32(p * c["w"][ee[j]])
            assert p.view(np.int32) == score[q, hop].view(np.int32)
    assert score[0, 0] > 0                                   # a pair with a direct edge
    if Q >= 5:
        assert users[1] == 0 and (score[1] == 0).all() and res.best_len[1] == 0   # the isolated user: no walk
        assert n_found > Q // 2
    if Q == 130:
        assert len(set(users)) < Q - 15                      # repeated users


def test_explain_method_and_refusals(dev, ckg):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import explain
    c = ckg
    users, items = c["users"][:7].tolist(), c["items"][:7].tolist()
    a = c["model"].explain(c["g"], users, items)
    b = explain.attention_paths(c["g"], c["g"].edata["w"], users, items, max_len=len(c["model"].layers))
    assert a.score.shape == (7, 3)
    for f in ("score", "edges", "nodes", "relations", "best_len"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    short = c["model"].explain(c["g"], users, items, max_len=2)
    assert torch.equal(short.score, a.score[:, :2]) and torch.equal(short.edges, a.edges[:, :2, :2])
    with pytest.raises(ValueError):
        explain.attention_paths(c["g"], c["g"].edata["w"], [c["n"]], [1])
    with pytest.raises(ValueError):
        explain.attention_paths(c["g"], c["g"].edata["w"], [1], [-1])
    with pytest.raises(ValueError):
        explain.attention_paths(c["g"], c["g"].edata["w"], [1, 2], [3])
    empty = K.DGLGraph()                                  # no edges at all: every query comes back padded
    empty.add_nodes(4)
    res = explain.attention_paths(empty, torch.zeros(0, 1, device=dev), [1, 2], [3, 0], max_len=2)
    assert (res.score == 0).all() and (res.edges == -1).all() and (res.nodes == -1).all() and (res.best_len == 0).all()
    assert res.score.shape == (2, 2) and res.relations is None
    sharded = c["g"].local_var()
    sharded.partition = object()
    with pytest.raises(K.DGLError):
        explain.attention_paths(sharded, c["g"].edata["w"], [1], [2])


_CHILD = """
import json
import sys
import numpy as np
sys.path.insert(0, %(examples)r)
import train_kgat
import dgl_kgat_amd as K

rec = train_kgat.metrics.recommend
def recommend(emb, users, items, k, seen=None):       # what the harness asks of metrics.recommend, and its answer
    out = rec(emb, users, items, k, seen=seen)
    print("recommend | " + json.dumps({"users": [int(u) for u in users], "top1": out[0][:, 0].tolist(), "k": int(k)}))
    return out
train_kgat.metrics.recommend = recommend

explain = K.KGATPropagation.explain
def explained(self, g, users, items, max_len=None):   # the graph the walks are searched in
    src, dst = g._st._host_edges()
    np.savez(%(dump)r, src=src, dst=dst, type=g.edata["type"].cpu().numpy())
    return explain(self, g, users, items, max_len)
K.KGATPropagation.explain = explained

train_kgat.main(["--planted", "--epochs", "1", "--max_iters", "2", "--explain", "3"])
"""


def test_example_explains_its_top1(dev, tmp_path):
    """examples/train_kgat.py --explain 3, in a child process (main() alters process-wide state).  The child records
    what the harness asked of metrics.recommend and the graph it handed to explain: every printed walk must join the
    recommended top-1 item to its user over typed edges of that graph."""
    import json
    dump = str(tmp_path / "explain_graph.npz")
    code = _CHILD % dict(examples=os.path.join(ROOT, "examples"), dump=dump)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = [ln for ln in r.stdout.splitlines() if ln.startswith("recommend | ")]
    assert len(rec) == 1, r.stdout[-2000:]
    rec = json.loads(rec[0][len("recommend | "):])
    assert rec["k"] == 1 and len(rec["users"]) == 3 and len(set(rec["users"])) == 3 and min(rec["top1"]) >= 0
    assert rec["users"] == sorted(rec["users"])
    top1 = dict(zip(rec["users"], rec["top1"]))
    graph = np.load(dump)
    typed_edges = set(zip(graph["src"].tolist(), graph["type"].tolist(), graph["dst"].tolist()))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("explain |")]
    assert len(lines) == 3, r.stdout[-2000:]
    for ln, user in zip(lines, rec["users"]):
        m = re.match(r"explain \| user (\d+) item (\d+) \| score (\S+) \| (.*)$", ln)
        assert m, ln
        assert int(m.group(1)) == user and int(m.group(2)) == top1[user], (ln, top1)   # the top-1 of metrics.recommend
        toks = m.group(4).split()
        assert float(m.group(3)) > 0 and len(toks) in (3, 5, 7), ln   # a walk of 1..3 edges: node (-rel-> node)+
        assert int(toks[0]) == top1[user] and int(toks[-1]) == user, ln
        for j in range(0, len(toks) - 2, 2):                          # every hop is a typed edge of the graph, in flow order
            rel = re.fullmatch(r"-(\d+)->", toks[j + 1])
            assert rel and (int(toks[j]), int(rel.group(1)), int(toks[j + 2])) in typed_edges, (ln, j)


@pytest.mark.parametrize("D", [16, 64])
def test_kernel_parity_production_tiles(dev, D):
    """The small graph above only reaches the quarter-length runs (tiles of 128 / 256 edges, one pass of a run's edge
    loop at D >= 64).  At E = 1.05 M the launch takes the tiles of the full-size graphs - 512 edges at D = 16, 1,024 at
    D = 64, four passes per run - with a hub row of 20,000 in-edges across them."""
    from dgl_kgat_amd import ops
    n, e, n_hub = 20000, 1050000, 20000   # (the smallest E with full-length tiles at D = 64 is 2^20)
    rng = np.random.default_rng(77 + D)
    dst = np.concatenate([rng.integers(n // 20, n, e - n_hub), np.full(n_hub, n // 2)])   # the first 5 %: no in-edges
    src = rng.integers(0, n, e)
    perm = rng.permutation(e)
    src, dst = src[perm], dst[perm]
    X = rng.standard_normal((n, D)).astype(np.float32)
    w = rng.random(e).astype(np.float32) * np.float32(0.9) + np.float32(0.1)
    assert ops._lib.load().kgat_spmm_tile_edges(e, D) == {16: 512, 64: 1024}[D]
    indptr, col, eid, row_of = ops.csr_from_coo(n, torch.as_tensor(src, dtype=torch.int32, device=dev),
                                                torch.as_tensor(dst, dtype=torch.int32, device=dev))
    w_csr = torch.as_tensor(w, device=dev)[eid.long()].contiguous()
    out, arg = ops.spmm_max(indptr, col, row_of, torch.as_tensor(X, device=dev), w_csr, eid=eid)
    ref_out, ref_eid, _ = _max_ref.spmm_max(n, src, dst, X, w)
    _same(out, arg, ref_out, ref_eid, "production tiles")
