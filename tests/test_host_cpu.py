"""CPU tests (no GPU): the C-ABI library loads and exports every symbol the header declares,
the DGLGraph surface behaves like the DGL 0.4.x calls the reference makes, the sparse ops
refuse to run without a HIP device (no silent fallback), and the multi-GPU partition logic
works under a world_size-2 gloo group."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import dgl_kgat_amd as K
from dgl_kgat_amd import _lib, function as fn, partition, synth


def test_abi_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), "libkgat_hip.so lacks %s" % name
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert lib.kgat_version() == _lib.ABI_VERSION == int(re.search(r"#define KGAT_ABI_VERSION (\d+)", header).group(1))
    assert lib.kgat_build_hash().decode() == "kgat-src-hash:" + _lib.source_hash() and not _lib.needs_build()
    # argument validation happens before any device work: callable without a GPU
    assert lib.kgat_spmm_umule_sum_f32(-1, 0, 0, 0, 64, None, None, None, None, None, None, None, None, None,
                                       0, 0, 0, None, 0, None) == -1
    assert b"spmm" in lib.kgat_last_error()
    assert lib.kgat_csr_from_coo_workspace_bytes(10, 1000) > 3 * 4000
    assert lib.kgat_spmm_workspace_bytes(3663302, 64) > 0
    # host-only queries of the round-4 entries
    assert lib.kgat_spmm_tile_edges(3663302, 64) == 1024 and lib.kgat_spmm_tile_edges(1000, 64) == 256
    assert lib.kgat_spmm_tile_edges(1000, 8) == 0
    assert lib.kgat_bi_interaction_bwd_input_supported(64, 32) == 1 and lib.kgat_bi_interaction_bwd_input_supported(8, 8) == 0
    assert lib.kgat_bi_interaction_bwd_weight_partials(159251) == 768 and lib.kgat_bi_interaction_bwd_weight_partials(1) == 1
    # host-only queries of the round-5 entries (evaluation)
    assert lib.kgat_eval_supported(176, 20) == 1 and lib.kgat_eval_supported(176, 33) == 0 and lib.kgat_eval_supported(4000, 20) == 0
    assert lib.kgat_eval_items_elems(24915, 176) == 779 * 88 * 64 and lib.kgat_eval_items_elems(0, 176) == 0
    assert lib.kgat_eval_workspace_bytes(70679, 24915, 176, 20) >= 2 * 70679 * 20 * 4
    assert lib.kgat_eval_recall_ndcg_f32(1, None, 10, 176, None, 176, None, None, None, None, None, 40, None, None, 0,
                                         None, None, None, None) == -2 and b"eval" in lib.kgat_last_error()
    # the binding stub of INTEGRATION.md states the version it was written against
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lib.kgat_version() == %d" % _lib.ABI_VERSION in doc


def test_no_oracle_import_in_product():
    pkg = os.path.join(ROOT, "dgl-kgat_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            text = open(os.path.join(pkg, f)).read()
            assert "oracle" not in text, "product file %s mentions the oracle" % f


def _toy_graph():
    g = K.DGLGraph()
    g.add_nodes(5)
    g.add_edges(np.array([1, 2, 3, 0, 1], np.int32), np.array([0, 0, 2, 3, 0], np.int32))
    g.readonly()
    g.ndata["id"] = torch.arange(5)
    g.edata["type"] = torch.tensor([0, 1, 0, 2, 1])
    return g


def test_graph_construction_and_frames():
    g = _toy_graph()
    assert g.number_of_nodes() == 5 and g.number_of_edges() == 5 and g.is_readonly
    assert g.in_degrees().tolist() == [3, 0, 1, 1, 0]
    with pytest.raises(K.DGLError):
        g.add_edges([0], [1])  # readonly
    with pytest.raises(K.DGLError):
        g.ndata["bad"] = torch.zeros(4, 2)  # wrong number of rows
    with pytest.raises(K.DGLError):
        g.edata["bad"] = torch.zeros(6)
    with pytest.raises(KeyError):
        g.ndata["missing"]
    g.edata["w"] = torch.ones(5, 1)
    assert g.edata.pop("w").shape == (5, 1) and "w" not in g.edata
    h = K.DGLGraph()
    h.add_nodes(3)
    with pytest.raises(K.DGLError):
        h.add_edges([0, 5], [1, 2])  # id out of range
    h.add_edges(0, [1, 2])  # scalar broadcast
    assert h.number_of_edges() == 2


def test_local_var_does_not_leak():
    g = _toy_graph()
    lv = g.local_var()
    lv.ndata["h"] = torch.zeros(5, 2)
    lv.edata["type"] = torch.zeros(5, dtype=torch.long)
    assert "h" not in g.ndata and g.edata["type"].tolist() == [0, 1, 0, 2, 1]
    assert lv.ndata["id"] is g.ndata["id"]  # columns are shared, not copied
    with g.local_scope():
        g.ndata["tmp"] = torch.zeros(5)
    assert "tmp" not in g.ndata


def test_filter_and_apply_edges_semantics():
    g = _toy_graph()
    e1 = g.filter_edges(lambda edges: edges.data["type"] == 1)
    assert e1.dtype == torch.int64 and e1.tolist() == [1, 4]
    seen = {}

    def udf(edges):
        seen["src"] = edges.src["id"].tolist()
        seen["dst"] = edges.dst["id"].tolist()
        seen["n"] = edges.batch_size()
        return {"att_w": torch.full((len(edges), 1), 2.5)}

    lv = g.local_var()
    lv.apply_edges(udf, e1)
    assert seen == {"src": [2, 1], "dst": [0, 0], "n": 2}
    # new column is zero-initialised, only the selected rows are written (DGL partial write)
    assert lv.edata["att_w"].reshape(-1).tolist() == [0, 2.5, 0, 0, 2.5]
    lv.apply_edges(lambda edges: {"att_w": torch.full((len(edges), 1), -1.0)}, torch.tensor([0]))
    assert lv.edata["att_w"].reshape(-1).tolist() == [-1.0, 2.5, 0, 0, 2.5]
    with pytest.raises(K.DGLError):
        lv.apply_edges(lambda edges: {"x": torch.zeros(3)}, e1)
    # partial writes go in place only into a column this view allocated itself: a column that came
    # from the parent (or was assigned by the caller) is never written through
    g.edata["keep"] = torch.ones(5, 1)
    lv2 = g.local_var()
    lv2.apply_edges(lambda edges: {"keep": torch.full((len(edges), 1), 7.0)}, torch.tensor([2]))
    assert g.edata["keep"].reshape(-1).tolist() == [1, 1, 1, 1, 1] and lv2.edata["keep"].reshape(-1).tolist() == [1, 1, 7, 1, 1]
    mine = torch.zeros(5, 1)
    lv2.edata["att_w"] = mine
    lv2.apply_edges(lambda edges: {"att_w": torch.full((len(edges), 1), 3.0)}, torch.tensor([1]))
    assert mine.reshape(-1).tolist() == [0, 0, 0, 0, 0] and lv2.edata["att_w"].reshape(-1).tolist() == [0, 3, 0, 0, 0]
    lv3 = lv2.local_var()  # a view of a view starts without owned columns
    lv3.apply_edges(lambda edges: {"att_w": torch.full((len(edges), 1), 9.0)}, torch.tensor([0]))
    assert lv2.edata["att_w"].reshape(-1).tolist() == [0, 3, 0, 0, 0] and lv3.edata["att_w"].reshape(-1).tolist() == [9, 3, 0, 0, 0]


def test_sparse_ops_refuse_cpu_tensors():
    """No CPU fallback: without a HIP device the aggregation and the softmax raise."""
    g = _toy_graph()
    g.ndata["h"] = torch.randn(5, 8)
    g.edata["w"] = torch.rand(5, 1)
    with pytest.raises(K.KGATLibraryError):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "h_neighbor"))
    with pytest.raises(K.KGATLibraryError):
        K.edge_softmax(g, torch.randn(5, 1))
    with pytest.raises(NotImplementedError):
        g.update_all(lambda e: {"m": e.src["h"]}, fn.sum("m", "o"))
    with pytest.raises(K.DGLError):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("other", "o"))
    with pytest.raises(KeyError):
        g.update_all(fn.u_mul_e("nope", "w", "m"), fn.sum("m", "o"))


def test_model_parameters_match_reference_layout():
    g = load_golden("toy_d8")
    m = K.KGATPropagation(g["n"], g["R"], 8, 8, 3, 8, dropout=0.0)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"entity_embed.weight": (g["n"], 8), "relation_embed.weight": (g["R"], 8),
                      "W_R": (g["R"], 8, 8), "layers.0.res_fc_2.weight": (8, 8),
                      "layers.1.res_fc_2.weight": (4, 8), "layers.2.res_fc_2.weight": (2, 4)}


def test_install_as_dgl_aliases():
    K.install_as_dgl()
    import dgl
    import dgl.function as dfn
    from dgl.nn.pytorch.softmax import edge_softmax
    assert dgl.DGLGraph is K.DGLGraph and dfn.u_mul_e is fn.u_mul_e and edge_softmax is K.edge_softmax
    for name in [n for n in sys.modules if n == "dgl" or n.startswith("dgl.")]:
        del sys.modules[name]


def test_synthetic_ckg_shapes():
    n, trip, R = synth.amazon_book_ckg(scale=0.01)
    assert trip.dtype == np.int32 and trip.shape[1] == 3 and R == 41
    assert trip[:, [0, 2]].min() >= 0 and trip[:, [0, 2]].max() < n and trip[:, 1].max() == 40
    n_uv = (trip[:, 1] == 39).sum()
    uv, vu = trip[trip[:, 1] == 39], trip[trip[:, 1] == 40]
    assert n_uv == len(vu) and np.array_equal(uv[:, 0], vu[:, 2]) and np.array_equal(uv[:, 2], vu[:, 0])
    n2, t2, _ = synth.amazon_book_ckg(scale=0.01)
    assert np.array_equal(trip, t2)  # seeded
    g = synth.build_graph(n, trip)
    assert g.number_of_edges() == len(trip) and g.edata["type"].dtype == torch.int64
    n3, t3, r3 = synth.power_law_ckg(2000, 30000, 8, max_in_degree=500)
    assert np.bincount(t3[:, 0], minlength=n3).max() <= 500 + 60


def test_balanced_bounds_and_shards_cover_graph():
    n, trip, R = synth.amazon_book_ckg(scale=0.02)
    g = synth.build_graph(n, trip)
    g.edata["w"] = torch.rand(len(trip), 1)
    deg = np.bincount(trip[:, 0], minlength=n)
    for world in (1, 2, 4, 8):
        b = partition.balanced_row_bounds(deg, world)
        assert b[0] == 0 and b[-1] == n and all(x <= y for x, y in zip(b, b[1:]))
        per = [deg[b[i]:b[i + 1]].sum() for i in range(world)]
        assert sum(per) == len(trip) and max(per) <= len(trip) / world + deg.max()
        # the shards balance edges + ROW_WEIGHT per row (the dense part and the slice exchange cost
        # rows, not edges); the device-side bounds are the host-side ones
        b = partition.balanced_row_bounds(deg, world, partition.ROW_WEIGHT)
        cost = [deg[b[i]:b[i + 1]].sum() + partition.ROW_WEIGHT * (b[i + 1] - b[i]) for i in range(world)]
        assert max(cost) <= sum(cost) / world + deg.max() + partition.ROW_WEIGHT
        for rw in (0, partition.ROW_WEIGHT, 100):
            assert partition.balanced_row_bounds_device(torch.as_tensor(trip[:, 0].astype(np.int64)), n, world, rw) == \
                partition.balanced_row_bounds(deg, world, rw)
        seen = []
        for r in range(world):
            sg, keep = partition.shard_graph(g, r, world)
            assert sg.number_of_nodes() == n and sg.partition.lo == b[r] and sg.partition.hi == b[r + 1]
            assert np.all((trip[keep, 0] >= b[r]) & (trip[keep, 0] < b[r + 1])) and np.all(np.diff(keep) > 0)
            assert torch.equal(sg.edata["w"], g.edata["w"][torch.as_tensor(keep)])
            seen.append(keep)
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(len(trip)))


def test_lazy_edge_weights_mechanics():
    """lazy.LazyEdgeWeights: metadata never triggers the deferred fill, any value-level operation
    triggers it exactly once (before the operation runs), frames accept it, autograd functions
    pass the very object through forward and saved_tensors."""
    from dgl_kgat_amd.lazy import LazyEdgeWeights, pending_csr_weights
    calls, st = [], object()
    base, src = torch.empty(5, 1), torch.arange(5.0).reshape(5, 1)

    def fill():
        calls.append(1)
        base.copy_(src)
    w = LazyEdgeWeights(base, fill, st, "csr-copy")
    assert isinstance(w, torch.Tensor) and w.shape == (5, 1) and w.dim() == 2 and len(w) == 5 and w.dtype == torch.float32
    assert w.device.type == "cpu" and w.is_contiguous() and w.numel() == 5 and not w.requires_grad and not calls
    g = _toy_graph()
    g.edata["w"] = w                      # Frame checks type, dim and length only
    assert g.edata["w"] is w and w.pending and pending_csr_weights(w, st) == "csr-copy"
    assert pending_csr_weights(w, object()) is None and pending_csr_weights(torch.zeros(1), st) is None

    class Pass(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, ww):
            assert ww is w and ww.pending
            ctx.save_for_backward(x, ww)
            return x * 1

        @staticmethod
        def backward(ctx, grad):
            assert ctx.saved_tensors[1] is w and w.pending
            return grad, None
    x = torch.ones(5, 1, requires_grad=True)
    Pass.apply(x, w).sum().backward()
    assert not calls
    flat = w.reshape(-1)                  # value-level: fill first, result is an ordinary tensor
    assert calls == [1] and type(flat) is torch.Tensor and flat.tolist() == [0, 1, 2, 3, 4] and not w.pending
    assert pending_csr_weights(w, st) is None and float(w.sum()) == 10 and calls == [1]
    assert w.data_ptr() == base.data_ptr()
    for op in (lambda t: t.cpu(), lambda t: t.data_ptr(), lambda t: repr(t), lambda t: torch.cat([t, t]),
               lambda t: t[0], lambda t: t.detach(), lambda t: t.numpy(), lambda t: t.add_(1)):
        hits = []
        op(LazyEdgeWeights(torch.zeros(3, 1), lambda: hits.append(1), st, None))
        assert hits == [1], op


def test_shard_layer_under_autograd_reaches_the_kernels():
    """A destination-range shard is differentiable since round 3 (partition.shard_conv: local
    backward + all-reduce of the replicated operands' gradients; gradient parity with the one-GPU
    run is a -m gpu test).  On CPU tensors it must fail loudly in the op layer - there is no CPU
    implementation to fall back to - not raise the old 'forward-only' refusal or return garbage."""
    n, trip, R = synth.amazon_book_ckg(scale=0.002)
    g = synth.build_graph(n, trip)
    g.edata["w"] = torch.rand(len(trip), 1)
    sg, _ = partition.shard_graph(g, 0, 2)
    m = K.KGATPropagation(n, R, 16, 16, 1, 16, dropout=0.0)
    with pytest.raises(_lib.KGATLibraryError, match="only runs on a HIP device"):
        m.layers[0](sg, m.entity_embed.weight)
    with pytest.raises(_lib.KGATLibraryError, match="only runs on a HIP device"):
        m.gnn(sg)


def test_identity_id_cache_is_keyed_on_the_tensor_object():
    n = 40
    m = K.KGATPropagation(n, 2, 8, 8, 1, 8, dropout=0.0)
    g1, g2 = K.DGLGraph(), K.DGLGraph()
    for g in (g1, g2):
        g.add_nodes(n)
    g1.ndata["id"] = torch.arange(n)
    assert m._node_embeddings(g1) is m.entity_embed.weight
    g2.ndata["id"] = torch.arange(n).flip(0)
    assert torch.equal(m._node_embeddings(g2), m.entity_embed.weight.flip(0))
    g1.ndata["id"][0] = 3  # in-place edit of a cached tensor: the version counter invalidates the hit
    assert torch.equal(m._node_embeddings(g1)[0], m.entity_embed.weight[3])


_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
from dgl_kgat_amd import partition, synth
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
n, trip, R = synth.amazon_book_ckg(scale=0.005)
g = synth.build_graph(n, trip)
sg, keep = partition.shard_graph(g, rank, world)
p = sg.partition
torch.manual_seed(0)
full_ref = torch.randn(n, 16)                      # what a single process would hold
mine = full_ref[p.lo:p.hi].clone()                 # this rank's rows of a layer output
full = p.exchange(mine, 16)                        # zero-padded buffer + all-reduce (gloo here, RCCL on GPUs)
assert torch.equal(full, full_ref), "exchange did not reassemble the layer output"
for mode in partition.EXCHANGE_MODES:              # the cheaper equivalents leave the same bits
    if mode == "allgather":                        # gloo's all_gather wants equal slices: an even split of the rows
        even = [n * r // world for r in range(world + 1)]
        if len({even[r + 1] - even[r] for r in range(world)}) == 1:
            q = partition.Partition(rank, world, even, n, mode=mode)
            assert torch.equal(q.exchange(full_ref[q.lo:q.hi].clone(), 16), full_ref), mode
        continue
    q = partition.Partition(rank, world, p.bounds, n, mode=mode)
    assert torch.equal(q.exchange(mine, 16), full_ref), mode
    empty = partition.Partition(rank, world, [0] + [n] * world, n, mode=mode)   # rank 0 owns everything
    got = empty.exchange(full_ref[empty.lo:empty.hi].clone(), 16)
    assert torch.equal(got, full_ref), mode + " with empty slices"
# the chunked exchange (Partition.propagate_overlapped moves one row block per rank at a time): block cuts known to
# all ranks (plan_chunks: all_gather_object), every mode assembles the same bits piece by piece
indptr = torch.zeros(n + 1, dtype=torch.int32)
dst_loc = torch.as_tensor(np.asarray(trip)[np.asarray(keep), 0].astype(np.int64))
indptr[1:] = torch.cumsum(torch.bincount(dst_loc, minlength=n), 0).to(torch.int32)
for mode in ("allreduce", "broadcast", "p2p"):
    q = partition.Partition(rank, world, p.bounds, n, mode=mode)
    plan = q.plan_chunks(3, indptr)
    rows = plan["rows"]
    assert len(rows) == world and all(r[0] == q.bounds[i] and r[-1] == q.bounds[i + 1] and sorted(r) == r
                                      for i, r in enumerate(rows))
    assert plan["edges"][0] == int(indptr[q.lo]) and plan["edges"][-1] == int(indptr[q.hi])
    full = q.new_buffer(16, torch.device("cpu"))
    for k in range(3):
        full[rows[rank][k]:rows[rank][k + 1]] = full_ref[rows[rank][k]:rows[rank][k + 1]]
        q._assemble_pieces(full, [rows[r][k] for r in range(world)], [rows[r][k + 1] for r in range(world)])
    assert torch.equal(full, full_ref), mode + " (chunked)"
cnt = torch.tensor([len(keep)]); dist.all_reduce(cnt)
assert int(cnt) == len(trip)
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_partition_exchange_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % ROOT)
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:   # a free rendezvous port, not a fixed one
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    logs = [tmp_path / ("rank%d.log" % r) for r in range(2)]
    procs = []
    for r in range(2):   # output to files: a rank blocked on a full pipe while its peer waits in a collective would hang
        with open(logs[r], "wb") as fh:
            procs.append(subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=fh,
                                          stderr=subprocess.STDOUT))
    try:
        for p in procs:
            p.wait(timeout=300)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log.read_text()[-3000:]


@pytest.mark.parametrize("case", ["toy_d8", "toy_d16_k32", "toy_d64"])
def test_dense_losses_match_reference(case):
    """transR (models.py:114-133) and the BPR loss (models.py:170-178): torch-only parts of the
    reference Model, checked against values produced by the reference's own code."""
    g = load_golden(case)
    d, k = g["entity_embed"].shape[1], g["W_R"].shape[2]
    m = K.KGATPropagation(g["n"], g["R"], d, k, len(g["W2"]), g["W2"][0].shape[0], dropout=0.0).double()
    sd = {"entity_embed.weight": g["entity_embed"], "relation_embed.weight": g["relation_embed"], "W_R": g["W_R"]}
    sd.update({"layers.%d.res_fc_2.weight" % i: W for i, W in enumerate(g["W2"])})
    m.load_state_dict({k_: torch.as_tensor(v, dtype=torch.float64) for k_, v in sd.items()})
    h, r, pt, nt = (torch.as_tensor(x) for x in g["transR_idx"])
    with torch.no_grad():
        assert abs(float(m.transR(h, r, pt, nt)) - float(g["transR_loss"])) < 1e-12
        assert abs(float(m.get_loss(torch.as_tensor(g["gnn_out"]), h, pt, nt)) - float(g["bpr_loss"])) < 1e-12


def test_tall_linear_gradients_match_torch():
    from dgl_kgat_amd.kgat_layer import _TallLinear
    torch.manual_seed(0)
    for n in (5, 2048, 2048 + 77, 5000):
        x = torch.randn(n, 24, dtype=torch.float64, requires_grad=True)
        w = torch.randn(12, 24, dtype=torch.float64, requires_grad=True)
        g = torch.randn(n, 12, dtype=torch.float64)
        _TallLinear.apply(x, w).backward(g)
        gx, gw = x.grad.clone(), w.grad.clone()
        x.grad = w.grad = None
        torch.nn.functional.linear(x, w).backward(g)
        assert torch.allclose(gx, x.grad, rtol=1e-12, atol=1e-12) and torch.allclose(gw, w.grad, rtol=1e-11, atol=1e-11)


def test_all_edges_orders():
    g = K.DGLGraph()
    g.add_nodes(4)
    g.add_edges([2, 0, 2, 1], [1, 3, 0, 1])
    u, v = g.all_edges(order="eid")
    assert u.tolist() == [2, 0, 2, 1] and v.tolist() == [1, 3, 0, 1]
    u, v, e = g.all_edges(form="all", order="srcdst")
    assert list(zip(u.tolist(), v.tolist())) == [(0, 3), (1, 1), (2, 0), (2, 1)] and e.tolist() == [1, 3, 2, 0]
    with pytest.raises(Exception):
        g.all_edges(order="random")


def test_device_graph_generator_on_cpu():
    """synth.power_law_coo_device (torch RNG; runs on any device): both capping modes keep the
    heaviest in-degree near the cap, ids in range, int32 outputs, seeded."""
    n, e, cap = 200_000, 4_000_000, 20_000
    for mode in ("redraw", "shift"):
        s1, d1, t1 = synth.power_law_coo_device(n, e, 7, "cpu", seed=3, max_in_degree=cap, cap=mode)
        s2, d2, t2 = synth.power_law_coo_device(n, e, 7, "cpu", seed=3, max_in_degree=cap, cap=mode)
        assert torch.equal(d1, d2) and torch.equal(s1, s2) and torch.equal(t1, t2)
        assert d1.dtype == s1.dtype == t1.dtype == torch.int32 and len(d1) == e
        assert int(d1.min()) >= 0 and int(d1.max()) < n and int(s1.max()) < n and int(t1.max()) == 6
        deg = np.bincount(d1.numpy(), minlength=n)
        assert 0.8 * cap < deg.max() < 1.15 * cap, (mode, deg.max())
        assert np.sort(deg)[-50:].mean() > 20 * np.median(deg[deg > 0])   # heavy tail
    with pytest.raises(ValueError):
        synth.power_law_coo_device(10, 10, 2, "cpu", cap="nope")


def test_tile_parts_restatement_balances_cost():
    from oracle import kgat_oracle as orc
    rng = np.random.default_rng(5)
    # three relations; tiles with 1..256 positions, a few heavy ones
    tiles, rel_tptr, p = [], [0], 0
    for r, cnt in enumerate((300, 5, 900)):
        for _ in range(cnt):
            w = int(rng.integers(1, 257)) if rng.random() < 0.2 else int(rng.integers(1, 65))
            tiles.append((r, 0, p, p + w))
            p += w
        rel_tptr.append(len(tiles))
    tiles = np.asarray(tiles)
    cost = (64, 12, 466)
    parts = orc.fold_tile_parts(tiles, rel_tptr, 16, cost)
    assert parts[0] == 0 and parts[-1] == len(tiles) and np.all(np.diff(parts) >= 0) and len(parts) == 17
    P = tiles[:, 3] - tiles[:, 2]
    c = cost[0] + cost[1] * np.where(P > 64, (P - 64 + 63) // 64, 0) + np.where(np.isin(np.arange(len(tiles)), rel_tptr[:-1]), cost[2], 0)
    per = np.array([c[parts[b]:parts[b + 1]].sum() for b in range(16)])
    assert per.max() <= per.mean() + c.max() + 1   # within one tile of the mean
    assert np.array_equal(orc.fold_tile_parts(tiles, rel_tptr, 1, cost), [0, len(tiles)])


def test_bench_traffic_records_are_keyed_on_the_kernel_sources(tmp_path, monkeypatch):
    """bench.py pairs a committed PMC figure with a timing only while the record's hash equals the
    hash of the kernel sources beside the library."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    srcs = ("kgat_spmm.hip", "kgat_common.h")
    h = bench.source_hash(*srcs)
    assert len(h) == 16 and h == bench.source_hash(*srcs) and h != bench.source_hash("kgat_softmax.hip", "kgat_common.h")
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r00_pmc_spmm_traffic.json").write_text(json.dumps({"kernel_source_sha16": "0" * 16, "traffic_bytes_per_launch": 1}))
    (prof / "r01_pmc_spmm_traffic.json").write_text(json.dumps({"kernel_source_sha16": h, "traffic_bytes_per_launch": 42}))
    (prof / "r02_pmc_spmm_traffic.json").write_text(json.dumps({"traffic_bytes_per_launch": 7}))   # no hash: never used
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    os.makedirs(tmp_path / "dgl-kgat_amd" / "csrc")
    for f in srcs:
        (tmp_path / "dgl-kgat_amd" / "csrc" / f).write_bytes(open(os.path.join(ROOT, "dgl-kgat_amd", "csrc", f), "rb").read())
    assert bench.committed_traffic("pmc_spmm_traffic.json", srcs) == (42, "r01_pmc_spmm_traffic.json")
    with open(tmp_path / "dgl-kgat_amd" / "csrc" / "kgat_spmm.hip", "ab") as fh:
        fh.write(b"// edited\n")
    assert bench.committed_traffic("pmc_spmm_traffic.json", srcs) == (None, None)


def test_attention_product_form_switches(monkeypatch):
    """Host-side choice of the attention kernels' product form: the split cost follows the form the
    kernel will take at a width, and KGAT_ATT_F32_PRODUCTS is read as a boolean switch."""
    import dgl_kgat_amd  # noqa: F401
    from dgl_kgat_amd import graph, ops
    assert ops.fold_tile_cost(64) == ops.FOLD_TILE_COST and ops.fold_tile_cost(32) == ops.FOLD_TILE_COST
    assert ops.fold_tile_cost(16) == ops.FOLD_TILE_COST_F32          # no bf16-piece form below 32
    assert ops.fold_tile_cost(64, f32_products=True) == ops.FOLD_TILE_COST_F32
    assert ops.ATT_F32_PRODUCTS == 1
    from dgl_kgat_amd import options
    for val, want in (("", False), ("0", False), ("1", True), ("yes", True)):
        before = graph._f32_products()
        monkeypatch.setenv("KGAT_ATT_F32_PRODUCTS", val)
        assert graph._f32_products() is before     # the environment is read once, at import ...
        options.reload()                            # ... or when a launcher asks for it
        assert graph._f32_products() is want
    monkeypatch.delenv("KGAT_ATT_F32_PRODUCTS")
    options.reload()
    assert graph._f32_products() is False
    with options.override(att_f32_products=True, fuse_bi=True):
        assert graph._f32_products() is True and options.options.fuse_bi is True
    assert graph._f32_products() is False and options.options.fuse_bi is False
    # no module of the package reads the environment for behaviour outside options.py (_lib: the compiler path)
    pkg = os.path.join(ROOT, "dgl-kgat_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py") and f not in ("options.py", "_lib.py"):
            assert "os.environ" not in open(os.path.join(pkg, f)).read(), f
    # the header and the loader agree on the flag and on the ABI version that introduced it
    hdr = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    assert "KGAT_ATT_F32_PRODUCTS = 1" in hdr and "#define KGAT_ABI_VERSION %d" % _lib.ABI_VERSION in hdr and _lib.ABI_VERSION >= 3


def test_lazy_edge_weights_value_paths_outside_torch_function():
    """Round-2 review: reads that bypass the __torch_function__ hook.  `type(dtype)` is a cast (the
    argument-less form is metadata), `copy.deepcopy` / pickling copy the values, the legacy
    torch.utils.dlpack.to_dlpack is a C function that never consults the hook.  Each must see the
    filled values, and after the fill the object is a plain torch.Tensor."""
    import copy
    import pickle
    import torch.utils.dlpack as dlpack
    from dgl_kgat_amd import lazy
    from dgl_kgat_amd.lazy import LazyEdgeWeights
    # importing the package leaves torch alone: the to_dlpack wrapper exists only after lazy.enable()
    probe = ("import sys; sys.path.insert(0, %r); import torch.utils.dlpack as d; import dgl_kgat_amd as K; "
             "from dgl_kgat_amd import lazy; assert not getattr(d.to_dlpack, '_kgat_guarded', False); "
             "assert not lazy.enabled(); K.enable_lazy_edge_weights(); assert d.to_dlpack._kgat_guarded and lazy.enabled(); "
             "K.enable_lazy_edge_weights(False); assert not getattr(d.to_dlpack, '_kgat_guarded', False)" % ROOT)
    subprocess.run([sys.executable, "-c", probe], check=True, env={k: v for k, v in os.environ.items()
                                                                  if k not in ("KGAT_LAZY_EDGE_WEIGHTS",)})
    lazy.enable()
    try:
        _lazy_value_paths(copy, pickle, dlpack, LazyEdgeWeights)
    finally:
        lazy.enable(False)


def _lazy_value_paths(copy, pickle, dlpack, LazyEdgeWeights):
    def make():
        base = torch.full((5, 1), float("nan"))
        calls = []

        def fill():
            calls.append(1)
            base.copy_(torch.arange(5.0).reshape(5, 1))
        return LazyEdgeWeights(base, fill, object(), "csr"), calls
    want = [0.0, 1.0, 2.0, 3.0, 4.0]
    w, calls = make()
    assert w.type() == "torch.FloatTensor" and w.pending and not calls         # metadata form
    assert w.type(torch.float64).reshape(-1).tolist() == want and calls == [1]  # cast form
    assert type(w) is torch.Tensor and w.pending is False
    w, calls = make()
    assert w.type("torch.DoubleTensor").reshape(-1).tolist() == want and calls == [1]
    w, calls = make()
    c = copy.deepcopy(w)
    assert type(c) is torch.Tensor and c.reshape(-1).tolist() == want and calls == [1] and type(w) is torch.Tensor
    assert copy.deepcopy(w).reshape(-1).tolist() == want and calls == [1]       # again, after the fill
    w, calls = make()
    g = _toy_graph()
    g.edata["w"] = w
    g2 = copy.deepcopy(g)                                                        # a graph holding it in edata
    assert g2.edata["w"].reshape(-1).tolist() == want and calls == [1]
    w, calls = make()
    assert torch.from_dlpack(dlpack.to_dlpack(w)).reshape(-1).tolist() == want and calls == [1]
    w, calls = make()
    assert torch.from_dlpack(w).reshape(-1).tolist() == want and calls == [1]
    w, calls = make()
    assert pickle.loads(pickle.dumps(w)).reshape(-1).tolist() == want and calls == [1]
    w, calls = make()
    assert w.data_ptr() != 0 and calls == [1]                                    # the raw pointer is a value-level read
    w, calls = make()
    assert (w * w).reshape(-1).tolist() == [x * x for x in want] and calls == [1]  # the same tensor twice in one call


def test_lazy_fill_failure_leaves_the_tensor_pending():
    """a fill that raises (launch error, out of memory) must not leave a plain tensor over
    unwritten storage - the object stays pending with its fill intact and the next read tries again."""
    from dgl_kgat_amd.lazy import LazyEdgeWeights
    base = torch.full((3, 1), float("nan"))
    state = {"fail": True, "calls": 0}

    def fill():
        state["calls"] += 1
        if state["fail"]:
            raise RuntimeError("launch failed")
        base.copy_(torch.arange(3.0).reshape(3, 1))
    w = LazyEdgeWeights(base, fill, object(), "csr")
    with pytest.raises(RuntimeError):
        w.sum()
    assert isinstance(w, LazyEdgeWeights) and w.pending and state["calls"] == 1
    state["fail"] = False
    assert w.reshape(-1).tolist() == [0.0, 1.0, 2.0] and state["calls"] == 2 and type(w) is torch.Tensor


def test_partial_edge_writes_do_not_leak_into_handed_out_columns():
    """Round-2 review: the in-place continuation of a partial apply_edges write must stop as soon as
    the column has been handed out (g.edata[k]) or shared with a local_var()/local_scope() view -
    DGL's update_rows is out of place, and local_var promises isolation."""
    g = _toy_graph()
    one = lambda edges: {"a": torch.ones(len(edges), 1)}    # noqa: E731
    two = lambda edges: {"a": torch.full((len(edges), 1), 2.0)}  # noqa: E731
    g.apply_edges(one, torch.tensor([0, 1]))
    snap = g.edata["a"]
    lg = g.local_var()
    before = snap.clone()
    g.apply_edges(two, torch.tensor([2, 3]))
    assert torch.equal(snap, before) and torch.equal(lg.edata["a"], before)
    assert g.edata["a"].reshape(-1).tolist() == [1, 1, 2, 2, 0]
    # the relation loop of models.py:149-152 (no reads of the column in between) still accumulates
    h = _toy_graph()
    for r, f in enumerate((one, two)):
        h.apply_edges(f, h.filter_edges(lambda edges: edges.data["type"] == r))
    assert h.edata["a"].reshape(-1).tolist() == [1, 2, 1, 0, 2]
    with g.local_scope():
        g.apply_edges(one, torch.tensor([4]))
        assert g.edata["a"].reshape(-1).tolist() == [1, 1, 2, 2, 1]
    assert g.edata["a"].reshape(-1).tolist() == [1, 1, 2, 2, 0]


def test_accelerated_attention_uses_node_ids_and_deep_stacks_fall_back():
    """compat.accelerate: compute_attention goes through _node_embeddings (entity_embed(ndata['id']),
    models.py:140-141) - identical to the table only for ids = arange(N); and the sharded readout
    takes the one-pass concat kernel only for stacks it covers (<= 8 blocks)."""
    import inspect
    from dgl_kgat_amd import kgat_layer
    src = inspect.getsource(kgat_layer.KGATPropagation.compute_attention)
    assert "_node_embeddings(g)" in src
    assert "len(blocks) <= 8" in inspect.getsource(kgat_layer.KGATPropagation._gnn_fused_sharded)


def test_eval_plan_matches_per_user_construction():
    """metrics.EvalPlan's array construction against the per-user definition (reference metric.py:36-68 reads
    train_user_dict[u] / test_user_dict[u] per user): users in the test dict's key order, train lists sorted and
    de-duplicated (score[train] = 0.0 masks an item once), test lists sorted with their duplicates (len() counts them),
    users without a train list, empty lists, out-of-range items -> IndexError, and no state kept between calls."""
    import torch
    from dgl_kgat_amd import metrics
    rng = np.random.default_rng(3)
    n_i = 50
    users = [7, 3, 11, 0, 5]
    test = {u: rng.integers(0, n_i, rng.integers(0, 6)) for u in users}
    train = {u: rng.integers(0, n_i, rng.integers(0, 30)) for u in users if u != 11}
    train[99] = np.array([1, 2])                                      # a train-only user is ignored
    test[3] = np.array([4, 4, 9])
    plan = metrics.EvalPlan(train, test, np.arange(100, 100 + n_i), torch.device("cpu"))
    assert plan.user_ids.tolist() == users and plan.item_ids.tolist() == list(range(100, 150))
    for k, u in enumerate(users):
        tr = plan.train_items[plan.train_ptr[k]:plan.train_ptr[k + 1]].numpy()
        te = plan.test_items[plan.test_ptr[k]:plan.test_ptr[k + 1]].numpy()
        assert np.array_equal(tr, np.unique(train.get(u, np.zeros(0, np.int64))))
        assert np.array_equal(te, np.sort(test[u]))
    assert plan.max_node_id == 149
    with pytest.raises(IndexError):
        metrics.EvalPlan({7: np.array([n_i])}, test, np.arange(100, 100 + n_i), torch.device("cpu"))
    # the same dict object edited in place gives a different plan (round 5 cached on id() + len(): ADVICE round 5)
    test[3][:] = [1, 2, 3]
    plan2 = metrics.EvalPlan(train, test, np.arange(100, 100 + n_i), torch.device("cpu"))
    assert plan2.test_items[plan2.test_ptr[1]:plan2.test_ptr[2]].tolist() == [1, 2, 3]
    assert not hasattr(metrics, "_last_plan")
