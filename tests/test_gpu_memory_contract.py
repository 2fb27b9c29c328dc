"""Every entry of include/kgat_hip.h that takes scratch memory, held to the header's three promises about memory:

    scratch is "passed in by the caller (`*_workspace_bytes`)"  - a caller may allocate exactly that many bytes;
    "outputs are always fully overwritten";
    the library "allocates nothing persistent"                 - no result may depend on what a buffer held before.

Every case calls its op through the public ``ops`` function on the same inputs, five times (tests/_arena.py):

    clean      no patching: the result the other tests tie to fp64;
    zeroed     every workspace a guarded buffer of exactly the bytes the size function answered, filled with zeros;
    0x00000001 workspaces AND every ``torch.empty`` / ``torch.empty_like`` of the op layer guarded and filled with that
               word - as an int32 a count or an index of one, as a float a denormal;
    0xFFC0DEAD the same with a NaN word - only after the asserts of the pass before held (a kernel that takes
               uninitialised scratch for a count or an index shows up there as a wrong bit or a write into a band; a
               NaN word is never used as an address by a kernel that got this far);
    0xC2280000 the same with -42.0f, a finite word: scratch read as a float where a NaN would be skipped by a comparison.

After each patched pass, and after a device synchronize: every 4,096-byte guard band around every allocation is intact;
no returned tensor holds a poison word that the clean result does not hold at that place; every returned tensor has the
bits of the clean pass.  The asserts of a pass come before the next pass starts.  A case proves that it reached its
entries: the C calls made during a pass are noted (the library handle is wrapped for the pass) and every entry the
case names must be among them.

WAIVERS lists the outputs the header says are partly written, each with the sentence that grants it; there the written
words are held to the rules above and every OTHER word must still be the poison - nothing outside was touched.  Guard
bands have no waiver, and no entry is compared at a tolerance: the header calls every one of them reproducible.

test_every_scratch_entry_has_a_case parses the header for every function with a ``void* workspace`` parameter, every
function that writes a caller-sized partials buffer (sized by a ``kgat_*_partials`` function) and kgat_permute_f32's
``tmp``, and fails for one that no case names.

Left out for size: the softmax's 1,024-position form (more than 8 M edges) and the three-level scan (more than 16 M
keys); tests/test_gpu_softmax_wide.py and the sort-class tests of tests/test_gpu_parity.py run those shapes.  The blocks
kgat_transr_presort_f32 / kgat_mf_presort_f32 write are outputs whose pieces are 256-byte aligned with unwritten gaps:
they are held by their guard bands and through the bits of the steps that consume them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _arena  # noqa: E402

# 1: a count or an index of one, a denormal as a float.  0xFFC0DEAD: a NaN.  0xC2280000 = -42.0f: finite, so that it is
# taken where a comparison skips a NaN - the evaluation sweeps' shared thresholds decode both other words to a NaN
# (kgat_eval_common.h from_ordered_bits) and this one to a threshold of 42 - and negative as an int32
POISONS = (0x00000001, 0xFFC0DEAD, 0xC2280000)

# output (case function, name) -> the header sentence that says it is partly written
WAIVERS = {
    "edge_softmax shard: out, out_csr":
        "over the incoming edges of each destination, all relations together, for the CSR positions [e_begin, e_end) "
        "(the whole graph: 0, E; a destination-range shard: its indptr range)",
    "column slices of a wider buffer: self_out, norm_out":
        "the launch also writes X[v, :] to self_out[(v - row0) * self_stride + 0..D)" " / "
        "norm_out (may be NULL) receives Z / max(||Z_row||_2, 1e-12) with row stride norm_stride floats (a column slice "
        "of the concatenated output)",
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ the three passes
class Partial:
    """An output the header says is partly written: `written` is a bool tensor over the tensor's 32-bit words."""

    def __init__(self, tensor, written, waiver):
        assert waiver in WAIVERS
        self.tensor, self.written, self.waiver = tensor, written.reshape(-1), waiver


def _words(t):
    flat = t.contiguous().view(-1).view(torch.uint8)
    assert flat.numel() % 4 == 0, "outputs are whole 32-bit words"
    return flat.view(torch.int32)


def _split(outs):
    plain = {}
    for name, v in outs.items():
        plain[name] = (v.tensor, v.written) if isinstance(v, Partial) else (v, None)
    return plain


def _compare(tag, what, clean, got, poison):
    """The poison-left and same-bits asserts of one pass; `poison` None: bits only."""
    assert set(clean) == set(got)
    for name in clean:
        (ct, written), (gt, _) = clean[name], got[name]
        assert ct.shape == gt.shape and ct.dtype == gt.dtype, (tag, name)
        cw, gw = _words(ct), _words(gt)
        inside = torch.ones_like(cw, dtype=torch.bool) if written is None else written
        if poison is not None:
            is_poison = gw == _arena._signed32(poison)
            left = int((is_poison & (cw != gw) & inside).sum())
            assert left == 0, "%s: poison left: %d of %d words of `%s` still hold %#010x (%s)" % (
                tag, left, int(inside.sum()), name, poison, what)
            if written is not None:
                touched = int((~is_poison & ~inside).sum())
                assert touched == 0, "%s: %d words of `%s` outside what the header says is written were written (%s)" % (
                    tag, touched, name, what)
        diff = int(((cw != gw) & inside).sum())
        assert diff == 0, "%s: bits changed: %d of %d words of `%s` differ from the clean pass (%s)" % (
            tag, diff, int(inside.sum()), name, what)


def check_contract(tag, entries, run, dev):
    """`run(alloc)` -> {name: tensor | Partial}; alloc(shape, dtype) makes the buffers the CALLER hands to the op."""
    from dgl_kgat_amd import ops

    def plain(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    clean = _split(run(plain))
    torch.cuda.synchronize()
    with _arena.patched(ops, 0, scratch_only=True) as ar:
        got = _split(run(plain))
        torch.cuda.synchronize()
    bad = ar.broken_bands()
    assert not bad, "%s %s: band: %s (zero-filled scratch of exactly the size asked for)" % (tag, entries, bad)
    _compare("%s %s" % (tag, entries), "zero-filled scratch", clean, got, None)
    for poison in POISONS:
        with _arena.patched(ops, poison) as ar:
            got = _split(run(lambda shape, dtype: ar.empty(tuple(shape), dtype, dev, "caller's buffer")))
            torch.cuda.synchronize()
        missing = [e for e in entries if e not in ar.calls]
        assert not missing, "%s: the case never called %s (called: %s)" % (tag, missing, sorted(set(ar.calls)))
        bad = ar.broken_bands()
        assert not bad, "%s %s: band: %s (poison %#010x)" % (tag, entries, bad, poison)
        _compare("%s %s" % (tag, entries), "poison %#010x" % poison, clean, got, poison)


# ------------------------------------------------------------------------------------------------ inputs
def t32(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)


def tf(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


R = 5
GRAPH_SPECS = {
    # n, e, hub, rows without in-edges: 256-key sort blocks / 256-edge tiles, several of them, a ragged last one
    "small": (300, 5000, 1500, 40),
    # 2^20 + 1: the sort's 4,096-key class and a two-level scan; the reducers' other tile class (see _tile_classes)
    "big": (3000, (1 << 20) + 1, 300000, 100),
}
_GRAPHS = {}


class Graph:
    def __init__(self, name, dev):
        from dgl_kgat_amd import ops
        from dgl_kgat_amd.graph import CSR
        from test_gpu_parity import random_graph
        self.n, self.e, hub, iso = GRAPH_SPECS[name]
        src, dst = random_graph(5, self.n, self.e, hub, iso)
        for row in range(200, 205):                                   # five single-edge rows: all but one edge go to row 0
            dst[np.flatnonzero(dst == row)[1:]] = 0
        rng = np.random.default_rng(6)
        et = rng.integers(0, R + 2, self.e).astype(np.int32)          # types R and R + 1 are never scored
        self.dev, self.src, self.dst, self.et = dev, t32(src, dev), t32(dst, dev), t32(et, dev)
        self.csr = CSR(*ops.csr_from_coo(self.n, self.src, self.dst))
        self.rev = CSR(*ops.csr_from_coo(self.n, self.dst, self.src))
        self.w = tf(rng.random(self.e) + 0.01, dev)                   # CSR order
        self.logits = tf(3 * rng.standard_normal(self.e), dev)
        self._x, self._groups = {}, {}
        deg = np.bincount(dst, minlength=self.n)
        assert (deg == 0).sum() >= iso and deg.max() > 1024          # rows without in-edges, a hub across many tiles
        if name == "small":
            assert (deg == 1).sum() >= 5                              # single-edge rows

    def X(self, *shape):
        if shape not in self._x:
            rng = np.random.default_rng(100 + sum(shape))
            self._x[shape] = tf(rng.standard_normal((self.n,) + shape), self.dev)
        return self._x[shape]

    def groups(self, n_rel):
        """The relation-grouped statics of graph.rel_groups, rebuilt per n_rel."""
        from dgl_kgat_amd import ops
        from dgl_kgat_amd.graph import RelGroups
        if n_rel not in self._groups:
            csr = self.csr
            rel_ptr, idx = ops.group_by_relation(ops.gather(csr.eid, self.et), n_rel)
            dst_g = ops.gather(idx, csr.row_of)
            gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
            self._groups[n_rel] = RelGroups(rel_ptr, ops.gather(idx, csr.eid), ops.gather(idx, csr.col), dst_g, idx, gid, gptr,
                                            g_node, n_groups, {})
        return self._groups[n_rel]


def graph(name, dev):
    if name not in _GRAPHS:
        _GRAPHS[name] = Graph(name, dev)
    return _GRAPHS[name]


def _tile(e, D):
    from dgl_kgat_amd import _lib
    return int(_lib.load().kgat_spmm_tile_edges(e, D))


def test_the_two_graphs_take_the_two_tile_classes():
    """e = 90,000 still takes the short runs at every width (4,096 tiles of 256 edges reach 1,048,576 edges): the second
    graph is the smallest that does not."""
    small, big = GRAPH_SPECS["small"][1], GRAPH_SPECS["big"][1]
    for D in (16, 32, 64, 128):
        assert _tile(90000, D) == _tile(small, D), D
        if D < 128:                                # (rows of 512 bytes leave the short runs at 2^19 edges already)
            assert _tile(big - 1, D) == _tile(small, D), D
        assert _tile(big, D) > _tile(small, D), D
        assert small > 2 * _tile(small, D) and small % _tile(small, D) and big % _tile(big, D)


def _slice_mask(n, width, lo, hi, dev):
    m = torch.zeros((n, width), dtype=torch.bool, device=dev)
    m[:, lo:hi] = True
    return m


# ------------------------------------------------------------------------------------------------ graph structure
@pytest.mark.parametrize("name", ["small", "big"])
@pytest.mark.gpu
def test_csr_from_coo(dev, name):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    check_contract("csr_from_coo %s" % name, ["kgat_csr_from_coo"],
                   lambda alloc: dict(zip(("indptr", "col", "eid", "row_of"), ops.csr_from_coo(g.n, g.src, g.dst))), dev)


@pytest.mark.parametrize("name, n_rel", [("small", R), ("small", 1), ("big", 41)])
@pytest.mark.gpu
def test_group_by_relation(dev, name, n_rel):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    et = t32(np.random.default_rng(7).integers(-2, n_rel + 3, g.e), dev)       # types outside [0, R) included
    check_contract("group_by_relation %s R=%d" % (name, n_rel), ["kgat_group_by_relation"],
                   lambda alloc: dict(zip(("rel_ptr", "perm"), ops.group_by_relation(et, n_rel))), dev)


@pytest.mark.parametrize("n", [300, (1 << 20) + 1])
@pytest.mark.gpu
def test_row_order_by_degree(dev, n):
    from dgl_kgat_amd import ops
    if n == 300:
        indptr = graph("small", dev).csr.indptr
    else:
        deg = np.random.default_rng(8).integers(0, 4, n)
        deg[5], deg[n - 2] = 70000, 65536
        indptr = t32(np.concatenate([[0], np.cumsum(deg)]), dev)
    check_contract("row_order_by_degree n=%d" % n, ["kgat_row_order_by_degree"],
                   lambda alloc: dict(order=ops.row_order_by_degree(indptr)), dev)


@pytest.mark.parametrize("n_rel", [R, 1])
@pytest.mark.gpu
def test_head_groups_fold_tiles_pack_records(dev, n_rel):
    from dgl_kgat_amd import ops
    g = graph("small", dev)
    gr = g.groups(n_rel)
    assert gr.n_groups > 32

    def run(alloc):
        gid, gptr, g_node, n_groups = ops.head_groups(gr.rel_ptr, gr.dst_g)
        out = dict(gid=gid, gptr=gptr, g_node=g_node, n_groups=torch.tensor([n_groups], dtype=torch.int32, device=dev))
        for cap in (64, 256):
            tiles, rel_tptr, part_tptr = ops.fold_tiles(gr.rel_ptr, gid, gptr, n_groups, cap=cap, n_parts=37)
            out.update({"tiles%d" % cap: tiles, "rel_tptr%d" % cap: rel_tptr, "part_tptr%d" % cap: part_tptr})
        out["rec_g"] = ops.att_pack_records(gr.rel_ptr, gptr, gid, gr.src_g)
        return out
    check_contract("head_groups + fold_tiles R=%d" % n_rel,
                   ["kgat_head_groups", "kgat_fold_tiles", "kgat_fold_tile_parts", "kgat_att_pack_records"], run, dev)


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.gpu
def test_att_score_bwd(dev, d):
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.graph import att_bwd_statics
    g = graph("small", dev)
    gr = g.groups(R)
    s = att_bwd_statics(gr, g.n)
    rng = np.random.default_rng(9 + d)
    ent, W, rel = tf(rng.standard_normal((g.n, d)), dev), tf(rng.standard_normal((R, d, d)) / d ** 0.5, dev), \
        tf(rng.standard_normal((R, d)), dev)
    gamma = tf(rng.standard_normal(g.e), dev)
    assert 0 < s.n_scored < g.e

    def run(alloc):
        return dict(zip(("grad_ent", "grad_W", "grad_rel"),
                        ops.att_score_bwd(g.n, s.n_scored, gr.n_groups, gr.perm, gr.src_g, gr.gid, s.gstart, gr.gptr, gr.g_node,
                                          s.node_ptr, s.node_col, s.node_row, s.node_wsrc, ent, W, rel, gamma)))
    check_contract("att_score_bwd d=k=%d" % d, ["kgat_att_score_bwd_f32"], run, dev)


# ------------------------------------------------------------------------------------------------ edge softmax
@pytest.mark.parametrize("form", ["sweep", "three_pass", "shard"])
@pytest.mark.gpu
def test_edge_softmax(dev, form):
    from dgl_kgat_amd import ops
    g = graph("small", dev)
    csr = g.csr
    ip = csr.indptr.cpu().numpy()
    assert g.e > 9 * 512 and np.diff(ip).max() > 2 * 512

    def run(alloc):
        if form != "shard":
            out, out_csr = ops.edge_softmax(csr.indptr, csr.row_of, csr.eid, g.logits, want_csr=True, three_pass=form == "three_pass")
            return dict(out=out, out_csr=out_csr)
        e0, e1 = int(ip[3]), int(ip[151])                            # the rows [3, 151): the hub row 3 and what follows
        out, out_csr = ops.edge_softmax(csr.indptr, csr.row_of, csr.eid, g.logits, want_csr=True, e_range=(e0, e1))
        in_csr = torch.zeros(g.e, dtype=torch.bool, device=dev)
        in_csr[e0:e1] = True
        in_eid = torch.zeros(g.e, dtype=torch.bool, device=dev)
        in_eid[csr.eid[e0:e1].long()] = True
        w = "edge_softmax shard: out, out_csr"
        return dict(out=Partial(out, in_eid, w), out_csr=Partial(out_csr, in_csr, w))
    check_contract("edge_softmax %s" % form,
                   ["kgat_edge_softmax_3pass_f32" if form == "three_pass" else "kgat_edge_softmax_f32"], run, dev)


_PERM_GRAPHS = {}


@pytest.mark.parametrize("case", ["boundaries", "no cut rows"])
@pytest.mark.gpu
def test_edge_softmax_permuted_and_permute(dev, case):
    from dgl_kgat_amd import ops
    import test_gpu_softmax_permuted as P
    if case not in _PERM_GRAPHS:
        _PERM_GRAPHS[case] = P.Graph(case, dev)
    g = _PERM_GRAPHS[case]
    x, xg = g.logits[30.0]

    def run(alloc):
        a, a_csr = ops.edge_softmax_permuted(g.indptr, g.row_of, g.eid, x, g.plan, in_csr_order=True)
        b, b_csr = ops.edge_softmax_permuted(g.indptr, g.row_of, g.gmap, xg, g.plan, in_csr_order=False)
        return dict(out=a, out_csr=a_csr, out_grouped=b, out_csr_grouped=b_csr, permuted=ops.permute(g.plan, x))
    check_contract("edge_softmax_permuted + permute, %s" % case, ["kgat_edge_softmax_permuted_f32", "kgat_permute_f32"], run, dev)


# ------------------------------------------------------------------------------------------------ the reducers
@pytest.mark.parametrize("name", ["small", "big"])
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("algo", ["merge", "merge1", "rows", "generic", "mul_self", "self_out", "eid", "defer"])
@pytest.mark.gpu
def test_spmm(dev, algo, D, name):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    csr, X = g.csr, g.X(D)
    order = ops.row_order_by_degree(csr.indptr)
    w_eid = ops.gather(ops.invert_permutation(csr.eid), g.w)          # the same weights in edge-id order
    W = tf(np.random.default_rng(10).standard_normal((D, D)) / D ** 0.5, dev)
    entries = ["kgat_spmm_umule_sum_f32"]

    def run(alloc):
        if algo in ("merge", "merge1", "generic"):
            return dict(out=ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, algo=algo))
        if algo == "rows":
            return dict(out=ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, algo="rows", order=order),
                        unordered=ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, algo="rows"))
        if algo == "eid":
            return dict(out=ops.spmm(csr.indptr, csr.col, csr.row_of, X, w_eid, eid=csr.eid))
        if algo == "mul_self":
            return dict(out=ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, mul_self=True))
        if algo == "self_out":
            wide = alloc((g.n, 2 * D + 8), torch.float32)
            out = ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, mul_self=True, self_out=wide[:, 4:4 + D])
            return dict(out=out, wide=Partial(wide, _slice_mask(g.n, 2 * D + 8, 4, 4 + D, dev), "column slices of a wider buffer: self_out, norm_out"))
        hn, deferred = ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, defer_finish=True)
        h = ops.aggregator(ops.FORMS["Bi"], X, hn, W, deferred=deferred)
        hn2, deferred2 = ops.spmm(csr.indptr, csr.col, csr.row_of, X, g.w, defer_finish=True)
        h2 = ops.aggregator(ops.BI2_FORM, X, hn2, (W, W), deferred=deferred2)
        return dict(h=h, h_bi2=h2)
    if algo == "defer":
        entries += ["kgat_aggregator_deferred_f32", "kgat_bi2_deferred_f32"]
    check_contract("spmm %s D=%d %s" % (algo, D, name), entries, run, dev)


@pytest.mark.parametrize("name", ["small", "big"])
@pytest.mark.parametrize("d_in, d_out", [(64, 64), (32, 16)])
@pytest.mark.gpu
def test_spmm_bi_fused(dev, d_in, d_out, name):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    csr, X = g.csr, g.X(d_in)
    W2 = tf(np.random.default_rng(11).standard_normal((d_out, d_in)) / d_in ** 0.5, dev)
    width = d_in + d_out + 8

    def run(alloc):
        wide = alloc((g.n, width), torch.float32)
        h = ops.spmm_bi_fused(csr.indptr, csr.col, csr.row_of, X, g.w, W2, norm_out=wide[:, 4 + d_in:4 + d_in + d_out],
                              self_out=wide[:, 4:4 + d_in])
        return dict(h=h, wide=Partial(wide, _slice_mask(g.n, width, 4, 4 + d_in + d_out, dev), "column slices of a wider buffer: self_out, norm_out"))
    check_contract("spmm_bi_fused (%d, %d) %s" % (d_in, d_out, name), ["kgat_spmm_bi_fused_f32"], run, dev)


@pytest.mark.parametrize("name", ["small", "big"])
@pytest.mark.parametrize("D", [16, 64, 20])
@pytest.mark.gpu
def test_copy_reduce_and_max(dev, D, name):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    csr, X = g.csr, g.X(D)

    def run(alloc):
        out = dict(sum=ops.copy_reduce(csr.indptr, csr.col, csr.row_of, X, "sum"),
                   mean=ops.copy_reduce(csr.indptr, csr.col, csr.row_of, X, "mean"))
        out["max"], out["arg"] = ops.spmm_max(csr.indptr, csr.col, csr.row_of, X, g.w, eid=csr.eid)
        out["max_copy"], out["arg_copy"] = ops.spmm_max(csr.indptr, csr.col, csr.row_of, X)
        return out
    check_contract("copy_reduce + spmm_max D=%d %s" % (D, name), ["kgat_copy_reduce_f32", "kgat_spmm_umule_max_f32"], run, dev)


@pytest.mark.parametrize("name", ["small", "big"])
@pytest.mark.parametrize("Q", [4, 16])
@pytest.mark.gpu
def test_spmm_max4(dev, Q, name):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    csr, X = g.csr, g.X(Q, 4)
    check_contract("spmm_max4 Q=%d %s" % (Q, name), ["kgat_spmm_umule_max4_f32"],
                   lambda alloc: dict(zip(("out", "arg_edge", "arg_slot"),
                                          ops.spmm_max4(csr.indptr, csr.col, csr.row_of, X, g.w, eid=csr.eid))), dev)


# tile classes of the graph attention (tests/test_gpu_gat_shapes.py: 128 and 256 planted, 512 and 1,024 in production)
GAT_CASES = [("small", 8, 16, 128), ("small", 4, 4, 256), ("big", 8, 16, 512), ("big", 4, 16, 1024)]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("name, H, F, te", GAT_CASES)
@pytest.mark.gpu
def test_gat(dev, name, H, F, te, p):
    from dgl_kgat_amd import ops
    g = graph(name, dev)
    assert _tile(g.e, H * F) == te
    rng = np.random.default_rng(12 + H * F)
    ft = g.X(H, F)
    el, er = tf(2 * rng.standard_normal((g.n, H)), dev), tf(2 * rng.standard_normal((g.n, H)), dev)
    g_out = tf(rng.standard_normal((g.n, H, F)), dev)

    def run(alloc):
        out, m, l = ops.gat_forward(g.csr, ft, el, er, 0.2, p, 77)
        g_ft, g_el, g_er = ops.gat_backward(g.csr, g.rev, ft, el, er, m, l, out, g_out, 0.2, p, 77)
        return dict(out=out, m=m, l=l, g_ft=g_ft, g_el=g_el, g_er=g_er)
    check_contract("gat H=%d F=%d %s p=%.1f" % (H, F, name, p), ["kgat_gat_fwd_f32", "kgat_gat_bwd_f32"], run, dev)


# ------------------------------------------------------------------------------------------------ training steps
TRANSR = [(900, 3, 700, 20, 12), (3000, 41, 2048, 32, 64)]      # (n, R, B, d, k): the two sort paths


def _transr_inputs(dev, n, n_rel, B, d, k, n_batches=1):
    rng = np.random.default_rng(13 + B)
    ids = [t32(rng.integers(0, hi, (n_batches, B)), dev) for hi in (n, n_rel, n, n)]
    ids[0][:, : B // 3] = 7                                        # a popular head: long runs of one row
    ent, W, rel = tf(rng.standard_normal((n, d)), dev), tf(rng.standard_normal((n_rel, d, k)) / d ** 0.5, dev), \
        tf(rng.standard_normal((n_rel, k)), dev)
    return ids, ent, W, rel


@pytest.mark.parametrize("n, n_rel, B, d, k", TRANSR)
@pytest.mark.gpu
def test_transr_loss_forward_backward(dev, n, n_rel, B, d, k):
    from dgl_kgat_amd import ops
    assert ops.transr_supported(n, d, k, n_rel, B)
    (h, r, pt, nt), ent, W, rel = _transr_inputs(dev, n, n_rel, B, d, k)
    h, r, pt, nt = h[0], r[0], pt[0], nt[0]
    scale = tf([0.37], dev)

    def run(alloc):
        loss, ws = ops.transr_forward(h, r, pt, nt, ent, W, rel, 1e-3)
        g_ent, g_w, g_rel = ops.transr_backward(h, r, pt, nt, (ent.shape, W.shape), ws, grad_scale=scale)
        one = ops.transr_loss_grad(h, r, pt, nt, ent, W, rel, 1e-3)
        return dict(loss=loss.reshape(1), g_ent=g_ent, g_w=g_w, g_rel=g_rel, loss1=one[0].reshape(1), g_ent1=one[1], g_w1=one[2],
                    g_rel1=one[3])
    check_contract("transr (%d, %d, %d, %d, %d)" % (n, n_rel, B, d, k),
                   ["kgat_transr_forward_f32", "kgat_transr_backward_f32", "kgat_transr_loss_grad_f32"], run, dev)


@pytest.mark.parametrize("n, n_rel, B, d, k", TRANSR)
@pytest.mark.gpu
def test_transr_presort_and_two_adam_steps(dev, n, n_rel, B, d, k):
    """Two consecutive steps on one state object: the second step's tag must not take the first step's row_slot words."""
    from dgl_kgat_amd import ops
    ids, ent0, W0, rel0 = _transr_inputs(dev, n, n_rel, B, d, k, n_batches=2)

    def run(alloc):
        params = [t.clone() for t in (ent0, W0, rel0)]
        m, v = [torch.zeros_like(t) for t in params], [torch.zeros_like(t) for t in params]
        state = ops.TransRAdamState(n, d, k, n_rel, B, dev)
        sorted_all, stride = ops.transr_presort(*ids, n, n_rel)
        arr_m, arr_v = (C.c_void_p * 3)(*[t.data_ptr() for t in m]), (C.c_void_p * 3)(*[t.data_ptr() for t in v])
        losses = alloc((2,), torch.float32)
        for i in range(2):
            ops.transr_adam_step(ids[0][i], ids[1][i], ids[2][i], ids[3][i], sorted_all[i * stride:(i + 1) * stride], *params,
                                 arr_m, arr_v, [i + 1] * 3, 1e-2, 0.9, 0.999, 1e-8, 1e-3, losses[i:i + 1], state)
        assert state.tag == 2
        out = dict(losses=losses)
        for name, ts in (("p", params), ("m", m), ("v", v)):
            out.update({"%s%d" % (name, i): t for i, t in enumerate(ts)})
        return out
    check_contract("transr_presort + 2 adam steps (%d, %d, %d, %d, %d)" % (n, n_rel, B, d, k),
                   ["kgat_transr_presort_f32", "kgat_transr_adam_step_f32"], run, dev)


BPR = [(300, 16, 13), (4000, 128, 2730), (4000, 16, 2731)]          # (n, F, B); 3 x 2,731 > 8,192: the other presort


def _bpr_inputs(dev, n, F, B, n_batches=1):
    rng = np.random.default_rng(14 + B)
    ids = [t32(rng.integers(0, n, (n_batches, B)), dev) for _ in range(3)]
    ids[0][:, : B // 2] = 11                                       # a popular user: a run across many windows
    return ids, tf(rng.standard_normal((n, F)), dev)


@pytest.mark.parametrize("n, F, B", BPR)
@pytest.mark.gpu
def test_bpr_loss_and_grad(dev, n, F, B):
    from dgl_kgat_amd import ops
    (u, p, q), emb = _bpr_inputs(dev, n, F, B)
    u, p, q = u[0], p[0], q[0]
    scale = tf([0.5], dev)

    def run(alloc):
        loss, coef, ws = ops.bpr_loss(emb, u, p, q, 1e-3)
        grad = ops.bpr_grad(emb, u, p, q, coef, 1e-3, grad_scale=scale, workspace=ws)
        grad2 = ops.bpr_grad(emb, u, p, q, coef, 1e-3)                # a workspace of its own
        return dict(loss=loss.reshape(1), coef=coef, grad=grad, grad2=grad2)
    check_contract("bpr (%d, %d, %d)" % (n, F, B), ["kgat_bpr_loss_f32", "kgat_bpr_grad_f32"], run, dev)


@pytest.mark.parametrize("n, F, B", BPR)
@pytest.mark.gpu
def test_mf_presort_and_two_adam_steps(dev, n, F, B):
    from dgl_kgat_amd import ops
    assert ops.mf_supported(n, F, B)
    ids, emb0 = _bpr_inputs(dev, n, F, B, n_batches=2)

    def run(alloc):
        emb = emb0.clone()
        m, v = torch.zeros_like(emb), torch.zeros_like(emb)
        state = ops.MFAdamState(n, F, B, dev)
        sorted_all, stride = ops.mf_presort(*ids, n)
        losses = alloc((2,), torch.float32)
        for i in range(2):
            ops.mf_adam_step(ids[0][i], ids[1][i], ids[2][i], sorted_all[i * stride:(i + 1) * stride], emb, m, v, i + 1, 1e-2, 0.9,
                             0.999, 1e-8, 1e-3, losses[i:i + 1], state)
        assert state.tag == 2
        return dict(losses=losses, emb=emb, m=m, v=v)
    check_contract("mf_presort + 2 adam steps (%d, %d, %d)" % (n, F, B), ["kgat_mf_presort_f32", "kgat_mf_adam_step_f32"], run, dev)


# ------------------------------------------------------------------------------------------------ evaluation
# (n_users, n_items, F): the register form with several segments, KG 22, the LDS form with one wavefront per workgroup
EVAL = [(97, 2300, 96), (70, 1800, 352), (40, 300, 520)]


def _eval_inputs(dev, n_u, n_i, F):
    rng = np.random.default_rng(15 + F)
    emb = tf(rng.standard_normal((n_u + n_i, F)), dev)

    def lists(lo, hi):
        rows = [np.sort(rng.choice(n_i, rng.integers(lo, hi), replace=False)) for _ in range(n_u)]
        rows[n_u // 2] = rows[n_u // 2][:0]                        # one user without a list
        return t32(np.concatenate([[0], np.cumsum([len(x) for x in rows])]), dev), t32(np.concatenate(rows), dev)
    return (emb, t32(np.arange(n_u), dev), t32(n_u + np.arange(n_i), dev)) + lists(0, 60) + lists(1, 30)


@pytest.mark.parametrize("n_u, n_i, F", EVAL)
@pytest.mark.gpu
def test_eval_entries(dev, n_u, n_i, F):
    from dgl_kgat_amd import ops
    emb, users, items, tr_ptr, tr_items, te_ptr, te_items = _eval_inputs(dev, n_u, n_i, F)

    def run(alloc):
        out = dict(zip(("recall", "ndcg", "topk20"),
                       ops.eval_recall_ndcg(emb, users, items, tr_ptr, tr_items, te_ptr, te_items, 20, want_topk=True)))
        for K in (40, 100):
            for drop in (False, True):
                out["topk%d%d" % (K, drop)], out["scores%d%d" % (K, drop)] = ops.eval_topk(emb, users, items, tr_ptr, tr_items, K,
                                                                                         drop_train=drop)
        for drop in (False, True):
            above, scores = ops.eval_rank(emb, users, items, tr_ptr, tr_items, te_ptr, te_items, drop_train=drop, want_scores=True)
            cand = n_i if not drop else (n_i - (tr_ptr[1:] - tr_ptr[:-1])).to(torch.int32).contiguous()
            at_k, scalar = ops.eval_rank_metrics(above, te_ptr, te_items, cand, [1, 20, 100], n_items=n_i)
            out.update({"above%d" % drop: above, "rank_scores%d" % drop: scores, "at_k%d" % drop: at_k, "scalar%d" % drop: scalar})
        return out
    check_contract("eval (%d, %d, %d)" % (n_u, n_i, F),
                   ["kgat_eval_recall_ndcg_f32", "kgat_eval_topk_f32", "kgat_eval_rank_f32", "kgat_eval_rank_metrics"], run, dev)


# ------------------------------------------------------------------------------------------------ partial sums
@pytest.mark.gpu
def test_grad_norm_and_clipped_adam_step(dev):
    from dgl_kgat_amd import ops
    from dgl_kgat_amd.optim import FusedAdam
    rng = np.random.default_rng(16)
    sizes = [1, 7, 4099, 64000]
    p0 = [tf(rng.standard_normal(s), dev) for s in sizes]
    grads = [tf(rng.standard_normal(s), dev) for s in sizes]

    def run(alloc):
        params = [torch.nn.Parameter(t.clone()) for t in p0]
        for p, g_ in zip(params, grads):
            p.grad = g_.clone()
        opt = FusedAdam(params, lr=1e-2)
        norm_out = alloc((1,), torch.float32)
        opt.step(max_grad_norm=0.5, norm_out=norm_out)
        norm, coef = ops.grad_norm(grads, 0.5)
        out = dict(norm_out=norm_out, norm=norm.reshape(1), coef=coef.reshape(1))
        out.update({"p%d" % i: p.detach() for i, p in enumerate(params)})
        return out
    check_contract("grad_norm + clipped FusedAdam step", ["kgat_grad_sumsq_f32", "kgat_grad_norm_finish_f32",
                                                          "kgat_adam_step_clipped_f32"], run, dev)


@pytest.mark.parametrize("n_rows", [1, 5000])
@pytest.mark.gpu
def test_weight_gradient_partials(dev, n_rows):
    from dgl_kgat_amd import ops
    rng = np.random.default_rng(17 + n_rows)
    d_in, d_out = 32, 16
    H, HN = tf(rng.standard_normal((n_rows, d_in)), dev), tf(rng.standard_normal((n_rows, d_in)), dev)
    gz, gz2 = tf(rng.standard_normal((n_rows, d_out)), dev), tf(rng.standard_normal((n_rows, d_out)), dev)

    def run(alloc):
        out = {}
        for form in ("Bi", "GCN", "GraphSage"):
            out[form] = ops.aggregator_bwd_weight(ops.FORMS[form], gz, H, HN)
            out[form + " partials"] = ops.sum_partials([ops.aggregator_bwd_weight(ops.FORMS[form], gz, H, HN, want_partials=True)])[0]
        out["bi_interaction_bwd_weight"] = ops.bi_interaction_bwd_weight(gz, H, HN)
        out["Bi2 w1"], out["Bi2 w2"] = ops.aggregator_bwd_weight(ops.BI2_FORM, (gz, gz2), H, HN)
        out["sage self"], out["sage neigh"], out["sage bias"] = ops.sage_bwd_weight(gz, H, HN)
        return out
    check_contract("weight-gradient partials, %d rows" % n_rows,
                   ["kgat_aggregator_bwd_weight_f32", "kgat_bi2_bwd_weight_f32", "kgat_sage_bwd_weight_f32", "kgat_sum_partials_f32"],
                   run, dev)


# ------------------------------------------------------------------------------------------------ completeness
# entry -> the test(s) above that reach it (check_contract asserts the call was made)
COVERAGE = {
    "kgat_csr_from_coo": "test_csr_from_coo",
    "kgat_group_by_relation": "test_group_by_relation",
    "kgat_row_order_by_degree": "test_row_order_by_degree",
    "kgat_head_groups": "test_head_groups_fold_tiles_pack_records",
    "kgat_fold_tiles": "test_head_groups_fold_tiles_pack_records",
    "kgat_fold_tile_parts": "test_head_groups_fold_tiles_pack_records",
    "kgat_att_score_bwd_f32": "test_att_score_bwd",
    "kgat_edge_softmax_f32": "test_edge_softmax",
    "kgat_edge_softmax_3pass_f32": "test_edge_softmax",
    "kgat_edge_softmax_permuted_f32": "test_edge_softmax_permuted_and_permute",
    "kgat_permute_f32": "test_edge_softmax_permuted_and_permute",
    "kgat_spmm_umule_sum_f32": "test_spmm",
    "kgat_spmm_umule_max_f32": "test_copy_reduce_and_max",
    "kgat_spmm_umule_max4_f32": "test_spmm_max4",
    "kgat_spmm_bi_fused_f32": "test_spmm_bi_fused",
    "kgat_copy_reduce_f32": "test_copy_reduce_and_max",
    "kgat_gat_fwd_f32": "test_gat",
    "kgat_gat_bwd_f32": "test_gat",
    "kgat_transr_loss_grad_f32": "test_transr_loss_forward_backward",
    "kgat_transr_forward_f32": "test_transr_loss_forward_backward",
    "kgat_transr_backward_f32": "test_transr_loss_forward_backward",
    "kgat_transr_adam_step_f32": "test_transr_presort_and_two_adam_steps",
    "kgat_bpr_loss_f32": "test_bpr_loss_and_grad",
    "kgat_bpr_grad_f32": "test_bpr_loss_and_grad",
    "kgat_mf_adam_step_f32": "test_mf_presort_and_two_adam_steps",
    "kgat_eval_recall_ndcg_f32": "test_eval_entries",
    "kgat_eval_topk_f32": "test_eval_entries",
    "kgat_eval_rank_f32": "test_eval_entries",
    "kgat_eval_rank_metrics": "test_eval_entries",
    "kgat_grad_sumsq_f32": "test_grad_norm_and_clipped_adam_step",
    "kgat_aggregator_bwd_weight_f32": "test_weight_gradient_partials",
    "kgat_bi2_bwd_weight_f32": "test_weight_gradient_partials",
    "kgat_sage_bwd_weight_f32": "test_weight_gradient_partials",
}


def scratch_entries():
    """Every function of the header with a `void* workspace` parameter, every one that WRITES a partials buffer the
    caller sizes with a kgat_*_partials function, and kgat_permute_f32 (`tmp`)."""
    from test_workspace_host import declarations
    found = set()
    for name, (_, params) in declarations().items():
        for ctype, pname in params:
            if (ctype, pname) == ("void *", "workspace"):
                found.add(name)
            if ctype == "float *" and (pname.startswith("partials") or pname.startswith("part_") or pname == "tmp"):
                found.add(name)
    return found


def test_every_scratch_entry_has_a_case():
    found = scratch_entries()
    assert len(found) >= 33 and "kgat_permute_f32" in found and "kgat_grad_sumsq_f32" in found
    assert not found - set(COVERAGE), "entries that take scratch and have no case: %s" % sorted(found - set(COVERAGE))
    assert not set(COVERAGE) - found, "not a scratch entry of the header: %s" % sorted(set(COVERAGE) - found)
    # what the arena's proxy cannot see: allocations made through a tensor's own methods
    ops_text = open(os.path.join(ROOT, "dgl-kgat_amd", "ops.py")).read()
    assert not any(w in ops_text for w in (".new_empty(", ".new_zeros(", ".new_full(", ".new_tensor("))
    text = open(os.path.abspath(__file__)).read()
    for entry, test in COVERAGE.items():
        assert test in globals() and callable(globals()[test]), (entry, test)
        body = text.split("def %s(" % test)[1].split("\ndef ")[0]
        assert '"%s"' % entry in body or "'%s'" % entry in body, "%s does not name %s among its entries" % (test, entry)

