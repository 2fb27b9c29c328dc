"""The workspace rule of every entry and the loader's argument types, without a GPU.

1. Every ``kgat_*_workspace_bytes`` function the header declares has a row in CASES (or is named in COVERED_ELSEWHERE
   with the host test that holds its entries to the same rule): the entry that carves the workspace, called with
   otherwise valid sizes and 16-byte aligned HOST buffers standing in for device pointers, refuses ``need - 1`` bytes
   with KGAT_E_WORKSPACE and a message that names the entry - before any device work, or the call could not come back
   with that code from a machine without a device - and returns KGAT_OK with ``need`` bytes at a size that makes it
   return early (no edges, users, rows or tiles).  The table is closed: a size function that is in neither list fails
   ``test_every_size_function_has_a_case``.
2. Every declaration of include/kgat_hip.h - return type and parameter list - is mapped to ctypes and compared with
   ``_lib.SIGNATURES`` position by position: a ``size_t`` bound as ``c_int`` or an ``int64_t`` bound as ``c_int`` loads,
   runs and passes every small-shape test.  (The name-set and argument-count assertions of the other host tests stay.)"""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dgl_kgat_amd import _lib  # noqa: E402

OK, BADARG, WORKSPACE = 0, -1, -3
HEADER = os.path.join(ROOT, "include", "kgat_hip.h")

_BUF = C.create_string_buffer((1 << 16) + 16)    # zeros: a non-null, 16-byte aligned address no case gets as far as using
P = (C.addressof(_BUF) + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ the header, parsed
def declarations():
    """name -> (return type, [(type, parameter name), ...]) for every function include/kgat_hip.h declares."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(kgat_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        plist = []
        if params.strip() != "void":
            for p in params.split(","):
                m = re.match(r"^(.*?)([A-Za-z_]\w*)$", " ".join(p.replace("*", " * ").split()))
                assert m, (name, p)
                plist.append((m.group(1).strip(), m.group(2)))
        assert name not in out, name
        out[name] = (ret, plist)
    return out


SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "unsigned": C.c_uint, "uint32_t": C.c_uint,
           "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


def ctype_of(ctype, is_return=False):
    if "*" in ctype or ctype == "kgat_stream_t":
        return C.c_char_p if is_return and ctype == "const char *" else C.c_void_p
    return SCALARS[ctype]


def test_header_parses_to_every_symbol():
    decl = declarations()
    names = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)))
    assert set(decl) == names - {"kgat_stream_t"}
    assert set(decl) == set(_lib.SIGNATURES)
    assert decl["kgat_version"] == ("int", []) and decl["kgat_last_error"][0] == "const char *"
    assert decl["kgat_permute_f32"][1][1] == ("const uint16_t *", "slot_a")
    assert decl["kgat_csr_from_coo"][1][-2:] == [("size_t", "workspace_bytes"), ("kgat_stream_t", "stream")]


@pytest.mark.parametrize("name", sorted(_lib.SIGNATURES))
def test_loader_binds_the_declared_types(name):
    ret, params = declarations()[name]
    res, args = _lib.SIGNATURES[name]
    assert res is ctype_of(ret, is_return=True), (name, "return type", ret, res)
    assert len(args) == len(params), (name, len(args), len(params))
    for i, ((ctype, pname), bound) in enumerate(zip(params, args)):
        assert bound is ctype_of(ctype), "%s: argument %d (%s %s) is bound as %s" % (name, i, ctype, pname, bound.__name__)


# ------------------------------------------------------------------------------------------------ the workspace rule
class Case:
    """One entry under one size function: `sizes` name -> value for every scalar parameter of the entry, `need` the
    size function's arguments as names of `sizes` (or callables of it), `early` the overrides that make the entry
    return before any device work, `word` what kgat_last_error must name, `code` what a short workspace returns."""

    def __init__(self, entry, word, sizes, need, early, pointers=None, code=WORKSPACE):
        self.entry, self.word, self.sizes, self.need, self.early = entry, word, sizes, need, early
        self.pointers, self.code = pointers or {}, code

    def call(self, lib, sizes, short):
        ret, params = declarations()[self.entry]
        fn_need = self.need(lib, sizes)
        args = []
        for ctype, pname in params:
            if pname == "workspace_bytes":
                args.append(fn_need - short)
            elif pname == "stream":
                args.append(None)
            elif pname in self.pointers:
                args.append(self.pointers[pname])
            elif "*" in ctype:
                args.append(P)
            else:
                assert pname in sizes, "%s: no value for %s %s" % (self.entry, ctype, pname)
                args.append(sizes[pname])
        rc = getattr(lib, self.entry)(*args)
        return rc, (lib.kgat_last_error() or b"").decode(), fn_need


# `early` is None where no size makes the entry do nothing: kgat_csr_from_coo, kgat_group_by_relation, kgat_head_groups,
# kgat_fold_tiles, kgat_fold_tile_parts and kgat_att_score_bwd_f32 write their offsets / zero gradients for an empty
# input too, and the TransR and MF steps refuse a batch of 0 as unsupported.
_EVAL = dict(n_users=97, n_items=2300, F=96, emb_stride=96, K=20)
_TRANSR = dict(n_nodes=1000, n_rel=41, d=64, k=64, batch=65, reg_lambda=0.01)
_ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
_BPR = dict(n_nodes=1000, F=176, emb_stride=176, batch=1366, reg_lambda=1e-5)
_GAT = dict(n_nodes=10, n_edges=20, H=4, F=16, negative_slope=0.2, drop_p=0.0, seed=0)
_MOMENTS = (C.c_void_p * 3)(P, P, P)
_STEPS = (C.c_int64 * 3)(1, 1, 1)


def _transr_need(lib, s):
    return lib.kgat_transr_workspace_bytes(s["batch"], s["d"], s["k"], s["n_rel"])

CASES = {
    "kgat_csr_from_coo_workspace_bytes": [
        Case("kgat_csr_from_coo", "csr_from_coo", dict(n_nodes=300, n_edges=5000),
             lambda lib, s: lib.kgat_csr_from_coo_workspace_bytes(s["n_nodes"], s["n_edges"]), None)],   # always writes indptr
    "kgat_group_by_relation_workspace_bytes": [
        Case("kgat_group_by_relation", "group_by_relation", dict(n_edges=5000, n_rel=5),
             lambda lib, s: lib.kgat_group_by_relation_workspace_bytes(s["n_edges"], s["n_rel"]), None)],   # always writes rel_ptr
    "kgat_row_order_workspace_bytes": [
        Case("kgat_row_order_by_degree", "row_order", dict(n_rows=300),
             lambda lib, s: lib.kgat_row_order_workspace_bytes(s["n_rows"]), dict(n_rows=0))],
    "kgat_head_groups_workspace_bytes": [
        Case("kgat_head_groups", "head_groups", dict(n_edges=5000, n_rel=5),
             lambda lib, s: lib.kgat_head_groups_workspace_bytes(s["n_edges"]), None)],
    "kgat_fold_tiles_workspace_bytes": [
        Case("kgat_fold_tiles", "fold_tiles", dict(n_edges=5000, n_rel=5, n_groups=1200, cap=256),
             lambda lib, s: lib.kgat_fold_tiles_workspace_bytes(s["n_groups"], s["n_rel"]), None)],
    "kgat_fold_tile_parts_workspace_bytes": [
        Case("kgat_fold_tile_parts", "fold_tile_parts",
             dict(t_max=400, n_rel=5, n_parts=37, cost_tile=64, cost_chunk=38, cost_relation=1051),
             lambda lib, s: lib.kgat_fold_tile_parts_workspace_bytes(s["t_max"]), None)],
    "kgat_att_score_bwd_workspace_bytes": [
        Case("kgat_att_score_bwd_f32", "att_score_bwd", dict(n_nodes=300, n_scored=5000, n_groups=1200, d=16, k=16, n_rel=5),
             lambda lib, s: lib.kgat_att_score_bwd_workspace_bytes(s["n_nodes"], s["n_scored"], s["n_groups"], s["d"],
                                                                   s["k"], s["n_rel"]), None)],
    "kgat_edge_softmax_workspace_bytes": [
        Case("kgat_edge_softmax_f32", "edge_softmax", dict(n_nodes=300, e_begin=0, e_end=5000, logits_in_csr_order=1),
             lambda lib, s: lib.kgat_edge_softmax_workspace_bytes(s["n_nodes"], s["e_end"] - s["e_begin"]), dict(e_end=0)),
        Case("kgat_edge_softmax_permuted_f32", "edge_softmax_permuted",
             dict(n_nodes=300, e_begin=0, e_end=5000, logits_in_csr_order=1),
             lambda lib, s: lib.kgat_edge_softmax_workspace_bytes(s["n_nodes"], s["e_end"] - s["e_begin"]), dict(e_end=0),
             pointers=dict(out=P + 16384, out_csr=P + 2 * 16384, tmp=P + 3 * 16384))],   # four distinct buffers
    "kgat_edge_softmax_3pass_workspace_bytes": [
        Case("kgat_edge_softmax_3pass_f32", "edge_softmax_3pass", dict(n_nodes=300, e_begin=0, e_end=5000, logits_in_csr_order=1),
             lambda lib, s: lib.kgat_edge_softmax_3pass_workspace_bytes(s["n_nodes"]), dict(e_end=0))],
    "kgat_transr_workspace_bytes": [
        Case("kgat_transr_loss_grad_f32", "transr", dict(_TRANSR), _transr_need, None),
        Case("kgat_transr_forward_f32", "transr", dict(_TRANSR), _transr_need, None),
        Case("kgat_transr_backward_f32", "transr", dict(_TRANSR), _transr_need, None)],
    "kgat_transr_step_workspace_bytes": [
        Case("kgat_transr_adam_step_f32", "transr_adam_step", dict(_TRANSR, tag=1, **_ADAM),
             lambda lib, s: lib.kgat_transr_step_workspace_bytes(s["batch"], s["d"], s["k"], s["n_rel"]), None,
             pointers=dict(exp_avg_host=C.addressof(_MOMENTS), exp_avg_sq_host=C.addressof(_MOMENTS),
                           steps_host=C.addressof(_STEPS)))],
    "kgat_bpr_workspace_bytes": [
        Case("kgat_bpr_loss_f32", "bpr_loss", dict(_BPR), lambda lib, s: lib.kgat_bpr_workspace_bytes(s["batch"], s["F"]), None),
        Case("kgat_bpr_grad_f32", "bpr_grad", dict(_BPR), lambda lib, s: lib.kgat_bpr_workspace_bytes(s["batch"], s["F"]), None)],
    "kgat_gat_workspace_bytes": [
        Case("kgat_gat_fwd_f32", "gat_fwd", dict(_GAT),
             lambda lib, s: lib.kgat_gat_workspace_bytes(s["n_nodes"], s["n_edges"], s["H"], s["F"], 0), None),
        Case("kgat_gat_bwd_f32", "gat_bwd", dict(_GAT),
             lambda lib, s: lib.kgat_gat_workspace_bytes(s["n_nodes"], s["n_edges"], s["H"], s["F"], 1), None)],
    # the header: "any other Q: KGAT_E_BADARG, as are a null pointer, a negative size and workspace_bytes <
    # kgat_spmm_max4_workspace_bytes(e_end - e_begin, Q)" - this entry's documented code for a short workspace
    "kgat_spmm_max4_workspace_bytes": [
        Case("kgat_spmm_umule_max4_f32", "spmm_max4", dict(n_rows=300, row0=0, e_begin=0, e_end=5000, Q=16),
             lambda lib, s: lib.kgat_spmm_max4_workspace_bytes(s["e_end"] - s["e_begin"], s["Q"]), dict(n_rows=0), code=BADARG)],
    "kgat_mf_step_workspace_bytes": [
        Case("kgat_mf_adam_step_f32", "mf_adam_step", dict(n_nodes=300, F=16, batch=13, step=1, reg_lambda=1e-5, tag=1, **_ADAM),
             lambda lib, s: lib.kgat_mf_step_workspace_bytes(s["batch"], s["F"]), None)],
    "kgat_eval_workspace_bytes": [
        Case("kgat_eval_recall_ndcg_f32", "eval", dict(_EVAL),
             lambda lib, s: lib.kgat_eval_workspace_bytes(s["n_users"], s["n_items"], s["F"], s["K"]), dict(n_users=0))],
    "kgat_eval_topk_workspace_bytes": [
        Case("kgat_eval_topk_f32", "eval_topk", dict(_EVAL, K=40, drop_train=0),
             lambda lib, s: lib.kgat_eval_topk_workspace_bytes(s["n_users"], s["n_items"], s["F"], s["K"]), dict(n_users=0))],
    "kgat_eval_rank_workspace_bytes": [
        Case("kgat_eval_rank_f32", "eval_rank", dict(_EVAL, n_train=900, n_test=400, drop_train=0),
             lambda lib, s: lib.kgat_eval_rank_workspace_bytes(s["n_users"], s["n_items"], s["F"], s["n_train"], s["n_test"]),
             dict(n_users=0, n_train=0, n_test=0))],
    "kgat_eval_rank_metrics_workspace_bytes": [
        Case("kgat_eval_rank_metrics", "eval_rank_metrics", dict(n_users=97, n_items=2300, n_test=400, n_ks=2),
             lambda lib, s: lib.kgat_eval_rank_metrics_workspace_bytes(s["n_test"]), dict(n_users=0, n_test=0),
             pointers=dict(ks=C.cast((C.c_int32 * 2)(5, 20), C.c_void_p)))],
}

# The sum, fused-Bi, copy and max reducers share one plan (kgat_spmm_plan.h): their entries check the bytes the carve
# uses, and their size functions answer those bytes rounded up to 256 plus 256 spare, so "one byte short of the size
# function" still holds what the carve needs.  tests/test_spmm_plan_host.py holds each entry's check at the carved size
# to the byte, with the exact message: size function -> [(test function there, entry it calls short)]
COVERED_ELSEWHERE = {
    "kgat_spmm_workspace_bytes": [("test_sum_entry_refusals", "kgat_spmm_umule_sum_f32"),
                                  ("test_fused_entry_refusals", "kgat_spmm_bi_fused_f32"),
                                  ("test_copy_entry_refusals", "kgat_copy_reduce_f32")],
    "kgat_spmm_max_workspace_bytes": [("test_max_entry_refusals", "kgat_spmm_umule_max_f32")],
}


def size_functions():
    return sorted(n for n in declarations() if n.endswith("_workspace_bytes"))


def test_every_size_function_has_a_case():
    """Closed table: a new kgat_*_workspace_bytes declaration needs a row in CASES; every entry with a `void* workspace`
    has a Case of its own or is called one byte short, with KGAT_E_WORKSPACE expected, by the test named above."""
    import inspect
    import test_spmm_plan_host as there
    for name in size_functions():
        assert (name in CASES) != (name in COVERED_ELSEWHERE), "%s: no case (or two)" % name
    assert set(CASES) | set(COVERED_ELSEWHERE) == set(size_functions())
    held = {c.entry for cases in CASES.values() for c in cases}
    for name, tests in COVERED_ELSEWHERE.items():
        for test, entry in tests:
            src = inspect.getsource(getattr(there, test))
            short = re.findall(r"_refused\(name, [^\n]*WORKSPACE,\s*\"[a-z_0-9]+: workspace too small \((\d+) < (\d+)\)\"", src)
            assert 'name = "%s"' % entry in src, (test, entry)
            assert any(int(a) + 1 == int(b) for a, b in short), "%s calls %s one byte short nowhere" % (test, entry)
            held.add(entry)
    for name, (_, params) in declarations().items():
        if ("void *", "workspace") in params:
            assert name in held, "%s takes a workspace and no case calls it one byte short" % name


ALL = [(fn, c) for fn in sorted(CASES) for c in CASES[fn]]


@pytest.mark.parametrize("fn, case", ALL, ids=[c.entry for _, c in ALL])
def test_one_byte_short_is_refused_before_device_work(fn, case):
    lib = _lib.load()
    rc, msg, need = case.call(lib, case.sizes, short=1)
    assert need > 0, (fn, need)
    assert rc == case.code, (case.entry, rc, msg)
    assert case.word in msg and "workspace" in msg, (case.entry, msg)


@pytest.mark.parametrize("fn, case", [(f, c) for f, c in ALL if c.early is not None],
                         ids=[c.entry for _, c in ALL if c.early is not None])
def test_exact_size_with_nothing_to_do_returns_ok(fn, case):
    lib = _lib.load()
    sizes = dict(case.sizes)
    sizes.update(case.early)
    rc, msg, _ = case.call(lib, sizes, short=0)
    assert rc == OK, (case.entry, rc, msg)
