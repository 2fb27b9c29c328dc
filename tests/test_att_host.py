"""The attention logits' forward entries without a GPU: every refusal below returns before the first HIP call, so the
return code and the text of kgat_last_error() are checked on the host; the four forward `_supported` predicates and the
backward's are tabulated against their rules restated here; the three Python wrappers refuse a wrong shape alike."""
import ctypes as C
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dgl_kgat_amd import _lib, ops  # noqa: E402

OK, BADARG, UNSUPPORTED = 0, -1, -2
_BUF = C.create_string_buffer(4096)   # a non-null address; no case below gets as far as reading it
P = C.addressof(_BUF)
N, E, R = 100, 10, 2


def _call(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def _refused(name, args, rc, fragment):
    got, msg = _call(name, *args)
    assert got == rc, (name, got, msg)
    assert fragment in msg, (name, msg)


def _one(n_nodes=N, n_edges=E, d=64, k=64, n_rel=R, ptrs=P, logits=P, logits_csr=None, pos_g=None, algo=0):
    return (n_nodes, n_edges, d, k, n_rel, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, logits, logits_csr, pos_g, algo,
            None)


def test_one_kernel_entry_refusals():
    _refused("kgat_att_score_f32", _one(n_nodes=-1), BADARG, "att_score: bad size")
    _refused("kgat_att_score_f32", _one(logits=None), BADARG, "att_score: logits is null")
    _refused("kgat_att_score_f32", _one(logits_csr=P), BADARG, "att_score: logits_csr needs pos_g")
    _refused("kgat_att_score_f32", _one(algo=9), BADARG, "att_score: bad algo")
    # the order of the checks: a null output is reported before a bad algo, a bad size before either
    _refused("kgat_att_score_f32", _one(logits=None, algo=9), BADARG, "logits is null")
    _refused("kgat_att_score_f32", _one(n_nodes=-1, logits=None, algo=9), BADARG, "bad size")
    assert _call("kgat_att_score_f32", *_one(n_edges=0, logits=None, algo=9))[0] == OK


def _grouped(n_nodes=N, n_edges=E, d=64, k=64, n_rel=R, ptrs=P, n_groups=4, tab=P, logits=None, logits_csr=P, pos_g=P,
             flags=None):
    tail = (None,) if flags is None else (flags, None)
    return (n_nodes, n_edges, d, k, n_rel, ptrs, ptrs, ptrs, pos_g, ptrs, ptrs, ptrs, n_groups, ptrs, ptrs, ptrs, tab,
            logits, logits_csr) + tail


def test_split_entry_refusals():
    name = "kgat_att_score_split_f32"
    _refused(name, _grouped(d=8, k=8), UNSUPPORTED,
             "att_score_split: needs d == k in {16,32,64}, 0 < R <= 4096, N*d*4 < 4 GiB (d=8 k=8 R=2)")
    _refused(name, _grouped(ptrs=None), BADARG, "att_score_split: null pointer")
    _refused(name, _grouped(n_groups=-1), BADARG, "att_score_split: bad size")
    _refused(name, _grouped(logits_csr=None), BADARG, "att_score_split: no output requested")
    _refused(name, _grouped(tab=None), BADARG, "att_score_split: null group table")
    _refused(name, _grouped(pos_g=None), BADARG, "att_score_split: logits_csr needs pos_g")
    # unsupported is reported before a null pointer; no edges is fine before either
    _refused(name, _grouped(d=8, k=8, ptrs=None), UNSUPPORTED, "att_score_split: needs")
    assert _call(name, *_grouped(n_edges=0, d=8, k=8, ptrs=None))[0] == OK


def test_folded_entry_refusals():
    name = "kgat_att_score_folded_f32"
    _refused(name, _grouped(flags=2), BADARG, "att_score_folded: unknown flag")
    _refused(name, _grouped(d=64, k=48, flags=0), UNSUPPORTED,
             "att_score_folded: needs d == k in {16,32,64,128} or d in {8,16,32} with k <= 32, 0 < R <= 4096, "
             "N*d*4 < 4 GiB (d=64 k=48 R=2)")
    _refused(name, _grouped(ptrs=None, flags=0), BADARG, "att_score_folded: null pointer")
    _refused(name, _grouped(n_edges=-1, flags=0), BADARG, "att_score_folded: bad size")
    _refused(name, _grouped(logits_csr=None, flags=0), BADARG, "att_score_folded: no output requested")
    _refused(name, _grouped(tab=None, flags=0), BADARG, "att_score_folded: null group table")
    _refused(name, _grouped(pos_g=None, flags=0), BADARG, "att_score_folded: logits_csr needs pos_g")
    _refused(name, _grouped(n_groups=1 << 32, flags=0), BADARG, "att_score_folded: group table too large")
    # an unknown flag is reported even without edges; unsupported before a null pointer
    _refused(name, _grouped(n_edges=0, flags=2), BADARG, "unknown flag")
    _refused(name, _grouped(d=64, k=48, ptrs=None, flags=0), UNSUPPORTED, "att_score_folded: needs")
    assert _call(name, *_grouped(n_edges=0, d=64, k=48, ptrs=None, flags=0))[0] == OK


def _fused(n_nodes=N, n_edges=E, d=64, k=64, n_rel=R, ptrs=P, perm=None, pos_g=None, part_tptr=None, n_parts=0,
           logits=None, logits_csr=None, logits_g=P, flags=0, clocks=False):
    tail = (None,) if clocks is False else (clocks, None)
    return (n_nodes, n_edges, d, k, n_rel, ptrs, perm, ptrs, pos_g, ptrs, ptrs, ptrs, ptrs, part_tptr, n_parts, ptrs,
            ptrs, ptrs, logits, logits_csr, logits_g, flags) + tail


def test_fused_entry_refusals():
    name = "kgat_att_score_fused_f32"
    _refused(name, _fused(d=128, k=128, flags=1), UNSUPPORTED,
             "att_score_fused: d = 128 runs the bf16-piece products only")
    _refused(name, _fused(ptrs=None), BADARG, "att_score_fused: null pointer")
    got, msg = _call(name, *_fused(n_rel=0))
    assert got == UNSUPPORTED and "att_score_fused: needs d == k in {16,32,64,128}, 0 < R <= 4096" in msg
    assert _call(name, *_fused(n_edges=0))[0] == OK
    assert _call(name, *_fused(n_edges=0, n_rel=0, ptrs=None))[0] == OK   # (before the support check)
    _refused(name, _fused(n_parts=3), BADARG, "att_score_fused: part_tptr and n_parts go together")
    _refused(name, _fused(part_tptr=P), BADARG, "go together")
    _refused(name, _fused(flags=2), BADARG, "att_score_fused: unknown flag")
    _refused(name, _fused(n_nodes=-1), BADARG, "att_score_fused: bad size")
    _refused(name, _fused(logits_g=None), BADARG, "att_score_fused: no output requested")
    _refused(name, _fused(logits=P), BADARG, "att_score_fused: edge-id ordered logits need perm")
    _refused(name, _fused(logits_csr=P), BADARG, "att_score_fused: logits_csr needs pos_g")
    _refused(name, _fused(n_nodes=(1 << 28) + 1, d=16, k=16), UNSUPPORTED, "att_score_fused: needs")
    # the order: unsupported width before the d = 128 product refusal before a null pointer
    _refused(name, _fused(d=128, k=64, flags=1, ptrs=None), UNSUPPORTED, "att_score_fused: needs")
    _refused(name, _fused(d=128, k=128, flags=1, ptrs=None), UNSUPPORTED, "bf16-piece products only")


def test_fused_timed_entry_refusals():
    name = "kgat_att_score_fused_timed_f32"
    _refused(name, _fused(part_tptr=P, n_parts=3, clocks=None), BADARG,
             "att_score_fused_timed: needs part_tptr and 2 * n_parts clock slots")
    _refused(name, _fused(clocks=P), BADARG, "att_score_fused_timed")
    # with its own arguments in place it refuses like the plain entry, under the plain entry's name
    _refused(name, _fused(part_tptr=P, n_parts=3, clocks=P, ptrs=None), BADARG, "att_score_fused: null pointer")
    _refused(name, _fused(part_tptr=P, n_parts=3, clocks=P, d=128, k=128, flags=1), UNSUPPORTED,
             "bf16-piece products only")


# ---- the support predicates, against their rules written out here (not read from the library)
WIDTHS = (4, 8, 16, 17, 32, 64, 128)
RELS = (0, 1, 4096, 4097)


def _fits(n_nodes, d):   # N * d * 4 < 4 GiB, in the library's unsigned 64-bit arithmetic
    return (n_nodes * d * 4) % (1 << 64) < (1 << 32)


def _rels_ok(n_rel):
    return 0 < n_rel <= 4096


def _rule_split(n, d, k, r):
    return d == k and d in (16, 32, 64) and _rels_ok(r) and _fits(n, d)


def _rule_folded(n, d, k, r):
    small = d in (8, 16, 32) and 1 <= k <= 32 and not (d == k and d >= 16)
    return ((d == k and d in (16, 32, 64, 128)) or small) and _rels_ok(r) and _fits(n, d)


def _rule_fused(n, d, k, r):
    return d == k and d in (16, 32, 64, 128) and _rels_ok(r) and n <= (1 << 28) and _fits(n, d)


def _rule_bwd(n, d, k, r):
    return d == k and d in (16, 32, 64, 128) and n >= 0 and _rels_ok(r) and _fits(n, d)


def _shapes():
    for d, k, r in itertools.product(WIDTHS, WIDTHS, RELS):
        yield 1000, d, k, r
    for n in ((1 << 24) - 1, 1 << 24):
        yield n, 64, 64, 41
    for n in (1 << 28, (1 << 28) + 1):
        yield n, 16, 16, 41
    for n in (-1, 0):
        yield n, 64, 64, 41
        yield n, 16, 16, 41
    for k in (1, 5, 31, 33):   # the folded form's small widths, d and k independent
        for d in (8, 16, 32, 64):
            yield 1000, d, k, 41


@pytest.mark.parametrize("entry,rule", [("kgat_att_score_split_supported", _rule_split),
                                        ("kgat_att_score_folded_supported", _rule_folded),
                                        ("kgat_att_score_fused_supported", _rule_fused),
                                        ("kgat_att_score_bwd_supported", _rule_bwd)])
def test_supported_tables(entry, rule):
    fn = getattr(_lib.load(), entry)
    shapes = list(_shapes())
    assert len(shapes) >= len(WIDTHS) ** 2 * len(RELS) + 8
    for n, d, k, r in shapes:
        assert fn(n, d, k, r) in (0, 1)
        assert bool(fn(n, d, k, r)) == rule(n, d, k, r), (entry, n, d, k, r)
    assert any(rule(*s) for s in shapes) and not all(rule(*s) for s in shapes)


def test_one_kernel_entry_has_no_width_refusal_before_its_outputs():
    # the one-kernel entry takes any (d, k): what it refuses on the host comes before the first launch
    _refused("kgat_att_score_f32", _one(d=12, k=20, logits=None), BADARG, "logits is null")


# ---- the Python wrappers
class _OnDevice(torch.Tensor):
    """A host tensor that says it is on the device: gets the wrappers' checks past the device test, so that the shape
    checks behind it run here.  Its address is a host address, so every case that uses it must be refused before the
    library is called; `no_library` turns a case that is not into a failure instead of a call."""
    is_cuda = property(lambda self: True)


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("a wrapper went on to the library with host tensors")
    monkeypatch.setattr(_lib, "load", load)


def _wrapper_calls(ent, W_R, rel, fake):
    wrap = (lambda t: t.as_subclass(_OnDevice)) if fake else (lambda t: t)
    n_rel = W_R.shape[0]
    i32 = lambda *shape: wrap(torch.zeros(shape, dtype=torch.int32))   # noqa: E731
    ent, W_R, rel = wrap(ent), wrap(W_R), wrap(rel)
    rp = i32(n_rel + 1)
    return {
        "att_score": lambda: ops.att_score(N, rp, i32(E), i32(E), i32(E), ent, W_R, rel),
        "att_score_split": lambda: ops.att_score_split(N, rp, i32(E), i32(E), i32(E), i32(E), rp, i32(4), 4, ent, W_R,
                                                       rel),
        "att_score_fused": lambda: ops.att_score_fused(N, rp, i32(E), i32(E), i32(E), i32(E), rp, i32(4), i32(3, 4), rp,
                                                       ent, W_R, rel, rec_g=i32(E)),
    }


def _raised(fn):
    with pytest.raises(Exception) as info:
        fn()
    return type(info.value), str(info.value)


def test_wrappers_refuse_host_tensors_alike():
    W_R = torch.zeros(R, 16, 16)
    for ent, rel in ((torch.zeros(N + 1, 16), torch.zeros(R, 16)), (torch.zeros(N, 16), torch.zeros(R + 1, 16))):
        got = {name: _raised(fn) for name, fn in _wrapper_calls(ent, W_R, rel, fake=False).items()}
        assert got["att_score"][0] is ops.KGATLibraryError and "ent is on cpu" in got["att_score"][1]
        assert got["att_score_split"] == got["att_score"] and got["att_score_fused"] == got["att_score"]


def test_wrappers_refuse_a_wrong_rel_shape_alike(no_library):
    got = {name: _raised(fn) for name, fn in
           _wrapper_calls(torch.zeros(N, 16), torch.zeros(R, 16, 16), torch.zeros(R + 1, 16), fake=True).items()}
    assert got["att_score"][0] is ValueError and "rel has shape (3, 16), expected (2, 16)" in got["att_score"][1]
    assert got["att_score_split"] == got["att_score"] and got["att_score_fused"] == got["att_score"]


def test_att_score_refuses_a_wrong_ent_shape(no_library):
    # (that the other two wrappers refuse it alike is new with the shared helper: tests/test_gpu_parity.py)
    kind, msg = _raised(_wrapper_calls(torch.zeros(N + 1, 16), torch.zeros(R, 16, 16), torch.zeros(R, 16),
                                       fake=True)["att_score"])
    assert kind is ValueError and "ent has shape (101, 16), expected (100, 16)" in msg
