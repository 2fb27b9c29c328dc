"""The fused RippleNet evaluation sweep without a GPU: the new entries' declarations and types, the envelope, the
refusals (made before any device work: they come back on a machine without a device), RippleNet's fused= refusals, the
untouched default route, the restatements of tests/_ripple_eval_ref.py against the model, and the harness's
--ripple_eval flag."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, metrics, ops  # noqa: E402

import _ripple_eval_ref as R  # noqa: E402
from test_workspace_host import BADARG, OK, P, WORKSPACE, declarations  # noqa: E402

UNSUPPORTED = -2
NEW = {"kgat_eval_ripple_supported", "kgat_eval_ripple_keys_f32", "kgat_eval_ripple_scratch_bytes",
       "kgat_eval_ripple_topk_f32"}
ENTRY, KEYS = "kgat_eval_ripple_topk_f32", "kgat_eval_ripple_keys_f32"
OPTIONAL = {"topk_scores", "train_items", "W"}
_SIZES = dict(n_call=40, n_items=1500, d=64, n_memory=32, n_hop=2, mode=3, all_hops=1, n_nodes=2000, n_users=40, n_rel=5, K=20)
CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "kgat_stream_t": ctypes.c_void_p}


def _call(entry=ENTRY, sizes=None, pointers=None, short=0):
    lib = _lib.load()
    s = dict(_SIZES, **(sizes or {}))
    args = []
    for ctype, pname in declarations()[entry][1]:
        if pname == "scratch_bytes":
            args.append(lib.kgat_eval_ripple_scratch_bytes(s["n_call"], s["n_items"], s["d"], s["n_memory"], s["n_hop"],
                                                           s["K"]) - short)
        elif pname == "stream":
            args.append(None)
        elif pointers and pname in pointers:
            args.append(pointers[pname])
        elif "*" in ctype:
            args.append(P)
        else:
            args.append(s[pname])
    rc = getattr(lib, entry)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def test_new_symbols_are_declared_exported_and_bound():
    decl = declarations()
    assert {n for n in decl if n.startswith("kgat_eval_ripple")} == NEW
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        ret, params = decl[name]
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params), name
        assert res is CTYPES[ret], (name, ret)
        for (ctype, pname), bound in zip(params, argtypes):
            assert bound is (ctypes.c_void_p if "*" in ctype else CTYPES[ctype]), (name, pname, ctype)
        # the closed tables of the ripple, workspace and memory-contract tests do not see these names
        assert not name.startswith("kgat_ripple") and not name.endswith("_workspace_bytes")
        assert not any(p == "workspace" or (t == "float *" and (p == "tmp" or p.startswith(("partials", "part_")))) for t, p in params)
    assert [p for _, p in decl[ENTRY][1]][-5:] == ["scratch", "scratch_bytes", "topk_items", "topk_scores", "stream"]
    assert "kgat_ripple_eval.hip" in _lib.SOURCES and _lib.ABI_VERSION == 16 and lib.kgat_version() == 16
    assert _lib.SOURCES["kgat_ripple_eval.hip"] == ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    text = open(os.path.join(ROOT, "dgl-kgat_amd", "ops.py")).read()
    body = text.split("# ---------------------------------------------------------------- all-pairs RippleNet evaluation")[1].split("# ------------------")[0]
    assert ".new_" not in body and ENTRY in body and KEYS in body and "_workspace(" in body
    # the selection is stated once: both sweeps include it
    for src in ("kgat_nfm_eval.hip", "kgat_ripple_eval.hip"):
        code = open(os.path.join(ROOT, "dgl-kgat_amd", "csrc", src)).read()
        assert '#include "kgat_topk_wave.h"' in code and "void nfm_prune" not in code and "void nfm_eval_merge_kernel" not in code


def test_supported_is_the_envelope():
    lib = _lib.load()
    ok = lambda d, m, h, mode, k: bool(lib.kgat_eval_ripple_supported(d, m, h, mode, k))   # noqa: E731
    assert all(ok(d, m, h, mode, k) for d in (16, 32, 64) for m in (1, 5, 32, 33, 64) for h in (1, 2) for mode in range(4)
               for k in (1, 20, 128))
    assert not any(ok(d, 32, 2, 3, 20) for d in (0, 8, 24, 48, 256, -64))
    assert not any(ok(64, m, 2, 3, 20) for m in (0, 129, -1))
    assert not any(ok(64, 32, h, 3, 20) for h in (0, 5, -1))
    assert not any(ok(64, 32, 2, mode, 20) for mode in (-1, 4))
    assert not any(ok(64, 32, 2, 3, k) for k in (0, 129, -1))
    # what is documented as not offered: d = 128, more than 64 triples per hop, more than two hops
    assert not ok(128, 32, 2, 3, 20) and not ok(64, 65, 2, 3, 20) and not ok(64, 128, 2, 3, 20)
    assert not ok(64, 32, 3, 3, 20) and not ok(64, 32, 4, 3, 20)
    assert ops.ripple_eval_supported(16, 32, 2, 3, 100) and not ops.ripple_eval_supported(64, 32, 2, 3, 129)
    need = lib.kgat_eval_ripple_scratch_bytes(40, 1500, 64, 32, 2, 20)
    assert need % 256 == 0 and need >= 2 * 40 * 4 * 20 * 4                  # a list per wavefront of a user's workgroup
    assert lib.kgat_eval_ripple_scratch_bytes(0, 1500, 64, 32, 2, 20) == 256 == lib.kgat_eval_ripple_scratch_bytes(40, 1500, 24, 32, 2, 20)


def test_refusals_come_before_device_work():
    word = "eval_ripple_topk"
    assert OK == 0
    rc, msg = _call(short=1)                                      # one byte short of the stated size
    assert rc == WORKSPACE and word in msg and "scratch" in msg, (rc, msg)
    for sizes in (dict(K=0), dict(K=129), dict(d=24), dict(d=0), dict(d=128), dict(n_memory=0), dict(n_memory=129),
                  dict(n_hop=0), dict(n_hop=5), dict(mode=-1), dict(mode=4)):
        rc, msg = _call(sizes=sizes)
        assert rc == UNSUPPORTED and word in msg, (sizes, rc, msg)
    for sizes in (dict(n_items=0), dict(n_items=-1), dict(n_call=-1), dict(n_items=2 ** 31), dict(n_nodes=0), dict(n_users=0),
                  dict(n_users=-3), dict(n_nodes=2 ** 31)):
        rc, msg = _call(sizes=sizes)
        assert rc == BADARG and word in msg, (sizes, rc, msg)
    for ctype, pname in declarations()[ENTRY][1]:
        if "*" in ctype and pname not in OPTIONAL:
            rc, msg = _call(pointers={pname: None})
            assert rc == BADARG and word in msg and "null" in msg, (pname, rc, msg)
    rc, msg = _call(pointers={"W": None})                         # the transform modes need W
    assert rc == BADARG and "null" in msg
    for pname in ("itemT", "keys", "ent", "scratch"):
        rc, msg = _call(pointers={pname: P + 4})
        assert rc == BADARG and word in msg and "aligned" in msg, (pname, rc, msg)
    # the keys pass
    word = "eval_ripple_keys"
    for sizes in (dict(d=24), dict(d=128), dict(n_memory=0), dict(n_memory=129), dict(n_hop=0), dict(n_hop=5)):
        rc, msg = _call(KEYS, sizes=sizes)
        assert rc == UNSUPPORTED and word in msg, (sizes, rc, msg)
    for sizes in (dict(n_call=-1), dict(n_rel=0), dict(n_nodes=0), dict(n_users=0)):
        rc, msg = _call(KEYS, sizes=sizes)
        assert rc == BADARG and word in msg, (sizes, rc, msg)
    for ctype, pname in declarations()[KEYS][1]:
        if "*" in ctype:
            rc, msg = _call(KEYS, pointers={pname: None})
            assert rc == BADARG and word in msg and "null" in msg, (pname, rc, msg)
    for pname in ("ent", "relation_emb", "keys"):
        rc, msg = _call(KEYS, pointers={pname: P + 4})
        assert rc == BADARG and word in msg and "aligned" in msg, (pname, rc, msg)


def _toy(d=16, M=5, mode="plus_transform", n_items=30, seed=3):
    rng = np.random.default_rng(seed)
    n_users, n_hop, n_rel = 6, 2, 3
    n_nodes = n_users + n_items + 10
    h, t = (rng.integers(0, n_nodes, (n_users, n_hop, M)) for _ in range(2))
    r = np.sort(rng.integers(0, n_rel, (n_users, n_hop, M)), axis=2)
    sets = K.RippleSets(h, r, t, n_nodes, n_rel)
    torch.manual_seed(seed)
    model = K.RippleNet(n_nodes, sets, dim=d, item_update_mode=mode, item_range=(n_users, n_users + n_items))
    train = {u: np.array([u % n_items, (3 * u + 1) % n_items]) for u in range(n_users)}
    test = {u: np.array([(u + 5) % n_items]) for u in range(n_users)}
    plan = metrics.EvalPlan(train, test, np.arange(n_users, n_users + n_items), "cpu")
    return model, plan


def test_fused_refuses_with_the_reason():
    model, plan = _toy()
    with pytest.raises(K.KGATLibraryError, match=r"evaluate\(fused=True\).*HIP device"):
        model.evaluate(plan, (2,), fused=True)
    with pytest.raises(K.KGATLibraryError, match="HIP device"):
        model.topk(plan, 2, fused=True)
    with pytest.raises(K.KGATLibraryError, match="HIP device"):
        model.recommend([0, 1], 2)
    assert "float32" in _toy()[0].double()._fused_refusal(2) or "HIP device" in _toy()[0].double()._fused_refusal(2)
    z = torch.zeros
    with pytest.raises(K.KGATLibraryError):
        ops.ripple_eval_keys(z(46, 16), z(3, 256), model.sets, z(2, dtype=torch.int32))
    with pytest.raises(K.KGATLibraryError):
        ops.ripple_eval_topk(z(46, 16), model.sets, z(2, dtype=torch.int32), z(2, 2, 5, 16), z(512), 30, None, 1, True,
                             z(3, dtype=torch.int32), z(0, dtype=torch.int32), 2)


def test_default_route_is_the_torch_route(monkeypatch):
    """fused=False: topk is metrics.topk_unseen over scores, evaluate hands its arguments to metrics.calc_metrics_unseen
    unchanged (that function's metric kernel needs a device; what it is given is checked here)."""
    model, plan = _toy()
    want = metrics.topk_unseen(model.scores, model.n_items, plan, 7, 1 << 28)
    assert torch.equal(model.topk(plan, 7), want) and torch.equal(model.topk(plan, 7, fused=False), want)
    seen = []
    monkeypatch.setattr(metrics, "calc_metrics_unseen", lambda *a: seen.append(a) or "dict")
    assert model.evaluate(plan, (2, 5), 1 << 20) == "dict" and model.evaluate(plan, (2, 5), 1 << 20, fused=False) == "dict"
    assert len(seen) == 2
    for a in seen:
        assert a[0] == model.scores and a[1:] == (model.n_items, plan, (2, 5), 1 << 20)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("all_hops", [True, False])
def test_the_restatement_is_the_models_scores(mode, all_hops):
    """tests/_ripple_eval_ref.scores64 against RippleNet.scores in float64 on the model's own parameters."""
    model, plan = _toy(mode=mode)
    model.using_all_hops = all_hops
    model = model.double()
    users = np.array([4, 0, 0, 5])
    lo, hi = model.item_range
    s = model.sets
    inp = dict(ent=model.entity_emb.weight.detach().numpy(), rel=model.relation_emb.weight.detach().numpy(),
               W=model.transform_matrix.weight.detach().numpy(), mem_h=s.mem_h.numpy(), mem_r=s.mem_r.numpy(),
               mem_t=s.mem_t.numpy(), item_lo=lo, n_items=hi - lo, mode=R.MODES.index(mode), all_hops=all_hops)
    got = R.scores64(inp, users)
    want = model.scores(torch.as_tensor(users)).numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_fma32_rounds_once():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(200000).astype(np.float32) for _ in range(3))
    c *= np.float32(2.0) ** rng.integers(-30, 30, c.shape).astype(np.float32)
    got = R.fma32(a, b, c)
    # against exact rational arithmetic on a sample, and against the double-rounded form everywhere it cannot differ
    from fractions import Fraction
    for i in range(0, 200000, 997):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo_, hi_ = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo_)) - exact), abs(Fraction(float(hi_)) - exact))
    # a case where rounding the float64 sum first goes wrong: a b = 1 - 2^-46, c = 2^24 + 2: the sum lies just below the
    # tie 2^24 + 3, float64 rounds it onto the tie, and the tie then goes up to even
    a1, b1, c1 = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 - 2.0 ** -23), np.float32(2.0 ** 24 + 2)
    assert np.float32(np.float64(a1) * np.float64(b1) + np.float64(c1)) == np.float32(2.0 ** 24 + 4)
    assert R.fma32(np.array([a1]), np.array([b1]), np.array([c1]))[0] == c1


def test_exact_families_are_exact():
    """Both families are representable in fp32 at every step's end: the float64 scores are fp32 numbers (the saturated
    family up to the float64 softmax's 1e-100 residues) and the saturated hop picks different slots for different items."""
    for M in (1, 2, 32, 64):
        inp = R.uniform_inputs(M, 95, 64, M, 2, 3, True)
        y = R.scores64(inp, np.arange(5))
        assert np.array_equal(y, y.astype(np.float32).astype(np.float64)) and len(np.unique(y)) > 20
    for order in ("ascending", "descending", "equal"):
        y = R.scores64(R.uniform_inputs(1, 200, 16, 32, 1, 1, True, order), np.arange(3))
        pos = np.arange(200.0)
        assert np.array_equal(y, np.broadcast_to({"ascending": pos, "descending": -pos, "equal": 0 * pos}[order] + 1, y.shape))
    for d, M in ((16, 5), (64, 33), (32, 64), (64, 1)):
        for mode in range(4):
            inp = R.saturated_inputs(d + M, 95, d, M, 2, mode, True)
            y = R.scores64(inp, np.arange(6))
            assert np.abs(y - np.round(y)).max() < 1e-90 and np.abs(y).max() < 2 ** 23
            if M > 1 and mode > 0:
                assert len(np.unique(np.round(y))) > 5


def test_cli_ripple_eval_rules():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    assert "ripple_eval" not in vars(train_kgat.parse_args([]))     # a run without the flag keeps its arguments
    assert "ripple_eval" not in vars(train_kgat.parse_args(["--model", "ripplenet"]))
    assert train_kgat.parse_args(["--model", "ripplenet", "--ripple_eval", "fused"]).ripple_eval == "fused"
    assert train_kgat.parse_args(["--model", "ripplenet", "--ripple_eval", "torch", "--n_memory", "16"]).ripple_eval == "torch"
    for flags in (["--ripple_eval", "fused"], ["--model", "nfm", "--ripple_eval", "fused"],
                  ["--model", "ripplenet", "--ripple_eval", "triton"], ["--model", "ripplenet", "--ripple_eval"]):
        with pytest.raises(SystemExit) as e:
            train_kgat.parse_args(flags)
        assert e.value.code == 2, flags


def test_header_states_the_arithmetic():
    text = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    block = text.split("all-pairs RippleNet evaluation")[1].split("int kgat_eval_ripple_supported")[0]
    for phrase in ("ascending c from 0", "e_i * fl(1 / sum)", "a padded slot is masked by its index", "fma(v_H[c], z[c], p)",
                   "no float atomic", "-1 / -inf", "gets an empty list"):
        assert phrase in block, phrase
