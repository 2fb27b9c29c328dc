"""The fused NFM evaluation sweep without a GPU: the new entries' declarations and types, the envelope, the refusals
(made before any device work: they come back on a machine without a device), NFM's fused= refusals and the harness's
--nfm_eval flag."""
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
from dgl_kgat_amd import _lib, ops  # noqa: E402

from test_workspace_host import BADARG, OK, P, WORKSPACE, declarations  # noqa: E402

UNSUPPORTED = -2
NEW = {"kgat_nfm_eval_supported", "kgat_nfm_eval_scratch_bytes", "kgat_nfm_eval_topk_f32"}
ENTRY = "kgat_nfm_eval_topk_f32"
OPTIONAL = {"user_const", "topk_scores", "train_items"}
_SIZES = dict(n_users=70, n_items=1500, d=64, hidden=64, v_stride=64, K=20)
CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "kgat_stream_t": ctypes.c_void_p}


def _call(sizes=None, pointers=None, short=0):
    lib = _lib.load()
    s = dict(_SIZES, **(sizes or {}))
    args = []
    for ctype, pname in declarations()[ENTRY][1]:
        if pname == "scratch_bytes":
            args.append(lib.kgat_nfm_eval_scratch_bytes(s["n_users"], s["n_items"], s["d"], s["hidden"], s["K"]) - short)
        elif pname == "stream":
            args.append(None)
        elif pointers and pname in pointers:
            args.append(pointers[pname])
        elif "*" in ctype:
            args.append(P)
        else:
            args.append(s[pname])
    rc = getattr(lib, ENTRY)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def test_new_symbols_are_declared_exported_and_bound():
    decl = declarations()
    assert {n for n in decl if n.startswith("kgat_nfm_")} == NEW
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        ret, params = decl[name]
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params), name
        assert res is CTYPES[ret], (name, ret)
        for (ctype, pname), bound in zip(params, argtypes):
            assert bound is (ctypes.c_void_p if "*" in ctype else CTYPES[ctype]), (name, pname, ctype)
        # the closed tables of the workspace and memory-contract tests do not see these names
        assert not name.endswith("_workspace_bytes")
        assert not any(p == "workspace" or (t == "float *" and (p == "tmp" or p.startswith(("partials", "part_")))) for t, p in params)
    assert [p for _, p in decl[ENTRY][1]][-5:] == ["scratch", "scratch_bytes", "topk_items", "topk_scores", "stream"]
    assert "kgat_nfm_eval.hip" in _lib.SOURCES and _lib.ABI_VERSION == 16 and lib.kgat_version() == 16
    text = open(os.path.join(ROOT, "dgl-kgat_amd", "ops.py")).read()
    body = text.split("# ---------------------------------------------------------------- all-pairs NFM evaluation")[1].split("# ------------------")[0]
    assert ".new_" not in body and ENTRY in body and "_workspace(" in body


def test_supported_is_the_envelope():
    lib = _lib.load()
    ok = lambda d, hd, k: bool(lib.kgat_nfm_eval_supported(d, hd, k))   # noqa: E731
    assert all(ok(d, hd, k) for d in (16, 32, 64, 128) for hd in (32, 64) for k in (1, 20, 100, 128))
    assert not any(ok(d, 64, 20) for d in (0, 8, 24, 48, 96, 256, -64))
    assert not any(ok(64, hd, 20) for hd in (0, 8, 16, 48, 96, 128, -32))      # 16: padded by the caller; 128: not offered
    assert not any(ok(64, 64, k) for k in (0, -1, 129, 1000))
    # the op layer pads 16 hidden units to 32
    assert ops.nfm_eval_supported(64, 16, 20) and ops.nfm_eval_supported(16, 32, 128) and ops.nfm_eval_supported(128, 64, 1)
    assert not ops.nfm_eval_supported(64, 128, 20) and not ops.nfm_eval_supported(24, 64, 20) and not ops.nfm_eval_supported(64, 64, 129)
    need = lib.kgat_nfm_eval_scratch_bytes(70, 1500, 64, 64, 20)
    assert need % 256 == 0 and need >= 47 * 64 * 32 * 4 + 2 * 70 * 20 * 4     # C's layout and one list per user
    assert lib.kgat_nfm_eval_scratch_bytes(0, 1500, 64, 64, 20) == 256 == lib.kgat_nfm_eval_scratch_bytes(70, 1500, 24, 64, 20)


def test_refusals_come_before_device_work():
    word = "nfm_eval_topk"
    assert OK == 0
    rc, msg = _call(short=1)                                      # one byte short of the stated size
    assert rc == WORKSPACE and word in msg and "scratch" in msg, (rc, msg)
    for sizes in (dict(K=0), dict(K=129), dict(d=24, v_stride=64), dict(d=0), dict(hidden=128), dict(hidden=16), dict(hidden=48)):
        rc, msg = _call(sizes)
        assert rc == UNSUPPORTED and word in msg, (sizes, rc, msg)
    for sizes in (dict(n_items=0), dict(n_items=-1), dict(n_users=-1), dict(v_stride=63), dict(v_stride=0), dict(n_items=2 ** 31)):
        rc, msg = _call(sizes)
        assert rc == BADARG and word in msg, (sizes, rc, msg)
    for ctype, pname in declarations()[ENTRY][1]:
        if "*" in ctype and pname not in OPTIONAL:
            rc, msg = _call(pointers={pname: None})
            assert rc == BADARG and word in msg and "null" in msg, (pname, rc, msg)
    for pname in ("itemT", "scratch"):
        rc, msg = _call(pointers={pname: P + 4})
        assert rc == BADARG and word in msg, (pname, rc, msg)


def _toy(layers, dim=16):
    z = np.load(os.path.join(ROOT, "tests", "golden", "toy_dataset.npz"))
    n_users, n_items, n = int(z["n_users"]), int(z["n_items"]), int(z["n_KG_entity"])
    fs = K.FeatureSets.from_kg(z["train_KG_triplet"], (n_users, n_users + n_items), n)
    torch.manual_seed(5)
    model = K.NFM(n, fs, dim=dim, layers=layers)
    train = {u: np.array([u % n_items]) for u in range(n_users)}
    test = {u: np.array([(u + 1) % n_items]) for u in range(n_users)}
    plan = K.metrics.EvalPlan(train, test, np.arange(n_users, n_users + n_items), "cpu")
    return model, plan


def test_fused_refuses_with_the_reason():
    """CPU tensors, two hidden layers, an unsupported width and K > 128: KGATLibraryError naming the reason, from
    evaluate, topk and recommend alike; the default route is untouched."""
    model, plan = _toy((64,))
    with pytest.raises(K.KGATLibraryError, match="HIP device"):
        model.evaluate(plan, (2,), fused=True)
    with pytest.raises(K.KGATLibraryError, match="HIP device"):
        model.topk(plan, 2, fused=True)
    with pytest.raises(K.KGATLibraryError, match="HIP device"):
        model.recommend([0, 1], 2)
    deep, plan = _toy((64, 32))
    with pytest.raises(K.KGATLibraryError, match="ONE hidden layer.*2"):
        deep.evaluate(plan, (2,), fused=True)
    none, plan = _toy(())
    with pytest.raises(K.KGATLibraryError, match="ONE hidden layer.*0"):
        none.topk(plan, 2, fused=True)
    # (a CPU model reports the device first; the other reasons are stated on the GPU, tests/test_gpu_nfm_eval.py)
    assert "HIP device" in _toy((128,))[0]._fused_refusal(20)
    assert model.topk(plan, 3).shape == (plan.n_users, 3)       # the torch route, as before


def test_cpu_tensors_are_refused_by_the_raw_wrapper():
    z = torch.zeros
    with pytest.raises(K.KGATLibraryError):
        ops.nfm_eval_topk(z(4, 16), z(2, dtype=torch.int32), z(32, 16), z(5, 16), z(5, 32), z(32), z(5), None,
                          z(3, dtype=torch.int32), z(0, dtype=torch.int32), 2)


def test_cli_nfm_eval_rules():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    assert "nfm_eval" not in vars(train_kgat.parse_args([]))        # a run without the flag keeps its arguments
    assert "nfm_eval" not in vars(train_kgat.parse_args(["--model", "nfm"]))
    assert train_kgat.parse_args(["--model", "nfm", "--nfm_eval", "fused"]).nfm_eval == "fused"
    assert train_kgat.parse_args(["--model", "nfm", "--nfm_eval", "torch", "--nfm_layers", "32"]).nfm_eval == "torch"
    for flags in (["--nfm_eval", "fused"], ["--model", "fm", "--nfm_eval", "fused"], ["--model", "ripplenet", "--nfm_eval", "torch"],
                  ["--model", "nfm", "--nfm_eval", "triton"], ["--model", "nfm", "--nfm_eval"]):
        with pytest.raises(SystemExit) as e:
            train_kgat.parse_args(flags)
        assert e.value.code == 2, flags


def test_header_states_the_arithmetic():
    text = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    block = text.split("all-pairs NFM evaluation")[1].split("int kgat_nfm_eval_supported")[0]
    for phrase in ("fl(W1[j, c] * V[user, c])", "ascending c from C", "fma(h_j, r[j], p)", "key_i    = s_i + item_lin[i]",
                   "user_const[u]", "no float atomic"):
        assert phrase in block, phrase
    assert re.search(r"-1 / -inf", block)
