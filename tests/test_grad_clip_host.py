"""Host-side checks of global-norm gradient clipping (no GPU): the ABI entries and their argument validation, the
refusals of the Python surface, the harness flag, and a self-check of the numpy restatement the GPU tests compare
against (tests/_grad_clip_ref.py): its replay of the kernel's order of additions stays inside the derived bound."""
import ctypes as C
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

import _grad_clip_ref as ref  # noqa: E402

NAMES = ("kgat_grad_norm_chain", "kgat_grad_sumsq_partials", "kgat_grad_sumsq_f32", "kgat_grad_norm_finish_f32",
         "kgat_adam_step_clipped_f32", "kgat_scale_grads_f32")
BADARG = -1


def test_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "kgat_hip.h")).read()
    declared = set(re.findall(r"\b(kgat_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        # every new entry's header comment cites the reference's flag and call
        assert re.search(r"\* %s \(kgat\.py:32,162\)" % name, header), name
    assert lib.kgat_version() == 16 and _lib.ABI_VERSION == 16


def test_chain_constant():
    assert isinstance(ops.GRAD_NORM_CHAIN, int) and 1 <= ops.GRAD_NORM_CHAIN <= 64
    assert ops.GRAD_NORM_CHAIN == _lib.load().kgat_grad_norm_chain()
    with pytest.raises(AttributeError):
        ops.NO_SUCH_CONSTANT


def test_bad_arguments_return_badarg():
    lib = _lib.load()
    cap = lib.kgat_adam_max_tensors()
    one = (C.c_int64 * 1)(8)
    neg = (C.c_int64 * 1)(-1)
    many = (C.c_int64 * (cap + 1))(*([8] * (cap + 1)))
    nullp = (C.c_void_p * 1)(None)
    somep = (C.c_void_p * 1)(256)     # never dereferenced: every call below is refused before any device work
    manyp = (C.c_void_p * (cap + 1))(*([256] * (cap + 1)))
    # the partial count
    assert lib.kgat_grad_sumsq_partials(1, None) == -1 and b"grad_sumsq_partials" in lib.kgat_last_error()
    assert lib.kgat_grad_sumsq_partials(1, neg) == -1
    assert lib.kgat_grad_sumsq_partials(cap + 1, many) == -1
    assert lib.kgat_grad_sumsq_partials(0, None) == 0
    sizes = (C.c_int64 * 6)(0, 1, 4095, 4096, 4097, 159251 * 64)
    assert lib.kgat_grad_sumsq_partials(6, sizes) == 0 + 1 + 1 + 1 + 2 + 2489
    # the sum of squares
    assert lib.kgat_grad_sumsq_f32(1, None, somep, 256, 1, None) == BADARG and b"grad_sumsq" in lib.kgat_last_error()
    assert lib.kgat_grad_sumsq_f32(1, one, None, 256, 1, None) == BADARG
    assert lib.kgat_grad_sumsq_f32(1, one, nullp, 256, 1, None) == BADARG
    assert lib.kgat_grad_sumsq_f32(1, one, somep, None, 1, None) == BADARG
    assert lib.kgat_grad_sumsq_f32(1, neg, somep, 256, 1, None) == BADARG
    assert lib.kgat_grad_sumsq_f32(cap + 1, many, manyp, 256, cap + 1, None) == BADARG
    assert lib.kgat_grad_sumsq_f32(-1, one, somep, 256, 1, None) == BADARG
    assert lib.kgat_grad_sumsq_f32(1, one, somep, 256, 0, None) == BADARG      # the partial does not fit the buffer
    # the finish
    assert lib.kgat_grad_norm_finish_f32(1, None, 1.0, 256, 256, None) == BADARG
    assert lib.kgat_grad_norm_finish_f32(-1, 256, 1.0, 256, 256, None) == BADARG
    assert lib.kgat_grad_norm_finish_f32(1, 256, 1.0, None, 256, None) == BADARG
    assert lib.kgat_grad_norm_finish_f32(1, 256, 1.0, 256, None, None) == BADARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.kgat_grad_norm_finish_f32(1, 256, bad, 256, 256, None) == BADARG, bad
        assert b"max_norm" in lib.kgat_last_error()
    # the clipped step: kgat_adam_step_f32's checks, and the coefficient's pointer
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0)
    assert lib.kgat_adam_step_clipped_f32(1, one, somep, somep, somep, somep, one, *hyper, None, None) == BADARG
    assert b"grad_coef" in lib.kgat_last_error()
    assert lib.kgat_adam_step_clipped_f32(0, None, None, None, None, None, None, *hyper, None, None) == BADARG
    assert lib.kgat_adam_step_clipped_f32(1, None, somep, somep, somep, somep, one, *hyper, 256, None) == BADARG
    assert lib.kgat_adam_step_clipped_f32(1, one, somep, nullp, somep, somep, one, *hyper, 256, None) == BADARG
    assert lib.kgat_adam_step_clipped_f32(1, neg, somep, somep, somep, somep, one, *hyper, 256, None) == BADARG
    assert lib.kgat_adam_step_clipped_f32(cap + 1, many, manyp, manyp, manyp, manyp, many, *hyper, 256, None) == BADARG
    assert lib.kgat_adam_step_clipped_f32(0, None, None, None, None, None, None, *hyper, 256, None) == 0   # nothing to do
    # the in-place scale
    assert lib.kgat_scale_grads_f32(1, one, somep, None, None) == BADARG and b"scale_grads" in lib.kgat_last_error()
    assert lib.kgat_scale_grads_f32(1, None, somep, 256, None) == BADARG
    assert lib.kgat_scale_grads_f32(1, one, nullp, 256, None) == BADARG
    assert lib.kgat_scale_grads_f32(1, neg, somep, 256, None) == BADARG
    assert lib.kgat_scale_grads_f32(cap + 1, many, manyp, 256, None) == BADARG
    assert lib.kgat_scale_grads_f32(0, None, None, 256, None) == 0


@pytest.mark.parametrize("bad", [0, -1, float("nan"), float("inf")])
def test_step_refuses_bad_max_grad_norm(bad):
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    opt = K.FusedAdam([p], lr=0.1)
    with pytest.raises(ValueError):
        opt.step(max_grad_norm=bad)
    assert not opt.state[p] and opt.last_grad_norm is None          # refused before anything moved
    with pytest.raises(ValueError):
        K.clip_grad_norm_([p], bad)
    with pytest.raises(ValueError):
        ops.grad_norm([p.grad], bad)


def test_python_surface():
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    for nt in (1, 1.0, float("inf"), 0):
        with pytest.raises(NotImplementedError):
            K.clip_grad_norm_([p], 1.0, norm_type=nt)
    # no CPU implementation, no fallback to torch's clip
    with pytest.raises(K.KGATLibraryError):
        K.clip_grad_norm_([p], 1.0)
    with pytest.raises(K.KGATLibraryError):
        K.clip_grad_norm_(p, 1.0, norm_type=2)
    with pytest.raises(K.KGATLibraryError):
        K.FusedAdam([p], lr=0.1).step(max_grad_norm=1.0)
    assert torch.equal(p.grad, torch.ones(4)) and torch.equal(p.detach(), torch.ones(4))
    with pytest.raises(ValueError):
        K.FusedAdam([p], lr=0.1).step(norm_out=torch.zeros(1))     # a norm is only taken when clipping
    # torch's return value when nothing has a gradient
    q = torch.nn.Parameter(torch.ones(3))
    assert float(K.clip_grad_norm_([q], 1.0)) == 0.0
    assert "clip_grad_norm_" in K.__all__
    import inspect
    sig = inspect.signature(K.FusedAdam.step)
    assert sig.parameters["max_grad_norm"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["max_grad_norm"].default is None and sig.parameters["norm_out"].default is None
    assert list(inspect.signature(K.clip_grad_norm_).parameters) == ["parameters", "max_norm", "norm_type"]
    assert "not rewritten" in K.FusedAdam.step.__doc__


def test_train_kgat_flag():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_kgat
    finally:
        sys.path.pop(0)
    assert train_kgat.parse_args([]).grad_norm == 0
    assert train_kgat.parse_args(["--grad_norm", "1.5"]).grad_norm == 1.5
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            train_kgat.parse_args(["--grad_norm", bad])


SIZES = [(1,), (3,), (4095,), (4096,), (4097,), (2 * 4096 + 5,), (41, 64, 64), (1000, 64), (0,), (5000,)]


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_restatement_inside_the_bound(scale):
    """The replay of the kernel's additions against fp64, under the bound the GPU test applies to the kernel."""
    rng = np.random.default_rng(11)
    grads = [(rng.standard_normal(s) * scale).astype(np.float32) for s in SIZES]
    norm, coef = ref.grad_norm(grads, 1.0)
    exact = ref.norm64(grads)
    assert norm.dtype == np.float32 and coef.dtype == np.float32
    err = abs(float(norm) - exact) / exact
    assert err <= ref.norm_bound(ops.GRAD_NORM_CHAIN), (err, ref.norm_bound(ops.GRAD_NORM_CHAIN))
    assert len(ref.partials(grads)) == sum(-(-int(np.prod(s)) // 4096) for s in SIZES)
    # adversarial for a serial sum: equal terms, where every addition rounds the same way
    ones = [np.full(159251 * 64, np.float32(0.1))]
    n1, _ = ref.grad_norm(ones, 1.0)
    assert abs(float(n1) - ref.norm64(ones)) / ref.norm64(ones) <= ref.norm_bound(ops.GRAD_NORM_CHAIN)


def test_restatement_exact_cases():
    assert ref.CHAIN == ops.GRAD_NORM_CHAIN       # the replay adds in the order the library declares
    # integers whose squares add up to 2^20: exact in any order
    grads = [np.full(4096, 8.0, np.float32), np.full(4097, 4.0, np.float32), np.full((41, 64, 64), 2.0, np.float32)]
    grads[1][-1] = 0
    grads.append(np.zeros(5000, np.float32))
    rest = 2 ** 20 - sum(int((g.astype(np.int64) ** 2).sum()) for g in grads)
    assert 0 < rest <= 16 * 5000 and rest % 16 == 0
    grads[-1][:rest // 16] = 4
    norm, coef = ref.grad_norm(grads, 512)
    assert norm.view(np.int32) == np.float32(1024).view(np.int32) and coef.view(np.int32) == np.float32(0.5).view(np.int32)
    # nothing to add: norm 0, coefficient 1; a NaN stays a NaN
    norm, coef = ref.grad_norm([np.zeros(7, np.float32)], 1.0)
    assert norm == 0 and coef == 1
    norm, coef = ref.grad_norm([], 1.0)
    assert norm == 0 and coef == 1
    with np.errstate(invalid="ignore"):
        norm, coef = ref.grad_norm([np.array([1.0, np.nan], np.float32)], 1.0)
    assert np.isnan(norm) and np.isnan(coef)
