"""Global-norm gradient clipping on the GPU (reference kgat.py:32,162): the norm against fp64 under the derived bound
and against the host replay of the kernel's order of additions, the coefficient's bits, the clipped Adam step against
scale-then-step, the in-place clip, reproducibility, and the harness flag end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _grad_clip_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# group 0: every size at which a path changes (one lane, a partial float4, one element short of a chunk, a chunk, one
# over, two chunks and a tail), the shapes of W_R and of a slice of the table, an empty tensor, 17 tensors with a
# gradient (two launches of 16 under one norm) and one without; group 1: two more, under other hyper-parameters.
SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (2 * 4096 + 5,), (41, 64, 64), (1000, 64), (0,), (5000,), (7,), (64,),
          (257,), (1024,), (5001,), (2,), (12289,), (33,), (130,), (4100,)]
OFF_BOTH = 9        # parameter AND gradient are views base[1:]: data pointers 4 bytes past a 16-byte boundary
OFF_GRAD = 14       # only the gradient is such a view
NO_GRAD = 17
GROUP0 = 18         # SHAPES[:18] -> group 0, the rest -> group 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _off16(values, dev):
    """A contiguous device copy of `values` whose data pointer is 4 bytes past a 16-byte boundary."""
    base = torch.empty(values.size + 1, dtype=torch.float32, device=dev)
    view = base[1:].view(values.shape)
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _values(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * scale).astype(np.float32) for s in SHAPES]


def _grads(values, dev):
    return [None if i == NO_GRAD else _off16(v, dev) if i in (OFF_BOTH, OFF_GRAD) else torch.from_numpy(v).to(dev)
            for i, v in enumerate(values)]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _State:
    """Parameters (fixed values), a FusedAdam over two groups, and one earlier plain step in which only every second
    parameter had a gradient - so moments are non-zero and the step counts of the others lag."""

    def __init__(self, dev, zero_grads):
        import dgl_kgat_amd as K
        self.params = []
        for i, v in enumerate(_values(100)):
            p = _off16(v, dev) if i == OFF_BOTH else torch.from_numpy(v).to(dev)
            self.params.append(p.requires_grad_())
        self.opt = K.FusedAdam([{"params": self.params[:GROUP0]}, {"params": self.params[GROUP0:], "lr": 3e-3,
                                                                    "betas": (0.8, 0.99)}], lr=1e-2, zero_grads=zero_grads)
        warm = _grads(_values(101, 0.5), dev)
        for i, p in enumerate(self.params):
            p.grad = warm[i] if i % 2 == 0 else None
        self.opt.step()
        assert int(self.opt.state[self.params[0]]["step"]) == 1 and not self.opt.state[self.params[1]]

    def set_grads(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g

    def tensors(self):
        out = []
        for p in self.params:
            st = self.opt.state[p]
            out += [p] + ([st["exp_avg"], st["exp_avg_sq"]] if st else [])
        return out


# ---------------------------------------------------------------- 1, 2: the norm and the coefficient
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_norm_against_fp64_and_coefficient_bits(dev, scale):
    from dgl_kgat_amd import ops
    values = _values(7, scale)
    grads = [g for g in _grads(values, dev) if g is not None]
    exact = ref.norm64([v for i, v in enumerate(values) if i != NO_GRAD])
    bound = ref.norm_bound(ops.GRAD_NORM_CHAIN)
    for max_norm in (0.37 * exact, 3.0 * exact):
        norm, coef = ops.grad_norm(grads, max_norm)
        assert norm.shape == () and coef.shape == () and norm.is_cuda and coef.is_cuda
        assert norm.dtype == torch.float32 and coef.dtype == torch.float32
        n, c = norm.cpu().numpy(), coef.cpu().numpy()
        err = abs(float(n) - exact) / exact
        print("scale %g: norm %.9g fp64 %.9g rel err %.3e (bound %.3e) coef %.9g" % (scale, n, exact, err, bound, c))
        assert err <= bound, (err, bound)
        want = ref.coef_of(n, max_norm)
        assert c.view(np.int32) == want.view(np.int32), (c, want)
        assert (c < 1) == (max_norm < exact)


def test_norm_has_the_bits_of_the_host_replay(dev):
    """The order of additions is part of the interface: replayed in numpy, it predicts the kernel's bits - with the
    tensors in one call of 19 (two launches) and the unaligned ones loaded 4 bytes at a time."""
    from dgl_kgat_amd import ops
    values = _values(8)
    grads = [g for g in _grads(values, dev) if g is not None]
    norm, coef = ops.grad_norm(grads, 1.0)
    n_ref, c_ref = ref.grad_norm([v for i, v in enumerate(values) if i != NO_GRAD], 1.0)
    assert _bits(norm)[0] == n_ref.view(np.int32) and _bits(coef)[0] == c_ref.view(np.int32)


# ---------------------------------------------------------------- 3: the exact case
def test_exact_case(dev):
    from dgl_kgat_amd import ops
    values = [np.zeros(s, np.float32) for s in SHAPES]
    values[3][:] = 8                      # 4096 x 64
    values[4][:4096] = -4                 # 4096 x 16, the chunk's tail element stays 0
    values[6][:] = 2                      # 41 x 64 x 64 x 4
    values[OFF_GRAD][:] = 3               # 5001 x 9     (unaligned)
    values[OFF_BOTH][:156] = 1            # 156          (unaligned)
    values[OFF_BOTH][156:159] = -5        # 3 x 25   (unaligned)
    total = sum(int((v.astype(np.int64) ** 2).sum()) for i, v in enumerate(values) if i != NO_GRAD)
    rest = 2 ** 20 - total
    assert 0 <= rest <= 4096 * 9
    q, r = divmod(rest, 9)
    values[16][:q] = 3                    # the remainder in 9s, then in 1s
    values[16][q:q + r] = 1
    assert sum(int((v.astype(np.int64) ** 2).sum()) for i, v in enumerate(values) if i != NO_GRAD) == 2 ** 20
    grads = [g for g in _grads(values, dev) if g is not None]
    norm, coef = ops.grad_norm(grads, 512)
    assert _bits(norm)[0] == np.float32(1024.0).view(np.int32)
    assert _bits(coef)[0] == np.float32(0.5).view(np.int32)


def test_zero_gradients_empty_lists_and_nan(dev):
    from dgl_kgat_amd import ops
    zeros = [torch.zeros(s, device=dev) for s in SHAPES[:10]]
    norm, coef = ops.grad_norm(zeros, 1.0)
    assert float(norm) == 0.0 and _bits(coef)[0] == np.float32(1).view(np.int32)
    norm, coef = ops.grad_norm([], 2.0)
    assert float(norm) == 0.0 and float(coef) == 1.0
    norm, coef = ops.grad_norm([torch.zeros(0, device=dev)], 2.0)
    assert float(norm) == 0.0 and float(coef) == 1.0
    # torch's error_if_nonfinite=False: the NaN propagates into norm and coefficient
    bad = torch.ones(5000, device=dev)
    bad[4321] = float("nan")
    norm, coef = ops.grad_norm([torch.ones(3, device=dev), bad], 2.0)
    assert torch.isnan(norm) and torch.isnan(coef)
    bad[4321] = float("inf")
    norm, coef = ops.grad_norm([bad], 2.0)
    assert torch.isinf(norm) and float(coef) == 0.0


# ---------------------------------------------------------------- 4: the clipped step against scale-then-step
@pytest.mark.parametrize("zero_grads", [False, True])
@pytest.mark.parametrize("case", ["clip", "no_clip", "zero"])
def test_clipped_step_same_bits_as_scale_then_step(dev, case, zero_grads):
    from dgl_kgat_amd import ops
    values = [np.zeros_like(v) for v in _values(0)] if case == "zero" else _values(102, 0.02)
    exact = ref.norm64([v for i, v in enumerate(values) if i != NO_GRAD])
    c = {"clip": 0.25 * exact, "no_clip": 1.5 * exact, "zero": 1.0}[case]
    a, b = _State(dev, zero_grads), _State(dev, zero_grads)
    assert all(_same(x, y) for x, y in zip(a.tensors(), b.tensors()))
    a.set_grads(_grads(values, dev))
    b.set_grads(_grads(values, dev))
    before = [None if g is None else g.clone() for g in (p.grad for p in a.params)]
    # b: the kernel's own coefficient, torch's in-place multiply, the plain step
    norm_b, coef = ops.grad_norm([p.grad for p in b.params if p.grad is not None], c)
    if case == "clip":
        assert float(coef) < 1
        for p in b.params:
            if p.grad is not None:
                p.grad.mul_(coef)
    else:   # coef is exactly 1: the plain step with no scaling at all
        assert _bits(coef)[0] == np.float32(1).view(np.int32)
        if case == "zero":
            assert float(norm_b) == 0.0
    b.opt.step()
    a.opt.step(max_grad_norm=c)
    assert _same(a.opt.last_grad_norm, norm_b) and a.opt.last_grad_norm.shape == ()
    ta, tb = a.tensors(), b.tensors()
    assert len(ta) == len(tb) == 3 * (len(SHAPES) - 1) + 1     # every parameter with a gradient now has its state
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert _same(x, y), ("tensor %d of the state differs" % i)
    # lagging step counts: parameters that sat out the first step are at 1, the others at 2
    assert [int(a.opt.state[p]["step"]) for p in a.params[:4]] == [2, 1, 2, 1]
    assert not a.opt.state[a.params[NO_GRAD]]
    if case == "clip":   # and the step did move the parameters differently from an unclipped one
        u = _State(dev, zero_grads)
        u.set_grads(_grads(values, dev))
        u.opt.step()
        assert not _same(u.params[6], a.params[6])
    for p, g0 in zip(a.params, before):
        if g0 is None:
            assert p.grad is None
        elif zero_grads:
            assert not _bits(p.grad).any()
        else:            # read, not rewritten: the one difference from torch's in-place clip
            assert _same(p.grad, g0)


def test_norm_out_view_and_parameters_on_two_devices(dev):
    import dgl_kgat_amd as K
    s = _State(dev, False)
    values = _values(103)
    s.set_grads(_grads(values, dev))
    norms = torch.full((3,), -1.0, device=dev)
    s.opt.step(max_grad_norm=1.0, norm_out=norms[1])
    assert s.opt.last_grad_norm is None
    got = norms.cpu().numpy()
    assert got[0] == -1 and got[2] == -1
    assert got[1].view(np.int32) == ref.grad_norm([v for i, v in enumerate(values) if i != NO_GRAD], 1.0)[0].view(np.int32)
    with pytest.raises(K.KGATLibraryError):
        s.opt.step(max_grad_norm=1.0, norm_out=torch.zeros(2, device=dev))
    with pytest.raises(K.KGATLibraryError):
        s.opt.step(max_grad_norm=1.0, norm_out=torch.zeros(1))
    # one norm cannot span devices (checked on the host, before any launch)
    p0 = torch.ones(4, device=dev).requires_grad_()
    p1 = torch.ones(4).requires_grad_()
    p0.grad, p1.grad = torch.ones(4, device=dev), torch.ones(4)
    with pytest.raises(K.KGATLibraryError):
        K.FusedAdam([p0, p1]).step(max_grad_norm=1.0)


# ---------------------------------------------------------------- 5: the in-place clip
@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_clip_grad_norm_in_place(dev, factor):
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops
    values = _values(104, 3.0)
    exact = ref.norm64([v for i, v in enumerate(values) if i != NO_GRAD])
    params = [torch.zeros(s, device=dev).requires_grad_() for s in SHAPES]
    for p, g in zip(params, _grads(values, dev)):
        p.grad = g
    before = [None if p.grad is None else p.grad.clone() for p in params]
    norm, coef = ops.grad_norm([g for g in before if g is not None], factor * exact)
    ptrs = [None if p.grad is None else p.grad.data_ptr() for p in params]
    total = K.clip_grad_norm_(params, factor * exact, norm_type=2.0)
    assert total.shape == () and total.is_cuda and _same(total, norm)
    assert (float(coef) < 1) == (factor < 1)
    for p, g0, ptr in zip(params, before, ptrs):
        if g0 is None:
            assert p.grad is None
            continue
        assert p.grad.data_ptr() == ptr                      # in place
        assert _same(p.grad, g0 * coef)                      # torch's fp32 product, element by element
    assert K.clip_grad_norm_(params[0], 1e9).shape == ()     # a single tensor, as torch accepts


# ---------------------------------------------------------------- 6: reproducibility
def test_reproducible_bits(dev):
    from dgl_kgat_amd import ops
    values = _values(105)
    grads = [g for g in _grads(values, dev) if g is not None]
    first = [_bits(t)[0] for t in ops.grad_norm(grads, 1.0)]
    for _ in range(3):
        assert [_bits(t)[0] for t in ops.grad_norm(grads, 1.0)] == first
    runs = []
    for _ in range(2):
        s = _State(dev, True)
        s.set_grads(_grads(values, dev))
        s.opt.step(max_grad_norm=1.0)
        runs.append([_bits(t) for t in s.tensors()] + [_bits(s.opt.last_grad_norm)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


# ---------------------------------------------------------------- 7: the harness
@pytest.fixture(scope="module")
def harness_runs(tmp_path_factory):
    """examples/train_kgat.py on its smallest synthetic CKG, one epoch of two iterations per phase, in three fresh child
    processes (started together): no flag, a bar no gradient reaches, a bar every gradient exceeds.  The CF batch is
    1,024 pairs: at the default 10,240 this CKG's few thousand training pairs make ONE iteration, --max_iters 2 would
    not bind, and cf_loss - taken before each step - could not show what the clip did to the step before."""
    tmp = tmp_path_factory.mktemp("grad_clip")
    procs = {}
    for name, extra in (("off", []), ("high", ["--grad_norm", "1e9"]), ("low", ["--grad_norm", "1e-6"])):
        log = tmp / (name + ".json")
        cmd = [sys.executable, os.path.join(ROOT, "examples", "train_kgat.py"), "--synthetic", "0.01", "--epochs", "1",
               "--max_iters", "2", "--batch_size", "1024", "--log_json", str(log)] + extra
        procs[name] = (subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), log)
    out = {}
    try:
        for name, (p, log) in procs.items():
            text, _ = p.communicate(timeout=300)
            assert p.returncode == 0, (name, text[-3000:])
            with open(log) as f:
                out[name] = json.load(f)["epochs"][0]
    finally:
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
    return out


def test_harness_flag(harness_runs):
    off, high, low = harness_runs["off"], harness_runs["high"], harness_runs["low"]
    assert "cf_grad_norm_max" not in off and "cf_clipped_steps" not in off
    assert off["cf_iters"] == high["cf_iters"] == low["cf_iters"] == 2
    metric_keys = [k for k in off if k.startswith(("valid_", "test_"))]
    assert metric_keys
    for k in ["cf_loss", "kg_loss"] + metric_keys:
        assert high[k] == off[k], (k, high[k], off[k])
    assert high["cf_clipped_steps"] == 0 and np.isfinite(high["cf_grad_norm_max"]) and high["cf_grad_norm_max"] > 0
    assert high["cf_grad_norm_mean"] <= high["cf_grad_norm_max"]
    assert low["cf_clipped_steps"] == low["cf_iters"]
    assert np.isfinite(low["cf_grad_norm_max"]) and low["cf_grad_norm_max"] > 1e-6
    assert low["cf_loss"] != off["cf_loss"]
    assert low["kg_loss"] == off["kg_loss"]          # the KG phase is not clipped
