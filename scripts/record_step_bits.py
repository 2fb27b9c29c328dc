#!/usr/bin/env python3
"""Bit patterns of the three fused train-and-step iterations (kgat_transr_adam_step_f32, kgat_transe_adam_step_f32,
kgat_mf_adam_step_f32): what tests/test_gpu_step_bits.py compares with tests/golden/step_bits.npz.  The test imports
CASES and run_case() from here, so the recorded values and the compared ones come from one piece of code; run as a
program (on the GPU, from a build of the commit whose bits are to be pinned) it writes the fixture:

    python scripts/record_step_bits.py --commit $(git rev-parse HEAD) --out tests/golden/step_bits.npz

Every case takes TWO consecutive steps on one state object (the second meets the first's row tags), batch 2 sharing
about half its entity rows with batch 1.  Recorded per case: both losses, every parameter and both moments after the
second step - full bit patterns for the losses and the relation tables, sha-256 for the rest.  Inputs come from seeds.
Only this package and numpy are needed."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, BETA1, BETA2, EPS, LAMBDA = 0.01, 0.9, 0.999, 1e-8, 0.01
HUB = 42      # KG cases: head of 150 samples and tail of 30 - a run of 180 gradient rows
MF_HUB = 11   # MF cases: the user of half of each batch

# name -> (model, sizes).  KG id pattern: n = 300, R = 5 with relation 3 unused, B = 400, relation 0 on 330 samples (six
# 64-sample chunks: more than one 4-row look of partials).
CASES = {
    "transr.d64k64": ("transr", dict(n=300, R=5, B=400, d=64, k=64)),      # MFMA partials, the LDS copy of W_r
    "transr.d20k12": ("transr", dict(n=300, R=5, B=400, d=20, k=12)),      # non-MFMA partials
    "transr.d128k64": ("transr", dict(n=300, R=5, B=400, d=128, k=64)),    # no LDS copy of W_r
    "transe.d64": ("transe", dict(n=300, R=5, B=400, d=64)),               # 16 lanes per sample
    "transe.d72": ("transe", dict(n=300, R=5, B=400, d=72)),               # 32 lanes per sample, dead lanes
    "transe.d256": ("transe", dict(n=300, R=5, B=400, d=256)),             # 64 lanes per sample
    "mf.small": ("mf", dict(n=300, F=16, B=13)),                           # one-workgroup presort
    "mf.slices": ("mf", dict(n=3000, F=32, B=2731)),                       # slice-sort presort; the hub's run crosses ~43 windows
}


def _t32(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)


def _tf(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _draw(rng, n, size, avoid):
    ids = rng.integers(0, n - 1, size).astype(np.int32)
    return ids + (ids >= avoid)   # [0, n) without `avoid`


def kg_batches(n, R, B, seed=5101):
    """(h, r, pos_t, neg_t), each (2, B) int32.  Batch 2 = batch 1 in another sample order with the entity ids of half
    the samples drawn again; HUB's 180 places stay."""
    rng = np.random.default_rng(seed)
    r = np.concatenate([np.zeros(330, np.int32), rng.choice(np.array([1, 2, 4], np.int32), B - 330)])
    h, pt, nt = (_draw(rng, n, B, HUB) for _ in range(3))
    hub = rng.permutation(B)
    h[hub[:150]] = HUB
    pt[hub[150:180]] = HUB
    mix = rng.permutation(B)
    r, h, pt, nt = r[mix], h[mix], pt[mix], nt[mix]
    again = rng.permutation(B)[:B // 2]
    h2, pt2, nt2 = h.copy(), pt.copy(), nt.copy()
    h2[again] = np.where(h[again] == HUB, HUB, _draw(rng, n, B // 2, HUB))
    pt2[again] = np.where(pt[again] == HUB, HUB, _draw(rng, n, B // 2, HUB))
    nt2[again] = _draw(rng, n, B // 2, HUB)
    order2 = rng.permutation(B)
    assert R == 5 and (r == 0).sum() == 330 and not (r == 3).any()
    for a, b_ in ((h, pt), (h2, pt2)):
        assert (a == HUB).sum() == 150 and (b_ == HUB).sum() == 30
    return tuple(np.stack([a, b_[order2]]) for a, b_ in ((h, h2), (r, r), (pt, pt2), (nt, nt2)))


def mf_batches(n, B, seed=5201):
    """(u, p, n), each (2, B) int32: MF_HUB is the user of half of each batch; batch 2 redraws half of the other ids."""
    rng = np.random.default_rng(seed)
    first = [_draw(rng, n, B, MF_HUB) for _ in range(3)]
    first[0][rng.permutation(B)[:B // 2]] = MF_HUB
    again = rng.permutation(B)[:B // 2]
    out = []
    for a in first:
        b_ = a.copy()
        b_[again] = np.where(a[again] == MF_HUB, MF_HUB, _draw(rng, n, B // 2, MF_HUB))
        out.append(np.stack([a, b_]))
    assert all((u == MF_HUB).sum() == B // 2 for u in out[0])
    return tuple(out)


def _pointers(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def run_case(name, dev):
    """key -> uint32 bit patterns (losses, relation tables) or a sha-256 hex string (everything else)."""
    import torch
    from dgl_kgat_amd import ops
    model, z = CASES[name]
    rng = np.random.default_rng(5300 + sorted(CASES).index(name))
    losses = torch.zeros(2, dtype=torch.float32, device=dev)
    if model == "mf":
        n, F, B = z["n"], z["F"], z["B"]
        ids = [_t32(a, dev) for a in mf_batches(n, B)]
        params = {"emb": _tf(rng.standard_normal((n, F)) * 0.1, dev)}
        st = ops.MFAdamState(n, F, B, dev)
        sorted_all, stride = ops.mf_presort(*ids, n)
    else:
        n, R, B, d = z["n"], z["R"], z["B"], z["d"]
        ids = [_t32(a, dev) for a in kg_batches(n, R, B)]
        params = {"ent": _tf(rng.standard_normal((n, d)), dev)}
        if model == "transr":
            k = z["k"]
            params["W_R"] = _tf((rng.random((R, d, k)) - 0.5) * (2.0 / np.sqrt(d)), dev)
            params["rel"] = _tf(rng.standard_normal((R, k)), dev)
            st = ops.TransRAdamState(n, d, k, R, B, dev)
            sorted_all, stride = ops.transr_presort(*ids, n, R)
        else:
            params["rel"] = _tf(rng.standard_normal((R, d)), dev)
            st = ops.TransEAdamState(n, d, R, B, dev)
            sorted_all, stride = ops.transe_presort(*ids, n, R)
    ps = list(params.values())
    m = [torch.zeros_like(p) for p in ps]
    v = [torch.zeros_like(p) for p in ps]
    arr_m, arr_v = _pointers(m), _pointers(v)
    for i in range(2):
        batch = [a[i] for a in ids]
        block = sorted_all[i * stride:(i + 1) * stride]
        if model == "mf":
            ops.mf_adam_step(*batch, block, ps[0], m[0], v[0], i + 1, LR, BETA1, BETA2, EPS, LAMBDA, losses[i:i + 1], st)
        else:
            step = ops.transr_adam_step if model == "transr" else ops.transe_adam_step
            step(*batch, block, *ps, arr_m, arr_v, [i + 1] * len(ps), LR, BETA1, BETA2, EPS, LAMBDA, losses[i:i + 1], st)
    torch.cuda.synchronize()
    out = {"losses": _bits(losses)}
    for key, p, m_, v_ in zip(params, ps, m, v):
        for kind, t in (("p", p), ("m", m_), ("v", v_)):
            out["%s.%s" % (key, kind)] = _bits(t) if key == "rel" else _digest(t)
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "step_bits.npz"))
    ap.add_argument("--commit", default=None, help="hash of the commit this build is of (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    version = [ln for ln in subprocess.check_output([hipcc, "--version"], text=True).splitlines() if "clang version" in ln]
    dev = torch.device("cuda:0")
    arrays = {}
    for name in CASES:
        arrays.update({"%s/%s" % (name, k): np.asarray(v) for k, v in run_case(name, dev).items()})
    arrays["commit"] = np.array(commit)
    arrays["hipcc"] = np.array(version[0] if version else "unknown")
    np.savez_compressed(a.out, **arrays)
    for k in sorted(arrays):
        print(k, arrays[k].shape if arrays[k].ndim else str(arrays[k]))
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
