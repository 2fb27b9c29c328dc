#!/usr/bin/env python3
"""Bit patterns of the attention logits, every MFMA form: what tests/test_gpu_att_bits.py compares with
tests/golden/att_bits.npz.  The test imports small_case() / ring_case() from here, so the recorded values
and the compared ones come from one piece of code; run as a program (on the GPU, from a build of the commit
whose bits are to be pinned) it writes the fixture:

    python scripts/record_att_bits.py --commit $(git rev-parse HEAD) --out tests/golden/att_bits.npz

Inputs come from seeds.  Only this package and numpy are needed."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTHS = (16, 32, 64, 128)
SMALL_CAPS = (64, 512)   # 512: the hub group's tiles have more than four 64-position chunks
SMALL_PARTS = 37


def _t32(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)


def _tf(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _structure(ops, n, src, dst, et, R, dev):
    """CSR-ordered edges grouped stably by relation (as DGLGraph.rel_groups builds them), and the head groups."""
    indptr, col, eid, row_of = ops.csr_from_coo(n, _t32(src, dev), _t32(dst, dev))
    rel_ptr, idx = ops.group_by_relation(ops.gather(eid, _t32(et, dev)), R)
    perm, src_g, dst_g = ops.gather(idx, eid), ops.gather(idx, col), ops.gather(idx, row_of)
    gid, gptr, g_node, n_groups = ops.head_groups(rel_ptr, dst_g)
    return dict(eid=eid, rel_ptr=rel_ptr, perm=perm, src_g=src_g, dst_g=dst_g, pos_g=idx, gid=gid, gptr=gptr,
                g_node=g_node, n_groups=n_groups)


def _params(rng, n, R, d, dev):
    ent = rng.standard_normal((n, d)).astype(np.float32)
    W = ((rng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
    rel = rng.standard_normal((R, d)).astype(np.float32)
    return _tf(ent, dev), _tf(W, dev), _tf(rel, dev)


def _one_kernel_and_split(ops, n, s, p):
    """CSR-order logits of the one-kernel form; the split form must give the same bits."""
    import torch
    full, full_csr = ops.att_score(n, s["rel_ptr"], s["perm"], s["src_g"], s["dst_g"], *p, pos_g=s["pos_g"], algo="mfma")
    split, split_csr = ops.att_score_split(n, s["rel_ptr"], s["perm"], s["src_g"], s["pos_g"], s["gid"], s["gptr"],
                                           s["g_node"], s["n_groups"], *p)
    assert torch.equal(split, full) and torch.equal(split_csr, full_csr)
    assert torch.equal(full_csr, full[s["eid"].long()])
    return full_csr, split_csr


def _folded(ops, n, s, p, f32_products):
    import torch
    fold, fold_csr = ops.att_score_split(n, s["rel_ptr"], s["perm"], s["src_g"], s["pos_g"], s["gid"], s["gptr"],
                                         s["g_node"], s["n_groups"], *p, folded=True, f32_products=f32_products)
    assert torch.equal(fold_csr, fold[s["eid"].long()])
    return fold_csr


def _fused(ops, n, s, p, tiles, rel_tptr, part_tptr, f32_products):
    """CSR-order logits of the fused form; its edge-id-order and grouped-order outputs are the same values permuted,
    and the even split over workgroups gives the same bits as the cost-balanced one."""
    import torch
    args = (n, s["rel_ptr"], s["perm"], s["src_g"], s["pos_g"], s["gid"], s["gptr"], s["g_node"], tiles, rel_tptr) + p
    f_eid, f_csr, f_g = ops.att_score_fused(*args, part_tptr=part_tptr, f32_products=f32_products, want_grouped=True)
    assert torch.equal(f_csr, f_eid[s["eid"].long()]) and torch.equal(f_g, f_csr[s["pos_g"].long()])
    only_g = ops.att_score_fused(*args, part_tptr=part_tptr, f32_products=f32_products, want_eid=False, want_csr=False,
                                 want_grouped=True)[2]
    only_csr = ops.att_score_fused(*args, part_tptr=part_tptr, f32_products=f32_products, want_eid=False)[1]
    even = ops.att_score_fused(*args, f32_products=f32_products, want_eid=False)[1]
    assert torch.equal(only_g, f_g) and torch.equal(only_csr, f_csr) and torch.equal(even, f_csr)
    return f_csr


def small_graph():
    """n = 300, e = 4,000, R = 5: types from [-1, R] (never-scored edges on both sides), relation 1 empty, half the
    edges in relation 3, 1,200 edges into node 3 - one (head, relation) group of about 600 positions."""
    n, e, R = 300, 4000, 5
    rng = np.random.default_rng(4101)
    src = rng.integers(0, n, e).astype(np.int32)
    dst = rng.integers(0, n, e).astype(np.int32)
    dst[rng.choice(e, 1200, replace=False)] = 3
    et = rng.integers(-1, R + 1, e).astype(np.int32)
    et[rng.choice(e, e // 2, replace=False)] = 3
    et[et == 1] = 2
    return n, e, R, src, dst, et


def small_case(dev):
    """name -> uint32 bit patterns of the CSR-order logits, every form at every width it supports."""
    from dgl_kgat_amd import ops
    n, e, R, src, dst, et = small_graph()
    s = _structure(ops, n, src, dst, et, R, dev)
    out = {}
    for d in WIDTHS:
        p = _params(np.random.default_rng(4200 + d), n, R, d, dev)
        if ops.att_score_split_supported(n, d, d, R):
            out["mfma.d%d" % d] = _bits(_one_kernel_and_split(ops, n, s, p)[0])
        if ops.att_score_folded_supported(n, d, d, R):
            for f32p in (False, True):
                out["folded.d%d.%s" % (d, "f32" if f32p else "pieces")] = _bits(_folded(ops, n, s, p, f32p))
        if not ops.att_score_fused_supported(n, d, d, R):
            continue
        for cap in SMALL_CAPS:
            for f32p in (False, True):
                # one product form at two widths: d = 16 has no piece products (the flag changes nothing), and at
                # d = 128 the entry refuses the fp32 ones
                if (d % 32 != 0 and not f32p) or (d == 128 and f32p):
                    continue
                tiles, rel_tptr, part_tptr = ops.fold_tiles(s["rel_ptr"], s["gid"], s["gptr"], s["n_groups"], cap=cap,
                                                            n_parts=SMALL_PARTS, cost=ops.fold_tile_cost(d, f32p))
                if cap > 256:  # the loop behind a tile's fourth chunk is reached
                    t = tiles.cpu().numpy()[:int(rel_tptr[-1])]
                    assert int((t[:, 3] - t[:, 2]).max()) > 4 * 64
                out["fused.d%d.%s.cap%d" % (d, "f32" if f32p else "pieces", cap)] = _bits(
                    _fused(ops, n, s, p, tiles, rel_tptr, part_tptr, f32p))
    return out


RING_N, RING_E, RING_R = 200000, 1200000, 3


def ring_case(dev):
    """name -> sha-256 of the CSR-order logits on a graph deep enough for the persistent kernels' rings and index
    look-ahead to reach their steady state: RING_N nodes, RING_E edges, RING_R relations, uniform, no hub."""
    from dgl_kgat_amd import ops
    n, e, R = RING_N, RING_E, RING_R
    rng = np.random.default_rng(4301)
    src = rng.integers(0, n, e).astype(np.int32)
    dst = rng.integers(0, n, e).astype(np.int32)
    et = rng.integers(0, R, e).astype(np.int32)
    s = _structure(ops, n, src, dst, et, R, dev)
    ent128 = rng.standard_normal((n, 128), dtype=np.float32)
    out = {}

    def digest(t):
        return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()

    for d in (64, 128):
        prng = np.random.default_rng(4400 + d)
        W = ((prng.random((R, d, d)) - 0.5) * (2.0 / np.sqrt(d))).astype(np.float32)
        rel = prng.standard_normal((R, d)).astype(np.float32)
        p = (_tf(ent128[:, :d], dev), _tf(W, dev), _tf(rel, dev))
        if d == 64:
            one, split = _one_kernel_and_split(ops, n, s, p)
            out["mfma.d64"], out["split.d64"] = digest(one), digest(split)
        out["folded.d%d" % d] = digest(_folded(ops, n, s, p, False))
        tiles, rel_tptr, part_tptr = ops.fold_tiles(s["rel_ptr"], s["gid"], s["gptr"], s["n_groups"],
                                                    cost=ops.fold_tile_cost(d))
        out["fused.d%d" % d] = digest(_fused(ops, n, s, p, tiles, rel_tptr, part_tptr, False))
    out["groups"] = str(s["n_groups"])
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "att_bits.npz"))
    ap.add_argument("--commit", default=None, help="hash of the commit this build is of (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    version = [ln for ln in subprocess.check_output([hipcc, "--version"], text=True).splitlines() if "clang version" in ln]
    dev = torch.device("cuda:0")
    arrays = {"small/" + k: v for k, v in small_case(dev).items()}
    arrays.update({"ring/" + k: np.array(v) for k, v in ring_case(dev).items()})
    arrays["commit"] = np.array(commit)
    arrays["hipcc"] = np.array(version[0] if version else "unknown")
    np.savez_compressed(a.out, **arrays)
    for k in sorted(arrays):
        print(k, arrays[k].shape if arrays[k].ndim else str(arrays[k]))
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
