#!/usr/bin/env python3
"""The relational convolution's aggregation on the amazon-book shape (developer tool; not part of the product path or
of bench.py's contract): N = 159,251, E = 3,663,302, D = 64, R relations of the synthetic CKG (41), B in {1, 2, 4, 8}
bases, norm = 1 / in-degree.  Two forms of the same computation, values equal to rounding (tests/test_gpu_rgcn.py):

  fused      autograd.rgcn_aggregate: kgat_rgcn_fwd_f32 (+ kgat_rgcn_bwd_x_f32, kgat_rgcn_bwd_coef_f32) - a source row
             is gathered once per edge and feeds B accumulators, nothing of size E x D or E x B is written
  composed   what the package offered before: per basis a torch-gathered weight stream norm * a[etype, b] (E,) and one
             u_mul_e_sum over it (B operator calls; B edge-sized temporaries, and the same again in backward)

each as forward (no grad) and as forward + backward (gradients to x and a).  Beside them, from the same run: ONE
kgat_spmm_umule_sum_f32 launch at the same D (CSR-ordered weights), and kgat_gather_probe_f32 fetching the E source
rows with the aggregation's access pattern and doing nothing else - the gather ceiling.  A round runs `--iters` calls
of every form, interleaved in one process, between device events; medians over the rounds with min / max and the
spread (max - min) / median.

  python scripts/kbench_rgcn.py [--rounds 10] [--iters 20] [--out profiles/kbench_rgcn.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 64
BASES = [1, 2, 4, 8]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from dgl_kgat_amd import autograd, ops, synth
    dev = torch.device("cuda:0")
    n, trip, R = synth.amazon_book_ckg()
    g = synth.build_graph(n, trip, dev)
    st = g._st
    csr = st.csr(dev)
    e = csr.col.numel()
    etypes = g.edata["type"]
    norm = g.laplacian_weights("si")
    norm_flat = norm.reshape(-1)
    w_csr = st.csr_weights(norm)
    say("N=%d E=%d D=%d R=%d iters/round=%d rounds=%d device=%s" % (n, e, D, R, args.iters, args.rounds,
                                                                     torch.cuda.get_device_name(0)))

    def composed(x, a):
        return torch.stack([autograd.u_mul_e_sum(g, x, norm_flat * a[etypes, b]) for b in range(a.shape[1])], 1)

    def fused(x, a):
        return autograd.rgcn_aggregate(g, x, a, etypes, norm)

    def timed(fn, iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters

    torch.manual_seed(64)
    x = torch.randn(n, D, device=dev)
    sink = ops.gather_probe(csr.col, x)
    for B in BASES:
        torch.manual_seed(B)
        a = torch.randn(R, B, device=dev)
        g_Z = torch.randn(n, B, D, device=dev)
        with torch.no_grad():
            ref, got = composed(x, a), fused(x, a)
        say("B=%d max |fused - composed| / max |composed| = %.2e" % (B, float((got - ref).abs().max() / ref.abs().max())))
        ins = [t.clone().requires_grad_(True) for t in (x, a)]

        def fwd(form):
            def run():
                with torch.no_grad():
                    form(x, a)
            return run

        def fwd_bwd(form):
            def run():
                for t in ins:
                    t.grad = None
                form(*ins).backward(g_Z)
            return run

        fns = {"fused fwd": fwd(fused), "composed fwd": fwd(composed), "fused fwd+bwd": fwd_bwd(fused),
               "composed fwd+bwd": fwd_bwd(composed),
               "one sum launch": lambda: ops.spmm(csr.indptr, csr.col, csr.row_of, x, w_csr),
               "gather probe": lambda: ops.gather_probe(csr.col, x, sink)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                ts[k].append(timed(fn, args.iters))
        med = {}
        for k in fns:
            v = np.array(ts[k])
            med[k] = float(np.median(v))
            say("B=%d %-17s median %.4f ms (min %.4f, max %.4f, spread %.1f %%)" % (
                B, k, med[k], v.min(), v.max(), 100.0 * (v.max() - v.min()) / med[k]))
        for what in ("fwd", "fwd+bwd"):
            say("B=%d composed / fused, %s: %.2f x" % (B, what, med["composed " + what] / med["fused " + what]))
        say("B=%d fused fwd = %.2f x one sum launch (B launches would be %d x), %.2f x the gather probe" % (
            B, med["fused fwd"] / med["one sum launch"], B, med["fused fwd"] / med["gather probe"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
