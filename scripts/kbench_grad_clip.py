#!/usr/bin/env python3
"""Global-norm gradient clipping on the amazon-book parameter set (developer tool; not part of the product path or of
bench.py's contract): the 159,251 x 64 entity table, W_R 41 x 64 x 64, relation_embed 41 x 64 and the three res_fc_2 of
the default model, every one with a gradient.  Three forms of the optimiser step in the same run,
  (a) FusedAdam.step()                                       no clipping
  (b) FusedAdam.step(max_grad_norm=1.0)                      norm (2 launches) + the clipped Adam launch
  (c) torch.nn.utils.clip_grad_norm_(params, 1.0); step()    torch's clip in front of the plain step
beside (d) this package's in-place clip_grad_norm_ + step(), the norm alone (ops.grad_norm: one read of the gradients)
and a device copy that reads as many bytes - interleaved rounds in one process, HIP events around each form.  Then the
kernel launches of one CF step with and without clipping, counted with torch.profiler.

  python scripts/kbench_grad_clip.py [--rounds 50] [--scale 1.0] [--no-step]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fns, rounds, warm=5):
    names = list(fns)
    for _ in range(warm):
        for n in names:
            fns[n]()
    ts = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[n]()
            b.record()
            ts[n].append((a, b))
    torch.cuda.synchronize()
    return {n: np.array([a.elapsed_time(b) for a, b in v]) for n, v in ts.items()}


def count_launches(fn):
    """Device kernels one call of `fn` enqueues (torch.profiler sees every HIP launch of the process)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.name
             and "Memset" not in e.name]
    return len(names), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-step", action="store_true", help="skip the CF step's launch counts")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops, synth
    dev = torch.device("cuda:0")
    n, trip, R = synth.amazon_book_ckg(scale=args.scale)
    D = 64

    def fresh():
        torch.manual_seed(0)
        model = K.KGATPropagation(n, R, D, D, 3, D, dropout=0.1).to(dev)
        params = [p for p in model.parameters() if p.requires_grad]
        g = torch.Generator(device=dev).manual_seed(1)
        for p in params:   # norm well above 1: the clip is active in (b), (c), (d)
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
        return model, params, K.FusedAdam(params, lr=1e-4)

    forms = {k: fresh() for k in "abcd"}
    params = forms["a"][1]
    elems = sum(p.numel() for p in params)
    print("N=%d R=%d rounds=%d | %d parameter tensors, %d elements, gradients %.1f MB | GRAD_NORM_CHAIN %d" % (
        n, R, args.rounds, len(params), elems, 4 * elems / 1e6, ops.GRAD_NORM_CHAIN))
    for name, p in forms["a"][0].named_parameters():
        print("   %-28s %s" % (name, tuple(p.shape)))
    grads_a = [p.grad for p in params]
    src = torch.empty(4 * elems, dtype=torch.uint8, device=dev)
    dst = torch.empty(2 * elems, dtype=torch.uint8, device=dev)
    fns = {
        "(a) step()": lambda o=forms["a"][2]: o.step(),
        "(b) step(max_grad_norm=1)": lambda o=forms["b"][2]: o.step(max_grad_norm=1.0),
        "(c) torch clip_grad_norm_ + step()": lambda o=forms["c"][2], ps=forms["c"][1]: (
            torch.nn.utils.clip_grad_norm_(ps, 1.0), o.step()),
        "(d) K.clip_grad_norm_ + step()": lambda o=forms["d"][2], ps=forms["d"][1]: (K.clip_grad_norm_(ps, 1.0), o.step()),
        "norm alone (ops.grad_norm)": lambda: ops.grad_norm(grads_a, 1.0),
        # half the gradients' bytes read and written = the gradients' byte count moved
        "copy moving the gradients' bytes": lambda: dst.copy_(src[:2 * elems]),
    }
    t = timeit(fns, args.rounds)
    med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    for k in fns:
        print("%-36s median %8.2f us  (min %8.2f, p90 %8.2f)" % (k, med[k], 1e3 * t[k].min(), 1e3 * float(np.percentile(t[k], 90))))
    a, b, c = med["(a) step()"], med["(b) step(max_grad_norm=1)"], med["(c) torch clip_grad_norm_ + step()"]
    rd = med["norm alone (ops.grad_norm)"]
    print("(b) - (a) = %.2f us  against the norm alone %.2f us (%.1f MB read: %.2f TB/s)" % (b - a, rd, 4 * elems / 1e6,
                                                                                           4 * elems / rd / 1e6))
    print("(c) - (a) = %.2f us;  (b) / (c) = %.3f  (%s)" % (c - a, b / c, "(b) is faster" if b < c else "(b) is NOT faster"))
    # what clipping computed: the same norm from torch on the untouched gradients of (a)
    norm, coef = ops.grad_norm(grads_a, 1.0)
    want = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.double()) for g in grads_a]))
    print("norm %.9g (fp64 on the device %.9g, rel. diff %.2e)  coef %.9g" % (
        float(norm), float(want), abs(float(norm) - float(want)) / float(want), float(coef)))
    if args.no_step:
        return
    # the CF step of kgat.py:146-168 (gnn -> BPR loss -> backward -> Adam), its launches with and without the clip
    B = 10240
    n_users = max(int(round(70679 * args.scale)), 4)
    n_items = max(int(round(24915 * args.scale)), 4)
    u = torch.randint(0, n_users, (B,), device=dev).int()
    pi = torch.randint(n_users, n_users + n_items, (B,), device=dev).int()
    ni = torch.randint(n_users, n_users + n_items, (B,), device=dev).int()
    torch.manual_seed(0)
    model = K.KGATPropagation(n, R, D, D, 3, D, dropout=0.1).to(dev)
    opt = K.FusedAdam(model.parameters(), lr=1e-4)
    g = synth.build_graph(n, trip, dev)
    with torch.no_grad():
        g.edata["w"] = model.compute_attention(g)
    norms = torch.zeros(4, device=dev)

    def step(clip):
        loss = model.get_loss(model.gnn(g), u, pi, ni)
        loss.backward()
        if clip:
            opt.step(max_grad_norm=1.0, norm_out=norms[0])
        else:
            opt.step()
        opt.zero_grad()

    for _ in range(3):
        step(False)
        step(True)
    counts = {}
    for clip in (False, True):
        try:
            counts[clip], names = count_launches(lambda: step(clip))
        except Exception as e:   # no count is reported where the profiler did not run
            print("CF step launches (%s): not measured - torch.profiler failed: %r" % ("clipped" if clip else "plain", e))
            continue
        print("CF step launches %-22s %d" % ("with max_grad_norm=1.0:" if clip else "without clipping:", counts[clip]))
        if clip:
            print("   kernels named *grad* or *adam*: %s" % sorted({x for x in names if "grad_" in x or "adam" in x}))
    res = {False: [], True: []}
    import time
    for _ in range(args.rounds):
        for clip in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(clip)
            torch.cuda.synchronize()
            res[clip].append(time.perf_counter() - t0)
    for clip in (False, True):
        print("CF step (fwd+bwd+Adam, batch %d) %-22s median %.4f ms  (min %.4f)" % (
            B, "max_grad_norm=1.0" if clip else "no clipping", 1e3 * float(np.median(res[clip])), 1e3 * min(res[clip])))
    print("last clipped step's gradient norm: %.6g" % float(norms[0]))


if __name__ == "__main__":
    main()
