#!/usr/bin/env python3
"""Laplacian edge weights and node dropout on the benchmark graph (developer tool; not part of the product path or of
bench.py's contract): kgat_edge_norm_f32 (si, bi, with and without the edge-id-ordered output), kgat_edge_dropout_f32
on the forward and the reversed stream, a plain device copy of the same byte count beside each, and the CF step with
node_dropout 0.1 against the same step at 0.  Interleaved rounds in one process; HIP events around single launches, a
host clock between two synchronisations around a whole step.

  python scripts/kbench_edge_weights.py [--rounds 30] [--scale 1.0] [--no-step]
"""
import argparse
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops, synth
    dev = torch.device("cuda:0")
    n, trip, R = synth.amazon_book_ckg(scale=args.scale)
    E = len(trip)
    print("N=%d E=%d R=%d rounds=%d" % (n, E, R, args.rounds))
    graph = synth.build_graph(n, trip, dev)
    st = graph._st
    csr, rev = st.csr(dev), st.csr_rev(dev)
    w = torch.rand(E, device=dev) + 0.1
    out = torch.empty(E, device=dev)

    # bytes a launch moves (streams of E 4-byte items; the two indptr arrays are 0.6 MB each and stay in cache)
    launches = {
        "edge_norm si (w_csr)": (lambda: ops.edge_norm(csr, None, "si", want_eid=False), 2),        # row_of -> w_csr
        "edge_norm si (w_csr + w_eid)": (lambda: ops.edge_norm(csr, None, "si"), 4),              # + eid -> w_eid
        "edge_norm bi (w_csr)": (lambda: ops.edge_norm(csr, rev.indptr, "bi", want_eid=False), 3),  # + col
        "edge_norm bi (w_csr + w_eid)": (lambda: ops.edge_norm(csr, rev.indptr, "bi"), 5),
        "edge_dropout forward stream": (lambda: ops.edge_dropout(w, csr.eid, 0.1, 7), 3),           # key, w_in -> w_out
        "edge_dropout reversed stream": (lambda: ops.edge_dropout(w, rev.eid, 0.1, 7), 3),
    }
    fns = {k: f for k, (f, _) in launches.items()}
    copies = {}
    for streams in sorted({s for _, s in launches.values()}):
        # a device copy that moves the same bytes: streams * 4E in all = a buffer of streams * 2E bytes read and written
        a = torch.empty(streams * 2 * E, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        copies[streams] = "copy of %d x 4E bytes moved" % streams
        fns[copies[streams]] = lambda a=a, b=b: b.copy_(a)
    t = timeit(fns, args.rounds)
    med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}   # us
    for k, (_, streams) in launches.items():
        moved = streams * 4 * E
        c = med[copies[streams]]
        print("%-32s median %7.2f us  (min %7.2f)  %6.1f MB moved  %6.2f TB/s | copy of the same bytes %7.2f us %6.2f TB/s "
              "| x %.2f of the copy's rate" % (k, med[k], 1e3 * t[k].min(), moved / 1e6, moved / med[k] / 1e6, c,
                                                moved / c / 1e6, c / med[k]))
    if args.no_step:
        return
    # the CF step of kgat.py:146-168: gnn (all layers, full graph) -> BPR loss -> backward -> Adam
    D, B = 64, 10240
    u = torch.randint(0, 70679, (B,), device=dev).int()
    pi = torch.randint(70679, 95594, (B,), device=dev).int()
    ni = torch.randint(70679, 95594, (B,), device=dev).int()
    steps = {}
    for name, kw in (("node_dropout=0 (a)", {}), ("node_dropout=0.1", {"node_dropout": 0.1}), ("node_dropout=0 (b)", {}),
                     ("no attention, si, node_dropout=0.1", {"use_attention": False, "node_dropout": 0.1})):
        torch.manual_seed(0)
        model = K.KGATPropagation(n, R, D, D, 3, D, dropout=0.1, **kw).to(dev)
        opt = K.FusedAdam(model.parameters(), lr=0.01)
        g = synth.build_graph(n, trip, dev)
        with torch.no_grad():
            g.edata["w"] = model.compute_attention(g)

        def step(model=model, opt=opt, g=g):
            loss = model.get_loss(model.gnn(g), u, pi, ni)
            loss.backward()
            opt.step()
            opt.zero_grad()
        steps[name] = step
    res = {k: [] for k in steps}
    for _ in range(5):
        for f in steps.values():
            f()
    for _ in range(args.rounds):
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            res[k].append(time.perf_counter() - t0)
    base = None
    for k, v in res.items():
        m = 1e3 * float(np.median(v))
        base = base or m
        print("CF step (fwd+bwd+Adam, 3 layers, d=64, batch %d) %-36s median %.4f ms  (min %.4f, x %.3f of the first)"
              % (B, k, m, 1e3 * min(v), m / base))


if __name__ == "__main__":
    main()
