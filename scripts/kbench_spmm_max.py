#!/usr/bin/env python3
"""The max reducer on the benchmark graph (developer tool; not part of the product path or of bench.py's contract):
kgat_spmm_umule_max_f32 with and without the argmax output, kgat_spmm_umule_sum_f32 beside it in the same rounds, at
D = 16, 32, 64, 128, and explain.attention_paths for 128 queries with max_len = 3.  Interleaved rounds in one process;
HIP events around ten back-to-back calls (per-call time = a tenth), a host clock between two synchronisations around
attention_paths.  Before timing, the values of every width are compared with torch's scatter-amax of the same fp32
products (bit equality) on this graph.

  python scripts/kbench_spmm_max.py [--rounds 30] [--scale 1.0] [--out profiles/kbench_spmm_max.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fns, rounds, warm=5, calls=10):
    """Per-call times (ms): every sample is one event pair around `calls` back-to-back calls, so that the queue stays
    full inside the window and a sample is 0.4 ms and more instead of one 40-us call; variants interleaved per round."""
    names = list(fns)
    for _ in range(warm):
        for n in names:
            fns[n]()
    ts = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fns[n]()
            b.record()
            ts[n].append((a, b))
    torch.cuda.synchronize()
    return {n: np.array([a.elapsed_time(b) / calls for a, b in v]) for n, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import explain, ops, synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    n, trip, R = synth.amazon_book_ckg(scale=args.scale)
    E = len(trip)
    say("N=%d E=%d R=%d rounds=%d (10 calls per sample) device=%s" % (n, E, R, args.rounds, torch.cuda.get_device_name(0)))
    graph = synth.build_graph(n, trip, dev)
    st = graph._st
    csr = st.csr(dev)
    torch.manual_seed(0)
    w = torch.rand(E, device=dev) + 0.1   # CSR order
    row = csr.row_of.long()
    has_in = (csr.indptr[1:] > csr.indptr[:-1])
    for D in (16, 32, 64, 128):
        X = torch.randn(n, D, device=dev)
        ws_max, ws_sum = ops.spmm_max_workspace(E, D, dev), ops.spmm_workspace(E, D, dev)
        o_max = torch.empty(n, D, device=dev)
        o_sum = torch.empty(n, D, device=dev)
        # values against torch (scatter-amax of the same products; rows without in-edges are 0 in both)
        out, arg = ops.spmm_max(csr.indptr, csr.col, csr.row_of, X, w, eid=csr.eid, workspace=ws_max)
        prod = w[:, None] * X[csr.col.long()]
        want = torch.full((n, D), float("-inf"), device=dev).scatter_reduce_(0, row[:, None].expand(E, D), prod, "amax")
        want = torch.where(has_in[:, None], want, torch.zeros_like(want))
        same = bool((out == want).all()) and bool(((arg >= 0) == has_in[:, None]).all())
        pos = st.csr_pos(dev).long()
        won = prod[pos[arg.clamp(min=0).long()], torch.arange(D, device=dev)[None, :].expand(n, D)]
        same = same and bool(torch.where(has_in[:, None], won == out, torch.ones_like(won, dtype=torch.bool)).all())
        say("D=%-3d values == torch scatter-amax and arg attains them: %s (tile %d edges)"
            % (D, same, ops._lib.load().kgat_spmm_tile_edges(E, D)))
        if not same:
            raise SystemExit("max reducer differs from torch at D=%d" % D)
        del prod, want, won
        fns = {
            "max + arg": lambda: ops.spmm_max(csr.indptr, csr.col, csr.row_of, X, w, eid=csr.eid, out=o_max, workspace=ws_max),
            "max, no arg": lambda: ops.spmm_max(csr.indptr, csr.col, csr.row_of, X, w, eid=csr.eid, want_arg=False, out=o_max,
                                                workspace=ws_max),
            "max + arg, copy_src": lambda: ops.spmm_max(csr.indptr, csr.col, csr.row_of, X, None, eid=csr.eid, out=o_max,
                                                        workspace=ws_max),
            "sum": lambda: ops.spmm(csr.indptr, csr.col, csr.row_of, X, w, out=o_sum, workspace=ws_sum),
            # the sum's first form hands (col, row, w) around with wavefront shuffles, as the max kernel does
            "sum, shuffle form": lambda: ops.spmm(csr.indptr, csr.col, csr.row_of, X, w, out=o_sum, workspace=ws_sum,
                                                  algo="merge1"),
        }
        t = timeit(fns, args.rounds)
        med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}   # us
        for k in fns:
            # (the argmax output is allocated inside the call: torch's caching allocator, no device work)
            say("D=%-3d %-22s median %8.2f us  (min %8.2f, max %8.2f)  x %.2f of the sum"
                % (D, k, med[k], 1e3 * t[k].min(), 1e3 * t[k].max(), med[k] / med["sum"]))
    # attention_paths: 128 queries, max_len 3 (three launches at D = 128 + the gathers of the backtrack)
    model = K.KGATPropagation(n, R, 64, 64, 3, 64, dropout=0.0).to(dev)
    with torch.no_grad():
        graph.edata["w"] = model.compute_attention(graph)
    n_users = max(int(round(70679 * args.scale)), 4)
    n_items = max(int(round(24915 * args.scale)), 4)
    rng = np.random.default_rng(0)
    users = rng.integers(0, n_users, 128).tolist()
    items = (n_users + rng.integers(0, n_items, 128)).tolist()
    for _ in range(3):
        res = explain.attention_paths(graph, graph.edata["w"], users, items, max_len=3)
    ts = []
    for _ in range(max(args.rounds // 3, 5)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = explain.attention_paths(graph, graph.edata["w"], users, items, max_len=3)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    say("attention_paths, 128 queries, max_len 3: median %.3f ms (min %.3f) host clock; %d of 128 queries have a walk"
        % (1e3 * float(np.median(ts)), 1e3 * min(ts), int((res.best_len > 0).sum())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
