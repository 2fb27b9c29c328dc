#!/usr/bin/env python3
"""The top-4 reducer on the benchmark graph (developer tool; not part of the product path or of bench.py's contract):
kgat_spmm_umule_max4_f32 at Q = 4, 8, 16, 32 with and without its back-pointer outputs, kgat_spmm_umule_max_f32 at the
same row width D = 4 Q beside it in the same rounds, and explain.attention_paths(top=4) against top=1 for 128 queries
with max_len = 3.  Interleaved rounds in one process; HIP events around ten back-to-back calls (per-call time = a tenth),
a host clock between two synchronisations around attention_paths.  Before timing, two query columns of every width are
compared with a torch restatement (two stable sorts of the same fp32 products: bit equality of the four values per row),
and every back-pointer is checked to attain its value and to stand in the kernel's order.

  python scripts/kbench_spmm_kmax.py [--rounds 30] [--scale 1.0] [--out profiles/kbench_spmm_kmax.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kbench_spmm_max import timeit  # noqa: E402  (the same sampling)


def torch_top4(prod, row, indptr, has_in):
    """(n, 4) the four largest of prod (E, 4) per destination row, 0 for rows without in-edges.  prod is in CSR order."""
    E = prod.shape[0]
    flat = prod.reshape(-1)
    rows = row.repeat_interleave(4)
    _, by_val = torch.sort(flat, descending=True, stable=True)
    _, by_row = torch.sort(rows[by_val], stable=True)
    order = by_val[by_row]                                    # (row ascending, value descending)
    first = (4 * indptr[:-1].long())[:, None] + torch.arange(4, device=prod.device)[None, :]
    top = flat[order[first.clamp(max=4 * E - 1)]]
    return torch.where(has_in[:, None], top, torch.zeros_like(top))


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
    pos = st.csr_pos(dev).long()
    for Q in (4, 8, 16, 32):
        D = 4 * Q
        X = torch.randn(n, Q, 4, device=dev)
        X2 = X.reshape(n, D)
        ws4, ws1 = ops.spmm_max4_workspace(E, D, dev), ops.spmm_max_workspace(E, D, dev)
        o1 = torch.empty(n, D, device=dev)
        out, edge, slot = ops.spmm_max4(csr.indptr, csr.col, csr.row_of, X, w, eid=csr.eid, workspace=ws4)
        same = True
        for q in sorted({0, Q - 1}):
            prod = w[:, None] * X[csr.col.long(), q]          # (E, 4), the kernel's products
            same = same and bool((out[:, q] == torch_top4(prod, row, csr.indptr, has_in)).all())
            p_at = pos[edge[:, q].clamp(min=0).long()]
            won = prod[p_at, slot[:, q].clamp(max=3).long()]
            same = same and bool(torch.where(has_in[:, None], won == out[:, q], (edge[:, q] == -1) & (slot[:, q] == 255)).all())
            a, b = out[:, q, :-1], out[:, q, 1:]
            i, k = edge[:, q, :-1], edge[:, q, 1:]
            r, s = slot[:, q, :-1], slot[:, q, 1:]
            ordered = (a > b) | ((a == b) & ((i < k) | ((i == k) & (r < s))))
            same = same and bool(ordered[has_in].all())
            del prod, won
        say("Q=%-2d values == torch's sorted products (2 columns), back-pointers attain them in order: %s (tile %d edges)"
            % (Q, same, ops._lib.load().kgat_spmm_tile_edges(E, D)))
        if not same:
            raise SystemExit("top-4 reducer differs from torch at Q=%d" % Q)
        fns = {
            "max4 + args": lambda: ops.spmm_max4(csr.indptr, csr.col, csr.row_of, X, w, eid=csr.eid, workspace=ws4),
            "max4, no args": lambda: ops.spmm_max4(csr.indptr, csr.col, csr.row_of, X, w, eid=csr.eid, want_arg=False,
                                                   workspace=ws4),
            "max + arg (D = 4 Q)": lambda: ops.spmm_max(csr.indptr, csr.col, csr.row_of, X2, w, eid=csr.eid, out=o1,
                                                        workspace=ws1),
        }
        t = timeit(fns, args.rounds)
        med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}   # us
        for k in fns:
            # (the outputs of max4 are allocated inside the call: torch's caching allocator, no device work)
            say("Q=%-2d %-22s median %8.2f us  (min %8.2f, max %8.2f)  x %.2f of the max kernel"
                % (Q, k, med[k], 1e3 * t[k].min(), 1e3 * t[k].max(), med[k] / med["max + arg (D = 4 Q)"]))
    # attention_paths: 128 queries, max_len 3.  top=1: three launches at D = 128; top=4: four chunks of 32 queries,
    # three launches each at Q = 32, and the backtrack's gathers for four walks per length
    model = K.KGATPropagation(n, R, 64, 64, 3, 64, dropout=0.0).to(dev)
    with torch.no_grad():
        graph.edata["w"] = model.compute_attention(graph)
    n_users = max(int(round(70679 * args.scale)), 4)
    n_items = max(int(round(24915 * args.scale)), 4)
    rng = np.random.default_rng(0)
    users = rng.integers(0, n_users, 128).tolist()
    items = (n_users + rng.integers(0, n_items, 128)).tolist()
    med = {}
    for top in (1, 4):
        for _ in range(3):
            res = explain.attention_paths(graph, graph.edata["w"], users, items, max_len=3, top=top)
        ts = []
        for _ in range(max(args.rounds // 3, 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = explain.attention_paths(graph, graph.edata["w"], users, items, max_len=3, top=top)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        med[top] = 1e3 * float(np.median(ts))
        found = int((res.best_len > 0).sum()) if top == 1 else int((res.ranked_len > 0).sum())
        say("attention_paths(top=%d), 128 queries, max_len 3: median %.3f ms (min %.3f) host clock; %d %s"
            % (top, med[top], 1e3 * min(ts), found,
               "of 128 queries have a walk" if top == 1 else "of 512 ranked walks exist"))
    say("attention_paths top=4 / top=1: x %.2f" % (med[4] / med[1]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
