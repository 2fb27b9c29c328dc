#!/usr/bin/env python3
"""TransR link prediction on the amazon-book-shaped synthetic CKG (developer tool; not part of the product path or of
bench.py's contract): kgat_transr_project_f32 alone (all entities, one relation), kgat_transr_rank_f32 alone (2,048
queries of one relation against all entities, filtered) and kg_metrics end to end (2,048 triples over all relations,
both sides), each beside the same computation in torch operators on the same device - per relation
F.normalize(ent @ W_r), one matmul against the queries, compare and sum - at d = k = 64 and d = k = 128.  Interleaved
rounds in one process, medians; HIP events around the single kernels, a host clock between two synchronisations around
kg_metrics.  Before timing, the kernels' counts are compared with the torch form's on the same inputs.

  python scripts/kbench_kg_rank.py [--rounds 20] [--scale 1.0] [--queries 2048] [--out profiles/kbench_kg_rank.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12     # MI355X fp32 matrix peak, flop/s


def timeit(fns, rounds, warm=3, calls=3):
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


def host_clock(fns, rounds, warm=2):
    names = list(fns)
    for _ in range(warm):
        for n in names:
            fns[n]()
    ts = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[n]()
            torch.cuda.synchronize()
            ts[n].append(1e3 * (time.perf_counter() - t0))
    return {n: np.array(v) for n, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import kg_eval, ops, synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    n, trip, R = synth.amazon_book_ckg(scale=args.scale)
    trip = np.asarray(trip, np.int64)
    say("N=%d triples=%d R=%d queries=%d rounds=%d device=%s" % (n, len(trip), R, args.queries, args.rounds,
                                                               torch.cuda.get_device_name(0)))
    known = K.KnownTriples(trip[:, 0], trip[:, 1], trip[:, 2], n, R, device=dev)
    rng = np.random.default_rng(0)
    sample = trip[rng.choice(len(trip), args.queries, replace=False)]
    rel_big = int(np.bincount(trip[:, 1], minlength=R).argmax())
    one_rel = trip[trip[:, 1] == rel_big]
    one_rel = one_rel[rng.choice(len(one_rel), args.queries, replace=len(one_rel) < args.queries)]
    for d in (64, 128):
        k = d
        torch.manual_seed(0)
        model = K.KGATPropagation(n, R, d, k, 1, 16, dropout=0.0).to(dev)
        ent, W_R, rel = (x.detach() for x in (model.entity_embed.weight, model.W_R, model.relation_embed.weight))
        W_r, rel_row = W_R[rel_big].contiguous(), rel[rel_big].contiguous()
        h32 = torch.as_tensor(one_rel[:, 0], device=dev).to(torch.int32)
        t32 = torch.as_tensor(one_rel[:, 2], device=dev).to(torch.int32)
        fptr, fids = known.lists((one_rel[:, 0], one_rel[:, 1]), "tail")
        P, n2 = ops.transr_project(ent, W_r)
        Q, _ = ops.transr_project(ent, W_r, rel_row=rel_row, ids=h32, want_n2=False)
        lt, eq = ops.transr_rank(Q, t32, P, n2, 0, fptr, fids)
        lt_t, eq_t = kg_eval._rank_torch(Q, t32, P, n2, 0, fptr, fids)
        same = int((lt == lt_t).sum()), int((eq == eq_t).sum())
        say("d=k=%d: kernel counts equal to the torch form's on the same P, Q: lt %d / %d, eq %d / %d queries "
            "(%d filter entries; a library GEMM sums in another order: near-ties may differ)"
            % (d, same[0], args.queries, same[1], args.queries, fids.numel()))
        if same[0] < 0.98 * args.queries:
            raise SystemExit("rank kernel differs from the torch form at d=%d" % d)
        Pb, n2b = torch.empty_like(P), torch.empty_like(n2)

        def torch_project():
            u = F.normalize(ent @ W_r, p=2, dim=1)
            return u, (u * u).sum(1)

        def torch_rank():
            return kg_eval._rank_torch(Q, t32, P, n2, 0, fptr, fids)

        t = timeit({"project kernel": lambda: ops.transr_project(ent, W_r, out=Pb, n2_out=n2b),
                    "project torch": torch_project}, args.rounds)
        med = {key: float(np.median(v)) for key, v in t.items()}
        out_bytes = n * k * 4 + n * 4
        flop = 2.0 * n * d * k
        for key in t:
            say("d=k=%-3d %-16s median %8.3f ms (min %8.3f, max %8.3f) | %6.1f GFLOP/s | output stream %6.1f GB/s "
                "(+ %.1f GB/s read)" % (d, key, med[key], t[key].min(), t[key].max(), flop / med[key] / 1e6,
                                        out_bytes / med[key] / 1e6, n * d * 4 / med[key] / 1e6))
        say("d=k=%-3d project: torch / kernel = %.2f" % (d, med["project torch"] / med["project kernel"]))
        # the check of the sorted lists costs a host read: timed apart from the launch
        lib = ops._lib.load()
        lt_b, eq_b = torch.empty_like(lt), torch.empty_like(eq)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def rank_launch():
            ops.check(lib.kgat_transr_rank_f32(args.queries, n, 0, k, Q.data_ptr(), t32.data_ptr(), P.data_ptr(),
                                               n2.data_ptr(), fptr.data_ptr(), fids.data_ptr(), fids.numel(),
                                               lt_b.data_ptr(), eq_b.data_ptr(), stream), "kgat_transr_rank_f32")

        t = timeit({"rank kernel": rank_launch, "rank torch": torch_rank}, args.rounds)
        med = {key: float(np.median(v)) for key, v in t.items()}
        flop = 2.0 * args.queries * n * k
        for key in t:
            say("d=k=%-3d %-16s median %8.3f ms (min %8.3f, max %8.3f) | %7.1f GFLOP/s = %.3f of the fp32 MFMA peak"
                % (d, key, med[key], t[key].min(), t[key].max(), flop / med[key] / 1e6, flop / med[key] / 1e-3 / PEAK_F32_MFMA))
        say("d=k=%-3d rank: torch / kernel = %.2f" % (d, med["rank torch"] / med["rank kernel"]))
        hrt = [torch.as_tensor(np.ascontiguousarray(sample[:, c]), device=dev) for c in range(3)]

        def metrics_kernels():
            return model.kg_metrics(*hrt, known=known, side="both")

        def metrics_torch():
            saved = kg_eval._use_kernels
            kg_eval._use_kernels = lambda *a: False
            try:
                return model.kg_metrics(*hrt, known=known, side="both")
            finally:
                kg_eval._use_kernels = saved

        a, b = metrics_kernels(), metrics_torch()
        say("d=k=%-3d kg_metrics both sides: kernels mrr %.6f mr %.2f | torch form mrr %.6f mr %.2f"
            % (d, a["mrr"], a["mr"], b["mrr"], b["mr"]))
        t = host_clock({"kg_metrics kernels": metrics_kernels, "kg_metrics torch": metrics_torch}, max(args.rounds // 4, 3))
        med = {key: float(np.median(v)) for key, v in t.items()}
        n_rel_used = len(np.unique(sample[:, 1]))
        for key in t:
            say("d=k=%-3d %-20s median %9.2f ms (min %9.2f) host clock, %d queries x 2 sides over %d relations"
                % (d, key, med[key], t[key].min(), args.queries, n_rel_used))
        say("d=k=%-3d kg_metrics: torch / kernels = %.2f" % (d, med["kg_metrics torch"] / med["kg_metrics kernels"]))
        del model, P, Q, Pb
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
