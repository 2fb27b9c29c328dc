#!/usr/bin/env python3
"""The ranking entries at the amazon-book evaluation shape (70,679 users x 24,915 items x 176 columns; x 352 once):
kgat_eval_recall_ndcg_f32 at K = 20 beside kgat_eval_topk_f32 at K = 20 ... 128, metrics.calc_metrics at the KGAT
paper's five cut-offs and metrics.calc_recall_ndcg_sorted(K = 100) - the torch route to the same numbers (developer
tool; not part of the product path or of bench.py's contract).  Interleaved rounds in one process after a warm-up of
every shape; device launches are timed with HIP events, whole calls (dict handling, the means' copy to the host) with
a host clock between two synchronisations; medians and the spread (min, max) are printed.

  python scripts/kbench_eval_topk.py [--rounds 15] [--only-old]     > profiles/kbench_eval_topk.txt

--only-old times the K = 20 entry alone; KGAT_TREE=<another checkout, built> imports the package from there instead
of from this tree - the two together alternate two builds of the library in one job.  Run it under a time limit of its
own (timeout -k 10 600 ...)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("KGAT_TREE", ROOT))


def event_rounds(fns, rounds, warm=2):
    names = list(fns)
    for _ in range(warm):
        for n in names:
            fns[n]()
    torch.cuda.synchronize()
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


def host_rounds(fns, rounds, warm=1):
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


def show(res):
    for n, t in res.items():
        print("   %-34s median %9.3f ms   min %9.3f   max %9.3f   (%d rounds)" % (n, np.median(t), t.min(), t.max(), len(t)))
    return {n: float(np.median(t)) for n, t in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--only-old", action="store_true")
    args = ap.parse_args()
    from dgl_kgat_amd import metrics, ops
    dev = torch.device("cuda:0")
    n_u, n_i = 70679, 24915
    rng = np.random.default_rng(6)
    item_range = np.arange(n_u, n_u + n_i)
    deg = np.minimum(rng.zipf(1.6, n_u) + 1, 3000)
    train = {u: np.unique(rng.integers(0, n_i, deg[u])) for u in range(n_u)}
    test = {u: np.unique(rng.integers(0, n_i, 1 + (u % 5))) for u in range(n_u)}
    plan = metrics.EvalPlan(train, test, item_range, dev)
    for F in (176, 352):
        g = torch.Generator(device="cpu").manual_seed(5)
        e = torch.randn((n_u + n_i, F), generator=g).to(dev)
        sweep = (e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items)
        fns = {"eval_recall_ndcg K=20": lambda: ops.eval_recall_ndcg(*sweep, plan.test_ptr, plan.test_items, 20)}
        print("%d users x %d items x %d columns: launches (items layout + sweep + merge), HIP events" % (n_u, n_i, F))
        if args.only_old:
            show(event_rounds(fns, args.rounds))
            return
        for K in ((20, 40, 64, 100, 128) if F == 176 else (100,)):
            fns["eval_topk K=%d" % K] = lambda K=K: ops.eval_topk(*sweep, K)
        med = show(event_rounds(fns, args.rounds))
        old = med["eval_recall_ndcg K=20"]
        print("   ratios to eval_recall_ndcg K=20: " + ", ".join(
            "%s %.2f" % (n.split()[1], v / old) for n, v in med.items() if n.startswith("eval_topk")))
        if F != 176:
            continue
        ws = ops._lib.load().kgat_eval_topk_workspace_bytes(n_u, n_i, F, 100)
        print("   workspace of eval_topk K=100: %.1f MB" % (ws / 1e6))
        print("whole calls with plan= (host clock between synchronisations)")
        ks = (20, 40, 60, 80, 100)
        calls = {"calc_recall_ndcg K=20": lambda: metrics.calc_recall_ndcg(e, train, test, item_range, K=20, plan=plan),
                 "calc_metrics Ks=20,40,60,80,100": lambda: metrics.calc_metrics(e, train, test, item_range, Ks=ks, plan=plan)}
        med = show(host_rounds(calls, args.rounds))
        srt = show(host_rounds({"calc_recall_ndcg_sorted K=100": lambda: metrics.calc_recall_ndcg_sorted(
            e, train, test, item_range, K=100)}, 3, warm=1))
        print("   calc_recall_ndcg_sorted(K=100) / calc_metrics(5 cut-offs) = %.1f"
              % (srt["calc_recall_ndcg_sorted K=100"] / med["calc_metrics Ks=20,40,60,80,100"]))
        a = metrics.calc_metrics(e, train, test, item_range, Ks=ks, plan=plan)
        b = metrics.calc_recall_ndcg_sorted(e, train, test, item_range, K=100)
        print("   recall@100 %.6f ndcg@100 %.6f (calc_metrics)   %.6f %.6f (sorted)" % (a["recall"][-1], a["ndcg"][-1], *b))


if __name__ == "__main__":
    main()
