#!/usr/bin/env python3
"""The exact-rank evaluation at the amazon-book shape (70,679 users x 24,915 items x 176 columns, about 8 test items
per user with a tail of long lists): metrics.calc_rank_metrics(Ks = 20, 200, 1000) beside the only other route to
recall@200 - metrics.calc_recall_ndcg_sorted(K = 200), a users x items score matrix and a full torch sort - and
beside metrics.calc_metrics at the KGAT paper's five cut-offs, the list-based sweep that issues the same MFMAs
(developer tool; not part of the product path or of bench.py's contract).  The protocol of kbench_eval_topk.py:
interleaved rounds in one process after a warm-up of every shape; device launches are timed with HIP events, whole
calls (the means' copy to the host included) with a host clock between two synchronisations; medians and the spread.

  python scripts/kbench_eval_rank.py [--rounds 15] [--F 176]     > profiles/kbench_eval_rank.txt

Run it under a time limit of its own (timeout -k 10 600 ...).  For the launches inside eval_rank run it with --rounds 3
under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("KGAT_TREE", ROOT))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kbench_eval_topk import event_rounds, host_rounds, show  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--F", type=int, default=176)
    ap.add_argument("--no-sorted", action="store_true", help="leave the torch-sort route out (a profiler run)")
    args = ap.parse_args()
    from dgl_kgat_amd import metrics, ops
    dev = torch.device("cuda:0")
    n_u, n_i, F = 70679, 24915, args.F
    rng = np.random.default_rng(6)
    item_range = np.arange(n_u, n_u + n_i)
    deg = np.minimum(rng.zipf(1.6, n_u) + 1, 3000)
    train = {u: np.unique(rng.integers(0, n_i, deg[u])) for u in range(n_u)}
    n_test = np.maximum(rng.poisson(8.0, n_u), 1)
    n_test[::1000] = 300                                   # a tail of long lists: 71 users with 300 entries
    test = {u: np.unique(rng.integers(0, n_i, n_test[u])) for u in range(n_u)}
    plan = metrics.EvalPlan(train, test, item_range, dev)
    lens = np.diff(plan.test_ptr.cpu().numpy())
    g = torch.Generator(device="cpu").manual_seed(5)
    e = torch.randn((n_u + n_i, F), generator=g).to(dev)
    print("%d users x %d items x %d columns; %d test entries (%.2f per user, longest %d), %d train entries" % (
        n_u, n_i, F, lens.sum(), lens.mean(), lens.max(), plan.train_items.numel()))
    sweep = (e, plan.user_ids, plan.item_ids, plan.train_ptr, plan.train_items)
    print("launches (items layout + the entry), HIP events")
    fns = {"eval_rank (mask)": lambda: ops.eval_rank(*sweep, plan.test_ptr, plan.test_items),
           "eval_rank (drop)": lambda: ops.eval_rank(*sweep, plan.test_ptr, plan.test_items, drop_train=True),
           "eval_topk K=100": lambda: ops.eval_topk(*sweep, 100, want_scores=False),
           "eval_topk K=128": lambda: ops.eval_topk(*sweep, 128, want_scores=False),
           "eval_recall_ndcg K=20": lambda: ops.eval_recall_ndcg(*sweep, plan.test_ptr, plan.test_items, 20)}
    show(event_rounds(fns, args.rounds))
    above = ops.eval_rank(*sweep, plan.test_ptr, plan.test_items)
    show(event_rounds({"eval_rank_metrics 3 cut-offs": lambda: ops.eval_rank_metrics(
        above, plan.test_ptr, plan.test_items, n_i, (20, 200, 1000))}, args.rounds))
    ws = ops._lib.load().kgat_eval_rank_workspace_bytes(n_u, n_i, F, plan.train_items.numel(), plan.test_items.numel())
    print("   workspace of eval_rank: %.1f MB" % (ws / 1e6))
    print("whole calls with plan= (host clock between synchronisations)")
    rank_ks, paper_ks = (20, 200, 1000), (20, 40, 60, 80, 100)
    calls = {"calc_rank_metrics Ks=20,200,1000": lambda: metrics.calc_rank_metrics(e, train, test, item_range, Ks=rank_ks, plan=plan),
             "calc_metrics Ks=20,40,60,80,100": lambda: metrics.calc_metrics(e, train, test, item_range, Ks=paper_ks, plan=plan)}
    med = show(host_rounds(calls, args.rounds))
    print("   calc_rank_metrics(3 cut-offs, MRR, MAP, AUC, mean rank) / calc_metrics(5 cut-offs <= 100) = %.2f" % (
        med["calc_rank_metrics Ks=20,200,1000"] / med["calc_metrics Ks=20,40,60,80,100"]))
    a = metrics.calc_rank_metrics(e, train, test, item_range, Ks=rank_ks, plan=plan)
    print("   recall@20 %.6f recall@200 %.6f recall@1000 %.6f ndcg@200 %.6f mrr %.6f map %.6f auc %.6f mean_rank %.1f" % (
        a["recall"][0], a["recall"][1], a["recall"][2], a["ndcg"][1], a["mrr"], a["map"], a["auc"], a["mean_rank"]))
    if args.no_sorted:
        return
    srt = show(host_rounds({"calc_recall_ndcg_sorted K=200": lambda: metrics.calc_recall_ndcg_sorted(
        e, train, test, item_range, K=200)}, 3, warm=1))
    print("   calc_recall_ndcg_sorted(K=200) / calc_rank_metrics(3 cut-offs) = %.1f" % (
        srt["calc_recall_ndcg_sorted K=200"] / med["calc_rank_metrics Ks=20,200,1000"]))
    b = metrics.calc_recall_ndcg_sorted(e, train, test, item_range, K=200)
    print("   recall@200 %.6f ndcg@200 %.6f (calc_rank_metrics)   %.6f %.6f (sorted)" % (a["recall"][1], a["ndcg"][1], *b))


if __name__ == "__main__":
    main()
