#!/usr/bin/env python3
"""RippleNet's evaluation at the amazon-book shape (70,679 users x 24,915 items, 32 triples per hop, two hops,
plus_transform, the KGAT paper's cut-offs 20 ... 100) at d = 16 (the paper's RippleNet setting) and d = 64, each at all
users and at 2,048 users: the fused route RippleNet.evaluate(fused=True), its entries kgat_eval_ripple_keys_f32 and
kgat_eval_ripple_topk_f32 alone, and the torch route RippleNet.evaluate(fused=False) in the same process (developer
tool; not part of the product path or of bench.py's contract).  Every shape is warmed up first; whole calls are timed
with a host clock between two synchronisations, the two routes alternating; the entries with HIP events.  Medians and
the spread (min, max) are printed.  The torch route is measured at 2,048 users; its figure at all users is that one
scaled by the user count and marked as extrapolated (its work is per user block, a block is about eight users at either
size).  The sweep's rate is 2 U I H (2 M d + d d) FLOP over the topk ENTRY's time - the merge launch included, so a
lower bound - as a fraction of the fp32-MFMA peak (157.3 TFLOP/s).

  python scripts/kbench_ripple_eval.py [--rounds 3] [--torch-rounds 1]     > profiles/kbench_ripple_eval.txt

Run it under a time limit of its own (timeout -k 10 900 ...)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from kbench_nfm_eval import PEAK_TFLOPS, event_rounds, host_rounds, show  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-rounds", type=int, default=1)
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import metrics, ops
    if not torch.cuda.is_available():
        raise SystemExit("kbench_ripple_eval: no HIP device - nothing is measured without one")
    dev = torch.device("cuda:0")
    n_u, n_i, n_attr, n_rel, M, H = 70679, 24915, 10000, 78, 32, 2
    n_nodes = n_u + n_i + n_attr
    rng = np.random.default_rng(6)
    mem = [rng.integers(n_u, n_nodes, (n_u, H, M)) for _ in range(2)]
    sets = K.RippleSets(mem[0], np.sort(rng.integers(0, n_rel, (n_u, H, M)), axis=2), mem[1], n_nodes, n_rel, device=dev)
    deg = np.minimum(rng.zipf(1.6, n_u) + 1, 3000)
    train = {u: np.unique(rng.integers(0, n_i, deg[u])) for u in range(n_u)}
    test = {u: np.unique(rng.integers(0, n_i, 1 + (u % 5))) for u in range(n_u)}
    item_range = np.arange(n_u, n_u + n_i)
    plans = {n_u: metrics.EvalPlan(train, test, item_range, dev),
             2048: metrics.EvalPlan({u: train[u] for u in range(2048)}, {u: test[u] for u in range(2048)}, item_range, dev)}
    Ks = (20, 40, 60, 80, 100)
    lib = ops._lib.load()
    for d in (16, 64):
        torch.manual_seed(3)
        m = K.RippleNet(n_nodes, sets, dim=d, item_update_mode="plus_transform", item_range=(n_u, n_u + n_i)).to(dev)
        with torch.no_grad():
            m.entity_emb.weight.mul_(6.0)             # logits of order one: the softmax is not flat
        m.eval()
        ent = m.entity_emb.weight.detach()
        rel = m.relation_emb.weight.detach()
        W = m.transform_matrix.weight.detach().contiguous()
        itemT = ops.ripple_eval_items(ent, n_u, n_u + n_i)
        t_torch_small = None
        for users in (2048, n_u):
            plan = plans[users]
            print("%d users x %d items, d = %d, M = %d, H = %d, plus_transform, Ks = %s" % (users, n_i, d, M, H, list(Ks)))
            t_keys = show("kgat_eval_ripple_keys_f32 (HIP events)",
                          event_rounds(lambda: ops.ripple_eval_keys(ent, rel, sets, plan.user_ids), args.rounds))
            keys = ops.ripple_eval_keys(ent, rel, sets, plan.user_ids)

            def entry(k=Ks[-1]):
                ops.ripple_eval_topk(ent, sets, plan.user_ids, keys, itemT, n_i, W, 3, True, plan.train_ptr, plan.train_items, k,
                                     want_scores=False)
            t_entry = show("kgat_eval_ripple_topk_f32 K=100 (HIP events)", event_rounds(entry, args.rounds))
            if users == n_u:
                for k in (1, 20):
                    show("kgat_eval_ripple_topk_f32 K=%d (HIP events)" % k, event_rounds(lambda k=k: entry(k), args.rounds))
            flop = 2.0 * users * n_i * H * (2 * M * d + d * d)
            print("   %.2f TFLOP: %.1f TFLOP/s over the entry = %.3f of the fp32-MFMA peak; keys %.1f MB, scratch %.1f MB" % (
                flop / 1e12, flop / t_entry / 1e9, flop / t_entry / 1e9 / PEAK_TFLOPS, keys.numel() * 4 / 1e6,
                lib.kgat_eval_ripple_scratch_bytes(users, n_i, d, M, H, Ks[-1]) / 1e6))
            del keys
            if users == 2048:
                res = host_rounds({"fused": lambda: m.evaluate(plan, Ks, fused=True), "torch": lambda: m.evaluate(plan, Ks)},
                                  {"fused": args.rounds, "torch": args.torch_rounds})
                t_f = show("RippleNet.evaluate(fused=True)  (whole call)", res["fused"])
                t_t = t_torch_small = show("RippleNet.evaluate(fused=False) (whole call)", res["torch"])
                print("   torch route / fused route = %.1f" % (t_t / t_f))
                a, b = m.evaluate(plan, Ks, fused=True), m.evaluate(plan, Ks)
                print("   recall@20 %.6f recall@100 %.6f ndcg@100 %.6f (fused)   %.6f %.6f %.6f (torch)" % (
                    a["recall"][0], a["recall"][-1], a["ndcg"][-1], b["recall"][0], b["recall"][-1], b["ndcg"][-1]))
            else:
                res = host_rounds({"fused": lambda: m.evaluate(plan, Ks, fused=True)}, args.rounds)
                t_f = show("RippleNet.evaluate(fused=True)  (whole call)", res["fused"])
                t_t = t_torch_small * users / 2048.0
                print("   RippleNet.evaluate(fused=False): %.0f ms EXTRAPOLATED by user count from the 2,048-user figure; "
                      "torch route / fused route = %.1f" % (t_t, t_t / t_f))
                a = m.evaluate(plan, Ks, fused=True)
                print("   recall@20 %.6f recall@100 %.6f ndcg@100 %.6f (fused)" % (a["recall"][0], a["recall"][-1], a["ndcg"][-1]))
            torch.cuda.empty_cache()
        del m, itemT
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
