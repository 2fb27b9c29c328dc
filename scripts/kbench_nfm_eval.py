#!/usr/bin/env python3
"""NFM's evaluation at the amazon-book shape (70,679 users x 24,915 items, d = 64, one hidden layer of 64, the KGAT
paper's cut-offs 20 ... 100): the fused route NFM.evaluate(fused=True), its entry kgat_nfm_eval_topk_f32 alone, and the
torch route NFM.evaluate(fused=False) in the same process; then d = 16 / hidden = 32, and 2,048 users (developer tool;
not part of the product path or of bench.py's contract).  Every shape is warmed up first; whole calls are timed with a
host clock between two synchronisations, the two routes alternating; the entry (C's layout + sweep + merge, three
launches) with HIP events.  Medians and the spread (min, max) are printed.  The sweep's rate is 2 U I d hidden FLOP
over the ENTRY's time - the two small launches included, so a lower bound - as a fraction of the fp32-MFMA peak
(157.3 TFLOP/s), next to the dot-product sweeps' 0.68 (top-K) and 0.41 - 0.50 (ranks).

  python scripts/kbench_nfm_eval.py [--rounds 5] [--torch-rounds 2]     > profiles/kbench_nfm_eval.txt

Run it under a time limit of its own (timeout -k 10 900 ...)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3   # fp32 MFMA, MI355X


def host_rounds(fns, rounds, warm=1):
    """name -> milliseconds per round; the functions alternate inside a round.  rounds: an int or name -> int."""
    names = list(fns)
    n_of = rounds if isinstance(rounds, dict) else {n: rounds for n in names}
    for _ in range(warm):
        for n in names:
            fns[n]()
    ts = {n: [] for n in names}
    for r in range(max(n_of.values())):
        for n in names:
            if r >= n_of[n]:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[n]()
            torch.cuda.synchronize()
            ts[n].append(1e3 * (time.perf_counter() - t0))
    return {n: np.array(v) for n, v in ts.items()}


def event_rounds(fn, rounds, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def show(name, t):
    print("   %-44s median %10.3f ms   min %10.3f   max %10.3f   (%d rounds)" % (name, np.median(t), t.min(), t.max(), len(t)))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-rounds", type=int, default=2)
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import fm_models, metrics, ops
    if not torch.cuda.is_available():
        raise SystemExit("kbench_nfm_eval: no HIP device - nothing is measured without one")
    dev = torch.device("cuda:0")
    n_u, n_i, n_attr = 70679, 24915, 10000
    rng = np.random.default_rng(6)
    # every item: itself and five attribute entities
    ids = np.concatenate([np.arange(n_u, n_u + n_i)[:, None], n_u + n_i + rng.integers(0, n_attr, (n_i, 5))], 1)
    feats = K.FeatureSets(np.arange(n_i + 1) * 6, ids.reshape(-1), n_u + n_i + n_attr, device=dev, item_offset=n_u)
    deg = np.minimum(rng.zipf(1.6, n_u) + 1, 3000)
    train = {u: np.unique(rng.integers(0, n_i, deg[u])) for u in range(n_u)}
    test = {u: np.unique(rng.integers(0, n_i, 1 + (u % 5))) for u in range(n_u)}
    item_range = np.arange(n_u, n_u + n_i)
    plans = {n_u: metrics.EvalPlan(train, test, item_range, dev),
             2048: metrics.EvalPlan({u: train[u] for u in range(2048)}, {u: test[u] for u in range(2048)}, item_range, dev)}
    Ks = (20, 40, 60, 80, 100)
    for d, hidden, users in ((64, 64, n_u), (16, 32, n_u), (64, 64, 2048)):
        torch.manual_seed(3)
        m = K.NFM(n_u + n_i + n_attr, feats, dim=d, layers=(hidden,)).to(dev)
        with torch.no_grad():
            m.w_lin.normal_(0, 0.1)
            m.embed.weight.mul_(4.0)
        m.eval()
        plan = plans[users]
        print("%d users x %d items, d = %d, hidden = %d, Ks = %s" % (users, n_i, d, hidden, list(Ks)))
        # the entry alone: operands made once
        with torch.no_grad():
            V, w = m.embed.weight.detach(), m.w_lin.detach()
            P, T, lin = fm_models.pool_items(V, w, feats)
            W1 = m.mlp[0].weight.detach().contiguous()
            C = torch.addmm(m.mlp[0].bias.detach(), T, W1.t())
            const = (m.w0.detach() + w[plan.user_ids.long()]).contiguous()
        lib = ops._lib.load()
        ws = ops._workspace(lib.kgat_nfm_eval_scratch_bytes(users, n_i, d, hidden, Ks[-1]), dev)
        itemT = ops._eval_items(lib, P, torch.arange(n_i, dtype=torch.int32, device=dev))
        top = torch.empty((users, Ks[-1]), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        h = m.h.detach().contiguous()

        def entry(k=Ks[-1]):
            ops.check(lib.kgat_nfm_eval_topk_f32(users, plan.user_ids.data_ptr(), n_i, d, hidden, V.data_ptr(), V.stride(0),
                                                 W1.data_ptr(), itemT.data_ptr(), C.data_ptr(), h.data_ptr(), lin.data_ptr(),
                                                 const.data_ptr(), plan.train_ptr.data_ptr(), plan.train_items.data_ptr(),
                                                 k, ws.data_ptr(), ws.numel(), top.data_ptr(), None, stream),
                      "kgat_nfm_eval_topk_f32")
        t_entry = show("kgat_nfm_eval_topk_f32 K=100 (HIP events)", event_rounds(entry, args.rounds))
        if (d, hidden, users) == (64, 64, n_u):
            # the depth moves only the candidate handling (appends, prunes, the lists): what it costs beside the products
            for k in (1, 20):
                show("kgat_nfm_eval_topk_f32 K=%d (HIP events)" % k, event_rounds(lambda k=k: entry(k), args.rounds))
        flop = 2.0 * users * n_i * d * hidden
        print("   first layer %.2f TFLOP: %.1f TFLOP/s over the entry = %.3f of the fp32-MFMA peak; scratch %.1f MB" % (
            flop / 1e12, flop / t_entry / 1e9, flop / t_entry / 1e9 / PEAK_TFLOPS, ws.numel() / 1e6))
        res = host_rounds({"fused": lambda: m.evaluate(plan, Ks, fused=True), "torch": lambda: m.evaluate(plan, Ks)},
                          {"fused": args.rounds, "torch": args.torch_rounds})
        t_f = show("NFM.evaluate(fused=True)  (whole call)", res["fused"])
        t_t = show("NFM.evaluate(fused=False) (whole call)", res["torch"])
        print("   torch route / fused route = %.1f" % (t_t / t_f))
        a, b = m.evaluate(plan, Ks, fused=True), m.evaluate(plan, Ks)
        print("   recall@20 %.6f recall@100 %.6f ndcg@100 %.6f (fused)   %.6f %.6f %.6f (torch)" % (
            a["recall"][0], a["recall"][-1], a["ndcg"][-1], b["recall"][0], b["recall"][-1], b["ndcg"][-1]))
        del m, V, P, T, C, itemT, ws, top
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
