#!/usr/bin/env python3
"""The differentiable attention on the benchmark graph (developer tool; not part of the product path or of bench.py's
contract): forward and forward + backward of ``compute_attention(differentiable=True)``, the backward operator
(kgat_att_score_bwd_f32) alone, the same gradient by the only route the package had before -
``compute_attention_surface`` under autograd -, and the CF step with the attention inside it against the default step.
Interleaved rounds in one process; HIP events around the attention calls, a host clock between two synchronisations
around a whole step.

  python scripts/kbench_att_bwd.py [--rounds 20] [--scale 1.0] [--surface-rounds 3] [--no-step]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fns, rounds, warm=3):
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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--surface-rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import ops, synth
    from dgl_kgat_amd.graph import att_bwd_statics
    dev = torch.device("cuda:0")
    n, trip, R = synth.amazon_book_ckg(scale=args.scale)
    E, D, B = len(trip), 64, 10240
    torch.manual_seed(0)
    model = K.KGATPropagation(n, R, D, D, 3, D, dropout=0.1).to(dev)
    g = synth.build_graph(n, trip, dev)
    coef = torch.randn(E, 1, device=dev)
    params = (model.entity_embed.weight, model.W_R, model.relation_embed.weight)

    def fwd_plain():
        with torch.no_grad():
            return model.compute_attention(g)

    def fwd_diff():
        return model.compute_attention(g, differentiable=True)

    def fwd_bwd():
        return torch.autograd.grad((fwd_diff() * coef).sum(), params)

    def surface_fwd_bwd():
        return torch.autograd.grad((model.compute_attention_surface(g) * coef).sum(), params)
    fwd_bwd()
    st = g._st
    groups = st.rel_groups(g.edata["type"], R, dev)
    s = att_bwd_statics(groups, st.n_nodes)
    print("N=%d E=%d R=%d d=%d | scored positions %d, (head, relation) groups %d, [V ; H] + A tables %.1f MB, form %s"
          % (n, E, R, D, s.n_scored, groups.n_groups, 3 * groups.n_groups * D * 4 / 1e6, st.last_att_form[0]))
    gamma = torch.randn(E, device=dev)
    ent, W, rel = (p.detach().contiguous() for p in params)

    def op_alone():
        return ops.att_score_bwd(st.n_nodes, s.n_scored, groups.n_groups, groups.perm, groups.src_g, groups.gid, s.gstart,
                                 groups.gptr, groups.g_node, s.node_ptr, s.node_col, s.node_row, s.node_wsrc, ent, W, rel,
                                 gamma)
    t = timeit({"attention forward, default (no_grad)": fwd_plain, "attention forward, differentiable": fwd_diff,
                "attention forward + backward": fwd_bwd, "ops.att_score_bwd alone (gather + entry)": op_alone}, args.rounds)
    for k, v in t.items():
        print("%-40s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)" % (k, np.median(v), v.min(), v.max(), len(v)))
    a, b = fwd_bwd(), surface_fwd_bwd()
    for name, x, y in zip(("entity_embed", "W_R", "relation_embed"), a, b):
        print("gradient %-15s fused vs surface route: max |diff| / max |surface| = %.3e"
              % (name, float((x - y).abs().max() / y.abs().max())))
    ts = timeit({"surface route forward + backward": surface_fwd_bwd}, args.surface_rounds, warm=1)
    v = ts["surface route forward + backward"]
    fused = float(np.median(t["attention forward + backward"]))
    print("%-40s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)  = x %.1f of the fused forward + backward"
          % ("surface route forward + backward", np.median(v), v.min(), v.max(), len(v), np.median(v) / fused))
    if args.no_step:
        return
    # the CF step of kgat.py:146-168: gnn (all layers, full graph) -> BPR loss -> backward -> Adam
    u = torch.randint(0, 70679, (B,), device=dev).int()
    pi = torch.randint(70679, 95594, (B,), device=dev).int()
    ni = torch.randint(70679, 95594, (B,), device=dev).int()
    steps = {}
    for name, diff in (("default (constant weights)", False), ("--attention_grad 1", True)):
        torch.manual_seed(0)
        m = K.KGATPropagation(n, R, D, D, 3, D, dropout=0.1).to(dev)
        opt = K.FusedAdam(m.parameters(), lr=0.01)
        gg = synth.build_graph(n, trip, dev)
        with torch.no_grad():
            gg.edata["w"] = m.compute_attention(gg)

        def step(m=m, opt=opt, gg=gg, diff=diff):
            if diff:
                gg.edata["w"] = m.compute_attention(gg, differentiable=True)
            loss = m.get_loss(m.gnn(gg), u, pi, ni)
            loss.backward()
            opt.step()
            opt.zero_grad()
        steps[name] = step
    res = {k: [] for k in steps}
    for _ in range(3):
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
        med = 1e3 * float(np.median(v))
        base = base or med
        print("CF step (fwd+bwd+Adam, 3 layers, d=64, batch %d) %-28s median %.4f ms  (min %.4f, x %.3f of the first)"
              % (B, k, med, 1e3 * min(v), med / base))


if __name__ == "__main__":
    main()
