#!/usr/bin/env python3
"""BPR-MF pretraining per iteration on the amazon-book shape (developer tool; not part of the product path or of
bench.py's contract): N = 159,251 rows (70,679 users, 24,915 items), F = 64, B = 1,024, 2,730 and 10,240.  Three forms of the same
iteration, each on its own copy of the model, bit-identical results (tests/test_gpu_mf_phase.py):

  phase      KGATPropagation.mf_phase with FusedAdam: one presort per phase + kgat_mf_adam_step_f32 (three launches)
  steps      a loop over mf_step with FusedAdam: kgat_bpr_loss_f32 + kgat_bpr_grad_f32 + kgat_adam_step_f32 (the baseline)
  autograd   get_loss(table, ...).backward(); torch.optim.Adam.step(); zero_grad()

A round runs `--iters` iterations of every form, interleaved in one process, between two synchronisations on a host
clock (the iteration is launch bound: the host's share is part of what is measured; the phase's presort is inside its
time); medians over the rounds, with min / max and the spread (max - min) / median of each form.  Batches as an
edge-uniform sampler draws them: users uniform, positives by a power law over the items, negatives uniform.

  python scripts/kbench_mf.py [--rounds 12] [--iters 50] [--out profiles/kbench_mf.txt]
  python scripts/kbench_mf.py --only phase --batch 1024 --iters 20     # one form, no warm-up: for a kernel trace
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_NODES, N_USERS, N_ITEMS, F = 159251, 70679, 24915, 64


def draw(n_it, B, dev, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, N_USERS, (n_it, B))
    pop = 1.0 / np.arange(1, N_ITEMS + 1) ** 0.8
    p = N_USERS + rng.choice(N_ITEMS, (n_it, B), p=pop / pop.sum())
    q = N_USERS + rng.integers(0, N_ITEMS, (n_it, B))
    return [torch.as_tensor(x.astype(np.int32), device=dev) for x in (u, p, q)]


def make(form, dev):
    import dgl_kgat_amd as K
    torch.manual_seed(0)
    m = K.KGATPropagation(N_NODES, 4, F, F, 1, 16, dropout=0.0, reg_lambda_gnn=1e-5).to(dev)
    opt = (torch.optim.Adam if form == "autograd" else K.FusedAdam)([m.entity_embed.weight], lr=1e-4)
    return m, opt


def runner(form, m, opt, ids):
    u, p, q = ids
    ent = m.entity_embed.weight
    if form == "phase":
        return lambda: m.mf_phase(u, p, q, opt)
    if form == "steps":
        def steps():
            for i in range(u.shape[0]):
                m.mf_step(u[i], p[i], q[i], opt)
        return steps

    def autograd():
        for i in range(u.shape[0]):
            loss = m.get_loss(ent, u[i], p[i], q[i])
            loss.backward()
            opt.step()
            opt.zero_grad()
    return autograd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 2730, 10240])
    ap.add_argument("--only", choices=("phase", "steps", "autograd"), default=None)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    forms = [args.only] if args.only else ["phase", "steps", "autograd"]
    say("N=%d F=%d iters/round=%d rounds=%d device=%s" % (N_NODES, F, args.iters, args.rounds, torch.cuda.get_device_name(0)))
    for B in args.batch:
        ids = draw(args.iters, B, dev, seed=B)
        fns = {}
        for form in forms:
            m, opt = make(form, dev)
            fns[form] = runner(form, m, opt, ids)
        if args.only:
            fns[args.only]()
            torch.cuda.synchronize()
            say("B=%d %s: %d iterations run once" % (B, args.only, args.iters))
            continue
        for _ in range(2):
            for form in forms:
                fns[form]()
        ts = {form: [] for form in forms}
        for _ in range(args.rounds):
            for form in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fns[form]()
                torch.cuda.synchronize()
                ts[form].append(1e3 * (time.perf_counter() - t0) / args.iters)
        med = {}
        for form in forms:
            v = np.array(ts[form])
            med[form] = float(np.median(v))
            say("B=%-5d %-9s median %.4f ms/iteration (min %.4f, max %.4f, spread %.1f %%)" % (
                B, form, med[form], v.min(), v.max(), 100.0 * (v.max() - v.min()) / med[form]))
        spread = float(np.max(ts["steps"]) - np.min(ts["steps"]))
        gain = med["steps"] - med["phase"]
        say("B=%-5d steps - phase = %.4f ms/iteration (%.2f x); run-to-run spread of the steps loop %.4f ms: %s" % (
            B, gain, med["steps"] / med["phase"], spread,
            "the phase is faster by more than the spread" if gain > spread else "NOT faster by more than the spread"))
        say("B=%-5d autograd / phase = %.2f" % (B, med["autograd"] / med["phase"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
