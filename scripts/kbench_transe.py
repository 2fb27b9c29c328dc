#!/usr/bin/env python3
"""The TransE KG iteration (CFKG's whole training) on the amazon-book shape (developer tool; not part of the product
path or of bench.py's contract): N = 159,251, R = 41, d = 64, B = 2,048.  Four forms, each on its own copy of its model:

  phase      CFKG.kg_phase with FusedAdam: one presort per phase + kgat_transe_adam_step_f32 (three launches)
  steps      a loop over CFKG.kg_step with FusedAdam: kgat_transe_loss_grad_f32 + kgat_adam_step_f32 (the same kernels)
  torch      autograd over the torch restatement (transE(fused=False)) + torch.optim.Adam: what a user could write
             without csrc/kgat_transe.hip
  transr     KGATPropagation.kg_phase at d = k = 64 with FusedAdam: the TransR iteration, which does strictly more work

The first three give bit-identical results between phase and steps (tests/test_gpu_transe.py).  A round runs `--iters`
iterations of every form, interleaved in one process, between two synchronisations on a host clock (the iteration is
launch bound: the host's share is part of what is measured; a phase's presort is inside its time); medians over the
rounds, with min / max and the spread (max - min) / median of each form.  Batches as an edge-uniform sampler draws them:
heads and positive tails by a power law over the entities, relations by a power law over 41, negatives uniform.

  python scripts/kbench_transe.py [--rounds 12] [--iters 50] [--out profiles/kbench_transe.txt]
  python scripts/kbench_transe.py --only phase --iters 20     # one form, no warm-up: for a kernel trace
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_NODES, N_REL, D, B = 159251, 41, 64, 2048
FORMS = ("phase", "steps", "torch", "transr")


def draw(n_it, dev, seed):
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, N_NODES + 1) ** 0.8
    pop /= pop.sum()
    rp = 1.0 / np.arange(1, N_REL + 1)
    h = rng.choice(N_NODES, (n_it, B), p=pop)
    t = rng.choice(N_NODES, (n_it, B), p=pop)
    r = rng.choice(N_REL, (n_it, B), p=rp / rp.sum())
    q = rng.integers(0, N_NODES, (n_it, B))
    return [torch.as_tensor(x.astype(np.int32), device=dev) for x in (h, r, t, q)]


def make(form, dev):
    import dgl_kgat_amd as K
    torch.manual_seed(0)
    if form == "transr":
        m = K.KGATPropagation(N_NODES, N_REL, D, D, 1, 16, dropout=0.0).to(dev)
        params = [m.entity_embed.weight, m.W_R, m.relation_embed.weight]
    else:
        m = K.CFKG(N_NODES, N_REL, dim=D).to(dev)
        params = list(m.parameters())
    return m, (torch.optim.Adam if form == "torch" else K.FusedAdam)(params, lr=1e-4)


def runner(form, m, opt, ids):
    if form in ("phase", "transr"):
        return lambda: m.kg_phase(*ids, opt)
    if form == "steps":
        def steps():
            for i in range(ids[0].shape[0]):
                m.kg_step(ids[0][i], ids[1][i], ids[2][i], ids[3][i], opt)
        return steps

    def restated():
        for i in range(ids[0].shape[0]):
            loss = m.transE(ids[0][i], ids[1][i], ids[2][i], ids[3][i], fused=False)
            loss.backward()
            opt.step()
            opt.zero_grad()
    return restated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=FORMS, default=None)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    forms = [args.only] if args.only else list(FORMS)
    say("N=%d R=%d d=%d B=%d iters/round=%d rounds=%d device=%s" % (N_NODES, N_REL, D, B, args.iters, args.rounds,
                                                                    torch.cuda.get_device_name(0)))
    ids = draw(args.iters, dev, seed=B)
    fns = {}
    for form in forms:
        m, opt = make(form, dev)
        fns[form] = runner(form, m, opt, ids)
    if args.only:
        fns[args.only]()
        torch.cuda.synchronize()
        say("%s: %d iterations run once" % (args.only, args.iters))
    else:
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
            say("%-7s median %.4f ms/iteration (min %.4f, max %.4f, spread %.1f %%)" % (
                form, med[form], v.min(), v.max(), 100.0 * (v.max() - v.min()) / med[form]))
        say("steps / phase = %.2f, torch / phase = %.2f, transr / phase = %.2f (the TransE iteration is %s the TransR one)" % (
            med["steps"] / med["phase"], med["torch"] / med["phase"], med["transr"] / med["phase"],
            "at or under" if med["phase"] <= med["transr"] else "ABOVE"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
