#!/usr/bin/env python3
"""RippleNet's hop operator and step on fused ripple-set attention at the amazon-book shape (developer tool; not part of
the product path or of bench.py's contract): the synthetic amazon-book-shaped CKG (70,679 users, N = 159,251, 39 KG
relations), ripple sets of M = 32 triples over H = 2 hops, d in {16, 64}, n_samples in {2,048, 20,480} (a step's 2 B
samples, positives first).  Per (d, n_samples), one hop (hop 0) on the same inputs:

  fused   ops.ripple_hop_fwd alone; autograd.ripple_hop forward + backward (towards ent and U), and its backward's parts
          one by one: ops.ripple_hop_bwd, the two csr_from_coo calls of ops.ripple_scatter, its two spmm calls
  torch   autograd.ripple_hop_torch, the restatement in torch operators (index_select / softmax; index_add_ under
          autograd): what a user could write before - the baseline
  matmul  the query table U = v R of the hop (shared by both routes; not part of the legs above)

and a whole step - RippleNet.get_loss + backward + FusedAdam.step - on both routes.  Also the host time of
RippleSets.build at that shape.

A round runs `--iters` calls of every leg, interleaved in one process, between two synchronisations on a host clock
(the host's share is part of a step); medians over the rounds with min / max and the spread (max - min) / median.

  python scripts/kbench_ripple.py [--rounds 10] [--iters 20] [--out profiles/kbench_ripple.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_USERS, N_ITEMS = 70679, 24915
N_MEMORY, N_HOP = 32, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="scale of the synthetic CKG (a rehearsal takes a small one)")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import autograd, ops, synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    n, trip, n_rel_all = synth.amazon_book_ckg(scale=args.scale)
    n_users, n_items = max(int(round(N_USERS * args.scale)), 4), max(int(round(N_ITEMS * args.scale)), 4)
    pairs = trip[trip[:, 1] == n_rel_all - 2][:, [0, 2]]
    t0 = time.perf_counter()
    sets = K.RippleSets.build(trip, pairs, n_users, n, n_hop=N_HOP, n_memory=N_MEMORY, seed=0, device=dev)
    t_build = time.perf_counter() - t0
    say("N=%d users=%d pairs=%d n_rel=%d M=%d H=%d iters/round=%d rounds=%d device=%s" % (
        n, n_users, len(pairs), sets.n_rel, N_MEMORY, N_HOP, args.iters, args.rounds, torch.cuda.get_device_name(0)))
    say("RippleSets.build on the host: %.2f s (%d users x %d hops, %d users without a triple)" % (
        t_build, n_users, N_HOP, int((~sets.valid).sum())))

    for d in (16, 64):
        torch.manual_seed(d)
        model = K.RippleNet(n, sets, dim=d, item_range=(n_users, n_users + n_items)).to(dev)
        opt = K.FusedAdam(model.parameters(), lr=1e-3)
        for n_samples in (2048, 20480):
            B = n_samples // 2
            g = torch.Generator(device="cpu").manual_seed(n_samples)
            pick = torch.randint(0, len(pairs), (B,), generator=g)
            u = torch.as_tensor(pairs[:, 0].astype(np.int32))[pick].to(dev)
            p = torch.as_tensor(pairs[:, 1].astype(np.int32))[pick].to(dev)
            q = torch.randint(n_users, n_users + n_items, (B,), generator=g).to(torch.int32).to(dev)
            users = torch.cat([u, u]).contiguous()
            ent = model.entity_emb.weight.detach().clone().requires_grad_(True)
            v = ent.detach()[torch.cat([p, q]).long()]
            U = model.queries(v).detach().contiguous().requires_grad_(True)
            g_o = torch.randn(n_samples, d, device=dev)
            say("")
            say("d=%d n_samples=%d: %d gathered rows per hop and side, U is %.1f MB, a (samples, M, d) block %.1f MB" % (
                d, n_samples, n_samples * N_MEMORY, U.numel() * 4 / 2 ** 20, n_samples * N_MEMORY * d * 4 / 2 ** 20))
            o, pw = ops.ripple_hop_fwd(ent.detach(), U.detach(), sets, users, 0)
            grad_U, gl = ops.ripple_hop_bwd(ent.detach(), U.detach(), sets, users, 0, pw, g_o)
            # the two incidence lists of ops.ripple_scatter, to time its parts
            sample = torch.arange(n_samples, dtype=torch.int32, device=dev).unsqueeze(1)
            h, r, t = (getattr(sets, name)[users.long(), 0] for name in ("mem_h", "mem_r", "mem_t"))
            lists = [(t.reshape(-1).contiguous(), sample.expand(n_samples, N_MEMORY).reshape(-1).contiguous(), pw.reshape(-1), g_o),
                     (h.reshape(-1).contiguous(), (sample * sets.n_rel + r).reshape(-1).contiguous(), gl.reshape(-1),
                      U.detach().view(n_samples * sets.n_rel, d))]
            csrs = [ops.csr_from_coo(n, src, row) for row, src, _, _ in lists]

            def leg_fb(fn):
                def run():
                    ent.grad = U.grad = None
                    fn(ent, U, sets, users, 0).backward(g_o)
                return run

            def leg_fwd(fn):
                def run():
                    with torch.no_grad():
                        fn(ent, U, sets, users, 0)
                return run

            def step(route):
                def run():
                    keep = autograd.ripple_hop
                    if route == "torch":
                        autograd.ripple_hop = autograd.ripple_hop_torch
                    try:
                        loss = model.get_loss(u, p, q)
                        loss.backward()
                        opt.step()
                        opt.zero_grad()
                    finally:
                        autograd.ripple_hop = keep
                return run

            legs = {
                "matmul U = v R": lambda: model.queries(v),
                "fused fwd (ripple_hop_fwd)": lambda: ops.ripple_hop_fwd(ent.detach(), U.detach(), sets, users, 0),
                "fused bwd kernel (ripple_hop_bwd)": lambda: ops.ripple_hop_bwd(ent.detach(), U.detach(), sets, users, 0, pw, g_o),
                "scatter: 2 x csr_from_coo": lambda: [ops.csr_from_coo(n, src, row) for row, src, _, _ in lists],
                "scatter: 2 x spmm": lambda: [ops.spmm(c[0], c[1], c[3], tab, w, eid=c[2]) for c, (_, _, w, tab) in zip(csrs, lists)],
                "fused fwd (autograd, no_grad)": leg_fwd(autograd.ripple_hop),
                "fused fwd+bwd (autograd)": leg_fb(autograd.ripple_hop),
                "torch fwd (no_grad)": leg_fwd(autograd.ripple_hop_torch),
                "torch fwd+bwd": leg_fb(autograd.ripple_hop_torch),
                "step fused (get_loss+backward+Adam)": step("fused"),
                "step torch (get_loss+backward+Adam)": step("torch"),
            }
            for fn in legs.values():
                fn()
                fn()
            ts = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        fn()
                    torch.cuda.synchronize()
                    ts[k].append(1e3 * (time.perf_counter() - t0) / args.iters)
            med = {}
            for k in legs:
                x = np.array(ts[k])
                med[k] = float(np.median(x))
                say("%-38s median %.4f ms (min %.4f, max %.4f, spread %.1f %%)" % (k, med[k], x.min(), x.max(),
                                                                                  100.0 * (x.max() - x.min()) / med[k]))
            say("hop fwd: torch / fused = %.2f; hop fwd+bwd: torch / fused = %.2f; step: torch / fused = %.2f" % (
                med["torch fwd (no_grad)"] / med["fused fwd (autograd, no_grad)"],
                med["torch fwd+bwd"] / med["fused fwd+bwd (autograd)"],
                med["step torch (get_loss+backward+Adam)"] / med["step fused (get_loss+backward+Adam)"]))
            say("backward's parts: kernel %.4f + csr_from_coo %.4f + spmm %.4f ms" % (
                med["fused bwd kernel (ripple_hop_bwd)"], med["scatter: 2 x csr_from_coo"], med["scatter: 2 x spmm"]))
            del U, ent, g_o, lists, csrs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
