#!/usr/bin/env python3
"""The FM / NFM step on fused Bi-Interaction pooling at the amazon-book shape (developer tool; not part of the product
path or of bench.py's contract): the synthetic amazon-book-shaped CKG, d = 64, B = 1,024 and 10,240 (2 B pooled sets
{user} + F(item) per step, positives first).  Per model and batch, three routes of the same loss:

  fused   fm_models.FM / NFM: autograd.bi_pool on csrc/kgat_bi_pool.hip (beyond 8,192 sets: calls of 8,192)
  torch   (a) the torch restatement under autograd: index_select / index_add_ over the batch's pairs
  graph   (b) the composition from entries that existed before: copy_reduce of [V | V^2] (2 d columns) and of w_lin (one
          column of a zero-padded 16-wide block, copy_reduce's narrowest width) over the WHOLE item-feature graph, the
          batch's rows picked from the results, backward through copy_reduce over the reversed CSR

each forward only (no_grad) and forward + backward (no optimiser step: the three share it).  Also the operator alone -
ops.bi_pool_fwd, ops.bi_pool_bwd - against the bare gather of the batch's rows (kgat_gather_probe_f32 on its ids).

A round runs `--iters` calls of every leg, interleaved in one process, between two synchronisations on a host clock
(the host's share is part of a step); medians over the rounds with min / max and the spread (max - min) / median.

  python scripts/kbench_fm.py [--rounds 10] [--iters 20] [--out profiles/kbench_fm.txt]
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

D = 64
N_USERS, N_ITEMS = 70679, 24915


class _GraphPool(torch.autograd.Function):
    """[P | Q] = copy_reduce(sum) of [V | V^2] over every item's list; backward over the reversed CSR."""

    @staticmethod
    def forward(ctx, X, feats, row_of, rev_row_of):
        from dgl_kgat_amd import ops
        ctx.feats, ctx.rev_row_of = feats, rev_row_of
        return ops.copy_reduce(feats.indptr, feats.ids, row_of, X)

    @staticmethod
    def backward(ctx, g):
        from dgl_kgat_amd import ops
        f = ctx.feats
        return ops.copy_reduce(f.rev_indptr, f.rev_items, ctx.rev_row_of, g.contiguous()), None, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    import dgl_kgat_amd as K
    from dgl_kgat_amd import fm_models, ops, synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    n, trip, _ = synth.amazon_book_ckg()
    feats = K.FeatureSets.from_kg(trip, (N_USERS, N_USERS + N_ITEMS), n, device=dev)
    lens = np.diff(feats._host["indptr"])
    say("N=%d items=%d pairs=%d (list length mean %.1f, max %d) d=%d iters/round=%d rounds=%d device=%s" % (
        n, feats.n_items, feats.n_pairs, lens.mean(), lens.max(), D, args.iters, args.rounds, torch.cuda.get_device_name(0)))
    row_of = torch.repeat_interleave(torch.arange(feats.n_items, device=dev, dtype=torch.int32), torch.as_tensor(lens, device=dev))
    rev_row_of = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32),
                                         (feats.rev_indptr[1:] - feats.rev_indptr[:-1]).long())
    torch.manual_seed(0)
    models = {"fm": K.FM(n, feats, dim=D).to(dev), "nfm": K.NFM(n, feats, dim=D).to(dev)}

    def loss_of(m, route, u, p, q):
        b = u.numel()
        users, pos = torch.cat([u, u]), torch.cat([p, q]) - N_USERS
        V, w = m.embed.weight, m.w_lin
        if route == "fused":
            bi, lin, sq = m.pool(users, torch.cat([p, q]))
        elif route == "torch":
            bi, lin, sq = fm_models.bi_pool_torch(V, w, feats, pos, users)
        else:
            PQ = _GraphPool.apply(torch.cat([V, V * V], 1), feats, row_of, rev_row_of)[pos.long()]
            W = _GraphPool.apply(torch.nn.functional.pad(w.unsqueeze(1), (0, 15)), feats, row_of, rev_row_of)[:, 0]
            vu = V[users.long()]
            S, Q = PQ[:, :D] + vu, PQ[:, D:] + vu * vu
            bi, sq = 0.5 * (S * S - Q), Q.sum(1)
            lin = W[pos.long()] + w[users.long()]
        y = m.w0 + lin + m._head(bi)
        return F.softplus(y[b:] - y[:b]).mean() + m.reg_lambda * (0.5 * (sq[:b] + sq[b:])).mean()

    for B in (1024, 10240):
        g = torch.Generator(device="cpu").manual_seed(B)
        pop = 1.0 / np.arange(1, N_ITEMS + 1) ** 0.9
        rng = np.random.default_rng(B)
        u = torch.randint(0, N_USERS, (B,), generator=g).to(dev).to(torch.int32)
        p = torch.as_tensor(N_USERS + rng.choice(N_ITEMS, B, p=pop / pop.sum()), device=dev).to(torch.int32)
        q = torch.randint(N_USERS, N_USERS + N_ITEMS, (B,), generator=g).to(dev).to(torch.int32)
        pos = (torch.cat([p, q]) - N_USERS).contiguous()
        users = torch.cat([u, u]).contiguous()
        batch_pairs = int(lens[pos.cpu().numpy()].sum()) + 2 * B
        say("")
        say("B=%d: %d pooled sets, %d feature rows gathered per step (%.3f of the %d pairs the graph route walks)%s" % (
            B, 2 * B, batch_pairs, batch_pairs / feats.n_pairs, feats.n_pairs,
            "" if ops.bi_pool_supported(D, 2 * B) else "; beyond 8,192 sets per call: the fused route makes %d calls" % -(-2 * B // 8192)))
        legs = {}
        for name, m in models.items():
            for route in ("fused", "torch", "graph"):
                def fwd(m=m, route=route):
                    with torch.no_grad():
                        loss_of(m, route, u, p, q)

                def fb(m=m, route=route):
                    for t in m.parameters():
                        t.grad = None
                    loss_of(m, route, u, p, q).backward()
                legs["%s %s fwd" % (name, route)] = fwd
                legs["%s %s fwd+bwd" % (name, route)] = fb
        # the operator alone (one call's worth of sets) against the bare gather of its rows
        m = models["fm"]
        V, w = m.embed.weight.detach(), m.w_lin.detach()
        n_op = min(2 * B, 8192)
        it, ex = pos[:n_op].contiguous(), users[:n_op].contiguous()
        ip, ids = feats._host["indptr"].astype(np.int64), feats._host["ids"]
        flat = np.concatenate([np.concatenate([[e], ids[ip[j]:ip[j + 1]]]) for j, e in zip(it.cpu().numpy(), ex.cpu().numpy())])
        col = torch.as_tensor(flat.astype(np.int32), device=dev)
        S, bi, lin, sq = ops.bi_pool_fwd(V, w, feats, it, ex)
        gb, gl, gs = torch.randn_like(bi), torch.randn_like(lin), torch.randn_like(sq)
        sink = ops.gather_probe(col, V)
        scratch = ops._workspace(ops._lib.load().kgat_bi_pool_scratch_bytes(n_op, feats.n_items, n, feats.n_pairs), dev)
        legs["op bi_pool_fwd (%d sets)" % n_op] = lambda: ops.bi_pool_fwd(V, w, feats, it, ex)
        legs["op bi_pool_bwd (%d sets)" % n_op] = lambda: ops.bi_pool_bwd(V, feats, it, ex, S, gb, gl, gs, scratch=scratch)
        legs["op gather_probe (%d rows)" % col.numel()] = lambda: ops.gather_probe(col, V, sink)
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
            v = np.array(ts[k])
            med[k] = float(np.median(v))
            say("%-34s median %.4f ms (min %.4f, max %.4f, spread %.1f %%)" % (k, med[k], v.min(), v.max(),
                                                                              100.0 * (v.max() - v.min()) / med[k]))
        for name in models:
            for what in ("fwd", "fwd+bwd"):
                f_, t_, g_ = (med["%s %s %s" % (name, r, what)] for r in ("fused", "torch", "graph"))
                say("%s %s: torch / fused = %.2f, graph / fused = %.2f" % (name, what, t_ / f_, g_ / f_))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
