"""Developer probe: bench.py's step (compute_attention + edata['w'] + gnn, amazon-book-shaped CKG, d = 64, 3 layers)
with the softmax's cut-row rescale folded into the permutation's bin pass (kgat_edge_softmax_permuted_f32: three
launches, `options.softmax_permuted`, the default) against the same step with the switch off (kgat_edge_softmax_f32 +
kgat_permute_f32: four launches, what the parent commit ran), alternating in one process: R rounds of K steps per arm,
W untimed steps in front of each.  Per round and arm: wall time per step (host clock around K steps ending in a
synchronise, bench.py's protocol) and the median of the K per-step device times.  The two arms must return the same bits.

    python scripts/micro/softmax_permuted_step_ab.py [--rounds 6] [--steps 100] [--warmup 10] [--out FILE]"""
import argparse
import gc
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import ops, synth  # noqa: E402
from dgl_kgat_amd.options import options  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
n, trip, n_rel = synth.amazon_book_ckg(seed=1234, scale=args.scale)
g = synth.build_graph(n, trip, dev)
torch.manual_seed(1234)
model = K.KGATPropagation(n, n_rel, input_node_dim=64, relation_dim=64, num_gnn_layers=3, n_hidden=64, dropout=0.0).to(dev)


def step():
    with torch.no_grad():
        a = model.compute_attention(g)
        g.edata["w"] = a
        return model.gnn(g), a


results = {}
for fused in (False, True):   # setup: structures, the plan; the two arms' bits; which entry each arm calls
    options.softmax_permuted = fused
    with ops.KernelTimer() as timer:
        out, a = step()
    torch.cuda.synchronize()
    assert ("edge_softmax_permuted" in {r[0] for r in timer.records}) == fused, "the arm did not take its entry"
    results[fused] = (out.clone(), a.clone())
assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)), "readout differs between the arms"
assert torch.equal(results[0][1].view(torch.int32), results[1][1].view(torch.int32)), "attention differs between the arms"
del results
gc.collect()
gc.freeze()

rows = []
for r in range(args.rounds):
    row = []
    for fused in (False, True):
        options.softmax_permuted = fused
        res = None
        for _ in range(args.warmup):
            res = step()
        torch.cuda.synchronize()
        evs = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = step()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.steps * 1e3
        row.append((wall, float(np.median([x.elapsed_time(y) for x, y in evs]))))
    rows.append(row)
options.softmax_permuted = True

E = g.number_of_edges()
lines = ["step A/B, amazon-book-shaped CKG (scale %g, E = %d), %d rounds x %d steps per arm (+ %d untimed), arms alternating; "
         "ms per step" % (args.scale, E, args.rounds, args.steps, args.warmup),
         "  round   unfused: wall  device-median   fused: wall  device-median"]
for r, ((uw, ud), (fw, fd)) in enumerate(rows):
    lines.append("  %5d         %7.4f        %7.4f        %7.4f        %7.4f" % (r, uw, ud, fw, fd))
uw, fw = np.array([r[0][0] for r in rows]), np.array([r[1][0] for r in rows])
ud, fd = np.array([r[0][1] for r in rows]), np.array([r[1][1] for r in rows])
for name, a_, b_ in (("wall", uw, fw), ("device-median", ud, fd)):
    lines.append("  %-13s unfused median %.4f (min %.4f, max %.4f, spread %.4f)   fused median %.4f (min %.4f, max %.4f)   "
                 "difference of medians %.4f   every fused round below every unfused round: %s"
                 % (name, np.median(a_), a_.min(), a_.max(), a_.max() - a_.min(), np.median(b_), b_.min(), b_.max(),
                    np.median(a_) - np.median(b_), bool(b_.max() < a_.min())))
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "a") as fh:
        fh.write(text + "\n")
