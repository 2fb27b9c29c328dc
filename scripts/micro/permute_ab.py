"""Developer probe: the edge-id-ordered copy of the attention weights on the benchmark graph's csr_pos - the shipped
gather (kgat_gather_f32) against the planned two-pass form (kgat_permute_f32), event-timed in alternation.  Before every
launch the table is rewritten by an E-sized store on the same stream (what the softmax leaves behind in the step), so
both arms start from the step's cache state.  ``--lib SO`` times the planned form of another build of
csrc/kgat_permute.hip beside the library's (a build with -DKGAT_PERMUTE_TILE=8192: the tile A/B).

    python scripts/micro/permute_ab.py [--launches 120] [--scale 1.0] [--lib other.so] [--out FILE]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dgl_kgat_amd import _lib, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=120)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
n, trip, n_rel = synth.amazon_book_ckg(seed=1234, scale=args.scale)
g = synth.build_graph(n, trip, dev)
st = g._st
pos = st.csr_pos(dev)
E = pos.numel()
src = torch.rand(E, device=dev)
table, out, tmp = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
stream = torch.cuda.current_stream().cuda_stream
P = ctypes.c_void_p


def planned(lib):
    lib.kgat_permute_tile.restype = ctypes.c_int
    lib.kgat_permute_f32.argtypes = [ctypes.c_int64, P, P, P, P, P, P, P]
    tile = lib.kgat_permute_tile()
    slot_a, dst_a, slot_b = ops.permute_plan_arrays(pos, tile)

    def run():
        rc = lib.kgat_permute_f32(E, slot_a.data_ptr(), dst_a.data_ptr(), slot_b.data_ptr(), table.data_ptr(),
                                  out.data_ptr(), tmp.data_ptr(), stream)
        assert rc == 0, rc
    run.keep = (slot_a, dst_a, slot_b)
    return tile, run


arms = [("gather  kgat_gather_f32", lambda: ops.gather(pos, table, out=out))]
tile, run = planned(_lib.load())
arms.append(("planned kgat_permute_f32, tile %d (%d workgroups per pass, mean run %.0f)"
             % (tile, -(-E // tile), tile * tile / E), run))
if args.lib:
    tile2, run2 = planned(ctypes.CDLL(os.path.abspath(args.lib)))
    arms.append(("planned %s, tile %d (%d workgroups per pass, mean run %.0f)"
                 % (os.path.basename(args.lib), tile2, -(-E // tile2), tile2 * tile2 / E), run2))

table.copy_(src)
want = table[pos.long()]
for name, fn in arms:
    out.zero_()
    fn()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), name
times = [[] for _ in arms]
for it in range(args.launches + 10):
    for k, (name, fn) in enumerate(arms):
        table.copy_(src)   # the softmax-sized store in front of the launch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if it >= 10:
            times[k].append(a.elapsed_time(b) * 1e3)
lines = ["stand-alone A/B on csr_pos of the amazon-book-shaped CKG (scale %g): E = %d, %d alternating launches per arm, "
         "the table rewritten before every launch; device events, microseconds" % (args.scale, E, args.launches)]
for (name, _), t in zip(arms, times):
    t = np.array(t)
    lines.append("  %-86s median %6.1f   p10 %6.1f   p90 %6.1f   min %6.1f" % (name, np.median(t), np.percentile(t, 10),
                                                                           np.percentile(t, 90), t.min()))
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "a") as fh:
        fh.write(text + "\n")
