#!/usr/bin/env python3
"""BPR-MF pretraining on the planted-structure CKG with the torch operators on the CPU: the reference trajectory of
tests/test_gpu_mf_phase.py::test_planted_structure_mf_pretraining.  The same data (planted_data_dir),
the same draws in kind (uniform training pair, uniform negative item), KGATPropagation.mf_phase on a CPU module with
torch.optim.Adam, held-out recall@20 of the raw table (metrics.calc_recall_ndcg_sorted: torch operators) before and
after every epoch.

  python scripts/mf_planted_cpu.py --epochs 6 --lr 0.01 --batch 1024 --seeds 1234 1 2
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import ckg_io, metrics  # noqa: E402
import train_kgat  # noqa: E402


def run(seed, epochs, lr, batch, dim, regs):
    torch.manual_seed(seed)
    ds = ckg_io.CKGDataset(train_kgat.planted_data_dir(seed=seed))
    model = K.KGATPropagation(ds.n_KG_entity, ds.n_KG_relation, dim, dim, 1, dim, 0.0)
    opt = torch.optim.Adam([model.entity_embed.weight], lr=lr)
    off = ds.n_users
    pairs = torch.as_tensor(ds.train_pairs[:, :2].astype(np.int64))
    seen = train_kgat.user_dict(np.vstack([ds.train_pairs, ds.valid_pairs]), off)
    held = train_kgat.user_dict(ds.test_pairs, off)

    def recall():
        return metrics.calc_recall_ndcg_sorted(model.entity_embed.weight.detach(), seen, held, ds.item_id_range, K=20)[0]

    traj, losses = [recall()], []
    for _ in range(epochs):
        n_it, bs = len(pairs) // batch + 1, min(batch, len(pairs))
        idx = torch.randint(0, len(pairs), (n_it, bs))
        neg = torch.randint(off, off + ds.n_items, (n_it, bs))
        losses.append(float(model.mf_phase(pairs[:, 0][idx], pairs[:, 1][idx], neg, opt, reg_lambda=regs).mean()))
        traj.append(recall())
    return traj, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--regs", type=float, default=None)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1234, 1, 2])
    a = ap.parse_args()
    for seed in a.seeds:
        traj, losses = run(seed, a.epochs, a.lr, a.batch, a.dim, a.regs)
        print("seed %d | test recall@20 by epoch %s (x%.2f) | mf_loss %s" % (
            seed, " ".join("%.4f" % r for r in traj), traj[-1] / max(traj[0], 1e-12), " ".join("%.4f" % x for x in losses)))


if __name__ == "__main__":
    main()
