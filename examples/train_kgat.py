#!/usr/bin/env python3
"""Minimal KGAT training / evaluation harness over this package: the epoch
structure of the reference's ``kgat.py:114-196`` - KG phase (TransR), attention refresh under
no_grad, CF phase (full-graph ``gnn`` + BPR loss per batch), evaluation (recall@20 / ndcg@20
on the validation and test interactions) - with the propagation path running on the HIP
kernels.  Samplers are the reference's "uniform" modes (uniform positive edge, uniformly random
negative) drawn with torch on the device instead of DGL's C++ EdgeSampler: a phase's batches are drawn
up front (one gather per id column), the KG phase runs as ``KGATPropagation.kg_phase`` (one sort
launch for all batches + three launches per iteration), losses are summed on the device and read
once per phase (the reference reads ``loss.item()`` every step), and every phase is timed with a
host clock between two synchronisations (``--log_json`` keeps the per-epoch records).  Evaluation runs
in eval mode (the reference never leaves training mode, so its evaluation passes through dropout).

  python examples/train_kgat.py --data_dir datasets/amazon-book/data      # reference file format
  python examples/train_kgat.py --synthetic 1.0 --epochs 3               # amazon-book shape: 0.17 s per epoch
  python examples/train_kgat.py --planted --epochs 12 --lr 0.03 --batch_size 512 --batch_size_kg 512 --eval_before
                                                                          # planted structure: recall@20 must rise
  python examples/train_kgat.py --synthetic 0.01 --gpus 2                # CF phase on destination shards
  python examples/train_kgat.py --planted --epochs 3 --explain 5         # + why the top-1 item: its best attention walk
  python examples/train_kgat.py --planted --epochs 3 --explain 5 --explain_top 3   # + its three best walks, ranked
  python examples/train_kgat.py --synthetic 1.0 --grad_norm 1.0          # clip the CF gradient's global norm (kgat.py:32,162)
  python examples/train_kgat.py --planted --epochs 6 --kg_eval 2000 --kg_holdout 0.1   # + filtered MRR / MR / Hits@10 of
                                                                          # held-out KG triples under the TransR score
  python examples/train_kgat.py --planted --model cfkg --epochs 3 --lr 0.03 --batch_size_kg 512 --eval_before
                                                                          # the paper's CFKG baseline (TransE over the CKG);
                                                                          # --model cke: TransR + BPR on cf + entity rows
  python examples/train_kgat.py --planted --model fm --epochs 3 --lr 0.03 --batch_size 512 --eval_before
                                                                         # --model nfm: the same features under an MLP
  python examples/train_kgat.py --planted --model ripplenet --ripple_inverse 1 --entity_embed_dim 16 --epochs 3 --lr 0.03 \
      --batch_size 512 --eval_before                                     # the path-based baseline on ripple-set attention
  python examples/train_kgat.py --planted --pretrain_epochs 5 --pretrain_lr 0.1 --pretrain_save mf.npz --epochs 3
                                                                          # BPR-MF pretraining of the table first (the paper's
                                                                          # initialisation); --pretrain_load mf.npz reuses it

``--gpus N``: one process per GPU (started here as a child ``torch.distributed.run``),
parameters replicated, the training graph sharded by destination range.  Every rank draws the same
batches (same seed); the attention refresh and the CF forward run on the local shard with one
layer-output exchange per layer, the CF backward sums the per-rank gradients of the replicated
operands (all-reduce), so all ranks apply the one-GPU run's update.  The KG phase (dense TransR
batches, no graph) runs replicated.

Every ``--model`` runs through one ``Driver`` (samplers, phase loops, recorders, epoch skeleton, ``--log_json``); a model
is a ``Family``: its phases and what its evaluation ranks.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from collections import namedtuple

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import ckg_io, metrics, synth  # noqa: E402


def synthetic_data_dir(scale, seed=1234):
    """An amazon-book-shaped CKG written in the reference's file format (90/5/5 split)."""
    n, trip, n_rel = synth.amazon_book_ckg(seed=seed, scale=scale)
    n_users = max(int(round(70679 * scale)), 4)
    kg = trip[trip[:, 1] < n_rel - 2].copy()
    uv = trip[trip[:, 1] == n_rel - 2][:, [0, 2]].copy()
    kg[:, 0] -= n_users
    kg[:, 2] -= n_users
    uv[:, 1] -= n_users
    uv = np.unique(uv, axis=0)
    rng = np.random.default_rng(seed)
    rng.shuffle(uv)
    # every user / item must appear in the training split (the reference assumes it, dataset.py:31)
    first = np.unique(np.concatenate([np.unique(uv[:, 0], return_index=True)[1], np.unique(uv[:, 1], return_index=True)[1]]))
    rest = np.setdiff1d(np.arange(len(uv)), first)
    n_hold = len(rest) // 10
    train = uv[np.concatenate([first, rest[2 * n_hold:]])]
    val, test = uv[rest[:n_hold]], uv[rest[n_hold:2 * n_hold]]
    remap_u = {u: i for i, u in enumerate(np.unique(train[:, 0]))}
    remap_v = {v: i for i, v in enumerate(np.unique(train[:, 1]))}
    fix = lambda a: np.array([[remap_u[u], remap_v[v]] for u, v in a if u in remap_u and v in remap_v], np.int32).reshape(-1, 2)  # noqa: E731
    n_items_old = int(kg[:, [0, 2]].max()) + 1
    ent_map = np.full(n_items_old, -1, np.int64)
    for v, i in remap_v.items():
        ent_map[v] = i
    nxt = len(remap_v)
    for e in np.unique(kg[:, [0, 2]]):
        if ent_map[e] < 0:
            ent_map[e] = nxt
            nxt += 1
    kg[:, 0], kg[:, 2] = ent_map[kg[:, 0]], ent_map[kg[:, 2]]
    kg[:, 1] = np.unique(kg[:, 1], return_inverse=True)[1]
    d = os.path.join(tempfile.mkdtemp(prefix="kgat_synth_"), "data")
    ckg_io.save_ckg_files(d, len(remap_u), fix(train), fix(val), fix(test), np.unique(kg, axis=0))
    return d


def planted_data_dir(n_users=2000, n_items=1000, n_attrs=40, per_user=24, seed=1234):
    """A small CKG with PLANTED structure, written in the reference's file format: every item carries two
    attributes (KG triplets ``item -has-> attribute``), every user has one preferred attribute and draws 90 % of
    its interactions among the items that carry it (10 % uniformly).  A user's held-out items therefore share a KG
    neighbour with its training items: a model whose gradients, optimiser and attention refresh compose must push
    recall@20 well above the 20 / n_items of a random ranking within a few short epochs - the end-to-end check the
    kernels' stand-alone parity tests cannot give (tests/test_gpu_train_ops.py::test_planted_structure_recall_rises)."""
    rng = np.random.default_rng(seed)
    attr_of = np.stack([rng.integers(0, n_attrs, n_items), rng.integers(0, n_attrs, n_items)], 1)
    by_attr = [np.nonzero((attr_of == a).any(1))[0] for a in range(n_attrs)]
    taste = rng.integers(0, n_attrs, n_users)
    pairs = []
    for u in range(n_users):
        own = by_attr[taste[u]]
        k_own = min(int(round(0.9 * per_user)), len(own))
        items = np.concatenate([rng.choice(own, k_own, replace=False), rng.integers(0, n_items, per_user - k_own)])
        pairs.append(np.stack([np.full(len(items), u), items], 1))
    uv = np.unique(np.vstack(pairs), axis=0)
    rng.shuffle(uv)
    first = np.unique(np.concatenate([np.unique(uv[:, 0], return_index=True)[1], np.unique(uv[:, 1], return_index=True)[1]]))
    rest = np.setdiff1d(np.arange(len(uv)), first)
    n_hold = len(rest) // 8
    train, val, test = uv[np.concatenate([first, rest[2 * n_hold:]])], uv[rest[:n_hold]], uv[rest[n_hold:2 * n_hold]]
    items_seen = np.unique(train[:, 1])                 # item ids must be 0..n-1 over the training split
    remap = np.full(n_items, -1, np.int64)
    remap[items_seen] = np.arange(len(items_seen))
    keep = lambda a: a[remap[a[:, 1]] >= 0]             # noqa: E731
    fix = lambda a: np.stack([a[:, 0], remap[a[:, 1]]], 1)   # noqa: E731
    n_it = len(items_seen)
    kg = np.vstack([np.stack([remap[items_seen], np.zeros(n_it, np.int64), n_it + attr_of[items_seen, 0]], 1),
                    np.stack([remap[items_seen], np.ones(n_it, np.int64), n_it + attr_of[items_seen, 1]], 1)])
    ents = np.unique(kg[:, 2])                          # attribute entities numbered densely after the items
    kg[:, 2] = n_it + np.searchsorted(ents, kg[:, 2])
    d = os.path.join(tempfile.mkdtemp(prefix="kgat_planted_"), "data")
    ckg_io.save_ckg_files(d, n_users, fix(train), fix(keep(val)), fix(keep(test)), np.unique(kg, axis=0))
    return d


def user_dict(pairs, item_offset):
    order = np.argsort(pairs[:, 0], kind="stable")
    p = pairs[order]
    users, start = np.unique(p[:, 0], return_index=True)
    return {int(u): p[s:e, 1] - item_offset for u, s, e in zip(users, start, list(start[1:]) + [len(p)])}


def kg_holdout_mask(triplets, is_interaction, fraction, seed):
    """Which rows of ``triplets`` (h, r, t) stay when a ``fraction`` of the item-KG triples is held out for
    --kg_eval: a boolean keep mask.  Interaction rows (``is_interaction``) always stay.  The draw is over unordered
    entity pairs {h, t}: a triple leaves together with every triple between the same two entities - its reverse twin
    (t, ., h) in particular - so an inverse relation cannot leak it.  Only the item-KG rows enter the draw, so two
    arrays that share them (the training and the test CKG) lose the same triples."""
    triplets = np.asarray(triplets)
    keep = np.ones(len(triplets), bool)
    kg = np.flatnonzero(~np.asarray(is_interaction, bool))
    if fraction <= 0 or len(kg) == 0:
        return keep
    h, t = triplets[kg, 0].astype(np.int64), triplets[kg, 2].astype(np.int64)
    pair = np.minimum(h, t) * (int(max(h.max(), t.max())) + 1) + np.maximum(h, t)
    pairs, inverse = np.unique(pair, return_inverse=True)
    rng = np.random.default_rng(seed)
    out = np.zeros(len(pairs), bool)
    out[rng.permutation(len(pairs))[:int(round(fraction * len(pairs)))]] = True
    keep[kg[out[inverse]]] = False
    return keep


def _cutoffs(text):
    try:
        ks = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("a comma-separated list of integers, e.g. 20,40,60,80,100")
    if not 1 <= len(ks) <= 8 or ks[0] < 1 or ks[-1] > 128 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise argparse.ArgumentTypeError("1 to 8 ascending, distinct cut-offs in 1..128")
    return ks


def _rank_cutoffs(text):
    try:
        ks = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("a comma-separated list of integers, e.g. 20,200,1000")
    if not 1 <= len(ks) <= 64 or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise argparse.ArgumentTypeError("1 to 64 ascending, distinct cut-offs >= 1")
    return ks


def _widths(text):
    try:
        ws = [int(x) for x in text.split(",")]
    except ValueError:
        ws = []
    if not ws or min(ws) < 1:
        raise argparse.ArgumentTypeError("layer widths: positive integers separated by commas")
    return ws


RIPPLE_FLAGS = ("n_hop", "n_memory", "kge_weight", "item_update_mode", "using_all_hops", "ripple_inverse")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", default=None)
    ap.add_argument("--synthetic", type=float, default=0.01, help="scale of the synthetic amazon-book-shaped CKG")
    ap.add_argument("--planted", action="store_true", help="the small planted-structure CKG (planted_data_dir)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--entity_embed_dim", type=int, default=64)
    ap.add_argument("--relation_embed_dim", type=int, default=64)
    ap.add_argument("--gnn_num_layer", type=int, default=3)
    ap.add_argument("--gnn_hidden_size", type=int, default=64)
    ap.add_argument("--gnn_model", choices=("kgat", "graphsage", "rgcn"), default="kgat",
                    help="propagation layers (reference kgat.py:23): bi-interaction KGATConv, SAGEConv (mean), or "
                         "RelGraphConv (R-GCN with basis decomposition over the edge types)")
    # (absent from the namespace unless given, as --num_bases: a run without it keeps its arguments and --log_json "args")
    ap.add_argument("--model", choices=("kgat", "cfkg", "cke", "fm", "nfm", "ripplenet"), default=argparse.SUPPRESS,
                    help="kgat (default), or one of the KGAT paper's baselines: cfkg - TransE over the whole "
                         "collaborative KG, recommendation as the ranking of (user, interact, ?) (kge_models.CFKG); cke - "
                         "TransR over the item KG + BPR on `cf latent + entity embedding` (kge_models.CKE); fm / nfm - a "
                         "factorisation machine / neural FM over the features {user, item, the item's KG neighbours} on "
                         "fused Bi-Interaction pooling (fm_models.FM / NFM); ripplenet - RippleNet, the path-based "
                         "baseline: the item vector attends over the user's ripple sets of KG triples, hop by hop, on fused "
                         "ripple-set attention (ripple_models.RippleNet; the paper ran it at --entity_embed_dim 16)")
    ap.add_argument("--n_hop", type=int, default=argparse.SUPPRESS, help="--model ripplenet: hops of the ripple sets, 1..4 (default 2)")
    ap.add_argument("--n_memory", type=int, default=argparse.SUPPRESS,
                    help="--model ripplenet: triples of a ripple set, 1..128 (default 32)")
    ap.add_argument("--kge_weight", type=float, default=argparse.SUPPRESS,
                    help="--model ripplenet: weight of the KGE term -mean sigmoid(h^T R t) (default 0.01; 0 skips it)")
    ap.add_argument("--item_update_mode", choices=("replace", "plus", "replace_transform", "plus_transform"),
                    default=argparse.SUPPRESS, help="--model ripplenet: the item vector between hops (default plus_transform)")
    ap.add_argument("--using_all_hops", type=int, choices=(0, 1), default=argparse.SUPPRESS,
                    help="--model ripplenet: 1 (default) scores with the sum of every hop's response, 0 with the last hop's")
    ap.add_argument("--ripple_inverse", type=int, choices=(0, 1), default=argparse.SUPPRESS,
                    help="--model ripplenet: 1 adds the inverse (t, r + n, h) of every KG triple to the ripple sets' adjacency "
                         "(the planted CKG holds item -> attribute triples only and needs it; the KGAT release's "
                         "kg_final.txt already contains the inverses).  Default 0")
    ap.add_argument("--ripple_eval", choices=("torch", "fused"), default=argparse.SUPPRESS,
                    help="--model ripplenet: how an epoch is evaluated - torch (default): block scores in torch operators "
                         "and torch.topk; fused: the all-pairs sweep of kgat_ripple_eval.hip (d 16, 32 or 64, up to 64 "
                         "triples per hop, 1 or 2 hops, cut-offs up to 128)")
    ap.add_argument("--nfm_layers", type=_widths, default=argparse.SUPPRESS, metavar="W[,W...]",
                    help="--model nfm: widths of the hidden layers above the pooling (default 64)")
    ap.add_argument("--nfm_eval", choices=("torch", "fused"), default=argparse.SUPPRESS,
                    help="--model nfm: how an epoch is evaluated - torch (default): block scores in torch operators and "
                         "torch.topk; fused: the all-pairs sweep of kgat_nfm_eval.hip (one hidden layer of 16, 32 or 64 "
                         "units, cut-offs up to 128)")
    ap.add_argument("--num_bases", type=int, default=argparse.SUPPRESS,
                    help="bases of the rgcn layers' relation weights (default 4; at most the number of relations)")
    ap.add_argument("--res_type", choices=("Bi", "GCN", "GraphSage", "Bi2"), default="Bi",
                    help="aggregator of the kgat layers (KGATConv res_type, reference models.py:50-58): Bi-Interaction "
                         "(the reference's one-term form), GCN, GraphSage, or Bi2, the KGAT paper's two-term "
                         "Bi-Interaction (eq. 8)")
    ap.add_argument("--dropout_rate", type=float, default=0.1)
    ap.add_argument("--use_attention", type=int, choices=(0, 1), default=1,
                    help="0: the attention ablation (reference kgat.py:27) - the edge weights are the Laplacian of "
                         "--adj_type instead of the attention")
    ap.add_argument("--adj_type", choices=("si", "bi"), default="si",
                    help="Laplacian of --use_attention 0 (reference kgat.py:19): si = D^-1 A, bi = D^-1/2 A D^-1/2")
    ap.add_argument("--node_dropout", type=float, default=0.0,
                    help="node dropout of the CF phase: every step drops each edge with this probability and scales "
                         "the survivors by 1 / (1 - p)")
    ap.add_argument("--attention_grad", type=int, choices=(0, 1), default=0,
                    help="1: train the attention end to end through the CF loss - every CF step recomputes the weights "
                         "with compute_attention(differentiable=True), so W_R, the relation embeddings and the entity "
                         "table also receive the BPR gradient through them (the reference computes them once per "
                         "epoch under no_grad, kgat.py:139-145)")
    ap.add_argument("--lr", type=float, default=0.0001)
    ap.add_argument("--grad_norm", type=float, default=0.0,
                    help="norm to clip the CF step's gradient to (reference kgat.py:32; its clip_grad_norm_ call, "
                         "kgat.py:162, ships commented out): global 2-norm clipping inside the fused Adam step.  0 = off")
    ap.add_argument("--batch_size", type=int, default=10240)
    ap.add_argument("--batch_size_kg", type=int, default=2048)
    ap.add_argument("--max_iters", type=int, default=0, help="cap on iterations per phase (0 = full epoch)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--eval_before", action="store_true", help="evaluate the untrained model first (epoch 0)")
    ap.add_argument("--log_json", default=None, help="write the per-epoch records (phase wall-clock, losses, metrics) here")
    ap.add_argument("--Ks", type=_cutoffs, default=[20], metavar="K[,K...]",
                    help="evaluation cut-offs, ascending (the KGAT paper's table: 20,40,60,80,100; at most 8, each <= "
                         "128).  The default keeps recall@20 / ndcg@20; a longer list logs recall, ndcg, precision and "
                         "hit ratio at every cut-off (metrics.calc_metrics)")
    # (both absent from the namespace unless given: a run without them has the arguments - and the --log_json "args" -
    #  it had before they existed; read with getattr below)
    ap.add_argument("--rank_metrics", type=int, choices=(0, 1), default=argparse.SUPPRESS,
                    help="1: at every evaluation also rank EVERY held-out item (metrics.calc_rank_metrics: one counting "
                         "sweep, no list, so no 128) and log a rank_metrics line - recall, ndcg, precision and hit ratio "
                         "at --rank_Ks, MRR, MAP, AUC and the mean rank")
    ap.add_argument("--rank_Ks", type=_rank_cutoffs, default=argparse.SUPPRESS, metavar="K[,K...]",
                    help="cut-offs of --rank_metrics, ascending, any depth (default 20,200,1000; cut-offs beyond the "
                         "number of items are left out)")
    ap.add_argument("--grad_digest", action="store_true",
                    help="print |grad| sums of the first CF step (to compare an N-GPU run with the one-GPU run)")
    ap.add_argument("--explain", type=int, default=0, metavar="N",
                    help="after the last evaluation: for the first N test users, the top-1 recommended item and the "
                         "highest-attention walk from it to the user (KGATPropagation.explain; the KGAT paper's case study)")
    ap.add_argument("--explain_top", type=int, default=1, metavar="K",
                    help="with --explain: also the K (1..4) highest-attention walks of each pair over all lengths, "
                         "ranked (explain.attention_paths(top=K)); 1 prints the best walk only")
    ap.add_argument("--kg_eval", type=int, default=0, metavar="N",
                    help="after each evaluation: filtered link-prediction metrics (kg_mrr, kg_mr, kg_hits@10; both "
                         "sides, KGATPropagation.kg_metrics) of N triples fixed by --seed - the triples --kg_holdout "
                         "removed, or without it training triples (a fit measure, not a generalisation one).  0 = off")
    ap.add_argument("--kg_holdout", type=float, default=0.0, metavar="F",
                    help="hold a fraction F of the item-KG triples (never an interaction; a triple leaves with its "
                         "reverse twin) out of the KG phase and of the propagation graphs, for --kg_eval to rank")
    ap.add_argument("--pretrain_epochs", type=int, default=0, metavar="N",
                    help="BPR-MF pretraining of the embedding table before the first KGAT epoch (the KGAT paper "
                         "initialises every run from MF embeddings): N epochs of KGATPropagation.mf_phase with an Adam of "
                         "its own.  0 = off")
    ap.add_argument("--pretrain_batch_size", type=int, default=1024, help="MF batch (the authors' 1,024; the fused "
                    "iteration takes up to 21,845, larger batches run launch by launch)")
    ap.add_argument("--pretrain_lr", type=float, default=None, help="MF learning rate (default: --lr)")
    ap.add_argument("--pretrain_regs", type=float, default=None,
                    help="MF regulariser (default: the CF phase's, the model's reg_lambda_gnn)")
    ap.add_argument("--pretrain_save", default=None, metavar="PATH",
                    help="write the user / item rows after pretraining as an mf.npz (ckg_io.save_pretrain: the layout of "
                         "the KGAT release's pretrain/<dataset>/mf.npz)")
    ap.add_argument("--pretrain_load", default=None, metavar="PATH",
                    help="initialise the user / item rows from an mf.npz (before --pretrain_epochs, if both are given)")
    args = ap.parse_args(argv)
    kind = getattr(args, "model", "kgat")
    if kind != "kgat":
        # a KG-embedding baseline has no propagation layers, no attention and no edge weights
        for flag, given in (("--gnn_model", args.gnn_model != "kgat"), ("--res_type", args.res_type != "Bi"),
                            ("--node_dropout", args.node_dropout != 0), ("--attention_grad", bool(args.attention_grad)),
                            ("--explain", args.explain != 0), ("--use_attention 0", not args.use_attention),
                            ("--num_bases", hasattr(args, "num_bases")), ("--grad_digest", args.grad_digest)):
            if given:
                ap.error("%s belongs to the propagation layers; --model %s has none" % (flag, kind))
        if args.gpus > 1:
            ap.error("--model %s runs on one GPU" % kind)
        if args.pretrain_epochs or args.pretrain_save:
            ap.error("--model %s takes --pretrain_load only: --pretrain_epochs / --pretrain_save train and write the "
                     "table of --model kgat" % kind)
    if kind in ("fm", "nfm"):
        # no KG phase: nothing to rank triples with, nothing to hold out
        if args.kg_eval or args.kg_holdout > 0:
            ap.error("--kg_eval / --kg_holdout rank triples; --model %s has no KG phase" % kind)
        if kind == "nfm" and getattr(args, "rank_metrics", 0):
            ap.error("--rank_metrics sweeps a dot-product table; --model nfm scores through an MLP")
    if kind == "ripplenet":
        if args.kg_eval or args.kg_holdout > 0:
            ap.error("--kg_eval / --kg_holdout rank triples; --model ripplenet has no KG phase")
        if getattr(args, "rank_metrics", 0):
            ap.error("--rank_metrics sweeps a dot-product table; --model ripplenet scores through its ripple sets")
        if args.pretrain_load:
            ap.error("--pretrain_load fills user rows; --model ripplenet has none")
        if not 1 <= getattr(args, "n_hop", 2) <= 4 or not 1 <= getattr(args, "n_memory", 32) <= 128:
            ap.error("--n_hop takes 1..4 hops, --n_memory 1..128 triples")
    for flag in RIPPLE_FLAGS:
        if hasattr(args, flag) and kind != "ripplenet":
            ap.error("--%s belongs to --model ripplenet" % flag)
    if hasattr(args, "ripple_eval") and kind != "ripplenet":
        ap.error("--ripple_eval chooses the evaluation route of --model ripplenet")
    if hasattr(args, "nfm_layers") and kind != "nfm":
        ap.error("--nfm_layers sets the hidden layers of --model nfm")
    if hasattr(args, "nfm_eval") and kind != "nfm":
        ap.error("--nfm_eval chooses the evaluation route of --model nfm")
    if args.pretrain_epochs < 0 or args.pretrain_batch_size < 1:
        ap.error("--pretrain_epochs takes a number of epochs >= 0, --pretrain_batch_size a batch >= 1")
    if (args.pretrain_epochs or args.pretrain_load or args.pretrain_save) and args.gpus > 1:
        ap.error("pretraining (--pretrain_epochs / --pretrain_load / --pretrain_save) runs on one GPU")
    if args.kg_eval < 0:
        ap.error("--kg_eval takes a number of triples >= 0")
    if not 0.0 <= args.kg_holdout < 1.0:
        ap.error("--kg_holdout must be in [0, 1)")
    if args.kg_holdout > 0 and not args.kg_eval:
        ap.error("--kg_holdout holds triples out for --kg_eval N: give a number of triples")
    if args.kg_eval and args.gpus > 1:
        ap.error("--kg_eval runs on one GPU")
    # (before --gpus starts its ranks: a refused combination fails once, here)
    if args.explain < 0:
        ap.error("--explain takes a number of users >= 0")
    if not 1 <= args.explain_top <= 4:
        ap.error("--explain_top takes 1, 2, 3 or 4")
    if args.explain_top > 1 and not args.explain:
        ap.error("--explain_top ranks the walks of --explain N: give a number of users")
    if args.explain and args.gpus > 1:
        ap.error("--explain runs on one GPU: a walk crosses shards")
    if args.explain and args.gnn_model != "kgat":
        ap.error("--explain follows the edge weights; --gnn_model %s aggregates without them" % args.gnn_model)
    if args.res_type != "Bi" and args.gnn_model != "kgat":
        ap.error("--res_type %s selects the aggregator of --gnn_model kgat; %s takes none" % (args.res_type, args.gnn_model))
    if getattr(args, "num_bases", 4) < 1:
        ap.error("--num_bases takes a number of bases >= 1")
    if args.gnn_model == "rgcn" and args.gpus > 1:
        ap.error("--gnn_model rgcn runs on one GPU: sharded relational convolution is out of scope")
    if args.res_type != "Bi" and args.gpus > 1:
        ap.error("--res_type %s runs on one GPU: sharded models run the Bi aggregator only" % args.res_type)
    if not (0.0 <= args.grad_norm < float("inf")):
        ap.error("--grad_norm takes a finite norm > 0, or 0 for no clipping")
    if not 0.0 <= args.node_dropout < 1.0:
        ap.error("--node_dropout must be in [0, 1)")
    if args.node_dropout > 0 and args.gnn_model != "kgat":
        ap.error("--node_dropout scales the edge weights; --gnn_model %s aggregates without them" % args.gnn_model)
    if args.node_dropout > 0 and args.gpus > 1:
        ap.error("--node_dropout runs on one GPU")
    if not args.use_attention and args.adj_type == "bi" and args.gpus > 1:
        ap.error("--adj_type bi runs on one GPU: a shard holds only part of a source's out-edges")
    if args.attention_grad:
        if not args.use_attention:
            ap.error("--attention_grad 1 needs the attention: --use_attention 0 has no parameter to differentiate towards")
        if args.node_dropout > 0:
            ap.error("--attention_grad 1 with --node_dropout: node dropout treats the edge weights as constants")
        if args.gpus > 1:
            ap.error("--attention_grad 1 runs on one GPU: a shard holds only part of a tail's out-edges")
        if args.gnn_model != "kgat":
            ap.error("--attention_grad 1 needs --gnn_model kgat: %s aggregates without the attention" % args.gnn_model)
    return args


# ---- the epoch driver: what every --model shares.  A model supplies a `Family`; the driver draws the batches, runs and
# times the phases, evaluates, prints and keeps the records.  The torch.randint calls of an epoch are the run's only
# random draws on the device, so their order and arguments ARE its reproducibility: the KG phase draws before the CF
# phase, a phase draws its row indices before its negatives, and the negatives are drawn as int32.
class Splits(namedtuple("Splits", "train_dict valid_dict test_dict train_valid_dict plans")):
    def of(self, name):
        """(seen, held, plan) of the split "valid" or "test"."""
        seen, held = (self.train_dict, self.valid_dict) if name == "valid" else (self.train_valid_dict, self.test_dict)
        return seen, held, self.plans[name]


def eval_splits(ds, dev):
    """The user -> items dicts of the data's three files and the evaluation's static side (users, item lists as CSR
    arrays; once per split, not once per call): validation ranks the items a user has not trained on, test the items it
    has neither trained nor validated on."""
    off = ds.n_users
    train_dict = user_dict(ds.train_pairs, off)
    valid_dict, test_dict = user_dict(ds.valid_pairs, off), user_dict(ds.test_pairs, off)
    train_valid_dict = user_dict(np.vstack([ds.train_pairs, ds.valid_pairs]), off)
    plans = {name: metrics.EvalPlan(seen, held, ds.item_id_range, dev)
             for name, seen, held in (("valid", train_dict, valid_dict), ("test", train_valid_dict, test_dict))}
    return Splits(train_dict, valid_dict, test_dict, train_valid_dict, plans)


def cap(n, max_iters):
    return n if max_iters <= 0 else min(n, max_iters)


def clock(dev):
    """The host clock once `dev` has run everything queued on it (a CPU queues nothing)."""
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter()


def id_columns(rows, dev):
    """A sampled table column by column (int32 ids go to the kernels as they are): a phase's batches are rows of ONE
    gather per column, so a step's host work is the two library calls, not five indexing launches."""
    return torch.as_tensor(np.ascontiguousarray(np.asarray(rows).T.astype(np.int32)), device=dev)


def draw_pairs(pair_cols, batch, item_range, max_iters):
    """A phase's (user, positive, negative) batches, drawn up front: ``(n_it, u, p, n)``, each (n_it, batch) - uniform
    training pairs, then uniformly random negative items."""
    n_pairs, dev = pair_cols.shape[1], pair_cols.device
    n_it, bs = cap(n_pairs // batch + 1, max_iters), min(batch, n_pairs)
    idx = torch.randint(0, n_pairs, (n_it, bs), device=dev)
    neg = torch.randint(item_range[0], item_range[1], (n_it, bs), device=dev, dtype=torch.int32)
    return n_it, pair_cols[0][idx], pair_cols[1][idx], neg


def draw_triples(trip_cols, batch, n_entities, max_iters):
    """A KG phase's batches, drawn up front: ``(n_it, h, r, t, neg)`` - uniform training triples, then uniformly random
    negative tails among all entities."""
    n_trip, dev = trip_cols.shape[1], trip_cols.device
    n_it, bs = cap(n_trip // batch + 1, max_iters), min(batch, n_trip)
    idx = torch.randint(0, n_trip, (n_it, bs), device=dev)
    neg = torch.randint(0, n_entities, (n_it, bs), device=dev, dtype=torch.int32)
    return n_it, trip_cols[0][idx], trip_cols[1][idx], trip_cols[2][idx], neg


# What a model gives the driver.  `phases`: the epoch's training phases in order, each a callable (epoch, rec) - built from
# Driver.kg_phase / Driver.cf_phase, or the model's own; `eval_inputs()`: what ranks the validation and then the test
# split - an embedding table whose dot products are the scores, or the metric dict of the model's own `evaluate`;
# `n_train_triplets`: the KG phase's table size for the --log_json header (None: no KG phase).
Family = namedtuple("Family", "model phases eval_inputs n_train_triplets")


class Driver:
    """The run's shared state - arguments, data, device, evaluation splits, the training pairs' columns - and the pieces
    every model's epoch is made of.  `kg_pool` (n, 3): the triples --kg_eval ranks after every evaluation, filtered by
    `kg_true`, every triple that counts as true.  Only rank 0 prints and writes."""

    def __init__(self, args, ds, dev, rank=0, kg_pool=None, kg_true=None):
        self.args, self.ds, self.dev, self.rank = args, ds, dev, rank
        self.say = print if rank == 0 else (lambda *a, **k: None)
        self.splits = eval_splits(ds, dev)
        self.pair_cols = id_columns(ds.train_pairs[:, :2], dev)
        self.items = (ds.n_users, ds.n_users + ds.n_items)
        self.kg_pool = self.kg_known = None
        if kg_pool is not None:
            self.kg_known = K.KnownTriples(kg_true[:, 0], kg_true[:, 1], kg_true[:, 2], ds.n_KG_entity, ds.n_KG_relation,
                                           device=dev)
            self.kg_pool = [torch.as_tensor(np.ascontiguousarray(kg_pool[:, c]), device=dev) for c in range(3)]
        self._lead = ""

    def head(self):
        """The left margin of a phase's line: the epoch number on the epoch's first line, blank after it."""
        lead, self._lead = self._lead, "           |"
        return lead

    def kg_phase(self, rec, model, opt, trip_cols):
        """The KG phase (kgat.py:116-136) as ``model.kg_phase``: every iteration = loss -> backward -> step -> zero_grad
        of kgat.py:127-131 - one launch sorts all batches, then one library call (three launches) per iteration.  The
        reference reads loss.item() after every step (a host round trip per iteration, kgat.py:132); here the losses stay
        on the device and their sum is read once per phase."""
        args, dev = self.args, self.dev
        t0 = clock(dev)
        n_it, h_all, r_all, t_all, neg_all = draw_triples(trip_cols, args.batch_size_kg, self.ds.n_KG_entity, args.max_iters)
        total = model.kg_phase(h_all, r_all, t_all, neg_all, opt).sum()
        rec["kg_s"], rec["kg_iters"] = clock(dev) - t0, n_it
        rec["kg_loss"] = float(total) / n_it
        self.say("%s KGE %.4fs (%d it, %.4f ms/it) loss %.4f" % (self.head(), rec["kg_s"], n_it, 1e3 * rec["kg_s"] / n_it,
                                                                rec["kg_loss"]))

    def cf_phase(self, epoch, rec, opt, loss_of, label="CF", kgat=None):
        """The CF phase (kgat.py:146-168): per batch ``loss_of(u, p, n)`` -> backward -> step -> zero_grad, --grad_norm
        clipping the gradient's global norm inside the step (clip_grad_norm_ of kgat.py:162); the running loss stays on
        the device and is read once.  `kgat`: a KGATPropagation, for which the phase also keeps every step's gradient norm
        (one readback at the end of the phase), records how far W_R moved, and prints --grad_digest."""
        args, dev, say = self.args, self.dev, self.say
        t0 = clock(dev)
        n_it, u_all, p_all, n_all = draw_pairs(self.pair_cols, args.batch_size, self.items, args.max_iters)
        total = torch.zeros((), dtype=torch.float32, device=dev)
        w_r_before = kgat.W_R.detach().clone() if kgat is not None else None
        norms = torch.zeros(n_it, dtype=torch.float32, device=dev) if kgat is not None and args.grad_norm > 0 else None
        for i in range(n_it):
            loss = loss_of(u_all[i], p_all[i], n_all[i])
            loss.backward()
            if kgat is not None and args.grad_digest and epoch == 1 and i == 0:
                say("           | grad digest: loss %.9g  " % loss.item() + "  ".join(
                    "%s %.9g" % (k, p.grad.double().abs().sum().item()) for k, p in kgat.named_parameters()
                    if p.grad is not None))
            if norms is not None:
                opt.step(max_grad_norm=args.grad_norm, norm_out=norms[i])
            elif args.grad_norm > 0:
                opt.step(max_grad_norm=args.grad_norm)
            else:
                opt.step()
            opt.zero_grad()
            total += loss.detach()
        rec["cf_s"], rec["cf_iters"] = clock(dev) - t0, n_it
        rec["cf_loss"] = float(total) / n_it
        if kgat is not None:
            rec["cf_W_R_change"] = float((kgat.W_R.detach() - w_r_before).abs().max())   # 0 unless --attention_grad 1
        if norms is not None:
            seen = norms.cpu().numpy()
            if not np.isfinite(seen).all():
                raise RuntimeError("epoch %d: the gradient norm of CF step %d is %r" % (
                    epoch, int(np.flatnonzero(~np.isfinite(seen))[0]), float(seen[~np.isfinite(seen)][0])))
            rec["cf_grad_norm_max"], rec["cf_grad_norm_mean"] = float(seen.max()), float(seen.mean())
            # (the test the kernel applies: coef = min(c / (norm + 1e-6), 1) in fp32 is below 1)
            c32 = np.float32(args.grad_norm)
            rec["cf_clipped_steps"] = int((c32 / (seen + np.float32(1e-6)) < np.float32(1)).sum())
            say("           | grad norm max %.4g mean %.4g, %d of %d steps clipped at %g" % (
                rec["cf_grad_norm_max"], rec["cf_grad_norm_mean"], rec["cf_clipped_steps"], n_it, args.grad_norm))
        say("%s %s %.4fs (%d it, %.4f ms/it) loss %.4f" % (self.head(), label, rec["cf_s"], n_it, 1e3 * rec["cf_s"] / n_it,
                                                          rec["cf_loss"]))

    def record_split(self, rec, name, given):
        """Record and print the metrics of the split `name`.  `given`: an embedding table - ranked here, with
        --rank_metrics also by the exact rank of every held-out item - or the dict of means ``metrics.calc_metrics``
        returns, already computed by a model that scores otherwise."""
        args, say = self.args, self.say
        seen, held, plan = self.splits.of(name)
        items = self.ds.item_id_range
        if isinstance(given, dict):
            m = given
        else:
            if getattr(args, "rank_metrics", 0):
                rank_Ks = getattr(args, "rank_Ks", [20, 200, 1000])
                rank_Ks = [k for k in rank_Ks if k <= plan.n_items] or [plan.n_items]
                m = metrics.calc_rank_metrics(given, seen, held, items, Ks=rank_Ks, plan=plan)
                for metric in metrics.RANK_SCALAR_NAMES:
                    rec["%s_%s" % (name, metric)] = float(m[metric])
                for j, k in enumerate(rank_Ks):
                    for metric in metrics.METRIC_NAMES:
                        rec["%s_rank_%s@%d" % (name, metric, k)] = float(m[metric][j])
                say("           | rank_metrics %s auc %.5f mrr %.5f map %.5f mean_rank %.1f | %s" % (
                    name, m["auc"], m["mrr"], m["map"], m["mean_rank"],
                    " ".join("recall@%d %.5f ndcg@%d %.5f" % (k, m["recall"][j], k, m["ndcg"][j]) for j, k in enumerate(rank_Ks))))
            if args.Ks == [20]:
                recall, ndcg = metrics.calc_recall_ndcg(given, seen, held, items, K=20, plan=plan)
                m = {"recall": [recall], "ndcg": [ndcg]}
            else:
                m = metrics.calc_metrics(given, seen, held, items, Ks=args.Ks, plan=plan)
        if args.Ks == [20]:
            rec[name + "_recall"], rec[name + "_ndcg"] = float(m["recall"][0]), float(m["ndcg"][0])
            say("           | %s recall@20 %.5f ndcg@20 %.5f" % (name, rec[name + "_recall"], rec[name + "_ndcg"]))
            return
        for j, k in enumerate(args.Ks):
            for metric in metrics.METRIC_NAMES:
                rec["%s_%s@%d" % (name, metric, k)] = float(m[metric][j])
            say("           | %s recall@%d %.5f ndcg@%d %.5f precision@%d %.5f hit_ratio@%d %.5f" % (
                name, k, m["recall"][j], k, m["ndcg"][j], k, m["precision"][j], k, m["hit_ratio"][j]))

    def record_kg(self, rec, model):
        """--kg_eval: record and print the filtered link-prediction metrics of the fixed triples, both sides."""
        dev = self.dev
        t0 = clock(dev)
        m = model.kg_metrics(*self.kg_pool, known=self.kg_known, side="both", hits=(1, 3, 10))
        rec["kg_eval_s"] = clock(dev) - t0
        rec["kg_mrr"], rec["kg_mr"], rec["kg_hits@10"] = m["mrr"], m["mr"], m["hits@10"]
        self.say("           | KG link prediction, %d %s triples, both sides, filtered: kg_mrr %.5f kg_mr %.1f kg_hits@10 %.5f "
                 "| %.4fs" % (self.kg_pool[0].numel(), "held-out" if self.args.kg_holdout > 0 else "TRAINING (a fit measure)",
                              m["mrr"], m["mr"], m["hits@10"], rec["kg_eval_s"]))

    def evaluate(self, fam, rec):
        """Evaluation (kgat.py:53-62, 171-196) of the validation and the test split, then --kg_eval."""
        t0 = clock(self.dev)
        with torch.no_grad():
            for name, given in zip(("valid", "test"), fam.eval_inputs()):
                self.record_split(rec, name, given)
        rec["eval_s"] = clock(self.dev) - t0
        self.say("           | eval %.4fs" % rec["eval_s"])
        if self.kg_pool is not None:
            self.record_kg(rec, fam.model)

    def run(self, fam, history=None):
        """The epochs: --eval_before, then per epoch the model's phases in training mode and the evaluation in eval mode.
        Returns the records, appended to `history` (a record of epoch 0 already there takes --eval_before's metrics)."""
        args, dev = self.args, self.dev
        history = [] if history is None else history
        if args.eval_before:
            fam.model.eval()
            if not history:
                history.append({"epoch": 0})
            self.say("Epoch 0000 | (untrained)")
            self.evaluate(fam, history[-1])
        for epoch in range(1, args.epochs + 1):
            rec = {"epoch": epoch}
            t_epoch = clock(dev)
            self._lead = "Epoch %04d |" % epoch
            fam.model.train()
            for phase in fam.phases:
                phase(epoch, rec)
            fam.model.eval()
            self.evaluate(fam, rec)
            rec["epoch_s"] = clock(dev) - t_epoch
            self.say("           | epoch %.4fs" % rec["epoch_s"])
            history.append(rec)
        return history

    def write_log(self, fam, history):
        """--log_json: the arguments, the data's sizes and the per-epoch records."""
        args, ds = self.args, self.ds
        if not args.log_json or self.rank != 0:
            return
        log = {"args": vars(args), "n_users": ds.n_users, "n_items": ds.n_items, "n_entities": ds.n_KG_entity,
               "n_relations": ds.n_KG_relation}
        if fam.n_train_triplets is not None:
            log["n_train_triplets"] = int(fam.n_train_triplets)
        log.update(n_train_pairs=int(self.pair_cols.shape[1]), epochs=history)
        with open(args.log_json, "w") as f:
            json.dump(log, f, indent=1)


def load_mf(drv, model):
    """--pretrain_load: the user / item rows of the table the model ranks with, from an mf.npz."""
    if drv.args.pretrain_load:
        model.load_pretrained(*ckg_io.load_pretrain(drv.args.pretrain_load), drv.ds.n_users)
        drv.say("Pretrain   | user / item rows from %s" % drv.args.pretrain_load)


def main(argv=None):
    args = parse_args(argv)
    # the attention refresh hands back its edge-id-ordered copy unwritten (nothing here reads it)
    lazy_before = K.enable_lazy_edge_weights()
    try:
        return _run(args, argv)
    finally:
        # leave the process-wide lazy setting as this call found it: --attention_grad 1 turns it off inside, and a
        # --model without propagation layers computes no attention, so the setting is not its to keep switched on
        if args.attention_grad or getattr(args, "model", "kgat") != "kgat":
            K.enable_lazy_edge_weights(lazy_before)


def _run(args, argv):
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        argv = list(sys.argv[1:] if argv is None else argv)
        if args.data_dir is None:   # every rank must read the same files
            args.data_dir = planted_data_dir(seed=args.seed) if args.planted else synthetic_data_dir(args.synthetic, args.seed)
            argv += ["--data_dir", args.data_dir]
        sys.exit(subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
                                 str(args.gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
                                 os.path.abspath(__file__)] + argv).returncode)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", int(os.environ.get("KGAT_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    torch.cuda.set_device(dev)
    if world > 1:
        backend = os.environ.get("KGAT_DIST_BACKEND", "nccl")
        dist.init_process_group(backend, rank=rank, world_size=world, **({"device_id": dev} if backend == "nccl" else {}))
    say = print if rank == 0 else (lambda *a, **k: None)
    if args.data_dir is None:
        args.data_dir = planted_data_dir(seed=args.seed) if args.planted else synthetic_data_dir(args.synthetic, args.seed)
    ds = ckg_io.CKGDataset(args.data_dir)
    say("users %d items %d | CKG: %d entities, %d relations, %d train triplets" % (
        ds.n_users, ds.n_items, ds.n_KG_entity, ds.n_KG_relation, len(ds.train_KG_triplet)))
    kg_pool = full = None
    if args.kg_eval:
        # every triple that counts as true, before anything is held out; n_KG_entity / n_KG_relation stay the full data's
        full = np.unique(np.vstack([ds.train_KG_triplet, ds.test_KG_triplet]), axis=0)
        if args.kg_holdout > 0:
            held = []
            for name in ("train_KG_triplet", "test_KG_triplet"):
                trip = getattr(ds, name)
                keep = kg_holdout_mask(trip, (trip[:, 0] < ds.n_users) | (trip[:, 2] < ds.n_users), args.kg_holdout,
                                       args.seed)
                held.append(trip[~keep])
                setattr(ds, name, trip[keep])
            kg_pool = held[0]
            say("kg_holdout %.3f: %d item-KG triples held out of the KG phase and the graphs" % (args.kg_holdout, len(kg_pool)))
        else:
            kg_pool = ds.train_KG_triplet
        if len(kg_pool) == 0:
            raise SystemExit("--kg_eval: no triple to rank")
        pick = np.random.default_rng(args.seed).permutation(len(kg_pool))[:args.kg_eval]
        kg_pool = kg_pool[pick].astype(np.int64)
    drv = Driver(args, ds, dev, rank, kg_pool, full)
    kind = getattr(args, "model", "kgat")
    if kind == "kgat":
        return _run_kgat(drv, world)
    fam = {"cfkg": _kge_family, "cke": _kge_family, "fm": _fm_family, "nfm": _fm_family, "ripplenet": _ripple_family}[kind](drv)
    history = drv.run(fam)
    drv.write_log(fam, history)
    return history


def _run_kgat(drv, world):
    """--model kgat, on `world` GPUs: an epoch is the KG phase (TransR), the attention refresh under no_grad, the CF phase
    (full-graph ``gnn`` + BPR loss per batch) and the evaluation on the propagated embeddings of the training / the test
    graph.  Only this model starts ranks, shards its graphs, pretrains its table and explains its recommendations."""
    args, ds, dev, say, splits = drv.args, drv.ds, drv.dev, drv.say, drv.splits
    rank = drv.rank
    model = K.KGATPropagation(ds.n_KG_entity, ds.n_KG_relation, args.entity_embed_dim, args.relation_embed_dim,
                              args.gnn_num_layer, args.gnn_hidden_size, args.dropout_rate,
                              gnn_model=args.gnn_model, res_type=args.res_type, use_attention=bool(args.use_attention),
                              adj_type=args.adj_type, node_dropout=args.node_dropout, num_bases=getattr(args, "num_bases", 4)).to(dev)

    def replicas_agree(tag):
        """Every rank holds a replica of the parameters and runs the same optimiser on the same gradients
        (only the shard layers' partial gradients are summed across ranks): a nondeterministic kernel or a
        diverging per-rank RNG would make the replicas drift silently.  Compare a checksum of all
        parameters across ranks (MAX - MIN of the per-rank sums) and stop when they differ."""
        if world == 1:
            return
        chk = torch.stack([p.detach().double().sum() for p in model.parameters()]).sum().reshape(1)
        hi, lo = chk.clone(), chk.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        if float(hi - lo) > 1e-9 * max(abs(float(hi)), 1.0):
            raise RuntimeError("%s: parameter replicas differ across ranks (checksum spread %.3e)" % (tag, float(hi - lo)))
    if world > 1:
        for p in model.parameters():   # one source of truth for the initial parameters, whatever the ranks' RNG drew
            dist.broadcast(p.data, src=0)
        replicas_agree("after the initial broadcast")
    # one Adam over all parameters (kgat.py:85): the same update, bit for bit, as one launch per step (optim.FusedAdam)
    opt = K.FusedAdam(model.parameters(), lr=args.lr)
    train_g, test_g = ds.train_graph(dev), ds.test_graph(dev)
    if world > 1:
        from dgl_kgat_amd import partition
        train_g, test_g = partition.shard_graph(train_g, rank, world)[0], partition.shard_graph(test_g, rank, world)[0]
    trip_cols = id_columns(ds.train_KG_triplet, dev)

    history = []
    if args.pretrain_epochs or args.pretrain_load or args.pretrain_save:
        # ---- BPR-MF pretraining of the embedding table (the KGAT paper's initialisation; the authors ship its result as
        # pretrain/<dataset>/mf.npz): get_loss on the raw table -> backward -> Adam, batches drawn as the CF phase's
        def evaluate_table(rec):
            emb = model.entity_embed.weight.detach()
            for name in ("valid", "test"):
                seen, held, plan = splits.of(name)
                rec[name + "_recall"], rec[name + "_ndcg"] = metrics.calc_recall_ndcg(
                    emb, seen, held, ds.item_id_range, K=20, plan=plan)
            return "test recall@20 %.5f ndcg@20 %.5f | valid recall@20 %.5f" % (
                rec["test_recall"], rec["test_ndcg"], rec["valid_recall"])

        pre = {"loaded": args.pretrain_load, "saved": args.pretrain_save, "epochs": []}
        load_mf(drv, model)
        pre["before"] = {}
        say("Pretrain 0000 | raw table: %s" % evaluate_table(pre["before"]))
        if args.pretrain_epochs:
            # an Adam of its own: the KGAT optimiser starts with clean moments
            mf_opt = K.FusedAdam([model.entity_embed.weight], lr=args.lr if args.pretrain_lr is None else args.pretrain_lr)
            model.train()
        for ep in range(1, args.pretrain_epochs + 1):
            t0 = clock(dev)
            n_it, u_all, p_all, n_all = draw_pairs(drv.pair_cols, args.pretrain_batch_size, drv.items, args.max_iters)
            total = model.mf_phase(u_all, p_all, n_all, mf_opt, reg_lambda=args.pretrain_regs).sum()
            rec = {"epoch": ep, "mf_s": clock(dev) - t0, "mf_iters": n_it}
            rec["mf_loss"] = float(total) / n_it
            say("Pretrain %04d | MF %.4fs (%d it, %.4f ms/it) mf_loss %.4f | %s" % (
                ep, rec["mf_s"], n_it, 1e3 * rec["mf_s"] / n_it, rec["mf_loss"], evaluate_table(rec)))
            pre["epochs"].append(rec)
            del u_all, p_all, n_all
        if args.pretrain_save:
            ckg_io.save_pretrain(args.pretrain_save, *model.pretrained_embeddings(ds.n_users, ds.n_items))
            say("Pretrain   | user / item rows written to %s" % args.pretrain_save)
        history.append({"epoch": 0, "pretrain": pre})

    def refresh(epoch, rec):
        # ---- attention refresh (kgat.py:139-145)
        t0 = clock(dev)
        if not args.attention_grad:   # (--attention_grad 1: every CF step computes its own, differentiable weights)
            with torch.no_grad():
                train_g.edata["w"] = model.compute_attention(train_g)
        rec["attention_s"] = clock(dev) - t0
        say("           | attention %.4fs" % rec["attention_s"])

    def cf_loss(u, p, n):   # full-graph gnn for every batch
        if args.attention_grad:
            train_g.edata["w"] = model.compute_attention(train_g, differentiable=True)
        return model.get_loss(model.gnn(train_g, train_g.ndata["id"]), u, p, n)

    def eval_inputs():
        for g in (train_g, test_g):
            g.edata["w"] = model.compute_attention(g)
            yield model.gnn(g, g.ndata["id"])

    fam = Family(model, [lambda epoch, rec: drv.kg_phase(rec, model, opt, trip_cols), refresh,
                         lambda epoch, rec: drv.cf_phase(epoch, rec, opt, cf_loss, label="GNN", kgat=model),
                         lambda epoch, rec: replicas_agree("epoch %d" % epoch)], eval_inputs, trip_cols.shape[1])
    drv.run(fam, history)
    if args.explain:
        # why the top-1 item?  the walk of highest attention product from it to the user, within as many hops as the
        # model has layers (test graph, the weights of the last evaluation's parameters)
        model.eval()
        with torch.no_grad():
            test_g.edata["w"] = model.compute_attention(test_g)
            emb = model.gnn(test_g, test_g.ndata["id"])
            users = sorted(splits.test_dict)[:args.explain]
            top1 = metrics.recommend(emb, users, ds.item_id_range, 1, seen=splits.train_valid_dict)[0][:, 0].tolist()
            if args.explain_top == 1:
                paths, ranked = model.explain(test_g, users, [max(i, 0) for i in top1]), None
            else:
                ranked = model.explain(test_g, users, [max(i, 0) for i in top1], top=args.explain_top)
                paths = ranked.first()
        for q, (u, i) in enumerate(zip(users, top1)):
            if i < 0:
                say("explain | user %d: no unseen item" % u)
                continue
            say("explain | user %d item %d | score %.6g | %s" % (u, i, paths.best(q)[2], paths.describe(q)))
            for r in range(args.explain_top if ranked is not None else 0):
                if int(ranked.ranked_len[q, r]) == 0:
                    break
                say("explain+ | user %d item %d | rank %d | len %d | score %.6g | %s"
                    % (u, i, r + 1, int(ranked.ranked_len[q, r]), float(ranked.ranked_score[q, r]), ranked.describe(q, r)))
    drv.write_log(fam, history)
    if world > 1:
        dist.destroy_process_group()
    return history


def _kge_family(drv):
    """--model cfkg / cke.  cfkg: an epoch is a TransE KG phase over ALL training triples of the collaborative KG
    (interactions included), then evaluation on CFKG.readout.  cke: a TransR KG phase over the item-KG triples, a CF
    phase of BPR steps on CKE.readout, then evaluation.  One FusedAdam over all parameters."""
    args, ds, dev = drv.args, drv.ds, drv.dev
    kind, off, items = args.model, ds.n_users, drv.items
    trip = ds.train_KG_triplet
    if kind == "cfkg":
        forward = trip[(trip[:, 0] < off) & (trip[:, 2] >= off)]
        if len(forward) == 0:
            raise SystemExit("--model cfkg: the training triples hold no user -> item interaction")
        interact = int(forward[:, 1].min())
        model = K.CFKG(ds.n_KG_entity, ds.n_KG_relation, dim=args.entity_embed_dim).to(dev)
    else:
        trip = trip[~((trip[:, 0] < off) | (trip[:, 2] < off))]
        if len(trip) == 0:
            raise SystemExit("--model cke: the training triples hold no item-KG triple")
        model = K.CKE(ds.n_KG_entity, ds.n_KG_relation, dim=args.entity_embed_dim, relation_dim=args.relation_embed_dim).to(dev)
    print("--model %s | %d KG-phase triples" % (kind, len(trip)))
    load_mf(drv, model)
    opt = K.FusedAdam(model.parameters(), lr=args.lr)
    trip_cols = id_columns(trip, dev)
    phases = [lambda epoch, rec: drv.kg_phase(rec, model, opt, trip_cols)]
    if kind == "cke":
        phases.append(lambda epoch, rec: drv.cf_phase(
            epoch, rec, opt, lambda u, p, n: model.get_loss(model.readout(items), u, p, n)))

    def eval_inputs():
        emb = (model.readout(interact, (0, off), items) if kind == "cfkg" else model.readout(items)).contiguous()
        return emb, emb

    return Family(model, phases, eval_inputs, len(trip))


def _fm_family(drv):
    """--model fm / nfm: an epoch is a CF phase of BPR steps - one pooled call over the 2 B feature sets {user} + F(item),
    positives first, one FusedAdam over all parameters - then evaluation: FM on its dot-product table (FM.readout) with
    the metrics of the other models, NFM through NFM.evaluate (block scores in torch operators, torch.topk, the metric
    kernel; with --nfm_eval fused the all-pairs sweep instead of the first two)."""
    args, ds, dev = drv.args, drv.ds, drv.dev
    kind, items = args.model, drv.items
    feats = K.FeatureSets.from_kg(ds.train_KG_triplet, items, ds.n_KG_entity, device=dev)
    if kind == "fm":
        model = K.FM(ds.n_KG_entity, feats, dim=args.entity_embed_dim).to(dev)
    else:
        model = K.NFM(ds.n_KG_entity, feats, dim=args.entity_embed_dim, layers=tuple(getattr(args, "nfm_layers", [64])),
                      dropout=args.dropout_rate).to(dev)
    print("--model %s | %d items, %d (item, feature) pairs, longest list %d" % (
        kind, feats.n_items, feats.n_pairs, int(np.diff(feats._host["indptr"]).max())))
    load_mf(drv, model)
    opt = K.FusedAdam(model.parameters(), lr=args.lr)

    def eval_inputs():
        if kind == "nfm":
            fused = getattr(args, "nfm_eval", "torch") == "fused"
            return (model.evaluate(drv.splits.plans[name], args.Ks, fused=fused) for name in ("valid", "test"))
        emb = model.readout((0, ds.n_users), items).contiguous()
        return emb, emb

    return Family(model, [lambda epoch, rec: drv.cf_phase(epoch, rec, opt, model.get_loss)], eval_inputs, None)


def _ripple_family(drv):
    """--model ripplenet: the ripple sets are built once on the host; an epoch is a CF phase of steps on the pair stream
    of the other baselines - one pass over the 2 B samples, positives first, BCE with 1:1 negatives plus the KGE and L2
    terms (RippleNet.get_loss), one FusedAdam over all parameters - then evaluation through RippleNet.evaluate (block
    scores in torch operators, torch.topk, the metric kernel; with --ripple_eval fused the all-pairs sweep instead of the
    first two)."""
    args, ds, dev = drv.args, drv.ds, drv.dev
    t0 = time.perf_counter()
    sets = K.RippleSets.build(ds.train_KG_triplet, ds.train_pairs, ds.n_users, ds.n_KG_entity, n_hop=getattr(args, "n_hop", 2),
                              n_memory=getattr(args, "n_memory", 32), seed=args.seed,
                              add_inverse=bool(getattr(args, "ripple_inverse", 0)), device=dev)
    print("--model ripplenet | %d hops x %d triples per user, %d relations, %d of %d users without a triple, built in %.2fs" % (
        sets.n_hop, sets.n_memory, sets.n_rel, int((~sets.valid).sum()), sets.n_users, time.perf_counter() - t0))
    model = K.RippleNet(ds.n_KG_entity, sets, dim=args.entity_embed_dim, kge_weight=getattr(args, "kge_weight", 0.01),
                        item_update_mode=getattr(args, "item_update_mode", "plus_transform"),
                        using_all_hops=bool(getattr(args, "using_all_hops", 1)), item_range=drv.items).to(dev)
    opt = K.FusedAdam(model.parameters(), lr=args.lr)
    fused = getattr(args, "ripple_eval", "torch") == "fused"

    def eval_inputs():
        return (model.evaluate(drv.splits.plans[name], args.Ks, fused=fused) for name in ("valid", "test"))

    return Family(model, [lambda epoch, rec: drv.cf_phase(epoch, rec, opt, model.get_loss)], eval_inputs, None)


if __name__ == "__main__":
    main()
