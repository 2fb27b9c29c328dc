"""What the graph-attention tests share: a torch restatement of DGL 0.4.x GATConv's message passing (any dtype, an
optional keep mask for the attention dropout), the adversarial graph of tests/test_gpu_spmm_max.py restated with a hub
source beside the hub destination, and the scale metric."""
import numpy as np
import torch

N, E, HUB_DST, N_HUB_DST, HUB_SRC, N_HUB_SRC, N_DUP = 3000, 60000, 1500, 5000, 700, 4000, 500


def gat_aggregate(src, dst, n, ft, el, er, slope=0.2, keep=None, drop_p=0.0):
    """rst (N, H, F) from ft (N, H, F), el, er (N, H) - torch tensors of one dtype, differentiable; src, dst int64
    tensors in edge-id order; `keep` (E, H) bool: the attention dropout's mask, the kept entries scaled by
    1 / (1 - drop_p).  The softmax's denominator runs over all edges, as in DGL."""
    H = ft.shape[1]
    s = torch.nn.functional.leaky_relu(el[src] + er[dst], slope)
    m = torch.full((n, H), float("-inf"), dtype=ft.dtype).scatter_reduce(0, dst.unsqueeze(1).expand(-1, H), s.detach(), "amax")
    p = torch.exp(s - m[dst])
    a = p / torch.zeros((n, H), dtype=ft.dtype).index_add(0, dst, p)[dst]
    if keep is not None:
        a = a * keep.to(ft.dtype) / (1.0 - drop_p)
    return torch.zeros_like(ft).index_add(0, dst, a.unsqueeze(-1) * ft[src])


def adversarial_graph(seed=11):
    """(src, dst) int64 numpy arrays, E = 60,000 edges over N = 3,000 nodes in shuffled edge-id order: one hub
    destination with 5,000 in-edges, one hub source with 4,000 out-edges, 5 % of the rows without in-edges, 500
    duplicated (src, dst) pairs, a power-law remainder."""
    rng = np.random.default_rng(seed)
    empty = rng.choice(np.setdiff1d(np.arange(N), [HUB_DST]), N // 20, replace=False)
    allowed = np.setdiff1d(np.arange(N), empty)
    p = 1.0 / np.power(1.0 + rng.permutation(len(allowed)), 0.9)
    n_pl = E - N_HUB_DST - N_HUB_SRC - N_DUP - len(allowed)   # every other row has at least one in-edge
    dst = np.concatenate([allowed, rng.choice(allowed, n_pl, p=p / p.sum()), np.full(N_HUB_DST, HUB_DST),
                          rng.choice(allowed, N_HUB_SRC)])
    src = rng.integers(0, N, len(dst))
    src[-N_HUB_SRC:] = HUB_SRC
    dup = rng.choice(len(dst), N_DUP, replace=False)
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    perm = rng.permutation(len(src))
    src, dst = src[perm].astype(np.int64), dst[perm].astype(np.int64)
    deg = np.bincount(dst, minlength=N)
    assert len(src) == E and deg[HUB_DST] >= N_HUB_DST and (deg == 0).sum() == N // 20
    assert np.bincount(src, minlength=N)[HUB_SRC] >= N_HUB_SRC
    return src, dst


def scale_error(x, ref):
    """max|x - ref| / max|ref|"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())
