"""What the graph-attention tests share: a torch restatement of DGL 0.4.x GATConv's message passing (any dtype, an
optional keep mask for the attention dropout), the adversarial graph of tests/test_gpu_spmm_max.py restated with a hub
source beside the hub destination, and the scale metric; for tests/test_gpu_gat_shapes.py the per-element metric
(term_scales, scaled_error), the two inputs with an exact result as builders for any graph, and graphs whose CSR rows
are planted on the tile geometry (graph_from_degrees, planted_degrees) or sized for the longer run lengths."""
import numpy as np
import torch

N, E, HUB_DST, N_HUB_DST, HUB_SRC, N_HUB_SRC, N_DUP = 3000, 60000, 1500, 5000, 700, 4000, 500


def gat_aggregate(src, dst, n, ft, el, er, slope=0.2, keep=None, drop_p=0.0):
    """rst (N, H, F) from ft (N, H, F), el, er (N, H) - torch tensors of one dtype, differentiable; src, dst int64
    tensors in edge-id order; `keep` (E, H) bool: the attention dropout's mask, the kept entries scaled by
    1 / (1 - drop_p).  The softmax's denominator runs over all edges, as in DGL."""
    H = ft.shape[1]
    s = torch.nn.functional.leaky_relu(el[src] + er[dst], slope)
    m = torch.full((n, H), float("-inf"), dtype=ft.dtype, device=ft.device).scatter_reduce(
        0, dst.unsqueeze(1).expand(-1, H), s.detach(), "amax")
    p = torch.exp(s - m[dst])
    a = p / torch.zeros((n, H), dtype=ft.dtype, device=ft.device).index_add(0, dst, p)[dst]
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


# ---- the per-element metric of tests/test_gpu_gat_shapes.py

NAMES = ("out", "g_ft", "g_el", "g_er")


def term_scales(src, dst, n, ft, el, er, g_out, slope, keep=None, drop_p=0.0):
    """(S_out, S_gft, S_gel, S_ger) in fp64: for each element of out, g_ft, g_el and g_er the sum of the absolute
    values of the terms the element adds - what a rounding error of that element is proportional to, whatever the
    rest of its tensor holds.  With a the attention, c the dropout factor (0 or 1 / (1 - drop_p)), out the result,
    gamma_abs = sum_f |g_out[v,h,f] ft[u,h,f]|, sg_abs = sum_f |g_out[v,h,f] out[v,h,f]| and sl = (z > 0 ? 1 : slope):
      S_out[v,h,f] = sum_{e->v} c a |ft[u,h,f]|             S_gft[u,h,f] = sum_{e out of u} c a |g_out[v,h,f]|
      S_gel[u,h]   = sum_{e out of u} a (c gamma_abs + sg_abs) sl      S_ger[v,h] = the same sum over e -> v
    Tensors of any float dtype on one device (taken to fp64 there); src, dst int64; keep (E, H) bool or None."""
    ft, el, er, g_out = (t.detach().double() for t in (ft, el, er, g_out))
    H = ft.shape[1]
    z = el[src] + er[dst]
    s = torch.nn.functional.leaky_relu(z, slope)
    m = torch.full((n, H), float("-inf"), dtype=torch.float64, device=ft.device).scatter_reduce(
        0, dst.unsqueeze(1).expand(-1, H), s, "amax")
    p = torch.exp(s - m[dst])
    a = p / torch.zeros((n, H), dtype=torch.float64, device=ft.device).index_add(0, dst, p)[dst]
    del s, m, p
    ca = a if keep is None else a * keep.double() / (1.0 - drop_p)
    fu, gv = ft[src], g_out[dst]
    out = torch.zeros_like(ft).index_add(0, dst, ca.unsqueeze(-1) * fu)
    S_out = torch.zeros_like(ft).index_add(0, dst, ca.unsqueeze(-1) * fu.abs())
    S_gft = torch.zeros_like(ft).index_add(0, src, ca.unsqueeze(-1) * gv.abs())
    gamma_abs = (gv * fu).abs().sum(-1)
    del fu, gv
    sg_abs = (g_out * out).abs().sum(-1)
    sl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    t = (ca * gamma_abs + a * sg_abs[dst]) * sl
    S_gel = torch.zeros_like(el).index_add(0, src, t)
    S_ger = torch.zeros_like(el).index_add(0, dst, t)
    return S_out, S_gft, S_gel, S_ger


def scaled_error(x, ref, S):
    """max |x - ref| / S over the elements with S > 0; x must be exactly 0 where S == 0 (rows without edges, edges all
    dropped, slope 0 with every z <= 0: no term at all).  0.0 when no element has S > 0."""
    x, ref, S = (np.asarray(t, np.float64) for t in (x, ref, S))
    assert x.shape == ref.shape == S.shape and np.isfinite(x).all() and (S >= 0).all()
    nz = S > 0
    assert (x[~nz] == 0).all(), "%d elements without a term are not exactly 0" % (x[~nz] != 0).sum()
    return float((np.abs(x - ref)[nz] / S[nz]).max()) if nz.any() else 0.0


def references(src, dst, n, ft, el, er, g_out, slope=0.2, keep=None, drop_p=0.0, device="cpu"):
    """What an accuracy test compares with, from numpy inputs: (ref64, err32, scales) - the fp64 restatement's
    [out, g_ft, g_el, g_er], the scaled_error of the same restatement run in fp32 against it, and term_scales; lists of
    numpy arrays in the order of NAMES.  Everything runs on `device` and every edge-sized tensor is freed on return."""
    dev = torch.device(device)
    s, d = torch.as_tensor(src).to(dev), torch.as_tensor(dst).to(dev)
    k = None if keep is None else torch.as_tensor(keep).to(dev)
    res = {}
    for dt in (torch.float64, torch.float32):
        t = [torch.as_tensor(x).to(dev, dt).requires_grad_(True) for x in (ft, el, er)]
        out = gat_aggregate(s, d, n, t[0], t[1], t[2], slope, k, drop_p)
        out.backward(torch.as_tensor(g_out).to(dev, dt))
        res[dt] = [out.detach().cpu().numpy()] + [x.grad.cpu().numpy() for x in t]
        del out, t
    S = [x.cpu().numpy() for x in term_scales(s, d, n, *(torch.as_tensor(x).to(dev) for x in (ft, el, er, g_out)), slope, k, drop_p)]
    err32 = [scaled_error(a, b, c) for a, b, c in zip(res[torch.float32], res[torch.float64], S)]
    if dev.type == "cuda":
        torch.cuda.empty_cache()
    return res[torch.float64], err32, S


# ---- inputs whose result is exact (tests/test_gpu_gat.py holds the same two for the adversarial graph)

def uniform_attention_input(src, dst, n, H, F, seed, device="cpu"):
    """(ft, el, er, want): el constant per head, so every p = exp(0) = 1, l = deg and the sums are sums of integers:
    out = fp32(sum) / fp32(deg), bit for bit.  ft holds integers in [-8, 8]; every partial sum stays below 2^24
    (asserted).  The integer sum is an int64 index_add on `device`: exact and free of any order."""
    rng = np.random.default_rng(seed)
    ft = rng.integers(-8, 9, (n, H, F)).astype(np.float32)
    el = np.broadcast_to((0.75 * np.arange(H) - 1.0).astype(np.float32), (n, H)).copy()
    er = rng.standard_normal((n, H)).astype(np.float32)
    deg = np.bincount(dst, minlength=n)
    assert 8 * int(deg.max(initial=0)) < 2 ** 24
    dev = torch.device(device)
    s, d = torch.as_tensor(src).to(dev), torch.as_tensor(dst).to(dev)
    total = torch.zeros((n, H, F), dtype=torch.int64, device=dev).index_add_(0, d, torch.as_tensor(ft).to(dev).long()[s])
    total = total.cpu().numpy()
    del s, d
    assert np.abs(total).max(initial=0) < 2 ** 24
    want = np.zeros((n, H, F), np.float32)
    nz = deg > 0
    want[nz] = total[nz].astype(np.float32) / deg[nz].astype(np.float32)[:, None, None]
    return ft, el, er, want


def dominant_source_input(src, dst, n, H, F, seed):
    """(ft, el, er, want): el = 600 x a permutation per head, er = 0: the competing logits lie >= 120 below the row's
    largest after the slope and fp32 exp of that is exactly 0, so out is ft of the row's largest-el source (k parallel
    edges: k x / k).  Without the subtraction of the row maximum exp(600 ...) overflows."""
    rng = np.random.default_rng(seed)
    ft = rng.integers(-8, 9, (n, H, F)).astype(np.float32)
    rank = np.stack([rng.permutation(n) for _ in range(H)], 1)             # (n, H)
    el = (600.0 * rank).astype(np.float32)
    assert 600 * n < 2 ** 24 and np.exp(np.float32(-120.0)) == 0
    er = np.zeros((n, H), np.float32)
    best = np.full((n, H), -1, np.int64)
    np.maximum.at(best, dst, rank[src])
    inv = np.empty((n, H), np.int64)
    for h in range(H):
        inv[rank[:, h], h] = np.arange(n)
    want = np.zeros((n, H, F), np.float32)
    nz = np.bincount(dst, minlength=n) > 0
    for h in range(H):
        want[nz, h] = ft[inv[best[nz, h], h], h]
    return ft, el, er, want


def row_max_fp32(src, dst, n, el, er, slope):
    """m of the rows with in-edges: max_e leaky_relu(el[src] + er[dst]), the exact sum rounded to fp32, then the product
    with fp32(slope) rounded to fp32 - what fp32 arithmetic gives in any order, the maximum being exact.  -inf elsewhere."""
    z = (el.astype(np.float64)[src] + er.astype(np.float64)[dst]).astype(np.float32)
    s = np.where(z > 0, z, (z.astype(np.float64) * np.float64(np.float32(slope))).astype(np.float32))
    m = np.full(el.shape, -np.inf, np.float32)
    np.maximum.at(m, dst, s)
    return m


# ---- graphs with planted geometry

def graph_from_degrees(deg, seed):
    """(src, dst) int64: dst = repeat(arange(N), deg) - the destination CSR's row boundaries sit exactly where `deg`
    puts them -, random sources, shuffled edge ids."""
    rng = np.random.default_rng(seed)
    deg = np.asarray(deg, np.int64)
    dst = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    src = rng.integers(0, len(deg), len(dst)).astype(np.int64)
    perm = rng.permutation(len(dst))
    return src[perm], dst[perm]


CHAINS = (1, 6, 7, 8, 9, 20)        # tiles a planted row reaches beyond the one it starts in; 8 is the first tree chain
LONG_CHAIN = 8                      # kLongChain of gat_finish_kernel


def planted_degrees(te):
    """In-degrees that put, with tiles of `te` CSR positions: a row that fills tile 0; two rows of te / 2 that meet on a
    tile edge; single-edge rows across a tile edge; rows that start mid-tile (slot 1 of their first tile) and reach
    k tiles on for k in CHAINS, then the same from a tile edge (slot 0); a row of three whole tiles that ends on a tile
    edge; one edge in the last tile; rows without edges at position 0, at the end and in between."""
    deg = [0, te, te, 0, te // 2, te // 2, te - 5] + [1] * 10          # ... now 5 positions into tile 4
    # slot 1: each starts where the last one ended.  k = 1 starts in tile 4 and k = 8 in tile 5: their finish items (9 and
    # 11) share a wavefront at every width but the widest, whose wavefront holds one tile's two items
    for k in (1, 8, 6, 9, 7, 20):
        deg += [k * te + 3, 0]
    deg += [te - (5 + 3 * len(CHAINS))]                                    # to the tile edge
    for k in (1, 8, 6, 9, 7, 20):                                          # slot 0, and a filler to the next tile edge
        deg += [k * te + 3, te - 3]
    # a tile whose first row lies inside it and whose last row is a tree chain that ends on a tile edge: a short and a
    # long item in one wavefront at the widest width too
    deg += [te // 2, LONG_CHAIN * te + te // 2]
    deg += [0, 0, 3 * te, 1, 0]
    assert sorted(CHAINS) == [1, 6, 7, 8, 9, 20]
    return np.asarray(deg, np.int64)


def row_owners(indptr, te):
    """For every row with edges what gat_finish_kernel derives: (tile, slot, tiles beyond the first) with slot 0 / 1 =
    first / last row of the tile the row starts in, or slot -1 for a row strictly inside one tile (no finish item)."""
    indptr = np.asarray(indptr, np.int64)
    rows = np.nonzero(indptr[1:] > indptr[:-1])[0]
    row_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    owners = {}
    for r in rows:
        rb, re = indptr[r], indptr[r + 1]
        b, bl = rb // te, (re - 1) // te
        t1 = min((b + 1) * te, indptr[-1])
        slot = 0 if row_of[b * te] == r else (1 if row_of[t1 - 1] == r else -1)
        owners[int(r)] = (int(b), slot, int(bl - b))
    return owners


def production_graph(e, seed=5, n=20000, hub=40000):
    """(src, dst) int64, `e` edges over n = 20,000 nodes in shuffled edge-id order: the first 5 % of the rows without
    in-edges, a hub destination with `hub` in-edges, a hub source with `hub` out-edges, the rest uniform."""
    rng = np.random.default_rng(seed)
    lo = n // 20
    hub_dst, hub_src = lo + 7, n - 3
    rest = e - 2 * hub
    dst = np.concatenate([np.full(hub, hub_dst), rng.integers(lo, n, hub), rng.integers(lo, n, rest)])
    src = np.concatenate([rng.integers(0, n, hub), np.full(hub, hub_src), rng.integers(0, n, rest)])
    perm = rng.permutation(e)
    src, dst = src[perm].astype(np.int64), dst[perm].astype(np.int64)
    deg = np.bincount(dst, minlength=n)
    assert (deg[:lo] == 0).all() and deg[hub_dst] >= hub and np.bincount(src, minlength=n)[hub_src] >= hub
    return src, dst
