"""Tensor-level wrappers around the C ABI (include/kgat_hip.h).

torch is used here for what it is good at on ROCm - device memory, the current HIP stream -
and nothing else: every arithmetic step of the path happens inside libkgat_hip.so.  All
functions validate device / dtype / contiguity before the call and turn a non-zero return
code into KGATLibraryError.  CPU tensors are rejected: this path has no CPU implementation.
"""
from collections import namedtuple

import torch

from . import _lib
from ._lib import KGATLibraryError, check

SPMM_MUL_SELF = 1
SPMM_DEFER_FINISH = 2
SPMM_ALGO = {"auto": 0, "merge": 1, "rows": 2, "generic": 3, "merge1": 4}
ATT_ALGO = {"auto": 0, "mfma": 1, "generic": 2, "mfma_chunk": 3}


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


class KernelTimer:
    """Optional per-op HIP-event timing (bench.py): while active, every wrapped C-ABI op
    records an event pair on the stream it launches on.  Costs nothing when inactive."""
    active = None

    def __init__(self):
        self.records = []  # (name, info, start_event, end_event)

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None
        return False

    def summary(self):
        """name -> list of (info, milliseconds); call after a device synchronize."""
        out = {}
        for name, info, a, b in self.records:
            out.setdefault(name, []).append((info, a.elapsed_time(b)))
        return out


class _timed:
    def __init__(self, name, info=None):
        self.t = KernelTimer.active
        self.name, self.info = name, info

    def __enter__(self):
        if self.t is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.t is not None:
            self.b.record()
            self.t.records.append((self.name, self.info, self.a, self.b))
        return False


def _need(t, dtype, name, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if type(t) is not torch.Tensor and hasattr(t, "materialize"):
        t.materialize()  # lazy.LazyEdgeWeights: the kernels read through the raw pointer
    if not t.is_cuda:
        raise KGATLibraryError("%s is on %s: the KGAT propagation path only runs on a HIP device "
                               "(no CPU implementation exists in this package)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _scratch(shape, dtype, device):
    """A scratch tensor of `shape` carved from `_workspace`: what a call hands to the library beside its workspace
    (partial sums, the permutation's intermediate array) comes from the same place as the workspace itself."""
    nbytes = dtype.itemsize
    for s in shape:
        nbytes *= int(s)
    return _workspace(nbytes, device)[:nbytes].view(dtype).view(shape)


def csr_from_coo(n_nodes, src, dst):
    """(indptr, col, eid, row_of) of the destination-major CSR; stable in edge id."""
    src = _need(src, torch.int32, "src")
    dst = _need(dst, torch.int32, "dst", src.shape)
    lib = _lib.load()
    e, dev = src.numel(), src.device
    indptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(e, dtype=torch.int32, device=dev)
    eid = torch.empty(e, dtype=torch.int32, device=dev)
    row_of = torch.empty(e, dtype=torch.int32, device=dev)
    nb = lib.kgat_csr_from_coo_workspace_bytes(n_nodes, e)
    ws = _workspace(nb, dev)
    check(lib.kgat_csr_from_coo(n_nodes, e, _ptr(src), _ptr(dst), _ptr(indptr), _ptr(col), _ptr(eid),
                                _ptr(row_of), _ptr(ws), ws.numel(), _stream(src)), "kgat_csr_from_coo")
    return indptr, col, eid, row_of


def group_by_relation(etype, n_rel):
    etype = _need(etype, torch.int32, "etype")
    lib = _lib.load()
    e, dev = etype.numel(), etype.device
    rel_ptr = torch.empty(n_rel + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    ws = _workspace(lib.kgat_group_by_relation_workspace_bytes(e, n_rel), dev)
    check(lib.kgat_group_by_relation(e, n_rel, _ptr(etype), _ptr(rel_ptr), _ptr(perm), _ptr(ws),
                                     ws.numel(), _stream(etype)), "kgat_group_by_relation")
    return rel_ptr, perm


def invert_permutation(perm):
    perm = _need(perm, torch.int32, "perm")
    inv = torch.empty_like(perm)
    check(_lib.load().kgat_invert_permutation(perm.numel(), _ptr(perm), _ptr(inv), _stream(perm)),
          "kgat_invert_permutation")
    return inv


def row_order_by_degree(indptr):
    indptr = _need(indptr, torch.int32, "indptr")
    lib = _lib.load()
    n = indptr.numel() - 1
    order = torch.empty(n, dtype=torch.int32, device=indptr.device)
    ws = _workspace(lib.kgat_row_order_workspace_bytes(n), indptr.device)
    check(lib.kgat_row_order_by_degree(n, _ptr(indptr), _ptr(order), _ptr(ws), ws.numel(),
                                       _stream(indptr)), "kgat_row_order_by_degree")
    return order


def gather(index, values, out=None):
    """out[i] = values[index[i]] (float32 or int32 values); `out` may be a preallocated flat tensor."""
    index = _need(index, torch.int32, "index")
    dtype = torch.float32 if values.dtype == torch.float32 else torch.int32
    values = _need(values, dtype, "values")
    if out is None:
        out = torch.empty(index.numel(), dtype=dtype, device=index.device)
    else:
        out = _need(out, dtype, "out", (index.numel(),))
    fn = _lib.load().kgat_gather_f32 if dtype == torch.float32 else _lib.load().kgat_gather_i32
    with _timed("gather", (index.numel(),)):
        check(fn(index.numel(), _ptr(index), _ptr(values), _ptr(out), _stream(index)), "kgat_gather")
    return out


def permute_tile():
    """Chunk / block length of the planned permutation (kgat_permute_tile)."""
    return int(_lib.load().kgat_permute_tile())


def permute_supported(n):
    """Whether the planned permutation streams at n items (kgat_permute_supported); beyond, call `gather`."""
    return bool(_lib.load().kgat_permute_supported(int(n)))


PermutePlan = namedtuple("PermutePlan", "n slot_a dst_a slot_b")


def permute_plan_arrays(src_of, tile):
    """(slot_a, dst_a, slot_b) of include/kgat_hip.h for the permutation `src_of` (an integer tensor holding every
    value of range(n) once; not checked here) at chunk / block length `tile` <= 32,768: index arithmetic and two
    stable sorts on whatever device `src_of` is on.  The 16-bit ranks are held as int16 (same bits below 2^15)."""
    n, dev = src_of.numel(), src_of.device
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    dst_of = torch.zeros_like(pos)
    dst_of[src_of.long()] = pos                                  # destination of every source position
    blk = dst_of // tile
    order = torch.argsort(blk, stable=True)                      # tmp[j] holds source position order[j]
    tmp_of = torch.empty_like(pos)
    tmp_of[order] = pos
    slot_b = (dst_of[order] % tile).to(torch.int16)
    n_blk = (n + tile - 1) // tile
    order2 = torch.argsort((pos // tile) * n_blk + blk, stable=True)  # order2[c * tile + i]: source at rank i of chunk c
    slot_a = torch.empty(n, dtype=torch.int16, device=dev)
    slot_a[order2] = (pos % tile).to(torch.int16)
    return slot_a, tmp_of[order2].to(torch.int32), slot_b


def permute_plan(src_of):
    """The static plan of kgat_permute_f32 for out[i] = in[src_of[i]] (`src_of` an int32 permutation of range(n)):
    one-off setup.  The sorts run on the HOST (about a second at 4 M items): on the device their temporaries - a dozen
    arrays of odd sizes - stay behind in torch's caching allocator as free blocks that the step's buffers are then carved
    from, and that placement cost bench.py's step 6 us (profiles/r07_permute_ab.txt); this way the device allocator
    sees the three plan arrays, which stay, and blocks of n floats.  The plan is proved before it is returned: it must
    move arange(n) onto src_of, bit for bit."""
    src_of = _need(src_of, torch.int32, "src_of")
    n, dev = src_of.numel(), src_of.device
    if not permute_supported(n):
        raise KGATLibraryError("permute_plan: %d items are beyond kgat_permute_supported" % n)
    host = src_of.cpu()
    if n and (int(host.min()) < 0 or int(host.max()) >= n):
        raise ValueError("permute_plan: src_of is not a permutation of range(%d)" % n)
    plan = PermutePlan(n, *(t.to(dev) for t in permute_plan_arrays(host, permute_tile())))
    probe = torch.arange(n, dtype=torch.int32, device=dev).view(torch.float32)
    if not torch.equal(permute(plan, probe).view(torch.int32), src_of):
        raise KGATLibraryError("permute_plan: the plan does not reproduce the permutation it was built from")
    return plan


def permute(plan, values, out=None, tmp=None):
    """out[i] = values[src_of[i]] through the plan of `permute_plan(src_of)`: two streaming launches
    (kgat_permute_f32).  `tmp`: n floats of scratch a caller may keep between calls on one stream."""
    values = _need(values, torch.float32, "values", (plan.n,))
    out = torch.empty_like(values) if out is None else _need(out, torch.float32, "out", (plan.n,))
    tmp = _scratch((plan.n,), torch.float32, values.device) if tmp is None else _need(tmp, torch.float32, "tmp", (plan.n,))
    with _timed("permute", (plan.n,)):
        check(_lib.load().kgat_permute_f32(plan.n, _ptr(plan.slot_a), _ptr(plan.dst_a), _ptr(plan.slot_b), _ptr(values),
                                           _ptr(out), _ptr(tmp), _stream(values)), "kgat_permute_f32")
    return out


def _att_params(n_nodes, ent, W_R, rel):
    """The parameters every attention entry takes, checked: (ent, W_R, rel, n_rel, d, k)."""
    ent = _need(ent, torch.float32, "ent")
    n_rel, d, k = W_R.shape
    W_R = _need(W_R, torch.float32, "W_R")
    rel = _need(rel, torch.float32, "rel", (n_rel, k))
    if ent.shape != (n_nodes, d):
        raise ValueError("ent has shape %s, expected %s" % (tuple(ent.shape), (n_nodes, d)))
    return ent, W_R, rel, n_rel, d, k


def _att_rel_arrays(n_rel, **arrays):
    """The per-relation index arrays of an attention entry (rel_ptr, gptr, rel_tptr): int32, (R+1,)."""
    for name, t in arrays.items():
        _need(t, torch.int32, name, (n_rel + 1,))


def att_score(n_nodes, rel_ptr, perm, src_g, dst_g, ent, W_R, rel, pos_g=None, algo="auto"):
    """Attention logits (E,) in edge-id order; with pos_g (CSR position of edge perm[i]) also
    in CSR order."""
    ent, W_R, rel, n_rel, d, k = _att_params(n_nodes, ent, W_R, rel)
    perm = _need(perm, torch.int32, "perm")
    e = perm.numel()
    _att_rel_arrays(n_rel, rel_ptr=rel_ptr)
    src_g = _need(src_g, torch.int32, "src_g", (e,))
    dst_g = _need(dst_g, torch.int32, "dst_g", (e,))
    logits = torch.empty(e, dtype=torch.float32, device=ent.device)
    logits_csr = None
    if pos_g is not None:
        pos_g = _need(pos_g, torch.int32, "pos_g", (e,))
        logits_csr = torch.empty(e, dtype=torch.float32, device=ent.device)
    with _timed("att_score", (e, d, k)):
        check(_lib.load().kgat_att_score_f32(n_nodes, e, d, k, n_rel, _ptr(rel_ptr), _ptr(perm), _ptr(src_g),
                                             _ptr(dst_g), _ptr(ent), _ptr(W_R), _ptr(rel), _ptr(logits),
                                             _ptr(logits_csr), _ptr(pos_g), ATT_ALGO[algo], _stream(ent)),
              "kgat_att_score_f32")
    return logits, logits_csr


def head_groups(rel_ptr, dst_g):
    """(gid, gptr, g_node, n_groups) of a relation-grouped, destination-sorted edge list.
    Reads the group count back to the host (one sync, once per graph)."""
    rel_ptr = _need(rel_ptr, torch.int32, "rel_ptr")
    dst_g = _need(dst_g, torch.int32, "dst_g")
    lib = _lib.load()
    e, n_rel, dev = dst_g.numel(), rel_ptr.numel() - 1, dst_g.device
    gid_pad = torch.zeros(e + 16, dtype=torch.int32, device=dev)  # kernels read 16-byte groups: 16 ids of slack
    gid = gid_pad[:e]
    gptr = torch.empty(n_rel + 1, dtype=torch.int32, device=dev)
    g_node = torch.empty(max(e, 1), dtype=torch.int32, device=dev)
    ws = _workspace(lib.kgat_head_groups_workspace_bytes(e), dev)
    check(lib.kgat_head_groups(e, n_rel, _ptr(rel_ptr), _ptr(dst_g), _ptr(gid), _ptr(gptr), _ptr(g_node),
                               _ptr(ws), ws.numel(), _stream(dst_g)), "kgat_head_groups")
    n_groups = int(gptr[n_rel].item())
    return gid, gptr, g_node[:max(n_groups, 1)].clone(), n_groups


ATT_F32_PRODUCTS = 1  # include/kgat_hip.h: KGAT_ATT_F32_PRODUCTS


def att_score_split_supported(n_nodes, d, k, n_rel):
    return bool(_lib.load().kgat_att_score_split_supported(int(n_nodes), int(d), int(k), int(n_rel)))


def att_score_folded_supported(n_nodes, d, k, n_rel):
    return bool(_lib.load().kgat_att_score_folded_supported(int(n_nodes), int(d), int(k), int(n_rel)))


def att_score_split(n_nodes, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, n_groups, ent, W_R, rel,
                    want_csr=True, g_tab=None, want_eid=True, folded=False, f32_products=False):
    """Attention logits via head groups (see kgat_att_score_split_f32; folded=True:
    kgat_att_score_folded_f32, whose scratch table is n_groups x d; f32_products: its
    KGAT_ATT_F32_PRODUCTS flag).  Returns (logits edge-id order, logits CSR order or None)."""
    ent, W_R, rel, n_rel, d, k = _att_params(n_nodes, ent, W_R, rel)
    perm = _need(perm, torch.int32, "perm")
    e = perm.numel()
    for name, t in (("src_g", src_g), ("pos_g", pos_g), ("gid", gid)):
        _need(t, torch.int32, name, (e,))
    _att_rel_arrays(n_rel, rel_ptr=rel_ptr, gptr=gptr)
    _need(g_node, torch.int32, "g_node")
    width = d if folded else k
    if g_tab is None:
        g_tab = _scratch((max(n_groups, 1), width), torch.float32, ent.device)
    else:
        _need(g_tab, torch.float32, "g_tab")
        if g_tab.numel() < max(n_groups, 1) * width:
            raise ValueError("g_tab holds %d floats, needs %d" % (g_tab.numel(), max(n_groups, 1) * width))
    logits = torch.empty(e, dtype=torch.float32, device=ent.device) if want_eid else None
    logits_csr = torch.empty(e, dtype=torch.float32, device=ent.device) if want_csr else None
    name = "kgat_att_score_folded_f32" if folded else "kgat_att_score_split_f32"
    extra = ((ATT_F32_PRODUCTS if f32_products else 0),) if folded else ()
    with _timed("att_score", (e, d, k)):
        check(getattr(_lib.load(), name)(n_nodes, e, d, k, n_rel, _ptr(rel_ptr), _ptr(perm), _ptr(src_g),
                                         _ptr(pos_g), _ptr(gid), _ptr(gptr), _ptr(g_node), n_groups,
                                         _ptr(ent), _ptr(W_R), _ptr(rel), _ptr(g_tab), _ptr(logits),
                                         _ptr(logits_csr), *extra, _stream(ent)), name)
    return logits, logits_csr


# positions per tile of the fused kernel: a 16-group block with more positions is cut and every
# piece recomputes the block's V rows (1,459 ticks) where walking on would cost 267 ticks per 64
# positions, so pieces should be long - but one wave walks a piece alone, and a piece must stay a
# small part of its workgroup's time for the eight waves to balance.  Measured on MI355X with the
# cost-balanced split (amazon-book-shaped CKG): 128: 0.2135 ms, 256: 0.2019.
FOLD_TILE_CAP = 256
# per-tile cost model of the fused kernel (kgat_fold_tile_parts; from per-workgroup clock stamps,
# scripts/micro/att_stamps.py): a tile, a chunk of 64 positions past the first 64, a relation
# change inside a workgroup's range.  With the bf16-piece products (d % 32 == 0) the fit is 649
# ticks of workgroup time per tile, 389 per later chunk, 10,661 per relation change; with the fp32
# products 1,459 / 267 / 10,630.  Both in units of a 64th of a tile.  Round 3 re-scanned the triple
# for the kernel with packed records and coalesced stores.  Stand-alone launches (variants
# alternating, every launch with another tile split; the tool went with round 5's clean-up) preferred
# cheaper chunks - (64,24,800) 0.145 ms against 0.151 - but INSIDE the step, where the launch starts
# with the table and the index arrays partly evicted, the order is the opposite (KGAT_FOLD_TILE_COST
# A/B of bench.py on one box: (64,38,1051) 142.5-144.0 us, (64,30,1051) 145.2-146.4, (64,30,800)
# 146.4-146.5, (64,24,800) 154.1-154.6): later chunks, whose rows are not requested ahead, cost
# more there.  The step is what counts: the fitted triple stays.
FOLD_TILE_COST = (64, 38, 1051)
FOLD_TILE_COST_F32 = (64, 12, 466)
# d = 128 (att_fold_fused128_kernel): scanned inside the step on the amazon-book-shaped CKG
# (scripts/micro/att128_cost_scan.sh).  With round 5's products (two fp16 pieces per operand, three piece products:
# half the MFMAs of rounds 3-4) a later chunk weighs more against a tile's products than it did: (64,12,700) - round
# 3's choice - 0.385 ms, (64,18,700) 0.352, (64,24,700) 0.350, (64,32,700) 0.361, (64,24,400) 0.355, (64,24,1200) 0.351,
# (64,40,1000) 0.376.
FOLD_TILE_COST_128 = (64, 24, 700)


def fold_tile_cost(d, f32_products=False):
    """The split cost that goes with the product form att_score_fused takes at width d
    (``KGAT_FOLD_TILE_COST="tile,chunk,relation"`` overrides it: A/B runs of the whole step)."""
    from .options import options
    if options.fold_tile_cost:
        return options.fold_tile_cost
    if d == 128:
        return FOLD_TILE_COST_128
    return FOLD_TILE_COST if (d % 32 == 0 and not f32_products) else FOLD_TILE_COST_F32


def fold_tiles(rel_ptr, gid, gptr, n_groups, cap=FOLD_TILE_CAP, n_parts=None, cost=FOLD_TILE_COST):
    """Work tiles of the fused attention kernel (kgat_fold_tiles) and their cost-balanced split
    over `n_parts` workgroups (kgat_fold_tile_parts; default: one per compute unit).  Returns
    (tiles (T_max, 4) int32, rel_tptr (R+1,) int32, part_tptr (n_parts+1,) int32); rel_tptr[-1]
    is the number of tiles in use."""
    lib = _lib.load()
    rel_ptr = _need(rel_ptr, torch.int32, "rel_ptr")
    gptr = _need(gptr, torch.int32, "gptr", rel_ptr.shape)
    gid = _need(gid, torch.int32, "gid")
    n_rel = rel_ptr.numel() - 1
    e = gid.numel()
    dev = gid.device
    t_max = max(int(lib.kgat_fold_tiles_max(e, int(n_groups), n_rel, int(cap))), 1)
    tiles = torch.empty((t_max, 4), dtype=torch.int32, device=dev)      # (the entry clears the rows no tile takes)
    rel_tptr = torch.empty(n_rel + 1, dtype=torch.int32, device=dev)
    ws = _workspace(lib.kgat_fold_tiles_workspace_bytes(int(n_groups), n_rel), dev)
    check(lib.kgat_fold_tiles(e, n_rel, int(n_groups), _ptr(rel_ptr), _ptr(gid), _ptr(gptr), int(cap),
                              _ptr(tiles), _ptr(rel_tptr), _ptr(ws), ws.numel(), _stream(gid)), "kgat_fold_tiles")
    if n_parts is None:
        n_parts = torch.cuda.get_device_properties(dev).multi_processor_count
    part_tptr = torch.empty(int(n_parts) + 1, dtype=torch.int32, device=dev)
    ws2 = _workspace(lib.kgat_fold_tile_parts_workspace_bytes(t_max), dev)
    check(lib.kgat_fold_tile_parts(t_max, n_rel, _ptr(tiles), _ptr(rel_tptr), int(n_parts), int(cost[0]), int(cost[1]),
                                   int(cost[2]), _ptr(part_tptr), _ptr(ws2), ws2.numel(), _stream(gid)),
          "kgat_fold_tile_parts")
    return tiles, rel_tptr, part_tptr


def att_score_fused_supported(n_nodes, d, k, n_rel):
    return bool(_lib.load().kgat_att_score_fused_supported(int(n_nodes), int(d), int(k), int(n_rel)))


def att_pack_records(rel_ptr, gptr, gid, src_g):
    """rec_g[p] = src_g[p] | (slot of p's head group in its 16-group block << 28): the one
    index the fused attention kernel reads per grouped position (kgat_att_pack_records; graph-static)."""
    rel_ptr = _need(rel_ptr, torch.int32, "rel_ptr")
    gptr = _need(gptr, torch.int32, "gptr", rel_ptr.shape)
    src_g = _need(src_g, torch.int32, "src_g")
    e = src_g.numel()
    gid = _need(gid, torch.int32, "gid", (e,))
    rec = torch.empty(e, dtype=torch.int32, device=src_g.device)
    check(_lib.load().kgat_att_pack_records(e, rel_ptr.numel() - 1, _ptr(rel_ptr), _ptr(gptr), _ptr(gid), _ptr(src_g),
                                            _ptr(rec), _stream(src_g)), "kgat_att_pack_records")
    return rec


def att_score_fused(n_nodes, rel_ptr, perm, src_g, pos_g, gid, gptr, g_node, tiles, rel_tptr, ent, W_R, rel,
                    want_csr=True, want_eid=True, part_tptr=None, f32_products=False, rec_g=None, want_grouped=False,
                    part_clocks=None):
    """Attention logits, fused folded form (kgat_att_score_fused_f32).  The kernel reads one packed
    record per grouped position (`rec_g`, att_pack_records; built here from `src_g` / `gid` when the
    caller does not keep one).  `part_tptr`: the tile range of every workgroup (fold_tiles); None:
    equal tile counts, one workgroup per compute unit.  `f32_products`: the two products on the fp32
    MFMA (KGAT_ATT_F32_PRODUCTS) instead of the three-bf16-piece products the kernel takes by
    default when d % 32 == 0.  `part_clocks` (int64, 2 x n_parts): measurement aid
    (kgat_att_score_fused_timed_f32) - every workgroup's start / end time in 100 MHz ticks.  Returns (logits edge-id
    order, logits CSR order) - unrequested ones None - and, with want_grouped, a third item: the logits in grouped order."""
    ent, W_R, rel, n_rel, d, k = _att_params(n_nodes, ent, W_R, rel)
    _att_rel_arrays(n_rel, rel_ptr=rel_ptr, gptr=gptr, rel_tptr=rel_tptr)
    if rec_g is None:
        rec_g = att_pack_records(rel_ptr, gptr, gid, src_g)
    rec_g = _need(rec_g, torch.int32, "rec_g")
    e = rec_g.numel()
    if want_eid:
        perm = _need(perm, torch.int32, "perm", (e,))
    if want_csr:
        pos_g = _need(pos_g, torch.int32, "pos_g", (e,))
    _need(g_node, torch.int32, "g_node")
    _need(tiles, torch.int32, "tiles")
    n_parts = 0
    if part_tptr is not None:
        part_tptr = _need(part_tptr, torch.int32, "part_tptr")
        n_parts = part_tptr.numel() - 1
    logits = torch.empty(e, dtype=torch.float32, device=ent.device) if want_eid else None
    logits_csr = torch.empty(e, dtype=torch.float32, device=ent.device) if want_csr else None
    logits_g = torch.empty(e, dtype=torch.float32, device=ent.device) if want_grouped else None
    flags = ATT_F32_PRODUCTS if f32_products else 0
    args = (n_nodes, e, d, k, n_rel, _ptr(rel_ptr), _ptr(perm) if want_eid else None, _ptr(rec_g),
            _ptr(pos_g) if want_csr else None, _ptr(gptr), _ptr(g_node), _ptr(tiles), _ptr(rel_tptr), _ptr(part_tptr), n_parts,
            _ptr(ent), _ptr(W_R), _ptr(rel), _ptr(logits), _ptr(logits_csr), _ptr(logits_g), flags)
    with _timed("att_score", (e, d, k)):
        if part_clocks is None:
            check(_lib.load().kgat_att_score_fused_f32(*args, _stream(ent)), "kgat_att_score_fused_f32")
        else:
            part_clocks = _need(part_clocks, torch.int64, "part_clocks", (2 * n_parts,))
            check(_lib.load().kgat_att_score_fused_timed_f32(*args, _ptr(part_clocks), _stream(ent)),
                  "kgat_att_score_fused_timed_f32")
    return (logits, logits_csr, logits_g) if want_grouped else (logits, logits_csr)


def att_score_bwd_supported(n_nodes, d, k, n_rel):
    return bool(_lib.load().kgat_att_score_bwd_supported(int(n_nodes), int(d), int(k), int(n_rel)))


def att_score_bwd(n_nodes, n_scored, n_groups, perm, src_g, gid, gstart, gptr, g_node, node_ptr, node_col, node_row,
                  node_wsrc, ent, W_R, rel, grad_logits):
    """Gradients (grad_ent (N,d), grad_W_R (R,d,k), grad_rel (R,k)) of the attention logits w.r.t. their three
    parameters, given the logits' gradient `grad_logits` (E,) in EDGE-ID order (kgat_att_score_bwd_f32; the index arrays
    are the graph-static ones its header comment names, `perm` the edge id of every grouped position).  All three are
    fully written by the call.  The one gather into grouped order happens here, into a buffer of this call's own with
    the float of room the entry writes its 1.0 to: no tensor of the caller is written."""
    ent = _need(ent, torch.float32, "ent")
    W_R = _need(W_R, torch.float32, "W_R")
    n_rel, d, k = W_R.shape
    rel = _need(rel, torch.float32, "rel", (n_rel, k))
    if ent.shape != (n_nodes, d):
        raise ValueError("ent has shape %s, expected %s" % (tuple(ent.shape), (n_nodes, d)))
    n_scored, n_groups = int(n_scored), int(n_groups)
    perm = _need(perm, torch.int32, "perm")
    grad_logits = _need(grad_logits, torch.float32, "grad_logits", perm.shape)
    if perm.numel() < n_scored:
        raise ValueError("perm holds %d positions, needs %d" % (perm.numel(), n_scored))
    grad_logits_g = torch.empty(n_scored + 1, dtype=torch.float32, device=ent.device)
    gather(perm[:n_scored], grad_logits, out=grad_logits_g[:n_scored])
    for name, t, n in (("src_g", src_g, n_scored), ("gid", gid, n_scored), ("gstart", gstart, n_groups + 1),
                       ("gptr", gptr, n_rel + 1), ("g_node", g_node, n_groups), ("node_ptr", node_ptr, n_nodes + 1),
                       ("node_col", node_col, n_scored + n_groups), ("node_row", node_row, n_scored + n_groups),
                       ("node_wsrc", node_wsrc, n_scored + n_groups)):
        if _need(t, torch.int32, name).numel() < n:
            raise ValueError("%s holds %d entries, needs %d" % (name, t.numel(), n))
    lib = _lib.load()
    dev = ent.device
    grad_ent = torch.empty((n_nodes, d), dtype=torch.float32, device=dev)
    grad_W = torch.empty((n_rel, d, k), dtype=torch.float32, device=dev)
    grad_rel = torch.empty((n_rel, k), dtype=torch.float32, device=dev)
    ws = _workspace(lib.kgat_att_score_bwd_workspace_bytes(n_nodes, n_scored, n_groups, d, k, n_rel), dev)
    with _timed("att_score_bwd", (n_scored, n_groups, d, k)):
        check(lib.kgat_att_score_bwd_f32(n_nodes, n_scored, n_groups, d, k, n_rel, _ptr(src_g), _ptr(gid), _ptr(gstart),
                                         _ptr(gptr), _ptr(g_node), _ptr(node_ptr), _ptr(node_col), _ptr(node_row),
                                         _ptr(node_wsrc), _ptr(ent), _ptr(W_R), _ptr(rel), _ptr(grad_logits_g),
                                         _ptr(grad_ent), _ptr(grad_W), _ptr(grad_rel), _ptr(ws), ws.numel(), _stream(ent)),
              "kgat_att_score_bwd_f32")
    return grad_ent, grad_W, grad_rel


def _triplet_ids(h, r, pos_t, neg_t):
    """The id tensors of a triplet batch: int32, contiguous, on the device, r / pos_t / neg_t as long as h.  Returns the
    batch size."""
    h = _need(h, torch.int32, "h")
    for name, t in (("r", r), ("pos_t", pos_t), ("neg_t", neg_t)):
        _need(t, torch.int32, name, (h.numel(),))
    return h.numel()


def _presort(model, names, ids, n_nodes, *n_rel):
    """The sorts of a whole phase's batches up front (kgat_<model>_presort_f32): `ids` are (n_batches, batch) int32
    tensors called `names`; returns (sorted, stride) - batch b's block is sorted[b * stride:(b + 1) * stride]."""
    first = _need(ids[0], torch.int32, names[0])
    if first.dim() != 2:
        raise ValueError("%s must be (n_batches, batch)" % names[0])
    for name, t in zip(names[1:], ids[1:]):
        _need(t, torch.int32, name, first.shape)
    lib = _lib.load()
    nb, b = first.shape
    entry = "kgat_%s_presort_f32" % model
    stride = int(getattr(lib, "kgat_%s_sorted_bytes" % model)(b, *n_rel))
    out = _workspace(nb * stride, first.device)
    with _timed(model + "_presort", (nb, b)):
        check(getattr(lib, entry)(int(n_nodes), *n_rel, nb, b, *[_ptr(t) for t in ids], _ptr(out), out.numel(), _stream(first)),
              entry)
    return out, stride


class StepState:
    """What a sequence of fused train-and-step calls (kgat_*_adam_step_f32) keeps between calls: the step workspace, the
    row_slot words (zero once, never cleared: a word is valid for the call whose tag it carries) and the tag counter.
    `key`: the sizes it was made for, n_nodes first, and the device."""

    def __init__(self, sizes, workspace_bytes, device):
        self.key = tuple(int(x) for x in sizes) + (str(device),)
        self.workspace = _workspace(workspace_bytes, device)
        self.row_slot = torch.zeros(self.key[0], dtype=torch.int64, device=device)
        self.tag = 0


def transr_supported(n_nodes, d, k, n_rel, batch):
    return bool(_lib.load().kgat_transr_supported(int(n_nodes), int(d), int(k), int(n_rel), int(batch)))


def transr_workspace(batch, d, k, n_rel, device):
    return _workspace(_lib.load().kgat_transr_workspace_bytes(batch, d, k, n_rel), device)


def transr_loss_grad(h, r, pos_t, neg_t, ent, W_R, rel, reg_lambda, want_grad=True, out=None, workspace=None):
    """TransR loss of a triplet batch and, if want_grad, its gradients with respect to the entity
    table (dense), W_R and the relation table (kgat_transr_loss_grad_f32).  Index tensors are
    int32.  Returns (loss 0-d tensor, grad_ent, grad_W, grad_rel) - gradients None without
    want_grad.  `out` = (loss, grad_ent, grad_W, grad_rel) and `workspace` reuse buffers of an earlier call."""
    ent = _need(ent, torch.float32, "ent")
    n_rel, d, k = W_R.shape
    W_R = _need(W_R, torch.float32, "W_R")
    rel = _need(rel, torch.float32, "rel", (n_rel, k))
    b = _triplet_ids(h, r, pos_t, neg_t)
    lib = _lib.load()
    dev = ent.device
    if out is not None:
        loss, g_ent, g_w, g_rel = out
        _need(g_ent, torch.float32, "grad_ent", ent.shape)
        _need(g_w, torch.float32, "grad_W", W_R.shape)
        _need(g_rel, torch.float32, "grad_rel", rel.shape)
    else:
        loss = torch.empty((), dtype=torch.float32, device=dev)
        g_ent = torch.empty_like(ent) if want_grad else None
        g_w = torch.empty_like(W_R) if want_grad else None
        g_rel = torch.empty_like(rel) if want_grad else None
    need = lib.kgat_transr_workspace_bytes(b, d, k, n_rel)
    ws = workspace if workspace is not None and workspace.numel() >= need else _workspace(need, dev)
    with _timed("transr", (b, d, k)):
        check(lib.kgat_transr_loss_grad_f32(ent.shape[0], n_rel, d, k, b, _ptr(h), _ptr(r), _ptr(pos_t), _ptr(neg_t),
                                            _ptr(ent), _ptr(W_R), _ptr(rel), float(reg_lambda), _ptr(loss),
                                            _ptr(g_ent), _ptr(g_w), _ptr(g_rel), _ptr(ws), ws.numel(), _stream(ent)),
              "kgat_transr_loss_grad_f32")
    return loss, g_ent, g_w, g_rel


def transr_presort(h, r, pos_t, neg_t, n_nodes, n_rel):
    """The sorts of a whole KG phase's batches in one launch (kgat_transr_presort_f32): h, r, pos_t, neg_t are
    (n_batches, batch) int32 tensors; returns (sorted, stride) - batch b's block is sorted[b * stride:(b + 1) * stride]."""
    return _presort("transr", ("h", "r", "pos_t", "neg_t"), (h, r, pos_t, neg_t), n_nodes, int(n_rel))


def TransRAdamState(n_nodes, d, k, n_rel, batch, device):
    """The StepState of a sequence of kgat_transr_adam_step_f32 calls."""
    return StepState((n_nodes, d, k, n_rel, batch), _lib.load().kgat_transr_step_workspace_bytes(batch, d, k, n_rel), device)


def transr_adam_step(h, r, pos_t, neg_t, sorted_block, ent, W_R, rel, exp_avg, exp_avg_sq, steps, lr, beta1, beta2, eps,
                     reg_lambda, loss_out, state):
    """One KG iteration (kgat_transr_adam_step_f32): TransR loss of the batch into `loss_out` (a 1-element fp32 view)
    and the Adam step on ent / W_R / rel in place.  exp_avg / exp_avg_sq: ctypes arrays of the three moment pointers
    (built once per phase by the caller); steps: the three step counts after this step.  Shapes and dtypes are the
    caller's responsibility here (KGATPropagation.kg_phase validates them once per phase): this is the per-iteration
    call of a 1,641-iteration loop."""
    import ctypes as C
    n_rel, d, k = W_R.shape
    state.tag += 1
    arr_t = (C.c_int64 * 3)(*steps)
    check(_lib.load().kgat_transr_adam_step_f32(ent.shape[0], n_rel, d, k, h.numel(), h.data_ptr(), r.data_ptr(),
                                                pos_t.data_ptr(), neg_t.data_ptr(), sorted_block.data_ptr(), ent.data_ptr(),
                                                W_R.data_ptr(), rel.data_ptr(), exp_avg, exp_avg_sq, arr_t, float(lr),
                                                float(beta1), float(beta2), float(eps), float(reg_lambda),
                                                loss_out.data_ptr(), state.row_slot.data_ptr(), state.tag,
                                                state.workspace.data_ptr(), state.workspace.numel(), _stream(ent)),
          "kgat_transr_adam_step_f32")


def transr_forward(h, r, pos_t, neg_t, ent, W_R, rel, reg_lambda):
    """TransR loss with the per-sample rows left in the returned workspace for transr_backward
    (kgat_transr_forward_f32)."""
    ent = _need(ent, torch.float32, "ent")
    n_rel, d, k = W_R.shape
    W_R = _need(W_R, torch.float32, "W_R")
    rel = _need(rel, torch.float32, "rel", (n_rel, k))
    b = _triplet_ids(h, r, pos_t, neg_t)
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=ent.device)
    ws = _workspace(lib.kgat_transr_workspace_bytes(b, d, k, n_rel), ent.device)
    with _timed("transr_forward", (b, d, k)):
        check(lib.kgat_transr_forward_f32(ent.shape[0], n_rel, d, k, b, _ptr(h), _ptr(r), _ptr(pos_t), _ptr(neg_t),
                                          _ptr(ent), _ptr(W_R), _ptr(rel), float(reg_lambda), _ptr(loss), _ptr(ws),
                                          ws.numel(), _stream(ent)), "kgat_transr_forward_f32")
    return loss, ws


def transr_backward(h, r, pos_t, neg_t, shapes, ws, grad_scale=None):
    """The three gradients of transr_forward's loss (kgat_transr_backward_f32), times the device scalar grad_scale."""
    (n_nodes, d), (n_rel, _, k) = shapes
    dev = ws.device
    g_ent = torch.empty((n_nodes, d), dtype=torch.float32, device=dev)
    g_w = torch.empty((n_rel, d, k), dtype=torch.float32, device=dev)
    g_rel = torch.empty((n_rel, k), dtype=torch.float32, device=dev)
    if grad_scale is not None:
        grad_scale = _need(grad_scale.reshape(1), torch.float32, "grad_scale")
    with _timed("transr_backward", (h.numel(), d, k)):
        check(_lib.load().kgat_transr_backward_f32(n_nodes, n_rel, d, k, h.numel(), _ptr(h), _ptr(r), _ptr(pos_t),
                                                   _ptr(neg_t), _ptr(grad_scale), _ptr(g_ent), _ptr(g_w), _ptr(g_rel),
                                                   _ptr(ws), ws.numel(), _stream(ws)), "kgat_transr_backward_f32")
    return g_ent, g_w, g_rel


def edge_softmax(indptr, row_of, eid, logits, in_csr_order=False, e_range=None, want_out=True,
                 want_csr=False, three_pass=False):
    """Softmax over each destination's in-edges (`indptr`, `row_of`, `eid` of the destination-major
    CSR).  `logits` (E,) is in edge-id order, or in CSR order with in_csr_order=True.  Returns
    (out in edge-id order, out_csr in CSR order); unrequested ones are None.  three_pass=True runs
    the independent three-pass implementation (kgat_edge_softmax_3pass_f32)."""
    logits = _need(logits, torch.float32, "logits")
    indptr = _need(indptr, torch.int32, "indptr")
    row_of = _need(row_of, torch.int32, "row_of", logits.shape)
    eid = _need(eid, torch.int32, "eid", logits.shape)
    n_nodes = indptr.numel() - 1
    lib = _lib.load()
    e0, e1 = (0, logits.numel()) if e_range is None else e_range
    out = torch.empty_like(logits) if want_out else None
    out_csr = torch.empty_like(logits) if want_csr else None
    with _timed("edge_softmax", (e1 - e0,)):
        if three_pass:
            ws = _workspace(lib.kgat_edge_softmax_3pass_workspace_bytes(n_nodes), logits.device)
            check(lib.kgat_edge_softmax_3pass_f32(n_nodes, e0, e1, _ptr(row_of), _ptr(eid), _ptr(logits),
                                                  1 if in_csr_order else 0, _ptr(out), _ptr(out_csr), _ptr(ws),
                                                  ws.numel(), _stream(logits)), "kgat_edge_softmax_3pass_f32")
        else:
            ws = _workspace(lib.kgat_edge_softmax_workspace_bytes(n_nodes, e1 - e0), logits.device)
            check(lib.kgat_edge_softmax_f32(n_nodes, e0, e1, _ptr(indptr), _ptr(row_of), _ptr(eid), _ptr(logits),
                                            1 if in_csr_order else 0, _ptr(out), _ptr(out_csr), _ptr(ws),
                                            ws.numel(), _stream(logits)), "kgat_edge_softmax_f32")
    return out, out_csr


def edge_softmax_permuted_supported(n_edges, e_begin=0):
    """Whether kgat_edge_softmax_permuted_f32 takes a softmax over CSR positions [e_begin, e_begin + n_edges)."""
    return bool(_lib.load().kgat_edge_softmax_permuted_supported(int(e_begin), int(e_begin) + int(n_edges)))


def edge_softmax_permuted(indptr, row_of, eid, logits, plan, in_csr_order=False, out=None, tmp=None):
    """`edge_softmax(..., want_out=False, want_csr=True)` followed by `permute(plan, out_csr)` in three launches instead
    of four, same bits (kgat_edge_softmax_permuted_f32): the permutation's bin pass finishes the rows the sweep's ranges
    cut.  `plan`: `permute_plan` of the permutation CSR position -> edge id.  Returns (out in edge-id order, out_csr)."""
    logits = _need(logits, torch.float32, "logits", (plan.n,))
    indptr = _need(indptr, torch.int32, "indptr")
    row_of = _need(row_of, torch.int32, "row_of", logits.shape)
    eid = _need(eid, torch.int32, "eid", logits.shape)
    out = torch.empty_like(logits) if out is None else _need(out, torch.float32, "out", (plan.n,))
    tmp = _scratch((plan.n,), torch.float32, logits.device) if tmp is None else _need(tmp, torch.float32, "tmp", (plan.n,))
    out_csr = torch.empty_like(logits)
    n_nodes = indptr.numel() - 1
    lib = _lib.load()
    with _timed("edge_softmax_permuted", (plan.n,)):
        ws = _workspace(lib.kgat_edge_softmax_workspace_bytes(n_nodes, plan.n), logits.device)
        check(lib.kgat_edge_softmax_permuted_f32(n_nodes, 0, plan.n, _ptr(indptr), _ptr(row_of), _ptr(eid), _ptr(logits),
                                                 1 if in_csr_order else 0, _ptr(plan.slot_a), _ptr(plan.dst_a),
                                                 _ptr(plan.slot_b), _ptr(out), _ptr(out_csr), _ptr(tmp), _ptr(ws),
                                                 ws.numel(), _stream(logits)), "kgat_edge_softmax_permuted_f32")
    return out, out_csr


def edge_softmax_bwd(indptr, eid, a, grad_a, row_range=None):
    a = _need(a, torch.float32, "a")
    grad_a = _need(grad_a, torch.float32, "grad_a", a.shape)
    indptr = _need(indptr, torch.int32, "indptr")
    if eid is not None:
        eid = _need(eid, torch.int32, "eid", a.shape)
    row0, n_rows = (0, indptr.numel() - 1) if row_range is None else row_range
    out = torch.zeros_like(a)
    if a.numel() == 0:  # rows without a single edge: nothing to write, and empty tensors have no storage to point at
        return out
    check(_lib.load().kgat_edge_softmax_bwd_f32(n_rows, row0, _ptr(indptr), _ptr(eid), _ptr(a),
                                                _ptr(grad_a), _ptr(out), _stream(a)),
          "kgat_edge_softmax_bwd_f32")
    return out


def spmm_workspace(n_edges, D, device):
    return _workspace(_lib.load().kgat_spmm_workspace_bytes(n_edges, D), device)


class DeferredRows:
    """What spmm(defer_finish=True) leaves to bi_interaction_mul(deferred=...): the row offsets of the call's rows, its
    CSR position range, the workspace holding the tiles' boundary partials and the tile size."""
    __slots__ = ("indptr_rows", "e_range", "workspace", "tile_edges", "n_rows", "D")

    def __init__(self, indptr_rows, e_range, workspace, tile_edges, n_rows, D):
        self.indptr_rows, self.e_range, self.workspace = indptr_rows, e_range, workspace
        self.tile_edges, self.n_rows, self.D = tile_edges, n_rows, D


def bi_interaction_deferral_supported(d_in, d_out):
    """The widths kgat_spmm_umule_sum_f32(KGAT_SPMM_DEFER_FINISH) + kgat_aggregator_deferred_f32 cover."""
    return int(d_in) in (16, 32, 64, 128) and int(d_out) in (16, 32, 64, 128)


def _csr_operands(X, indptr, col, row_of, eid, rows, e_range, workspace, workspace_for, out=None, want_out=True,
                  need_row_of=False):
    """What spmm, spmm_max, copy_reduce and spmm_bi_fused do alike with their operands: X is (N, D) float32, indptr and
    col are int32, row_of / eid int32 of col's shape or None (row_of not with need_row_of), `rows` = (row0, n_rows) and
    `e_range` = (e0, e1) default to the whole graph, `out` is allocated or checked as (n_rows, D) (not with
    want_out=False), and a missing workspace is sized by `workspace_for(n_edges, D, device)`.
    Returns X, indptr, col, row_of, eid, (row0, n_rows, e0, e1), out, workspace."""
    X = _need(X, torch.float32, "X")
    if X.dim() != 2:
        raise ValueError("X must be (N, D)")
    indptr = _need(indptr, torch.int32, "indptr")
    col = _need(col, torch.int32, "col")
    if row_of is not None or need_row_of:
        row_of = _need(row_of, torch.int32, "row_of", col.shape)
    if eid is not None:
        eid = _need(eid, torch.int32, "eid", col.shape)
    row0, n_rows = (0, indptr.numel() - 1) if rows is None else rows
    e0, e1 = (0, col.numel()) if e_range is None else e_range
    if want_out:
        if out is None:
            out = torch.empty((n_rows, X.shape[1]), dtype=torch.float32, device=X.device)
        else:
            out = _need(out, torch.float32, "out", (n_rows, X.shape[1]))
    if workspace is None:
        workspace = workspace_for(e1 - e0, X.shape[1], X.device)
    return X, indptr, col, row_of, eid, (row0, n_rows, e0, e1), out, workspace


def spmm(indptr, col, row_of, X, w, eid=None, out=None, order=None, mul_self=False, algo="auto",
         rows=None, e_range=None, workspace=None, self_out=None, defer_finish=False):
    """out[v - row0] = sum_p w_p X[col[p]] over the CSR rows `rows` = (row0, n_rows) whose CSR
    positions are `e_range` (defaults: the whole graph).  w is in CSR order, or in edge-id
    order when `eid` is given.  `self_out` (with mul_self): an (n_rows, D) column slice of a wider
    row-major buffer that also receives X[v] (the ego block of the readout).
    defer_finish=True (KGAT_SPMM_DEFER_FINISH): returns (out, DeferredRows) - the rows the edge tiles cut and the
    rows without in-edges are NOT in `out`; bi_interaction_mul(deferred=...) forms them on the way."""
    X, indptr, col, row_of, eid, (row0, n_rows, e0, e1), out, workspace = _csr_operands(
        X, indptr, col, row_of, eid, rows, e_range, workspace, spmm_workspace, out)
    D = X.shape[1]
    w = _need(w, torch.float32, "w", col.shape)
    if order is not None:
        order = _need(order, torch.int32, "order")
    self_stride = 0
    if self_out is not None:
        self_stride = _strided_rows(self_out, n_rows, D, "self_out")
    with _timed("spmm", (e1 - e0, n_rows, D)):
        check(_lib.load().kgat_spmm_umule_sum_f32(n_rows, row0, e0, e1, D, _ptr(indptr), _ptr(col), _ptr(row_of),
                                                  _ptr(eid), _ptr(X), _ptr(w), _ptr(out), _ptr(order),
                                                  _ptr(workspace), workspace.numel(),
                                                  (SPMM_MUL_SELF if mul_self else 0) | (SPMM_DEFER_FINISH if defer_finish else 0),
                                                  SPMM_ALGO[algo], _ptr(self_out), self_stride, _stream(X)),
              "kgat_spmm_umule_sum_f32")
    if defer_finish:
        te = int(_lib.load().kgat_spmm_tile_edges(e1 - e0, D))
        return out, DeferredRows(indptr[row0:row0 + n_rows + 1], (e0, e1), workspace, te, n_rows, D)
    return out


def spmm_max_workspace(n_edges, D, device):
    return _workspace(_lib.load().kgat_spmm_max_workspace_bytes(n_edges, D), device)


def spmm_max(indptr, col, row_of, X, w=None, eid=None, want_arg=True, out=None, rows=None, e_range=None, workspace=None):
    """(out, arg): out[v - row0] = max_p w_p X[col[p]] over the CSR rows `rows` = (row0, n_rows) whose CSR positions
    are `e_range` (defaults: the whole graph), arg (int32, None without want_arg) the edge that attains it - eid[p] when
    `eid` is given, else the position p (kgat_spmm_umule_max_f32: dgl.function.max over u_mul_e, or over copy_src with
    w=None).  w is in CSR order.  Equal products: the smallest edge id wins; a row without in-edges is (0, -1).  Exact
    and bitwise reproducible; no backward."""
    X, indptr, col, row_of, eid, (row0, n_rows, e0, e1), out, workspace = _csr_operands(
        X, indptr, col, row_of, eid, rows, e_range, workspace, spmm_max_workspace, out, need_row_of=True)
    D = X.shape[1]
    if w is not None:
        w = _need(w, torch.float32, "w", col.shape)
    arg = torch.empty((n_rows, D), dtype=torch.int32, device=X.device) if want_arg else None
    with _timed("spmm_max", (e1 - e0, n_rows, D)):
        check(_lib.load().kgat_spmm_umule_max_f32(n_rows, row0, e0, e1, D, _ptr(indptr), _ptr(col), _ptr(row_of),
                                                  _ptr(eid), _ptr(X), _ptr(w), _ptr(out), _ptr(arg), _ptr(workspace),
                                                  workspace.numel(), _stream(X)),
              "kgat_spmm_umule_max_f32")
    return out, arg


def spmm_max4_workspace(n_edges, D, device):
    """Workspace of spmm_max4 for rows of D = 4 Q floats."""
    return _workspace(_lib.load().kgat_spmm_max4_workspace_bytes(n_edges, D // 4), device)


def spmm_max4(indptr, col, row_of, X, w=None, eid=None, want_arg=True, rows=None, e_range=None, workspace=None):
    """(out, arg_edge, arg_slot): the four largest of {w_p X[col[p], q, s]} over the CSR positions p of a row and the
    slots s, per query q, in order (kgat_spmm_umule_max4_f32).  X is (N, Q, 4) or (N, 4 Q) float32 with Q in
    {4, 8, 16, 32}; out is (n_rows, Q, 4), arg_edge (int32) the winners' edges - eid[p] when `eid` is given, else p -
    and arg_slot (uint8) their source slots, both None without want_arg.  Equal products: the smallest edge, then the
    smallest slot wins; a row without in-edges is (0, -1, 255).  w is in CSR order.  Exact and bitwise reproducible; no
    backward."""
    X = _need(X, torch.float32, "X")
    if (X.dim() == 3 and X.shape[2] != 4) or (X.dim() == 2 and X.shape[1] % 4):
        raise ValueError("X must be (N, Q, 4) or (N, 4 Q), got %s" % (tuple(X.shape),))
    X2 = X.reshape(X.shape[0], -1) if X.dim() == 3 else X
    X2, indptr, col, row_of, eid, (row0, n_rows, e0, e1), out, workspace = _csr_operands(
        X2, indptr, col, row_of, eid, rows, e_range, workspace, spmm_max4_workspace, need_row_of=True)
    Q = X2.shape[1] // 4
    if w is not None:
        w = _need(w, torch.float32, "w", col.shape)
    arg_edge = torch.empty((n_rows, Q, 4), dtype=torch.int32, device=X.device) if want_arg else None
    arg_slot = torch.empty((n_rows, Q, 4), dtype=torch.uint8, device=X.device) if want_arg else None
    with _timed("spmm_max4", (e1 - e0, n_rows, Q)):
        check(_lib.load().kgat_spmm_umule_max4_f32(n_rows, row0, e0, e1, Q, _ptr(indptr), _ptr(col), _ptr(row_of),
                                                   _ptr(eid), _ptr(X2), _ptr(w), _ptr(out), _ptr(arg_edge),
                                                   _ptr(arg_slot), _ptr(workspace), workspace.numel(), _stream(X2)),
              "kgat_spmm_umule_max4_f32")
    return out.view(n_rows, Q, 4), arg_edge, arg_slot


def gat_supported(H, F):
    """The (heads, features per head) kgat_gat_fwd_f32 / kgat_gat_bwd_f32 cover: H F in {16, 32, 64, 128}, F % 4 == 0."""
    return bool(_lib.load().kgat_gat_supported(int(H), int(F)))


def _gat_operands(csr, ft, el, er):
    ft = _need(ft, torch.float32, "ft")
    if ft.dim() != 3:
        raise ValueError("ft must be (N, H, F), got %s" % (tuple(ft.shape),))
    n, H, F = ft.shape
    el = _need(el, torch.float32, "el", (n, H))
    er = _need(er, torch.float32, "er", (n, H))
    indptr = _need(csr.indptr, torch.int32, "indptr", (n + 1,))
    col = _need(csr.col, torch.int32, "col")
    row_of = _need(csr.row_of, torch.int32, "row_of", col.shape)
    eid = _need(csr.eid, torch.int32, "eid", col.shape)
    return ft, el, er, (n, col.numel(), H, F), (indptr, col, row_of, eid)


def _gat_workspace(n, e, H, F, backward, device):
    return _workspace(_lib.load().kgat_gat_workspace_bytes(n, e, H, F, int(backward)), device)


def gat_forward(csr, ft, el, er, negative_slope=0.2, drop_p=0.0, seed=0):
    """(out, m, l) of kgat_gat_fwd_f32: GATConv's aggregation over the destination-major `csr` (indptr, col, eid,
    row_of) - out[v,h,:] = sum_{e->v} c a ft[src e, h, :] with a the destination softmax of
    leaky_relu(el[src] + er[dst]) per head and c the attention dropout's factor
    (dropout_keep_mask(seed, E, H, drop_p)[edge id, h]) - plus the row maximum m and the denominator l (N, H) the
    backward recomputes a from.  ft (N, H, F), el, er (N, H) float32; (H, F) as gat_supported."""
    ft, el, er, (n, e, H, F), graph = _gat_operands(csr, ft, el, er)
    out = torch.empty_like(ft)
    m, l = torch.empty_like(el), torch.empty_like(el)
    ws = _gat_workspace(n, e, H, F, False, ft.device)
    with _timed("gat_fwd", (e, n, H, F)):
        check(_lib.load().kgat_gat_fwd_f32(n, e, H, F, *[_ptr(t) for t in graph], _ptr(ft), _ptr(el), _ptr(er),
                                           float(negative_slope), float(drop_p), int(seed) & (2 ** 64 - 1), _ptr(out),
                                           _ptr(m), _ptr(l), _ptr(ws), ws.numel(), _stream(ft)), "kgat_gat_fwd_f32")
    return out, m, l


def gat_backward(csr, csr_rev, ft, el, er, m, l, out, g_out, negative_slope=0.2, drop_p=0.0, seed=0):
    """(g_ft, g_el, g_er) of kgat_gat_bwd_f32 from what gat_forward returned and the gradient at `out`: one walk over
    `csr` and one over the reversed graph's `csr_rev`, the attention recomputed from m and l in both."""
    ft, el, er, (n, e, H, F), graph = _gat_operands(csr, ft, el, er)
    m = _need(m, torch.float32, "m", el.shape)
    l = _need(l, torch.float32, "l", el.shape)
    out = _need(out, torch.float32, "out", ft.shape)
    g_out = _need(g_out, torch.float32, "g_out", ft.shape)
    rev = (_need(csr_rev.indptr, torch.int32, "rev.indptr", (n + 1,)), _need(csr_rev.col, torch.int32, "rev.col", (e,)),
           _need(csr_rev.row_of, torch.int32, "rev.row_of", (e,)), _need(csr_rev.eid, torch.int32, "rev.eid", (e,)))
    g_ft, g_el, g_er = torch.empty_like(ft), torch.empty_like(el), torch.empty_like(el)
    ws = _gat_workspace(n, e, H, F, True, ft.device)
    with _timed("gat_bwd", (e, n, H, F)):
        check(_lib.load().kgat_gat_bwd_f32(n, e, H, F, *[_ptr(t) for t in graph + rev], _ptr(ft), _ptr(el), _ptr(er),
                                           _ptr(m), _ptr(l), _ptr(out), _ptr(g_out), float(negative_slope),
                                           float(drop_p), int(seed) & (2 ** 64 - 1), _ptr(g_ft), _ptr(g_el), _ptr(g_er),
                                           _ptr(ws), ws.numel(), _stream(ft)), "kgat_gat_bwd_f32")
    return g_ft, g_el, g_er


def rgcn_supported(D, B, R):
    """The (feature width, bases, relations) the kgat_rgcn_* entries cover: D in {16, 32, 64, 128}, 1 <= B <= 8,
    R B <= 4096."""
    return bool(_lib.load().kgat_rgcn_supported(int(D), int(B), int(R)))


def _rgcn_graph(csr, etype, norm, n):
    indptr = _need(csr.indptr, torch.int32, "indptr", (n + 1,))
    col = _need(csr.col, torch.int32, "col")
    row_of = _need(csr.row_of, torch.int32, "row_of", col.shape)
    etype = _need(etype, torch.int32, "etype", col.shape)
    if norm is not None:
        norm = _need(norm, torch.float32, "norm", col.shape)
    return (indptr, col, row_of, etype, norm), col.numel()


def _rgcn_scratch(n, e, D, B, R, which, device):
    return _workspace(_lib.load().kgat_rgcn_scratch_bytes(n, e, D, B, R, which), device)


def rgcn_forward(csr, etype_csr, norm_csr, x, a):
    """Z (N, B, D) of kgat_rgcn_fwd_f32: Z[v, b, :] = sum_{e: u->v} norm[e] a[etype[e], b] x[u, :] over the
    destination-major `csr`, `etype_csr` (int32) and `norm_csr` (float32 or None: 1) in its order.  x (N, D), a (R, B)
    float32; (D, B, R) as rgcn_supported."""
    x = _need(x, torch.float32, "x")
    a = _need(a, torch.float32, "a")
    if x.dim() != 2 or a.dim() != 2:
        raise ValueError("x must be (N, D) and a (R, B), got %s, %s" % (tuple(x.shape), tuple(a.shape)))
    (n, D), (R, B) = x.shape, a.shape
    graph, e = _rgcn_graph(csr, etype_csr, norm_csr, n)
    Z = torch.empty((n, B, D), dtype=torch.float32, device=x.device)
    ws = _rgcn_scratch(n, e, D, B, R, 0, x.device)
    with _timed("rgcn_fwd", (e, n, D, B, R)):
        check(_lib.load().kgat_rgcn_fwd_f32(n, e, D, B, R, *[_ptr(t) for t in graph], _ptr(x), _ptr(a), _ptr(Z),
                                            _ptr(ws), ws.numel(), _stream(x)), "kgat_rgcn_fwd_f32")
    return Z


def rgcn_backward_x(csr_rev, etype_rev, norm_rev, g_Z, a):
    """g_x (N, D) of kgat_rgcn_bwd_x_f32 from the gradient at Z (N, B, D): one walk over the reversed graph's
    `csr_rev`, `etype_rev` / `norm_rev` in its order."""
    g_Z = _need(g_Z, torch.float32, "g_Z")
    a = _need(a, torch.float32, "a")
    if g_Z.dim() != 3 or a.dim() != 2 or a.shape[1] != g_Z.shape[1]:
        raise ValueError("g_Z must be (N, B, D) and a (R, B), got %s, %s" % (tuple(g_Z.shape), tuple(a.shape)))
    (n, B, D), R = g_Z.shape, a.shape[0]
    graph, e = _rgcn_graph(csr_rev, etype_rev, norm_rev, n)
    g_x = torch.empty((n, D), dtype=torch.float32, device=g_Z.device)
    ws = _rgcn_scratch(n, e, D, B, R, 1, g_Z.device)
    with _timed("rgcn_bwd_x", (e, n, D, B, R)):
        check(_lib.load().kgat_rgcn_bwd_x_f32(n, e, D, B, R, *[_ptr(t) for t in graph], _ptr(g_Z), _ptr(a), _ptr(g_x),
                                              _ptr(ws), ws.numel(), _stream(g_Z)), "kgat_rgcn_bwd_x_f32")
    return g_x


def rgcn_backward_coef(csr, etype_csr, norm_csr, x, g_Z, R, B):
    """g_a (R, B) of kgat_rgcn_bwd_coef_f32: g_a[r, b] = sum_{e: etype[e] = r} norm[e] <x[src e], g_Z[dst e, b]> over
    the destination-major `csr`."""
    x = _need(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("x must be (N, D), got %s" % (tuple(x.shape),))
    n, D = x.shape
    g_Z = _need(g_Z, torch.float32, "g_Z", (n, int(B), D))
    R, B = int(R), int(B)
    graph, e = _rgcn_graph(csr, etype_csr, norm_csr, n)
    g_a = torch.empty((R, B), dtype=torch.float32, device=x.device)
    ws = _rgcn_scratch(n, e, D, B, R, 2, x.device)
    with _timed("rgcn_bwd_coef", (e, n, D, B, R)):
        check(_lib.load().kgat_rgcn_bwd_coef_f32(n, e, D, B, R, *[_ptr(t) for t in graph], _ptr(x), _ptr(g_Z),
                                                 _ptr(g_a), _ptr(ws), ws.numel(), _stream(x)), "kgat_rgcn_bwd_coef_f32")
    return g_a


REDUCE ={"sum": 0, "mean": 1}
ACT = {None: 0, "none": 0, "relu": 1}


def copy_reduce(indptr, col, row_of, X, reduce="sum", out=None, rows=None, e_range=None, workspace=None):
    """out[v - row0] = sum | mean_p X[col[p]] over the CSR rows `rows` = (row0, n_rows) whose CSR positions are
    `e_range` (kgat_copy_reduce_f32: update_all(copy_src, sum | mean); no edge weight is read; the mean divides by the
    row's number of positions, rows without in-edges are 0)."""
    if reduce not in REDUCE:
        raise ValueError("reduce must be 'sum' or 'mean', got %r" % (reduce,))
    X, indptr, col, row_of, _, (row0, n_rows, e0, e1), out, workspace = _csr_operands(
        X, indptr, col, row_of, None, rows, e_range, workspace, spmm_workspace, out)
    D = X.shape[1]
    with _timed("copy_reduce", (e1 - e0, n_rows, D, reduce)):
        check(_lib.load().kgat_copy_reduce_f32(n_rows, row0, e0, e1, D, _ptr(indptr), _ptr(col), _ptr(row_of), _ptr(X),
                                               _ptr(out), REDUCE[reduce], _ptr(workspace), workspace.numel(),
                                               _stream(X)),
              "kgat_copy_reduce_f32")
    return out


def sage_dense_supported(d_in, d_out):
    return bool(_lib.load().kgat_sage_dense_supported(int(d_in), int(d_out)))


def sage_dense(H, HN, W_self, W_neigh, b_self=None, b_neigh=None, act=None, want_h=True, norm_out=None, self_out=None):
    """Z = act(H W_self^T + HN W_neigh^T + b_self + b_neigh) (kgat_sage_dense_f32; act None or 'relu'); returns Z (None
    with want_h=False) and writes Z / ||Z_row|| into `norm_out` and H into `self_out` (column slices of a wider
    row-major buffer) where given."""
    H = _need(H, torch.float32, "H")
    if H.dim() != 2:
        raise ValueError("H must be (N, d_in)")
    n, d_in = H.shape
    HN = _need(HN, torch.float32, "HN", (n, d_in))
    W_self = _need(W_self, torch.float32, "W_self")
    d_out = W_self.shape[0]
    if W_self.shape != (d_out, d_in):
        raise ValueError("W_self has shape %s, expected (*, %d)" % (tuple(W_self.shape), d_in))
    W_neigh = _need(W_neigh, torch.float32, "W_neigh", (d_out, d_in))
    if b_self is not None:
        b_self = _need(b_self, torch.float32, "b_self", (d_out,))
    if b_neigh is not None:
        b_neigh = _need(b_neigh, torch.float32, "b_neigh", (d_out,))
    h_out = torch.empty((n, d_out), dtype=torch.float32, device=H.device) if want_h else None
    stride = _strided_rows(norm_out, n, d_out, "norm_out") if norm_out is not None else 0
    self_stride = _strided_rows(self_out, n, d_in, "self_out") if self_out is not None else 0
    with _timed("sage_dense", (n, d_in, d_out)):
        check(_lib.load().kgat_sage_dense_f32(n, d_in, d_out, _ptr(H), _ptr(HN), _ptr(W_self), _ptr(W_neigh),
                                              _ptr(b_self), _ptr(b_neigh), ACT[act], _ptr(h_out), _ptr(norm_out), stride,
                                              _ptr(self_out), self_stride, _stream(H)),
              "kgat_sage_dense_f32")
    return h_out


def dropout_rows(x, drop_p, seed, x2=None):
    """(x + x2) * keep / (1 - p) with the mask of dropout_keep_mask(seed, *x.shape, p) (kgat_dropout_rows_f32)."""
    x = _need(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("x must be (N, d)")
    if x2 is not None:
        x2 = _need(x2, torch.float32, "x2", x.shape)
    out = torch.empty_like(x)
    with _timed("dropout_rows", tuple(x.shape)):
        check(_lib.load().kgat_dropout_rows_f32(x.shape[0], x.shape[1], _ptr(x), _ptr(x2), float(drop_p),
                                                int(seed) & (2 ** 64 - 1), _ptr(out), _stream(x)),
              "kgat_dropout_rows_f32")
    return out


def sage_bwd_input(grad_pre, W_self, W_neigh, indptr):
    """(grad_pre @ W_self, (grad_pre @ W_neigh) / max(deg, 1)) in one pass (kgat_sage_bwd_input_f32)."""
    grad_pre = _need(grad_pre, torch.float32, "grad_pre")
    n, d_out = grad_pre.shape
    W_self = _need(W_self, torch.float32, "W_self")
    d_in = W_self.shape[1]
    if W_self.shape[0] != d_out:
        raise ValueError("W_self has shape %s, expected (%d, *)" % (tuple(W_self.shape), d_out))
    W_neigh = _need(W_neigh, torch.float32, "W_neigh", (d_out, d_in))
    indptr = _need(indptr, torch.int32, "indptr")
    if indptr.numel() < n + 1:
        raise ValueError("indptr has %d entries, expected %d" % (indptr.numel(), n + 1))
    g_self = torch.empty((n, d_in), dtype=torch.float32, device=grad_pre.device)
    g_agg = torch.empty_like(g_self)
    with _timed("sage_bwd_input", (n, d_in, d_out)):
        check(_lib.load().kgat_sage_bwd_input_f32(n, d_in, d_out, _ptr(grad_pre), _ptr(W_self), _ptr(W_neigh),
                                                  _ptr(indptr), _ptr(g_self), _ptr(g_agg), _stream(grad_pre)),
              "kgat_sage_bwd_input_f32")
    return g_self, g_agg


def sage_bwd_weight(grad_pre, H, HN, want_partials=False):
    """(grad_pre^T H, grad_pre^T HN, column sums of grad_pre) (kgat_sage_bwd_weight_f32's partials, summed by
    kgat_sum_partials_f32 - or, want_partials=True, handed back)."""
    grad_pre = _need(grad_pre, torch.float32, "grad_pre")
    n, d_out = grad_pre.shape
    H = _need(H, torch.float32, "H")
    d_in = H.shape[1]
    if H.shape[0] != n:
        raise ValueError("H has %d rows, grad_pre %d" % (H.shape[0], n))
    HN = _need(HN, torch.float32, "HN", (n, d_in))
    lib = _lib.load()
    nb = int(lib.kgat_bi_interaction_bwd_weight_partials(n))
    ps = _scratch((nb, d_out, d_in), torch.float32, H.device)
    pn = _scratch((nb, d_out, d_in), torch.float32, H.device)
    pb = _scratch((nb, d_out), torch.float32, H.device)
    with _timed("sage_bwd_weight", (n, d_in, d_out)):
        check(lib.kgat_sage_bwd_weight_f32(n, d_in, d_out, _ptr(grad_pre), _ptr(H), _ptr(HN), _ptr(ps), _ptr(pn),
                                           _ptr(pb), nb, _stream(H)), "kgat_sage_bwd_weight_f32")
    parts = [ps, pn, pb]
    return parts if want_partials else sum_partials(parts)


def spmm_bi_fused_supported(d_in, d_out):
    return bool(_lib.load().kgat_spmm_bi_fused_supported(int(d_in), int(d_out)))


def spmm_bi_fused(indptr, col, row_of, X, w, W2, negative_slope=0.01, h_out=None, norm_out=None, want_h=True,
                  rows=None, e_range=None, workspace=None, scratch=None, self_out=None):
    """One KGATConv forward in one pass (kgat_spmm_bi_fused_f32; reference models.py:63-66 + :165):
    Z = leaky_relu(((sum_p w_p X[col[p]]) * X[v]) @ W2^T) over the CSR rows `rows`; returns Z (or None with
    want_h=False) and writes Z / ||Z_row|| into `norm_out` (a column slice of a wider row-major buffer).  The
    same bits as spmm(mul_self=True) followed by bi_interaction."""
    X = _need(X, torch.float32, "X")
    W2 = _need(W2, torch.float32, "W2")
    if X.dim() != 2 or W2.dim() != 2 or W2.shape[1] != X.shape[1]:
        raise ValueError("X must be (N, d_in) and W2 (d_out, d_in)")
    d_in, d_out = X.shape[1], W2.shape[0]
    X, indptr, col, row_of, _, (row0, n_rows, e0, e1), _, workspace = _csr_operands(
        X, indptr, col, row_of, None, rows, e_range, workspace, spmm_workspace, want_out=False, need_row_of=True)
    w = _need(w, torch.float32, "w", col.shape)
    if want_h and h_out is None:
        h_out = torch.empty((n_rows, d_out), dtype=torch.float32, device=X.device)
    if h_out is not None:
        h_out = _need(h_out, torch.float32, "h_out", (n_rows, d_out))
    stride = 0
    if norm_out is not None:
        stride = _strided_rows(norm_out, n_rows, d_out, "norm_out")
    self_stride = 0
    if self_out is not None:
        self_stride = _strided_rows(self_out, n_rows, d_in, "self_out")
    if scratch is None:
        scratch = _scratch((n_rows, d_in), torch.float32, X.device)
    else:
        scratch = _need(scratch, torch.float32, "scratch", (n_rows, d_in))
    with _timed("spmm_bi_fused", (e1 - e0, n_rows, d_in, d_out)):
        check(_lib.load().kgat_spmm_bi_fused_f32(n_rows, row0, e0, e1, d_in, d_out, _ptr(indptr), _ptr(col),
                                                 _ptr(row_of), _ptr(X), _ptr(w), _ptr(W2), float(negative_slope),
                                                 _ptr(h_out), _ptr(norm_out), stride, _ptr(scratch), _ptr(workspace),
                                                 workspace.numel(), _ptr(self_out), self_stride, _stream(X)),
              "kgat_spmm_bi_fused_f32")
    return h_out


def bi_interaction_supported(d_in, d_out):
    return bool(_lib.load().kgat_bi_interaction_supported(int(d_in), int(d_out)))


def bi_interaction(P, W2, negative_slope=0.01, h_out=None, norm_out=None, want_h=True):
    """Z = leaky_relu(P @ W2^T); returns Z (next layer's input) and writes Z / ||Z_row|| into
    `norm_out`, which may be a column slice of a wider row-major buffer."""
    P = _need(P, torch.float32, "P")
    W2 = _need(W2, torch.float32, "W2")
    n, d_in = P.shape
    d_out = W2.shape[0]
    if W2.shape[1] != d_in:
        raise ValueError("W2 has shape %s, expected (*, %d)" % (tuple(W2.shape), d_in))
    if want_h and h_out is None:
        h_out = torch.empty((n, d_out), dtype=torch.float32, device=P.device)
    if h_out is not None:
        h_out = _need(h_out, torch.float32, "h_out", (n, d_out))
    stride = 0
    if norm_out is not None:
        if (not norm_out.is_cuda or norm_out.dtype != torch.float32 or tuple(norm_out.shape) != (n, d_out)
                or norm_out.stride(1) != 1):
            raise ValueError("norm_out must be an (n, d_out) float32 device view with unit column stride")
        stride = norm_out.stride(0)
    with _timed("bi_interaction", (n, d_in, d_out)):
        check(_lib.load().kgat_bi_interaction_f32(n, d_in, d_out, _ptr(P), _ptr(W2), float(negative_slope),
                                                  _ptr(h_out), _ptr(norm_out), stride, _stream(P)),
              "kgat_bi_interaction_f32")
    return h_out


def bi_interaction_mul(H, HN, W2, negative_slope=0.01, h_out=None, norm_out=None, want_h=True, self_out=None,
                       deferred=None):
    """Z = leaky_relu((H * HN) @ W2^T): `aggregator` with the "Bi" form."""
    return aggregator(FORMS["Bi"], H, HN, W2, negative_slope, h_out, norm_out, want_h, self_out, deferred)


def _strided_rows(t, n, d, name):
    if (not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, d) or t.stride(1) != 1):
        raise ValueError("%s must be an (n, %d) float32 device view with unit column stride" % (name, d))
    return t.stride(0)


def bi_interaction_train(H, HN, W2, negative_slope, drop_p, seed, norm_out=None, row0=0, self_out=None):
    """Training form of bi_interaction_mul: `aggregator_train` with the "Bi" form."""
    return aggregator_train(FORMS["Bi"], H, HN, W2, negative_slope, drop_p, seed, norm_out, row0, self_out)


def add3_rows(a, b, c):
    """(a + b) + c where `a` is an (n, d) column slice of a wider fp32 matrix and b, c are contiguous (n, d)
    (kgat_add3_rows_f32): the three gradient paths into the embedding table in one pass."""
    b = _need(b, torch.float32, "b")
    c = _need(c, torch.float32, "c", b.shape)
    n, d = b.shape
    stride = _strided_rows(a, n, d, "a")
    out = torch.empty_like(b)
    check(_lib.load().kgat_add3_rows_f32(n, d, _ptr(a), stride, _ptr(b), _ptr(c), _ptr(out), _stream(b)), "kgat_add3_rows_f32")
    return out


def bi_interaction_bwd_pre(h_out, grad_a, grad_b, grad_norm, negative_slope, drop_p, seed, row0=0):
    """grad_z of a one-weight training layer: `aggregator_bwd_pre` without a sign record."""
    return aggregator_bwd_pre(FORMS["Bi"], h_out, None, grad_a, grad_b, grad_norm, negative_slope, drop_p, seed, row0)


def bi_interaction_bwd_input_supported(d_in, d_out):
    return bool(_lib.load().kgat_bi_interaction_bwd_input_supported(int(d_in), int(d_out)))


def bi_interaction_bwd_input(grad_z, W2, H, HN):
    """((grad_z @ W2) * H, (grad_z @ W2) * HN): `aggregator_bwd_input` with the "Bi" form."""
    return aggregator_bwd_input(FORMS["Bi"], grad_z, W2, H, HN)


def sum_partials(partial_sets):
    """[(n_partials, ...) tensor, ...] -> [sum over dim 0, ...] for up to four sets in one launch
    (kgat_sum_partials_f32; a fixed order of additions)."""
    import ctypes as C
    outs = []
    for lo in range(0, len(partial_sets), 4):
        sets = [_need(t, torch.float32, "partials") for t in partial_sets[lo:lo + 4]]
        res = [torch.empty(t.shape[1:], dtype=torch.float32, device=t.device) for t in sets]
        n = len(sets)
        if any(t[0].numel() % 4 for t in sets):
            raise ValueError("sum_partials: partial sizes must be multiples of 4 floats")
        check(_lib.load().kgat_sum_partials_f32(n, (C.c_void_p * n)(*[t.data_ptr() for t in sets]),
                                                (C.c_void_p * n)(*[r.data_ptr() for r in res]),
                                                (C.c_int64 * n)(*[t.shape[0] for t in sets]),
                                                (C.c_int64 * n)(*[t[0].numel() for t in sets]), _stream(sets[0])),
              "kgat_sum_partials_f32")
        outs += res
    return outs


def bi_interaction_bwd_weight(grad_z, H, HN, want_partials=False):
    """grad_W2 = grad_z^T (H * HN): `aggregator_bwd_weight` with the "Bi" form."""
    return aggregator_bwd_weight(FORMS["Bi"], grad_z, H, HN, want_partials)


# The KGAT layer's aggregators (KGATConv res_type; include/kgat_hip.h KGAT_FORM_*): Bi-Interaction LeakyReLU(W (h * h_N)),
# GCN LeakyReLU(W (h + h_N)), GraphSage LeakyReLU(W [h | h_N]) - W is d_out x 2 d_in for GraphSage.
FORMS = {"Bi": 0, "GCN": 1, "GraphSage": 2}
# The KGAT paper's two-term Bi-Interaction (KGATConv res_type "Bi2"): LeakyReLU(W1 (h + h_N)) + LeakyReLU(W2 (h * h_N)),
# W1 = res_fc.weight, W2 = res_fc_2.weight.  The fourth form of the functions below; in the C interface it has entries
# of its own (kgat_bi2_*: two weights and a sign record), so the value is this layer's, not a KGAT_FORM_*.
# Convention: where a one-weight form takes or returns ONE tensor per weight - the weight W, the gradient grad_z, the
# weight gradient - this form takes or returns the pair, (W1, W2), (grad_z1, grad_z2), (grad_W1, grad_W2).
BI2_FORM = 3


def form_weights(form):
    """How many weights a layer of this form has."""
    return 2 if form == BI2_FORM else 1


def _entry(form, suffix):
    """The form's C entry: (function, its leading arguments, its name) - kgat_aggregator_* take the form first,
    kgat_bi2_* have none."""
    name = ("kgat_bi2" if form == BI2_FORM else "kgat_aggregator") + suffix
    return getattr(_lib.load(), name), ([] if form == BI2_FORM else [int(form)]), name


def aggregator_supported(form, d_in, d_out):
    """The widths the form's forward kernels cover (kgat_aggregator_supported / kgat_bi2_supported)."""
    fn, lead, _ = _entry(form, "_supported")
    return bool(fn(*lead, int(d_in), int(d_out)))


def aggregator_bwd_supported(form, d_in, d_out):
    """The widths the form's backward kernels cover (kgat_aggregator_bwd_supported / kgat_bi2_bwd_supported)."""
    fn, lead, _ = _entry(form, "_bwd_supported")
    return bool(fn(*lead, int(d_in), int(d_out)))


def _per_weight(form, x, name):
    """`x` as the list of the form's per-weight tensors: [x], or the pair's two for BI2_FORM (same shape)."""
    if form != BI2_FORM:
        return [_need(x, torch.float32, name)]
    if not (isinstance(x, (tuple, list)) and len(x) == 2):
        raise ValueError("%s: the two-term form takes a pair of tensors" % name)
    first = _need(x[0], torch.float32, name + "1")
    return [first, _need(x[1], torch.float32, name + "2", first.shape)]


def _form_weight(form, W, d_in):
    Ws = _per_weight(form, W, "W")
    k = 2 * d_in if form == FORMS["GraphSage"] else d_in
    if Ws[0].dim() != 2 or Ws[0].shape[1] != k:
        raise ValueError("W has shape %s, expected (*, %d) for form %d" % (tuple(Ws[0].shape), k, form))
    return Ws, Ws[0].shape[0]


def _agg_timed(form, n, d_in, d_out):
    # (Bi under the name and key of ops.bi_interaction: the KernelTimer summaries of the benchmark read that name)
    if form == BI2_FORM:
        return _timed("bi2", (n, d_in, d_out))
    return _timed("bi_interaction", (n, d_in, d_out)) if form == FORMS["Bi"] else _timed("aggregator", (form, n, d_in, d_out))


def aggregator(form, H, HN, W, negative_slope=0.01, h_out=None, norm_out=None, want_h=True, self_out=None,
               deferred=None):
    """Z = leaky_relu(combine(H, HN) @ W^T) with combine = H * HN (form 0), H + HN (1) or [H | HN] (2), or - BI2_FORM,
    W = (W1, W2) - leaky_relu((H + HN) @ W1^T) + leaky_relu((H * HN) @ W2^T)
    (kgat_aggregator_f32 / kgat_bi2_f32): the layer input H and the plain aggregation HN, combined while the rows are
    loaded; `self_out`: an (n, d_in) column slice that also receives H (the ego block of the readout).  Otherwise as
    bi_interaction.  `deferred`: the DeferredRows of the spmm(defer_finish=True) call that produced HN
    (kgat_aggregator_deferred_f32 / kgat_bi2_deferred_f32; same bits)."""
    H = _need(H, torch.float32, "H")
    HN = _need(HN, torch.float32, "HN", H.shape)
    n, d_in = H.shape
    Ws, d_out = _form_weight(form, W, d_in)
    if want_h and h_out is None:
        h_out = torch.empty((n, d_out), dtype=torch.float32, device=H.device)
    if h_out is not None:
        h_out = _need(h_out, torch.float32, "h_out", (n, d_out))
    stride = _strided_rows(norm_out, n, d_out, "norm_out") if norm_out is not None else 0
    self_stride = _strided_rows(self_out, n, d_in, "self_out") if self_out is not None else 0
    args = [n, d_in, d_out, _ptr(H), _ptr(HN), *map(_ptr, Ws), float(negative_slope), _ptr(h_out), _ptr(norm_out), stride,
            _ptr(self_out), self_stride]
    if deferred is not None:
        if deferred.n_rows != n or deferred.D != d_in:
            raise ValueError("deferred rows of a (%d, %d) aggregation with a (%d, %d) input" % (deferred.n_rows, deferred.D, n, d_in))
        args += [_ptr(deferred.indptr_rows), deferred.e_range[0], deferred.e_range[1], _ptr(deferred.workspace),
                 deferred.tile_edges]
    fn, lead, name = _entry(form, "_deferred_f32" if deferred is not None else "_f32")
    with _agg_timed(form, n, d_in, d_out):
        check(fn(*lead, *args, _stream(H)), name)
    return h_out


def aggregator_train(form, H, HN, W, negative_slope, drop_p, seed, norm_out=None, row0=0, self_out=None):
    """Training form of `aggregator`: h_out = dropout_p(leaky_relu(combine(H, HN) @ W^T)) and its normalised copy into
    `norm_out` (kgat_aggregator_train_f32; the mask is a hash of (seed, element); `row0`: the global index of row 0
    when H holds a row range of a larger matrix, so that a destination shard draws the mask the unsharded layer
    draws).  BI2_FORM (kgat_bi2_train_f32) returns (h_out, signs): the dropped sum of the two terms and the (n, d_out)
    uint8 sign record, bit 0 = (z1 > 0), bit 1 = (z2 > 0), that aggregator_bwd_pre reads."""
    H = _need(H, torch.float32, "H")
    HN = _need(HN, torch.float32, "HN", H.shape)
    n, d_in = H.shape
    Ws, d_out = _form_weight(form, W, d_in)
    h_out = torch.empty((n, d_out), dtype=torch.float32, device=H.device)
    signs = [torch.empty((n, d_out), dtype=torch.uint8, device=H.device)] if form == BI2_FORM else []
    stride = _strided_rows(norm_out, n, d_out, "norm_out") if norm_out is not None else 0
    self_stride = _strided_rows(self_out, n, d_in, "self_out") if self_out is not None else 0
    fn, lead, name = _entry(form, "_train_f32")
    with _agg_timed(form, n, d_in, d_out):
        check(fn(*lead, n, d_in, d_out, _ptr(H), _ptr(HN), *map(_ptr, Ws), float(negative_slope), float(drop_p),
                 int(seed) & (2 ** 64 - 1), int(row0), _ptr(h_out), *map(_ptr, signs), _ptr(norm_out), stride,
                 _ptr(self_out), self_stride, _stream(H)), name)
    return (h_out, signs[0]) if signs else h_out


def aggregator_bwd_pre(form, h_out, signs, grad_a, grad_b, grad_norm, negative_slope, drop_p, seed, row0=0):
    """grad_z of the training layer (kgat_bi_interaction_bwd_pre_f32; `signs` is None); grad_a / grad_b / grad_norm
    may be None; `row0` as in aggregator_train.  BI2_FORM (kgat_bi2_bwd_pre_f32): (grad_z1, grad_z2) - that gradient
    times LeakyReLU'(z1) and times LeakyReLU'(z2), the slopes from aggregator_train's sign record."""
    h_out = _need(h_out, torch.float32, "h_out")
    n, d = h_out.shape
    two = form == BI2_FORM
    if two:
        signs = _need(signs, torch.uint8, "signs", (n, d))
    for name, t in (("grad_a", grad_a), ("grad_b", grad_b)):
        if t is not None:
            _need(t, torch.float32, name, (n, d))
    stride = _strided_rows(grad_norm, n, d, "grad_norm") if grad_norm is not None else 0
    gz = [torch.empty_like(h_out) for _ in range(form_weights(form))]
    name = "kgat_bi2_bwd_pre_f32" if two else "kgat_bi_interaction_bwd_pre_f32"
    check(getattr(_lib.load(), name)(n, d, _ptr(h_out), *([_ptr(signs)] if two else []), _ptr(grad_a), _ptr(grad_b),
                                     _ptr(grad_norm), stride, float(negative_slope), float(drop_p),
                                     int(seed) & (2 ** 64 - 1), int(row0), *map(_ptr, gz), _stream(h_out)), name)
    return tuple(gz) if two else gz[0]


def _bwd_operands(form, grad_z, H, HN):
    gzs = _per_weight(form, grad_z, "grad_z")
    n, d_out = gzs[0].shape
    H = _need(H, torch.float32, "H")
    if H.shape[0] != n:
        raise ValueError("H has %d rows, grad_z %d" % (H.shape[0], n))
    HN = _need(HN, torch.float32, "HN", H.shape)
    return gzs, H, HN, n, H.shape[1], d_out


def aggregator_bwd_input(form, grad_z, W, H, HN):
    """(grad_agg, grad_self) of the form's dense part (kgat_aggregator_bwd_input_f32): what the reversed-CSR aggregation
    sums and what goes to h directly - (grad_P * H, grad_P * HN) for Bi, (grad_P, grad_P) - one tensor - for GCN,
    (grad_P[:, d_in:], grad_P[:, :d_in]) for GraphSage, grad_P = grad_z @ W.  BI2_FORM (kgat_bi2_bwd_input_f32):
    (P1 + P2 * H, P1 + P2 * HN) with P1 = grad_z1 @ W1, P2 = grad_z2 @ W2 in one pass."""
    gzs, H, HN, n, d_in, d_out = _bwd_operands(form, grad_z, H, HN)
    Ws, wd = _form_weight(form, W, d_in)
    if wd != d_out:
        raise ValueError("W has shape %s, expected (%d, *)" % (tuple(Ws[0].shape), d_out))
    t = torch.empty_like(H)
    gb = t if form == FORMS["GCN"] else torch.empty_like(H)
    fn, lead, name = _entry(form, "_bwd_input_f32")
    check(fn(*lead, n, d_in, d_out, *map(_ptr, gzs), *map(_ptr, Ws), _ptr(H), _ptr(HN), _ptr(t),
             _ptr(None if gb is t else gb), _stream(H)), name)
    return t, gb


def aggregator_bwd_weight(form, grad_z, H, HN, want_partials=False):
    """grad_W of the form's dense part (kgat_aggregator_bwd_weight_f32: per-workgroup partials over 64-row slabs,
    d_out x 2 d_in for GraphSage, the combination formed on the way; the partials are added here in index order - or,
    want_partials=True, handed back for sum_partials, which sums several layers' sets in one launch).  BI2_FORM
    (kgat_bi2_bwd_weight_f32): the pair (grad_z1^T (H + HN), grad_z2^T (H * HN)), H and HN read once for both."""
    gzs, H, HN, n, d_in, d_out = _bwd_operands(form, grad_z, H, HN)
    nb = int(_lib.load().kgat_bi_interaction_bwd_weight_partials(n))
    k = 2 * d_in if form == FORMS["GraphSage"] else d_in
    partials = [_scratch((nb, d_out, k), torch.float32, H.device) for _ in gzs]
    fn, lead, name = _entry(form, "_bwd_weight_f32")
    check(fn(*lead, n, d_in, d_out, *map(_ptr, gzs), _ptr(H), _ptr(HN), *map(_ptr, partials), nb, _stream(H)), name)
    res = partials if want_partials else [p.sum(0) for p in partials]
    return tuple(res) if form == BI2_FORM else res[0]


def mul2(a, b, c):
    """(a * b, a * c) in one pass."""
    a = _need(a, torch.float32, "a")
    b = _need(b, torch.float32, "b", a.shape)
    c = _need(c, torch.float32, "c", a.shape)
    ab, ac = torch.empty_like(a), torch.empty_like(a)
    check(_lib.load().kgat_mul2_f32(a.numel(), _ptr(a), _ptr(b), _ptr(c), _ptr(ab), _ptr(ac), _stream(a)), "kgat_mul2_f32")
    return ab, ac


def dropout_keep_mask(seed, n_rows, d, drop_p, row0=0):
    """The mask kgat_aggregator_train_f32 applies, restated in numpy (tests): element (row, col)
    is kept iff murmur3-finalised (((row0 + row)*d + col) * 0x9E3779B1 ^ seed32) >= p * 2^32."""
    import numpy as np
    seed = int(seed) & (2 ** 64 - 1)
    seed32 = np.uint32((seed ^ (seed >> 32)) & 0xFFFFFFFF)
    x = ((np.arange(n_rows * d, dtype=np.uint64) + np.uint64(int(row0) * d)) * np.uint64(0x9E3779B1)).astype(np.uint32) ^ seed32
    x ^= x >> np.uint32(16)
    x = (x.astype(np.uint64) * np.uint64(0x85EBCA6B)).astype(np.uint32)
    x ^= x >> np.uint32(13)
    x = (x.astype(np.uint64) * np.uint64(0xC2B2AE35)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    t = min(int(float(np.float32(drop_p)) * 4294967296.0), 0xFFFFFFFF)
    return (x >= np.uint32(t)).reshape(n_rows, d)


NORM_MODES = {"si": 0, "bi": 1}  # include/kgat_hip.h: KGAT_NORM_SI, KGAT_NORM_BI


def edge_norm(csr, out_indptr, mode, want_eid=True):
    """Laplacian edge weights from the device CSR (kgat_edge_norm_f32): (w_csr, w_eid), both (E,); w_eid (edge-id order)
    is None unless asked for.  `csr`: the destination-major (indptr, col, eid, row_of); `mode` "si": 1 / indeg(dst);
    "bi": 1 / sqrt(outdeg(src) * indeg(dst)) with `out_indptr` the reversed CSR's indptr (None for "si")."""
    if mode not in NORM_MODES:
        raise ValueError("edge_norm: mode must be 'si' or 'bi', got %r" % (mode,))
    indptr = _need(csr.indptr, torch.int32, "indptr")
    n, e = indptr.numel() - 1, csr.row_of.numel()
    row_of = _need(csr.row_of, torch.int32, "row_of")
    col = _need(csr.col, torch.int32, "col", (e,))
    eid = _need(csr.eid, torch.int32, "eid", (e,))
    if mode == "bi":
        if out_indptr is None:
            raise ValueError("edge_norm: mode 'bi' needs the reversed CSR's indptr")
        out_indptr = _need(out_indptr, torch.int32, "out_indptr", (n + 1,))
    else:
        out_indptr = None
    w_csr = torch.empty(e, dtype=torch.float32, device=indptr.device)
    w_eid = torch.empty(e, dtype=torch.float32, device=indptr.device) if want_eid else None
    with _timed("edge_norm", (e, mode)):
        check(_lib.load().kgat_edge_norm_f32(n, e, _ptr(indptr), _ptr(row_of), _ptr(col), _ptr(eid), _ptr(out_indptr),
                                             NORM_MODES[mode], _ptr(w_csr), _ptr(w_eid), _stream(indptr)),
              "kgat_edge_norm_f32")
    return w_csr, w_eid


def edge_dropout(w, key, p, seed):
    """Node dropout's dropped copy of a weight stream (kgat_edge_dropout_f32): w * keep / (1 - p) with
    keep = edge_keep_mask(seed, E, p)[key].  `key`: the edge id at every position of `w` - csr.eid of the CSR `w` is
    ordered by - or None for a stream in edge-id order.  `w` (E,) or (E,1), any 4-byte aligned start."""
    w = _need(w, torch.float32, "w")
    e = w.numel()
    if key is not None:
        key = _need(key, torch.int32, "key", (e,))
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("edge_dropout: p must be in [0, 1), got %r" % (p,))
    out = torch.empty_like(w)
    with _timed("edge_dropout", (e,)):
        check(_lib.load().kgat_edge_dropout_f32(e, _ptr(w), _ptr(key), float(p), int(seed) & (2 ** 64 - 1), _ptr(out),
                                                _stream(w)), "kgat_edge_dropout_f32")
    return out


def edge_keep_mask(seed, n_edges, p):
    """The edges node dropout keeps, by edge id, restated in numpy (tests): dropout_keep_mask over (row = edge id,
    d = 1, column 0)."""
    return dropout_keep_mask(seed, n_edges, 1, p).reshape(-1)


def l2_normalize_rows(x, out):
    """out[:, :] = x / max(||x_row||, 1e-12); `out` may be a column slice of a wider buffer."""
    x = _need(x, torch.float32, "x")
    if (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape) or out.stride(1) != 1):
        raise ValueError("out must be a float32 device view of x's shape with unit column stride")
    check(_lib.load().kgat_l2_normalize_rows_f32(x.shape[0], x.shape[1], _ptr(x), _ptr(out), out.stride(0), _stream(x)),
          "kgat_l2_normalize_rows_f32")
    return out


def readout_concat(blocks, normalize, out=None):
    """[b0 | b1 | ...] with the blocks flagged in `normalize` L2-normalised per row
    (kgat_readout_concat_f32): the readout of Model.gnn from separately held layer outputs."""
    import ctypes as C
    n = blocks[0].shape[0]
    widths = []
    for i, b in enumerate(blocks):
        _need(b, torch.float32, "blocks[%d]" % i)
        if b.dim() != 2 or b.shape[0] != n:
            raise ValueError("blocks must be (n, w_i) matrices with the same n")
        widths.append(int(b.shape[1]))
    if out is None:
        out = torch.empty((n, sum(widths)), dtype=torch.float32, device=blocks[0].device)
    else:
        out = _need(out, torch.float32, "out", (n, sum(widths)))
    k = len(blocks)
    ptrs = (C.c_void_p * k)(*[b.data_ptr() for b in blocks])
    w_arr = (C.c_int * k)(*widths)
    f_arr = (C.c_int * k)(*[1 if f else 0 for f in normalize])
    check(_lib.load().kgat_readout_concat_f32(n, k, ptrs, w_arr, f_arr, _ptr(out), out.stride(0), _stream(out)),
          "kgat_readout_concat_f32")
    return out


def gather_probe(col, X, sink=None):
    """Measurement aid (kgat_gather_probe_f32): fetch the rows X[col[p]] with the aggregation's access pattern and
    do nothing else; returns the scratch so a caller timing many launches can pass it back in."""
    X = _need(X, torch.float32, "X")
    col = _need(col, torch.int32, "col")
    if sink is None:
        sink = torch.zeros(((col.numel() + 2047) // 2048 * 4 + 4) * 4, dtype=torch.float32, device=X.device)
    with _timed("gather_probe", (col.numel(), X.shape[1])):
        check(_lib.load().kgat_gather_probe_f32(col.numel(), X.shape[1], _ptr(col), _ptr(X), _ptr(sink), _stream(X)),
              "kgat_gather_probe_f32")
    return sink


def sddmm_dot(src, dst, X, G):
    X = _need(X, torch.float32, "X")
    G = _need(G, torch.float32, "grad_out")
    src = _need(src, torch.int32, "src")
    dst = _need(dst, torch.int32, "dst", src.shape)
    if X.shape[1] != G.shape[1]:
        raise ValueError("feature widths differ")
    out = torch.empty(src.numel(), dtype=torch.float32, device=X.device)
    check(_lib.load().kgat_sddmm_dot_f32(src.numel(), X.shape[1], _ptr(src), _ptr(dst), _ptr(X), _ptr(G),
                                         _ptr(out), _stream(X)), "kgat_sddmm_dot_f32")
    return out


__all__ = ["csr_from_coo", "group_by_relation", "invert_permutation", "row_order_by_degree", "gather",
           "permute_tile", "permute_supported", "permute_plan_arrays", "permute_plan", "permute", "PermutePlan",
           "att_score", "att_score_split", "att_score_split_supported", "att_score_folded_supported", "att_score_fused", "att_pack_records", "att_score_fused_supported", "fold_tiles", "fold_tile_cost", "bi_interaction_train", "add3_rows", "bi_interaction_bwd_pre", "bi_interaction_bwd_input", "bi_interaction_bwd_input_supported", "bi_interaction_bwd_weight", "sum_partials", "mul2", "dropout_keep_mask", "transr_loss_grad", "transr_supported", "transr_presort", "transr_adam_step", "TransRAdamState", "head_groups", "edge_softmax", "edge_softmax_permuted", "edge_softmax_permuted_supported", "edge_softmax_bwd", "spmm", "spmm_workspace", "sddmm_dot",
           "bi_interaction", "bi_interaction_supported", "l2_normalize_rows", "readout_concat",
           "FORMS", "aggregator", "aggregator_supported", "aggregator_bwd_supported", "aggregator_train",
           "aggregator_bwd_input", "aggregator_bwd_weight",
           "KGATLibraryError"]


def eval_supported(F, K):
    return bool(_lib.load().kgat_eval_supported(int(F), int(K)))


def _eval_args(who, emb, user_ids, item_ids, train_ptr, train_items, test_ptr=None, test_items=None):
    """The arguments the evaluation wrappers share, checked (`who` names the wrapper in the message; the test lists are
    optional).  Returns (F, stride, n_users, n_items)."""
    if emb.dtype != torch.float32 or not emb.is_cuda or emb.dim() != 2 or emb.stride(1) != 1:
        raise KGATLibraryError("%s: `emb` must be a float32 HIP matrix with unit column stride" % who)
    _need(user_ids, torch.int32, "user_ids")
    _need(item_ids, torch.int32, "item_ids")
    n_users, n_items = user_ids.numel(), item_ids.numel()
    _need(train_ptr, torch.int32, "train_ptr", (n_users + 1,))
    if test_ptr is not None:
        _need(test_ptr, torch.int32, "test_ptr", (n_users + 1,))
    _need(train_items, torch.int32, "train_items")
    if test_items is not None:
        _need(test_items, torch.int32, "test_items")
    return emb.shape[1], emb.stride(0), n_users, n_items


def _eval_items(lib, emb, item_ids):
    """itemT: the item rows as the MFMA A fragments of the sweeps (kgat_eval_items_kmajor_f32)."""
    n_items, F = item_ids.numel(), emb.shape[1]
    itemT = torch.empty(max(int(lib.kgat_eval_items_elems(n_items, F)), 1), dtype=torch.float32, device=emb.device)
    with _timed("eval_items_kmajor", (n_items, F)):
        check(lib.kgat_eval_items_kmajor_f32(n_items, F, _ptr(emb), emb.stride(0), _ptr(item_ids), _ptr(itemT),
                                             _stream(emb)), "kgat_eval_items_kmajor_f32")
    return itemT


def _discounts(n, dev):
    """1 / log2(rank + 1) of the ranks 1 .. n, float64 (reference metric.py:23-34)."""
    import numpy as np
    return torch.as_tensor(1.0 / np.log2(np.arange(2, n + 2)), dtype=torch.float64, device=dev)


def _eval_cutoffs(who, ks, most, bad, limit=None):
    """`ks` as ints and as the C array, checked: 1 to `most` cut-offs, positive, ascending and (with `limit`) none
    beyond it; `bad` words the second refusal around the list."""
    import ctypes
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= most:
        raise ValueError("%s: 1 to %d cut-offs, got %d" % (who, most, len(ks)))
    if any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 1 or (limit is not None and ks[-1] > limit):
        raise ValueError("%s: %s" % (who, bad % (ks,)))
    return ks, ctypes.cast((ctypes.c_int32 * len(ks))(*ks), ctypes.c_void_p)


def eval_recall_ndcg(emb, user_ids, item_ids, train_ptr, train_items, test_ptr, test_items, K, want_topk=False):
    """recall@K / ndcg@K per test user (reference metric.py:36-68) on the device: kgat_eval_items_kmajor_f32 +
    kgat_eval_recall_ndcg_f32.  `emb` (N, F) fp32 rows (row stride = emb.stride(0)); user_ids / item_ids int32 node
    ids; the CSR lists hold item POSITIONS (ascending per user).  Returns (recall, ndcg[, topk]) - float64 (n_users,)
    and int32 (n_users, K)."""
    F, stride, n_users, n_items = _eval_args("eval_recall_ndcg", emb, user_ids, item_ids, train_ptr, train_items,
                                             test_ptr, test_items)
    lib = _lib.load()
    if not lib.kgat_eval_supported(F, K):
        raise KGATLibraryError("eval_recall_ndcg: K = %d / F = %d outside the kernel's range" % (K, F))
    dev = emb.device
    disc = _discounts(K, dev)
    recall = torch.empty(n_users, dtype=torch.float64, device=dev)   # (the merge launch writes every user)
    ndcg = torch.empty(n_users, dtype=torch.float64, device=dev)
    topk = torch.empty((n_users, K), dtype=torch.int32, device=dev) if want_topk else None
    if n_users == 0:
        return (recall, ndcg, topk) if want_topk else (recall, ndcg)
    ws = _workspace(lib.kgat_eval_workspace_bytes(n_users, n_items, F, K), dev)
    itemT = _eval_items(lib, emb, item_ids)
    with _timed("eval_recall_ndcg", (n_users, n_items, F, K)):
        check(lib.kgat_eval_recall_ndcg_f32(n_users, _ptr(user_ids), n_items, F, _ptr(emb), stride, _ptr(itemT),
                                            _ptr(train_ptr), _ptr(train_items), _ptr(test_ptr), _ptr(test_items), K,
                                            _ptr(disc), _ptr(ws), ws.numel(), _ptr(recall), _ptr(ndcg),
                                            _ptr(topk) if want_topk else None, _stream(emb)),
              "kgat_eval_recall_ndcg_f32")
    return (recall, ndcg, topk) if want_topk else (recall, ndcg)


def eval_topk_supported(F, K):
    return bool(_lib.load().kgat_eval_topk_supported(int(F), int(K)))


def eval_topk(emb, user_ids, item_ids, train_ptr, train_items, K, drop_train=False, want_scores=True):
    """The K best items of every user in rank order (reference metric.py:48-51), 1 <= K <= 128, on the device:
    kgat_eval_items_kmajor_f32 + kgat_eval_topk_f32.  Arguments as eval_recall_ndcg.  drop_train=False is the
    reference's rule (a training item scores 0.0 and can rank; needs n_items >= K); drop_train=True never lists a
    training item and pads a short list.  Returns (topk[, scores]) - int32 item POSITIONS (n_users, K), -1 padding,
    and float32 scores, -inf padding."""
    F, stride, n_users, n_items = _eval_args("eval_topk", emb, user_ids, item_ids, train_ptr, train_items)
    K = int(K)
    lib = _lib.load()
    if not lib.kgat_eval_topk_supported(F, K):
        raise KGATLibraryError("eval_topk: K = %d / F = %d outside the kernel's range" % (K, F))
    dev = emb.device
    topk = torch.empty((n_users, K), dtype=torch.int32, device=dev)
    scores = torch.empty((n_users, K), dtype=torch.float32, device=dev) if want_scores else None
    if n_users == 0:
        return (topk, scores) if want_scores else topk
    ws = _workspace(lib.kgat_eval_topk_workspace_bytes(n_users, n_items, F, K), dev)
    itemT = _eval_items(lib, emb, item_ids)
    with _timed("eval_topk", (n_users, n_items, F, K)):
        check(lib.kgat_eval_topk_f32(n_users, _ptr(user_ids), n_items, F, _ptr(emb), stride, _ptr(itemT),
                                     _ptr(train_ptr), _ptr(train_items), K, 1 if drop_train else 0, _ptr(ws),
                                     ws.numel(), _ptr(topk), _ptr(scores) if want_scores else None, _stream(emb)),
              "kgat_eval_topk_f32")
    return (topk, scores) if want_scores else topk


def eval_metrics_at_ks(topk, test_ptr, test_items, ks):
    """recall / ndcg / precision / hit ratio of ranked lists at the ascending cut-offs `ks` (at most 8, each <= the
    lists' width; reference metric.py:52-63 per cut-off) - kgat_eval_metrics_at_ks.  `topk` int32 (n_users, K) item
    positions (-1 never hits), the test lists as in eval_recall_ndcg.  Returns float64 (n_users, len(ks), 4)."""
    if topk.dtype != torch.int32 or not topk.is_cuda or topk.dim() != 2 or not topk.is_contiguous():
        raise KGATLibraryError("eval_metrics_at_ks: `topk` must be a contiguous int32 HIP matrix")
    n_users, K = topk.shape
    ks, ks_host = _eval_cutoffs("eval_metrics_at_ks", ks, 8, "the cut-offs must ascend within 1..%d: %%r" % K, K)
    test_ptr = _need(test_ptr, torch.int32, "test_ptr", (n_users + 1,))
    test_items = _need(test_items, torch.int32, "test_items")
    dev = topk.device
    disc = _discounts(K, dev)
    out = torch.zeros((n_users, len(ks), 4), dtype=torch.float64, device=dev)
    with _timed("eval_metrics_at_ks", (n_users, K, len(ks))):
        check(_lib.load().kgat_eval_metrics_at_ks(n_users, K, _ptr(topk), _ptr(test_ptr), _ptr(test_items), len(ks),
                                                  ks_host, _ptr(disc), _ptr(out), _stream(topk)),
              "kgat_eval_metrics_at_ks")
    return out


def eval_rank_supported(F):
    return bool(_lib.load().kgat_eval_rank_supported(int(F)))


def eval_rank(emb, user_ids, item_ids, train_ptr, train_items, test_ptr, test_items, drop_train=False,
              want_scores=False):
    """The number of candidates that rank before every test entry (reference metric.py:48-51 read from the other side:
    the place of each held-out item in the descending sort, at any depth) - kgat_eval_items_kmajor_f32 +
    kgat_eval_rank_f32.  Arguments as eval_recall_ndcg; drop_train as eval_topk (False: a training item is a candidate
    at score 0.0; True: it is none, and a test entry that is a training item gets -1).  Returns (above[, scores]) -
    int32 (n_test,) in test-CSR order, the rank is above + 1, and the float32 scores of the test entries."""
    F, stride, n_users, n_items = _eval_args("eval_rank", emb, user_ids, item_ids, train_ptr, train_items, test_ptr,
                                             test_items)
    n_train, n_test = train_items.numel(), test_items.numel()
    lib = _lib.load()
    if not lib.kgat_eval_rank_supported(F):
        raise KGATLibraryError("eval_rank: F = %d outside the kernel's range" % F)
    dev = emb.device
    above = torch.empty(n_test, dtype=torch.int32, device=dev)       # (the entry clears it on the stream)
    scores = torch.empty(n_test, dtype=torch.float32, device=dev) if want_scores else None
    if n_users == 0 or n_test == 0:
        return (above, scores) if want_scores else above
    ws = _workspace(lib.kgat_eval_rank_workspace_bytes(n_users, n_items, F, n_train, n_test), dev)
    itemT = _eval_items(lib, emb, item_ids)
    with _timed("eval_rank", (n_users, n_items, F, n_test)):
        check(lib.kgat_eval_rank_f32(n_users, _ptr(user_ids), n_items, F, _ptr(emb), stride, _ptr(itemT),
                                     _ptr(train_ptr), _ptr(train_items), n_train, _ptr(test_ptr), _ptr(test_items),
                                     n_test, 1 if drop_train else 0, _ptr(ws), ws.numel(), _ptr(above),
                                     _ptr(scores) if want_scores else None, _stream(emb)), "kgat_eval_rank_f32")
    return (above, scores) if want_scores else above


EVAL_RANK_MAX_KS = 64


def eval_rank_metrics(above, test_ptr, test_items, n_candidates, ks, n_items=None):
    """recall / ndcg / precision / hit ratio at the ascending cut-offs `ks` (at most 64, each within 1..n_items) and
    mrr / ap / auc / mean rank per user from eval_rank's counts - kgat_eval_rank_metrics.  `n_candidates`: the number
    of items a user's test entries were ranked among - an int (every user: n_items, the mask rule) or int32
    (n_users,) (n_items - |train(u)| under drop_train); `n_items` defaults to the largest of them.  Returns
    (at_k, scalar): float64 (n_users, len(ks), 4) and (n_users, 4)."""
    if above.dtype != torch.int32 or not above.is_cuda or above.dim() != 1 or not above.is_contiguous():
        raise KGATLibraryError("eval_rank_metrics: `above` must be a contiguous int32 HIP vector")
    test_ptr = _need(test_ptr, torch.int32, "test_ptr")
    n_users = test_ptr.numel() - 1
    if n_users < 0:
        raise ValueError("eval_rank_metrics: test_ptr is empty")
    test_items = _need(test_items, torch.int32, "test_items", (above.numel(),))
    if not isinstance(n_candidates, torch.Tensor):
        n_items = int(n_candidates) if n_items is None else int(n_items)
        n_candidates = torch.full((n_users,), int(n_candidates), dtype=torch.int32, device=above.device)
    n_candidates = _need(n_candidates, torch.int32, "n_candidates", (n_users,))
    ks, ks_host = _eval_cutoffs("eval_rank_metrics", ks, EVAL_RANK_MAX_KS,
                                "the cut-offs must be positive and ascend: %r")
    dev = above.device
    if n_items is None:
        n_items = int(n_candidates.max()) if n_users else ks[-1]
    if ks[-1] > n_items:
        raise ValueError("eval_rank_metrics: cut-off %d is beyond the %d items" % (ks[-1], n_items))
    disc = _discounts(ks[-1], dev)
    at_k = torch.empty((n_users, len(ks), 4), dtype=torch.float64, device=dev)   # (every word is written)
    scalar = torch.empty((n_users, 4), dtype=torch.float64, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.kgat_eval_rank_metrics_workspace_bytes(above.numel()), dev)
    with _timed("eval_rank_metrics", (n_users, above.numel(), len(ks))):
        check(lib.kgat_eval_rank_metrics(n_users, n_items, _ptr(above), _ptr(test_ptr), _ptr(test_items), above.numel(),
                                         _ptr(n_candidates), len(ks), ks_host, _ptr(disc), _ptr(ws), ws.numel(),
                                         _ptr(at_k), _ptr(scalar), _stream(above)), "kgat_eval_rank_metrics")
    return at_k, scalar


# ---------------------------------------------------------------- TransR link prediction (models.py:120-126)
def transr_project_supported(d, k):
    return bool(_lib.load().kgat_transr_project_supported(int(d), int(k)))


def transr_rank_supported(k):
    return bool(_lib.load().kgat_transr_rank_supported(int(k)))


def transr_project(ent, W_r, rel_row=None, sign=1.0, ids=None, rows=None, want_n2=True, out=None, n2_out=None):
    """normalise(ent[rows] W_r) + sign * normalise(rel_row) per row (kgat_transr_project_f32; the normalisation is
    x / max(|x|, 1e-12), the training kernel's).  `ent` (N, d), `W_r` (d, k); the rows are `ids` (int32 entity ids) or
    the contiguous range `rows = (lo, hi)` (default: all of ent); rel_row None: the pure projection.  Returns
    (out (n, k), n2 (n,)) - n2 the squared norm of the normalised projection (None with want_n2=False); `out` / `n2_out`: buffers to write them into.  Widths outside
    transr_project_supported raise KGATLibraryError (kg_eval restates them in torch)."""
    if not isinstance(ent, torch.Tensor) or not isinstance(W_r, torch.Tensor):
        raise TypeError("ent and W_r must be torch.Tensors")
    if ent.dtype != torch.float32 or W_r.dtype != torch.float32:
        raise TypeError("ent and W_r must be torch.float32, got %s and %s" % (ent.dtype, W_r.dtype))
    if ent.dim() != 2 or W_r.dim() != 2 or W_r.shape[0] != ent.shape[1]:
        raise ValueError("transr_project: ent (N, d) and W_r (d, k), got %s and %s" % (tuple(ent.shape), tuple(W_r.shape)))
    if float(sign) not in (1.0, -1.0):
        raise ValueError("transr_project: sign must be +1 or -1, got %r" % (sign,))
    if ids is not None and rows is not None:
        raise ValueError("transr_project: give `ids` or `rows`, not both")
    n_ent, d = ent.shape
    k = W_r.shape[1]
    if ids is not None:
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1:
            raise TypeError("ids must be a 1-d torch.int32 tensor")
        n, row0 = ids.numel(), 0
        if n and (int(ids.min()) < 0 or int(ids.max()) >= n_ent):
            raise IndexError("transr_project: ids outside [0, %d)" % n_ent)
    else:
        lo, hi = (0, n_ent) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi <= n_ent:
            raise IndexError("transr_project: rows (%d, %d) outside [0, %d]" % (lo, hi, n_ent))
        n, row0 = hi - lo, lo
    ent = _need(ent, torch.float32, "ent")
    W_r = _need(W_r, torch.float32, "W_r")
    if rel_row is not None:
        rel_row = _need(rel_row, torch.float32, "rel_row", (k,))
    if ids is not None:
        ids = _need(ids, torch.int32, "ids")
    lib = _lib.load()
    if not lib.kgat_transr_project_supported(d, k):
        raise KGATLibraryError("transr_project: widths %d -> %d outside the kernel's {16, 32, 64, 128}" % (d, k))
    out = torch.empty((n, k), dtype=torch.float32, device=ent.device) if out is None else \
        _need(out, torch.float32, "out", (n, k))
    if want_n2:
        n2 = torch.empty(n, dtype=torch.float32, device=ent.device) if n2_out is None else \
            _need(n2_out, torch.float32, "n2_out", (n,))
    else:
        n2 = None
    with _timed("transr_project", (n, d, k)):
        check(lib.kgat_transr_project_f32(n, n_ent, d, k, _ptr(ent), _ptr(ids), row0, _ptr(W_r), _ptr(rel_row),
                                          float(sign), _ptr(out), _ptr(n2), _stream(ent)), "kgat_transr_project_f32")
    return out, n2


def check_rank_lists(t, c0, n_c, filter_ptr, filter_ids):
    """What kgat_transr_rank_f32 leaves to its caller, on any device: every t inside [c0, c0 + n_c), filter_ptr from 0
    to len(filter_ids) without a decrease, every query's filter ids strictly ascending.  One host read."""
    n_q = t.numel()
    if filter_ptr.numel() != n_q + 1:
        raise ValueError("filter_ptr has %d entries, expected n_q + 1 = %d" % (filter_ptr.numel(), n_q + 1))
    bad_t = ((t < c0) | (t >= c0 + n_c)).any()
    ptr = filter_ptr.long()
    bad_ptr = (ptr[0] != 0) | (ptr[-1] != filter_ids.numel()) | (ptr[1:] < ptr[:-1]).any()
    flags = [bool(x) for x in torch.stack([bad_t, bad_ptr]).tolist()]
    if flags[0]:
        raise IndexError("transr_rank: a true answer `t` lies outside the candidate range [%d, %d)" % (c0, c0 + n_c))
    if flags[1]:
        raise ValueError("transr_rank: filter_ptr must run from 0 to len(filter_ids) without a decrease")
    if filter_ids.numel() > 1:
        # a descent (or a repeat) is allowed only where a new query's list begins
        starts = torch.zeros(filter_ids.numel() + 1, dtype=torch.bool, device=filter_ids.device)
        starts[ptr] = True
        if bool(((filter_ids[1:] <= filter_ids[:-1]) & ~starts[1:-1]).any()):
            raise ValueError("transr_rank: the filter ids of a query must be sorted (strictly ascending)")


def transr_rank(Q, t, P, n2, c0, filter_ptr, filter_ids):
    """Filtered rank counts (kgat_transr_rank_f32): queries `Q` (n_q, k) with the entity ids `t` of their true answers,
    candidates `P` (n_c, k) / `n2` (n_c,) = the entities [c0, c0 + n_c), per query the sorted ids
    filter_ids[filter_ptr[j]:filter_ptr[j + 1]] to leave out (the true answer always is).  Returns int32 (lt, eq): the
    candidates with n2_i - 2 Q_j . P_i below / equal to the true answer's.  Exact integer sums: bitwise reproducible."""
    for x, name, dt, nd in ((Q, "Q", torch.float32, 2), (t, "t", torch.int32, 1), (P, "P", torch.float32, 2),
                            (n2, "n2", torch.float32, 1), (filter_ptr, "filter_ptr", torch.int32, 1),
                            (filter_ids, "filter_ids", torch.int32, 1)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if x.dtype != dt:
            raise TypeError("%s must be %s, got %s" % (name, dt, x.dtype))
        if x.dim() != nd:
            raise ValueError("%s must have %d dimension(s), got shape %s" % (name, nd, tuple(x.shape)))
    n_q, k = Q.shape
    n_c, c0 = P.shape[0], int(c0)
    if P.shape[1] != k or n2.numel() != n_c or t.numel() != n_q:
        raise ValueError("transr_rank: Q (n_q, k), t (n_q,), P (n_c, k), n2 (n_c,): got %s, %s, %s, %s"
                         % (tuple(Q.shape), tuple(t.shape), tuple(P.shape), tuple(n2.shape)))
    if n_q < 1 or n_c < 1 or c0 < 0:
        raise ValueError("transr_rank: needs n_q, n_c >= 1 and c0 >= 0")
    check_rank_lists(t, c0, n_c, filter_ptr, filter_ids)
    Q, P, n2 = _need(Q, torch.float32, "Q"), _need(P, torch.float32, "P"), _need(n2, torch.float32, "n2")
    t = _need(t, torch.int32, "t")
    filter_ptr, filter_ids = _need(filter_ptr, torch.int32, "filter_ptr"), _need(filter_ids, torch.int32, "filter_ids")
    lib = _lib.load()
    if not lib.kgat_transr_rank_supported(k):
        raise KGATLibraryError("transr_rank: width %d outside the kernel's {16, 32, 64, 128}" % k)
    lt = torch.empty(n_q, dtype=torch.int32, device=Q.device)
    eq = torch.empty(n_q, dtype=torch.int32, device=Q.device)
    with _timed("transr_rank", (n_q, n_c, k)):
        check(lib.kgat_transr_rank_f32(n_q, n_c, c0, k, _ptr(Q), _ptr(t), _ptr(P), _ptr(n2), _ptr(filter_ptr),
                                       _ptr(filter_ids) if filter_ids.numel() else None, filter_ids.numel(), _ptr(lt),
                                       _ptr(eq), _stream(Q)), "kgat_transr_rank_f32")
    return lt, eq


def bpr_loss(emb, u, p, n, reg_lambda, out=None):
    """BPR loss of reference models.py:170-178 on the readout (kgat_bpr_loss_f32).  Returns (loss (0-dim), coef (B,),
    workspace) - the last two feed bpr_grad.  `out` = such a triple of an earlier call with the same batch and width:
    its buffers are written again."""
    if emb.dtype != torch.float32 or not emb.is_cuda or emb.dim() != 2 or emb.stride(1) != 1:
        raise KGATLibraryError("bpr_loss: `emb` must be a float32 HIP matrix with unit column stride")
    u, p, n = (_need(t, torch.int32, name) for t, name in ((u, "u"), (p, "p"), (n, "n")))
    b = u.numel()
    if p.numel() != b or n.numel() != b or b < 1:
        raise ValueError("bpr_loss: the three id lists must have one common, non-zero length")
    lib = _lib.load()
    if out is not None:
        loss, coef, ws = out
        _need(coef, torch.float32, "coef", (b,))
    else:
        loss = torch.empty((), dtype=torch.float32, device=emb.device)
        coef = torch.empty(b, dtype=torch.float32, device=emb.device)
        ws = _workspace(lib.kgat_bpr_workspace_bytes(b, emb.shape[1]), emb.device)
    with _timed("bpr_loss", (b, emb.shape[1])):
        check(lib.kgat_bpr_loss_f32(emb.shape[0], emb.shape[1], _ptr(emb), emb.stride(0), b, _ptr(u), _ptr(p), _ptr(n),
                                    float(reg_lambda), _ptr(loss), _ptr(coef), _ptr(ws), ws.numel(), _stream(emb)),
              "kgat_bpr_loss_f32")
    return loss, coef, ws


def bpr_grad(emb, u, p, n, coef, reg_lambda, grad_scale=None, workspace=None, out=None):
    """d loss / d emb, dense (N, F), scaled by the device scalar `grad_scale` (kgat_bpr_grad_f32); into `out` if given."""
    lib = _lib.load()
    b = u.numel()
    grad = torch.empty((emb.shape[0], emb.shape[1]), dtype=torch.float32, device=emb.device) if out is None else \
        _need(out, torch.float32, "out", (emb.shape[0], emb.shape[1]))
    if grad_scale is not None:
        grad_scale = _need(grad_scale.reshape(1), torch.float32, "grad_scale")
    ws = workspace if workspace is not None else _workspace(lib.kgat_bpr_workspace_bytes(b, emb.shape[1]), emb.device)
    with _timed("bpr_grad", (b, emb.shape[1])):
        check(lib.kgat_bpr_grad_f32(emb.shape[0], emb.shape[1], _ptr(emb), emb.stride(0), b, _ptr(u), _ptr(p), _ptr(n),
                                    _ptr(coef), float(reg_lambda), _ptr(grad_scale), _ptr(grad), _ptr(ws), ws.numel(),
                                    _stream(emb)), "kgat_bpr_grad_f32")
    return grad


# ---------------------------------------------------------------- BPR-MF pretraining (kgat_mf_*)
def mf_supported(n_nodes, F, batch):
    """Sizes of the fused MF iteration: F a multiple of 4 up to 256, 3 * batch <= 65536, n_nodes < 2^31."""
    return bool(_lib.load().kgat_mf_supported(int(n_nodes), int(F), int(batch)))


def mf_presort(u, p, n, n_nodes):
    """The sorts of a whole MF phase's batches up front (kgat_mf_presort_f32; one launch up to batch 2,730, three beyond): u, p, n are (n_batches, batch)
    int32 tensors; returns (sorted, stride) - batch b's block is sorted[b * stride:(b + 1) * stride]."""
    return _presort("mf", ("u", "p", "n"), (u, p, n), n_nodes)


def MFAdamState(n_nodes, F, batch, device):
    """The StepState of a sequence of kgat_mf_adam_step_f32 calls."""
    return StepState((n_nodes, F, batch), _lib.load().kgat_mf_step_workspace_bytes(batch, F), device)


def mf_adam_step(u, p, n, sorted_block, emb, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, reg_lambda, loss_out, state):
    """One MF iteration (kgat_mf_adam_step_f32): BPR loss of the batch on the table `emb` into `loss_out` (a 1-element
    fp32 view) and the Adam step on `emb` in place.  exp_avg / exp_avg_sq: the moment tensors, `step`: the step count
    after this step - or, as the KG steps take them, one-entry ctypes pointer arrays and a one-entry list (the entry
    itself takes scalars).  Shapes and dtypes are the caller's responsibility here (KGATPropagation.mf_phase validates
    them once per phase)."""
    state.tag += 1
    m, v = (t.data_ptr() if isinstance(t, torch.Tensor) else t[0] for t in (exp_avg, exp_avg_sq))
    check(_lib.load().kgat_mf_adam_step_f32(emb.shape[0], emb.shape[1], u.numel(), u.data_ptr(), p.data_ptr(), n.data_ptr(),
                                            sorted_block.data_ptr(), emb.data_ptr(), m, v,
                                            int(step if isinstance(step, int) else step[0]), float(lr), float(beta1), float(beta2),
                                            float(eps), float(reg_lambda), loss_out.data_ptr(), state.row_slot.data_ptr(),
                                            state.tag, state.workspace.data_ptr(), state.workspace.numel(), _stream(emb)),
          "kgat_mf_adam_step_f32")


# ---------------------------------------------------------------- TransE KG embedding, the CFKG baseline (kgat_transe_*)
def transe_supported(n_nodes, d, n_rel, batch):
    """Sizes of the TransE kernels: d a multiple of 4 up to 256, batch <= 2730, n_rel <= 4096, n_nodes < 2^31."""
    return bool(_lib.load().kgat_transe_supported(int(n_nodes), int(d), int(n_rel), int(batch)))


def transe_scratch(batch, d, n_rel, device):
    """The scratch of every TransE entry (kgat_transe_scratch_bytes: one size for all of them)."""
    return _workspace(_lib.load().kgat_transe_scratch_bytes(int(batch), int(d), int(n_rel)), device)


def _transe_operands(h, r, pos_t, neg_t, ent, rel):
    ent = _need(ent, torch.float32, "ent")
    if ent.dim() != 2:
        raise ValueError("ent must be (n_nodes, d)")
    rel = _need(rel, torch.float32, "rel")
    if rel.dim() != 2 or rel.shape[1] != ent.shape[1]:
        raise ValueError("rel must be (n_rel, %d), got %s" % (ent.shape[1], tuple(rel.shape)))
    return ent.shape[0], rel.shape[0], ent.shape[1], _triplet_ids(h, r, pos_t, neg_t)


def transe_forward(h, r, pos_t, neg_t, ent, rel, reg_lambda, scratch=None):
    """TransE loss of a triplet batch with the per-sample gradient rows left in the returned scratch for
    transe_backward (kgat_transe_forward_f32).  Index tensors are int32.  Returns (loss 0-d tensor, scratch)."""
    n, n_rel, d, b = _transe_operands(h, r, pos_t, neg_t, ent, rel)
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=ent.device)
    need = lib.kgat_transe_scratch_bytes(b, d, n_rel)
    ws = scratch if scratch is not None and scratch.numel() >= need else _workspace(need, ent.device)
    with _timed("transe_forward", (b, d)):
        check(lib.kgat_transe_forward_f32(n, n_rel, d, b, _ptr(h), _ptr(r), _ptr(pos_t), _ptr(neg_t), _ptr(ent), _ptr(rel),
                                          float(reg_lambda), _ptr(loss), _ptr(ws), ws.numel(), _stream(ent)),
              "kgat_transe_forward_f32")
    return loss, ws


def transe_backward(h, r, pos_t, neg_t, shapes, ws, grad_scale=None):
    """The two dense gradients of transe_forward's loss (kgat_transe_backward_f32), times the device scalar grad_scale."""
    (n_nodes, d), (n_rel, _) = shapes
    dev = ws.device
    g_ent = torch.empty((n_nodes, d), dtype=torch.float32, device=dev)
    g_rel = torch.empty((n_rel, d), dtype=torch.float32, device=dev)
    if grad_scale is not None:
        grad_scale = _need(grad_scale.reshape(1), torch.float32, "grad_scale")
    with _timed("transe_backward", (h.numel(), d)):
        check(_lib.load().kgat_transe_backward_f32(n_nodes, n_rel, d, h.numel(), _ptr(h), _ptr(r), _ptr(pos_t), _ptr(neg_t),
                                                   _ptr(grad_scale), _ptr(g_ent), _ptr(g_rel), _ptr(ws), ws.numel(),
                                                   _stream(ws)), "kgat_transe_backward_f32")
    return g_ent, g_rel


def transe_loss_grad(h, r, pos_t, neg_t, ent, rel, reg_lambda, out=None, scratch=None):
    """TransE loss and its dense gradients in one call (kgat_transe_loss_grad_f32): (loss, grad_ent, grad_rel), the bits
    of transe_forward + transe_backward.  `out` = (loss, grad_ent, grad_rel) and `scratch` reuse buffers of an earlier call."""
    n, n_rel, d, b = _transe_operands(h, r, pos_t, neg_t, ent, rel)
    lib = _lib.load()
    if out is not None:
        loss, g_ent, g_rel = out
        _need(g_ent, torch.float32, "grad_ent", ent.shape)
        _need(g_rel, torch.float32, "grad_rel", rel.shape)
    else:
        loss = torch.empty((), dtype=torch.float32, device=ent.device)
        g_ent, g_rel = torch.empty_like(ent), torch.empty_like(rel)
    need = lib.kgat_transe_scratch_bytes(b, d, n_rel)
    ws = scratch if scratch is not None and scratch.numel() >= need else _workspace(need, ent.device)
    with _timed("transe", (b, d)):
        check(lib.kgat_transe_loss_grad_f32(n, n_rel, d, b, _ptr(h), _ptr(r), _ptr(pos_t), _ptr(neg_t), _ptr(ent), _ptr(rel),
                                            float(reg_lambda), _ptr(loss), _ptr(g_ent), _ptr(g_rel), _ptr(ws), ws.numel(),
                                            _stream(ent)), "kgat_transe_loss_grad_f32")
    return loss, g_ent, g_rel


def transe_presort(h, r, pos_t, neg_t, n_nodes, n_rel):
    """The sorts of a whole TransE phase's batches in one launch (kgat_transe_presort_f32): h, r, pos_t, neg_t are
    (n_batches, batch) int32 tensors; returns (sorted, stride) - batch b's block is sorted[b * stride:(b + 1) * stride]."""
    return _presort("transe", ("h", "r", "pos_t", "neg_t"), (h, r, pos_t, neg_t), n_nodes, int(n_rel))


def TransEAdamState(n_nodes, d, n_rel, batch, device):
    """The StepState of a sequence of kgat_transe_adam_step_f32 calls (its workspace: the scratch of every TransE entry)."""
    return StepState((n_nodes, d, n_rel, batch), _lib.load().kgat_transe_scratch_bytes(int(batch), int(d), int(n_rel)), device)


def transe_adam_step(h, r, pos_t, neg_t, sorted_block, ent, rel, exp_avg, exp_avg_sq, steps, lr, beta1, beta2, eps,
                     reg_lambda, loss_out, state):
    """One TransE iteration (kgat_transe_adam_step_f32): the loss of the batch into `loss_out` (a 1-element fp32 view)
    and the Adam step on ent / rel in place.  exp_avg / exp_avg_sq: ctypes arrays of the two moment pointers (built
    once per phase by the caller); steps: the two step counts after this step.  Shapes and dtypes are the caller's
    responsibility here (CFKG.kg_phase validates them once per phase)."""
    import ctypes as C
    state.tag += 1
    arr_t = (C.c_int64 * 2)(*steps)
    check(_lib.load().kgat_transe_adam_step_f32(ent.shape[0], rel.shape[0], ent.shape[1], h.numel(), h.data_ptr(), r.data_ptr(),
                                                pos_t.data_ptr(), neg_t.data_ptr(), sorted_block.data_ptr(), ent.data_ptr(),
                                                rel.data_ptr(), exp_avg, exp_avg_sq, arr_t, float(lr), float(beta1),
                                                float(beta2), float(eps), float(reg_lambda), loss_out.data_ptr(),
                                                state.row_slot.data_ptr(), state.tag, state.workspace.data_ptr(),
                                                state.workspace.numel(), _stream(ent)), "kgat_transe_adam_step_f32")


# ---------------------------------------------------------------- Bi-Interaction pooling, the FM / NFM baselines (kgat_bi_pool_*)
def bi_pool_supported(d, n_sets):
    """Sizes of the pooling kernels: d in {16, 32, 64, 128} and 1 <= n_sets <= 8192 (kgat_bi_pool_supported)."""
    return bool(_lib.load().kgat_bi_pool_supported(int(d), int(n_sets)))


def _bi_pool_operands(V, feats, items, extra):
    V = _need(V, torch.float32, "V")
    if V.dim() != 2 or V.shape[0] != feats.n_features:
        raise ValueError("V must be (%d, d), got %s" % (feats.n_features, tuple(V.shape)))
    items = _need(items, torch.int32, "items")
    if items.dim() != 1:
        raise ValueError("items must be one-dimensional")
    if extra is not None:
        _need(extra, torch.int32, "extra", items.shape)
    for name in ("indptr", "ids", "rev_indptr", "rev_items"):
        _need(getattr(feats, name), torch.int32, "feats." + name)
    if feats.indptr.device != V.device:
        raise ValueError("the feature sets are on %s, V on %s" % (feats.indptr.device, V.device))
    return V.shape[0], V.shape[1], items.numel()


def bi_pool_fwd(V, w_lin, feats, items, extra=None, want_lin=True, want_sq=True):
    """Bi-Interaction pooling of the sets [extra[m]] + feats[items[m]] (kgat_bi_pool_fwd_f32): returns (S, bi, lin, sq),
    lin / sq None where not asked for (lin also without w_lin).  `feats`: a FeatureSets on V's device; items, extra int32."""
    n, d, m = _bi_pool_operands(V, feats, items, extra)
    if w_lin is not None:
        _need(w_lin, torch.float32, "w_lin", (n,))
    dev = V.device
    S = torch.empty((m, d), dtype=torch.float32, device=dev)
    bi = torch.empty((m, d), dtype=torch.float32, device=dev)
    lin = torch.empty(m, dtype=torch.float32, device=dev) if want_lin and w_lin is not None else None
    sq = torch.empty(m, dtype=torch.float32, device=dev) if want_sq else None
    with _timed("bi_pool_fwd", (m, d)):
        check(_lib.load().kgat_bi_pool_fwd_f32(m, d, n, feats.n_items, feats.n_pairs, _ptr(V), _ptr(w_lin), _ptr(feats.indptr),
                                               _ptr(feats.ids), _ptr(items), _ptr(extra), _ptr(S), _ptr(bi), _ptr(lin), _ptr(sq),
                                               _stream(V)), "kgat_bi_pool_fwd_f32")
    return S, bi, lin, sq


def bi_pool_bwd(V, feats, items, extra, S, g_bi=None, g_lin=None, g_sq=None, want_w=True, scratch=None):
    """The dense gradients of bi_pool_fwd's outputs (kgat_bi_pool_bwd_f32): (grad_V (n_nodes, d), grad_w (n_nodes) or
    None).  g_bi (n_sets, d), g_lin, g_sq (n_sets): None = zero.  S is the forward's."""
    n, d, m = _bi_pool_operands(V, feats, items, extra)
    _need(S, torch.float32, "S", (m, d))
    if g_bi is not None:
        _need(g_bi, torch.float32, "g_bi", (m, d))
    for name, t in (("g_lin", g_lin), ("g_sq", g_sq)):
        if t is not None:
            _need(t, torch.float32, name, (m,))
    lib = _lib.load()
    dev = V.device
    grad_V = torch.empty((n, d), dtype=torch.float32, device=dev)
    grad_w = torch.empty(n, dtype=torch.float32, device=dev) if want_w else None
    need = lib.kgat_bi_pool_scratch_bytes(m, feats.n_items, n, feats.n_pairs)
    ws = scratch if scratch is not None and scratch.numel() >= need else _workspace(need, dev)
    with _timed("bi_pool_bwd", (m, d)):
        check(lib.kgat_bi_pool_bwd_f32(m, d, n, feats.n_items, feats.n_pairs, _ptr(V), _ptr(feats.rev_indptr),
                                       _ptr(feats.rev_items), _ptr(items), _ptr(extra), _ptr(g_bi), _ptr(g_lin), _ptr(g_sq),
                                       _ptr(S), _ptr(grad_V), _ptr(grad_w), _ptr(ws), ws.numel(), _stream(V)),
              "kgat_bi_pool_bwd_f32")
    return grad_V, grad_w


# ---------------------------------------------------------------- all-pairs NFM evaluation: MLP scores into top-K (kgat_nfm_eval_*)
NFM_EVAL_MAX_K = 128


def nfm_eval_supported(d, hidden, K):
    """Sizes of the fused NFM evaluation sweep: d in {16, 32, 64, 128}, ONE hidden layer of 16, 32 or 64 units, 1 <= K <=
    128.  The library's own envelope (kgat_nfm_eval_supported) starts at hidden = 32; nfm_eval_topk pads 16 units to 32
    with zero rows of W1, zero columns of C and zero entries of h, which is exact (0 * relu(0) = 0)."""
    hidden = int(hidden)
    return bool(_lib.load().kgat_nfm_eval_supported(int(d), 32 if hidden == 16 else hidden, int(K)))


def nfm_eval_topk(V, user_ids, W1, P, C, h, item_lin, user_const, train_ptr, train_items, K, want_scores=True):
    """The K best unseen items of every user under a one-hidden-layer NFM (kgat_eval_items_kmajor_f32 over P +
    kgat_nfm_eval_topk_f32; the arithmetic is stated in include/kgat_hip.h).  V (N, d) fp32 rows, user_ids int32 rows of
    V; W1 (hidden, d), h (hidden); P (n_items, d), C = T W1^T + b1 (n_items, hidden), item_lin (n_items): the item side
    of fm_models.pool_items; user_const (n_users) or None: added to every listed score; the train CSR holds ascending
    item positions per user.  Returns (items, scores): int32 positions (n_users, K), -1 padding, and float32 scores, -inf
    padding (None without want_scores)."""
    if V.dtype != torch.float32 or not V.is_cuda or V.dim() != 2 or V.stride(1) != 1:
        raise KGATLibraryError("nfm_eval_topk: `V` must be a float32 HIP matrix with unit column stride")
    d, K = V.shape[1], int(K)
    user_ids = _need(user_ids, torch.int32, "user_ids")
    n_users = user_ids.numel()
    W1 = _need(W1, torch.float32, "W1")
    if W1.dim() != 2 or W1.shape[1] != d:
        raise ValueError("W1 must be (hidden, %d), got %s" % (d, tuple(W1.shape)))
    hidden = W1.shape[0]
    P = _need(P, torch.float32, "P")
    if P.dim() != 2 or P.shape[1] != d:
        raise ValueError("P must be (n_items, %d), got %s" % (d, tuple(P.shape)))
    n_items = P.shape[0]
    C = _need(C, torch.float32, "C", (n_items, hidden))
    h = _need(h, torch.float32, "h", (hidden,))
    item_lin = _need(item_lin, torch.float32, "item_lin", (n_items,))
    if user_const is not None:
        user_const = _need(user_const, torch.float32, "user_const", (n_users,))
    train_ptr = _need(train_ptr, torch.int32, "train_ptr", (n_users + 1,))
    train_items = _need(train_items, torch.int32, "train_items")
    if not nfm_eval_supported(d, hidden, K):
        raise KGATLibraryError("nfm_eval_topk: d = %d (16, 32, 64, 128), hidden = %d (16, 32, 64) or K = %d (1..%d) outside "
                               "the kernel's range" % (d, hidden, K, NFM_EVAL_MAX_K))
    if n_items < 1:
        raise KGATLibraryError("nfm_eval_topk: no items to rank")
    lib = _lib.load()
    dev = V.device
    if hidden == 16:   # zero units up to the kernel's block of 32
        W1 = torch.cat([W1, torch.zeros_like(W1)], 0)
        C = torch.cat([C, torch.zeros_like(C)], 1).contiguous()
        h = torch.cat([h, torch.zeros_like(h)], 0)
        hidden = 32
    topk = torch.empty((n_users, K), dtype=torch.int32, device=dev)
    scores = torch.empty((n_users, K), dtype=torch.float32, device=dev) if want_scores else None
    if n_users == 0:
        return topk, scores
    ws = _workspace(lib.kgat_nfm_eval_scratch_bytes(n_users, n_items, d, hidden, K), dev)
    itemT = _eval_items(lib, P, torch.arange(n_items, dtype=torch.int32, device=dev))
    with _timed("nfm_eval_topk", (n_users, n_items, d, hidden, K)):
        check(lib.kgat_nfm_eval_topk_f32(n_users, _ptr(user_ids), n_items, d, hidden, _ptr(V), V.stride(0), _ptr(W1),
                                         _ptr(itemT), _ptr(C), _ptr(h), _ptr(item_lin), _ptr(user_const), _ptr(train_ptr),
                                         _ptr(train_items), K, _ptr(ws), ws.numel(), _ptr(topk), _ptr(scores),
                                         _stream(V)), "kgat_nfm_eval_topk_f32")
    return topk, scores


# ---------------------------------------------------------------- ripple-set attention, the RippleNet baseline (kgat_ripple_*)
def ripple_supported(d, n_memory, n_rel, n_samples):
    """Sizes of the ripple-set kernels: d in {16, 32, 64, 128}, 1 <= n_memory <= 128, 1 <= n_rel <= 4096, n_samples >= 1
    (kgat_ripple_supported)."""
    return bool(_lib.load().kgat_ripple_supported(int(d), int(n_memory), int(n_rel), int(n_samples)))


def _ripple_operands(ent, U, sets, users):
    ent = _need(ent, torch.float32, "ent")
    if ent.dim() != 2 or ent.shape[0] != sets.n_nodes:
        raise ValueError("ent must be (%d, d), got %s" % (sets.n_nodes, tuple(ent.shape)))
    users = _need(users, torch.int32, "users")
    if users.dim() != 1:
        raise ValueError("users must be one-dimensional")
    b, d = users.numel(), ent.shape[1]
    _need(U, torch.float32, "U", (b, sets.n_rel, d))
    for name in ("mem_h", "mem_r", "mem_t"):
        _need(getattr(sets, name), torch.int32, "sets." + name, (sets.n_users, sets.n_hop, sets.n_memory))
    if sets.mem_h.device != ent.device:
        raise ValueError("the ripple sets are on %s, ent on %s" % (sets.mem_h.device, ent.device))
    return b, d


def ripple_hop_fwd(ent, U, sets, users, hop):
    """Attention of every sample over its user's ripple set of hop `hop` (kgat_ripple_hop_fwd_f32): returns (o, p),
    o (n_samples, d) and the softmax weights p (n_samples, n_memory).  `sets`: a RippleSets on ent's device; U
    (n_samples, n_rel, d) with U[b, r] = v_b R_r; users int32."""
    b, d = _ripple_operands(ent, U, sets, users)
    o = torch.empty((b, d), dtype=torch.float32, device=ent.device)
    p = torch.empty((b, sets.n_memory), dtype=torch.float32, device=ent.device)
    with _timed("ripple_hop_fwd", (b, sets.n_memory, d)):
        check(_lib.load().kgat_ripple_hop_fwd_f32(b, d, sets.n_memory, sets.n_rel, sets.n_hop, int(hop), sets.n_nodes,
                                                  sets.n_users, _ptr(ent), _ptr(U), _ptr(sets.mem_h), _ptr(sets.mem_r),
                                                  _ptr(sets.mem_t), _ptr(users), _ptr(o), _ptr(p), _stream(ent)),
              "kgat_ripple_hop_fwd_f32")
    return o, p


def ripple_hop_bwd(ent, U, sets, users, hop, p, g_o):
    """The backward of ripple_hop_fwd towards the query table and the logits (kgat_ripple_hop_bwd_f32): returns
    (grad_U (n_samples, n_rel, d), every row written, and gl (n_samples, n_memory), the gradient of the logits).  The
    gradient towards ent is ripple_scatter's."""
    b, d = _ripple_operands(ent, U, sets, users)
    _need(p, torch.float32, "p", (b, sets.n_memory))
    _need(g_o, torch.float32, "g_o", (b, d))
    grad_U = torch.empty((b, sets.n_rel, d), dtype=torch.float32, device=ent.device)
    gl = torch.empty((b, sets.n_memory), dtype=torch.float32, device=ent.device)
    with _timed("ripple_hop_bwd", (b, sets.n_memory, d)):
        check(_lib.load().kgat_ripple_hop_bwd_f32(b, d, sets.n_memory, sets.n_rel, sets.n_hop, int(hop), sets.n_nodes,
                                                  sets.n_users, _ptr(ent), _ptr(U), _ptr(sets.mem_h), _ptr(sets.mem_r),
                                                  _ptr(sets.mem_t), _ptr(users), _ptr(p), _ptr(g_o), _ptr(grad_U), _ptr(gl),
                                                  _stream(ent)), "kgat_ripple_hop_bwd_f32")
    return grad_U, gl


def ripple_scatter(U, sets, users, hop, p, gl, g_o):
    """The dense gradient of ripple_hop_fwd towards ent, (n_nodes, d): grad_ent[t_i] += p[b, i] g_o[b] and
    grad_ent[h_i] += gl[b, i] U[b, r_i] as two incidence lists in (sample, slot) order, each turned into a node-major
    CSR (csr_from_coo, stable in entry order) and summed by spmm - the merge-path sum, no float atomics - and the two
    dense results added."""
    b, n_rel, d = U.shape
    if b * n_rel >= 2 ** 31:
        raise ValueError("ripple_scatter: n_samples * n_rel must stay below 2^31")
    M, n = sets.n_memory, sets.n_nodes
    ul = users.long()
    sample = torch.arange(b, dtype=torch.int32, device=U.device).unsqueeze(1)
    h, r, t = (getattr(sets, name)[ul, int(hop)] for name in ("mem_h", "mem_r", "mem_t"))
    out = None
    for row, source, weight, table in ((t, sample.expand(b, M), p, g_o), (h, sample * n_rel + r, gl, U.view(b * n_rel, d))):
        indptr, col, eid, row_of = csr_from_coo(n, source.reshape(-1).contiguous(), row.reshape(-1).contiguous())
        part = spmm(indptr, col, row_of, table, weight.reshape(-1), eid=eid)
        out = part if out is None else out.add_(part)
    return out


# ---------------------------------------------------------------- all-pairs RippleNet evaluation: attention scores into top-K (kgat_eval_ripple_*)
RIPPLE_EVAL_MAX_K = 128
RIPPLE_EVAL_MODES = ("replace", "plus", "replace_transform", "plus_transform")


def ripple_eval_supported(d, n_memory, n_hop, mode, K):
    """Sizes of the fused RippleNet evaluation sweep: d in {16, 32, 64}, 1 <= n_memory <= 64, n_hop in {1, 2}, mode 0..3
    (the position in RIPPLE_EVAL_MODES), 1 <= K <= 128 (kgat_eval_ripple_supported)."""
    return bool(_lib.load().kgat_eval_ripple_supported(int(d), int(n_memory), int(n_hop), int(mode), int(K)))


def _ripple_eval_operands(who, ent, sets, user_ids):
    if not isinstance(ent, torch.Tensor) or ent.dtype != torch.float32 or not ent.is_cuda or ent.dim() != 2 or \
            not ent.is_contiguous():
        raise KGATLibraryError("%s: `ent` must be a contiguous float32 HIP matrix" % who)
    if ent.shape[0] != sets.n_nodes:
        raise ValueError("ent must be (%d, d), got %s" % (sets.n_nodes, tuple(ent.shape)))
    user_ids = _need(user_ids, torch.int32, "user_ids")
    if user_ids.dim() != 1:
        raise ValueError("user_ids must be one-dimensional")
    for name in ("mem_h", "mem_r", "mem_t"):
        _need(getattr(sets, name), torch.int32, "sets." + name, (sets.n_users, sets.n_hop, sets.n_memory))
    if sets.mem_h.device != ent.device:
        raise ValueError("the ripple sets are on %s, ent on %s" % (sets.mem_h.device, ent.device))
    return user_ids


def ripple_eval_keys(ent, relation_emb, sets, user_ids):
    """The key table of the users `user_ids` (int32): keys[u, k, i] = R_{r_i} ent[h_i] over every hop's set,
    (len(user_ids), n_hop, n_memory, d) float32 (kgat_eval_ripple_keys_f32; one fmaf chain per element in ascending
    column order).  relation_emb: (n_rel, d * d)."""
    user_ids = _ripple_eval_operands("ripple_eval_keys", ent, sets, user_ids)
    d = ent.shape[1]
    relation_emb = _need(relation_emb, torch.float32, "relation_emb", (sets.n_rel, d * d))
    if not ripple_eval_supported(d, sets.n_memory, sets.n_hop, 0, 1):
        raise KGATLibraryError("ripple_eval_keys: d = %d (16, 32, 64), n_memory = %d (1..64) or n_hop = %d (1, 2) outside "
                               "the kernel's range" % (d, sets.n_memory, sets.n_hop))
    n_call = user_ids.numel()
    keys = torch.empty((n_call, sets.n_hop, sets.n_memory, d), dtype=torch.float32, device=ent.device)
    with _timed("ripple_eval_keys", (n_call, sets.n_hop, sets.n_memory, d)):
        check(_lib.load().kgat_eval_ripple_keys_f32(n_call, _ptr(user_ids), d, sets.n_memory, sets.n_hop, sets.n_rel,
                                                    sets.n_nodes, sets.n_users, _ptr(ent), _ptr(relation_emb),
                                                    _ptr(sets.mem_h), _ptr(sets.mem_r), _ptr(keys), _stream(ent)),
              "kgat_eval_ripple_keys_f32")
    return keys


def ripple_eval_items(ent, item_lo, item_hi):
    """The rows ent[item_lo:item_hi] as the sweep's item fragments (kgat_eval_items_kmajor_f32): laid out once per
    evaluation, shared by every user block."""
    if not isinstance(ent, torch.Tensor) or ent.dtype != torch.float32 or not ent.is_cuda or ent.dim() != 2 or \
            ent.stride(1) != 1:
        raise KGATLibraryError("ripple_eval_items: `ent` must be a float32 HIP matrix with unit column stride")
    return _eval_items(_lib.load(), ent, torch.arange(int(item_lo), int(item_hi), dtype=torch.int32, device=ent.device))


def ripple_eval_topk(ent, sets, user_ids, keys, itemT, n_items, W, mode, all_hops, train_ptr, train_items, K,
                     want_scores=True):
    """The K best unseen items of every user of `user_ids` under RippleNet (kgat_eval_ripple_topk_f32; the arithmetic is
    stated in include/kgat_hip.h).  keys = ripple_eval_keys(.., user_ids), itemT = ripple_eval_items(ent, lo, lo +
    n_items); W (d, d) or None (modes 0, 1); mode 0..3; the train CSR holds ascending item positions per user.  Returns
    (items, scores): int32 positions (n_users, K), -1 padding, and float32 scores, -inf padding (None without
    want_scores)."""
    user_ids = _ripple_eval_operands("ripple_eval_topk", ent, sets, user_ids)
    d, K, mode, n_items = ent.shape[1], int(K), int(mode), int(n_items)
    n_call = user_ids.numel()
    if not ripple_eval_supported(d, sets.n_memory, sets.n_hop, mode, K):
        raise KGATLibraryError("ripple_eval_topk: d = %d (16, 32, 64), n_memory = %d (1..64), n_hop = %d (1, 2), mode = %d "
                               "(0..3) or K = %d (1..%d) outside the kernel's range"
                               % (d, sets.n_memory, sets.n_hop, mode, K, RIPPLE_EVAL_MAX_K))
    if n_items < 1:
        raise KGATLibraryError("ripple_eval_topk: no items to rank")
    keys = _need(keys, torch.float32, "keys", (n_call, sets.n_hop, sets.n_memory, d))
    itemT = _need(itemT, torch.float32, "itemT")
    lib = _lib.load()
    if itemT.numel() < int(lib.kgat_eval_items_elems(n_items, d)):
        raise ValueError("itemT holds %d elements, %d items of width %d need %d"
                         % (itemT.numel(), n_items, d, int(lib.kgat_eval_items_elems(n_items, d))))
    if mode >= 2:
        W = _need(W, torch.float32, "W", (d, d))
    elif W is not None:
        W = _need(W, torch.float32, "W", (d, d))
    train_ptr = _need(train_ptr, torch.int32, "train_ptr", (n_call + 1,))
    train_items = _need(train_items, torch.int32, "train_items")
    dev = ent.device
    topk = torch.empty((n_call, K), dtype=torch.int32, device=dev)
    scores = torch.empty((n_call, K), dtype=torch.float32, device=dev) if want_scores else None
    if n_call == 0:
        return topk, scores
    ws = _workspace(lib.kgat_eval_ripple_scratch_bytes(n_call, n_items, d, sets.n_memory, sets.n_hop, K), dev)
    with _timed("ripple_eval_topk", (n_call, n_items, d, sets.n_memory, sets.n_hop, K)):
        check(lib.kgat_eval_ripple_topk_f32(n_call, _ptr(user_ids), n_items, d, sets.n_memory, sets.n_hop, mode,
                                            1 if all_hops else 0, sets.n_nodes, sets.n_users, _ptr(itemT), _ptr(keys),
                                            _ptr(ent), _ptr(sets.mem_t), _ptr(W), _ptr(train_ptr), _ptr(train_items), K,
                                            _ptr(ws), ws.numel(), _ptr(topk), _ptr(scores), _stream(ent)),
              "kgat_eval_ripple_topk_f32")
    return topk, scores


# ---------------------------------------------------------------- global-norm gradient clipping (kgat.py:32,162)
def __getattr__(name):
    # GRAD_NORM_CHAIN: the compile-time constant of the library (kgat_grad_norm_chain), read when first asked for
    if name == "GRAD_NORM_CHAIN":
        return int(_lib.load().kgat_grad_norm_chain())
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def check_max_norm(max_norm):
    """`max_norm` as a float; ValueError unless it is finite and > 0."""
    import math
    max_norm = float(max_norm)
    if not (math.isfinite(max_norm) and max_norm > 0):
        raise ValueError("max_norm must be finite and > 0, got %r" % (max_norm,))
    return max_norm


def _grad_list(tensors, what):
    import ctypes as C
    tensors = [_need(t, torch.float32, "%s: tensor %d" % (what, i)) for i, t in enumerate(tensors)]
    if len({t.device for t in tensors}) > 1:
        raise KGATLibraryError("%s: tensors on more than one device (%s)" % (
            what, ", ".join(sorted({str(t.device) for t in tensors}))))
    cap = _lib.load().kgat_adam_max_tensors()
    groups = []
    for lo in range(0, len(tensors), cap):
        chunk = tensors[lo:lo + cap]
        groups.append((len(chunk), (C.c_int64 * len(chunk))(*[t.numel() for t in chunk]),
                       (C.c_void_p * len(chunk))(*[t.data_ptr() for t in chunk])))
    return tensors, groups


def grad_norm(tensors, max_norm, norm_out=None):
    """The global 2-norm of `tensors` (contiguous fp32 HIP tensors on one device: the gradients) and the coefficient
    torch.nn.utils.clip_grad_norm_ would scale them by, min(max_norm / (norm + 1e-6), 1), as 0-dim DEVICE tensors
    (norm, coef): one kgat_grad_sumsq_f32 launch per kgat_adam_max_tensors() tensors, then kgat_grad_norm_finish_f32.
    Fixed summation order (bitwise reproducible); nothing is read back.  `norm_out`: a 1-element fp32 tensor or view on
    the same device that receives the norm (and is returned, as a 0-dim view).  An empty list gives norm 0 and coef 1
    on `norm_out`'s device, else on the current one."""
    max_norm = check_max_norm(max_norm)
    tensors, groups = _grad_list(tensors, "grad_norm")
    if tensors:
        dev = tensors[0].device
    else:
        dev = norm_out.device if norm_out is not None else torch.device("cuda", torch.cuda.current_device())
    if norm_out is not None:
        if (not isinstance(norm_out, torch.Tensor) or not norm_out.is_cuda or norm_out.dtype != torch.float32
                or norm_out.numel() != 1 or norm_out.device != dev):
            raise KGATLibraryError("grad_norm: norm_out must be a 1-element float32 tensor on %s" % dev)
        norm = norm_out.view(())
    else:
        norm = torch.empty((), dtype=torch.float32, device=dev)
    lib = _lib.load()
    counts = [int(lib.kgat_grad_sumsq_partials(n, sizes)) for n, sizes, _ in groups]
    if any(c < 0 for c in counts):
        check(-1, "kgat_grad_sumsq_partials")
    total = sum(counts)
    partials = _scratch((max(total, 1),), torch.float32, dev)
    coef = torch.empty((), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev), _timed("grad_norm", (len(tensors), total)):
        off = 0
        for (n, sizes, ptrs), c in zip(groups, counts):
            check(lib.kgat_grad_sumsq_f32(n, sizes, ptrs, partials.data_ptr() + 4 * off, total - off, stream),
                  "kgat_grad_sumsq_f32")
            off += c
        check(lib.kgat_grad_norm_finish_f32(total, partials.data_ptr(), max_norm, norm.data_ptr(), coef.data_ptr(),
                                            stream), "kgat_grad_norm_finish_f32")
    return norm, coef


def scale_grads(tensors, coef):
    """tensors[i] *= coef in place (kgat_scale_grads_f32; `coef` a 1-element fp32 device tensor): one launch per
    kgat_adam_max_tensors() tensors."""
    tensors, groups = _grad_list(tensors, "scale_grads")
    if not tensors:
        return
    dev = tensors[0].device
    coef = _need(coef.reshape(1), torch.float32, "coef")
    if coef.device != dev:
        raise KGATLibraryError("scale_grads: coef is on %s, the tensors on %s" % (coef.device, dev))
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev), _timed("scale_grads", len(tensors)):
        for n, sizes, ptrs in groups:
            check(lib.kgat_scale_grads_f32(n, sizes, ptrs, coef.data_ptr(), stream), "kgat_scale_grads_f32")
