"""The workspaces of the TransR and BPR training steps without a GPU: the three workspace rules and the size of the
presort's per-batch block are restated here as sums of 256-aligned pieces (not read from the library) and tabulated
against the C size entries; and each entry that carves one of them refuses a workspace one byte short of its size -
before the first HIP call, so the return code and the text of kgat_last_error() are checked on the host."""
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dgl_kgat_amd import _lib  # noqa: E402

import _transr_ref as T  # noqa: E402
from _transr_ref import align256 as al  # noqa: E402

WORKSPACE = -3   # KGAT_E_WORKSPACE
_BUF = C.create_string_buffer(4096 + 16)   # a non-null, 16-byte aligned address; no case below gets as far as reading it
P = (C.addressof(_BUF) + 15) // 16 * 16

TRANSR_BATCHES = (1, 63, 64, 65, 2730)
TRANSR_WIDTHS = ((4, 4), (20, 12), (64, 64), (128, 128))
TRANSR_RELS = (1, 41, 4096)
BPR_BATCHES = (1, 1365, 1366, 21845, 21846)   # one slice, one id over, sixteen slices, the radix fallback
BPR_WIDTHS = (4, 8, 176, 260)


# ---- the rules
def sample_arrays_bytes(b, d, k, n_rel):
    """losses | GA | GR | DX | XS | the weight / relation gradient partials (fp32)"""
    return (al(4 * b) + al(4 * 3 * b * k) + al(4 * b * k) + 2 * al(4 * 3 * b * d)
            + al(4 * T.max_chunks(b, n_rel) * (d * k + k)))


def transr_workspace_bytes(b, d, k, n_rel):
    """order, seg, chunk_ptr, chunks | the per-sample arrays | sorted_ids, row_order"""
    return (al(4 * b) + 2 * al(4 * (n_rel + 2)) + al(8 * T.max_chunks(b, n_rel)) + sample_arrays_bytes(b, d, k, n_rel)
            + 2 * al(4 * 3 * b))


def transr_step_workspace_bytes(b, d, k, n_rel):
    return sample_arrays_bytes(b, d, k, n_rel)


def _scan_elems(n):   # the device scan's scratch: one level of block sums per factor of 4,096, 64-element aligned, + 64
    total = 0
    while n > 4096:
        n = -(-n // 4096)
        total += (n + 63) // 64 * 64
    return total + 64


def radix_sort_bytes(n):   # the device radix sort's: three arrays of n int32 | 256 counters per block | the scan's
    tile = 4096 if n >= 1 << 20 else 256
    hist = 256 * max(-(-n // tile), 1)
    return 3 * al(4 * n) + al(4 * hist) + al(4 * _scan_elems(hist))


def bpr_workspace_bytes(b, F):
    """part | keys | order | window partials | sort scratch = max(slice-sort lists + sorted keys, device radix sort),
    + 256"""
    windows = -(-3 * b // 32)
    slices = al(8 * 3 * b) + al(4 * 3 * b) if 3 * b <= 4096 * 16 else 0
    return al(4 * 4 * b) + 2 * al(4 * 3 * b) + al(4 * windows * 2 * F) + max(slices, radix_sort_bytes(3 * b)) + 256


# ---- the tables
def test_transr_workspace_sizes():
    lib = _lib.load()
    n = 0
    for b, (d, k), r in itertools.product(TRANSR_BATCHES, TRANSR_WIDTHS, TRANSR_RELS):
        assert lib.kgat_transr_workspace_bytes(b, d, k, r) == transr_workspace_bytes(b, d, k, r), (b, d, k, r)
        assert lib.kgat_transr_step_workspace_bytes(b, d, k, r) == transr_step_workspace_bytes(b, d, k, r), (b, d, k, r)
        n += 1
    assert n == 60


def test_transr_sorted_block_sizes():
    lib = _lib.load()
    for b, r in itertools.product(TRANSR_BATCHES, TRANSR_RELS):
        lay, nbytes = T.sorted_block_layout(b, r)
        assert lib.kgat_transr_sorted_bytes(b, r) == nbytes, (b, r)
        assert nbytes == (al(4 * b) + 2 * al(4 * (r + 2)) + al(8 * T.max_chunks(b, r)) + 4 * al(4 * 3 * b))
        assert list(lay) == ["order", "seg", "chunk_ptr", "chunks", "sorted_ids", "row_order", "inv_pos", "run_len"]
        assert all(off % 256 == 0 for off, _, _ in lay.values())


def test_bpr_workspace_sizes():
    lib = _lib.load()
    for b, F in itertools.product(BPR_BATCHES, BPR_WIDTHS):
        assert lib.kgat_bpr_workspace_bytes(b, F) == bpr_workspace_bytes(b, F), (b, F)
    assert 3 * 21845 <= 65536 < 3 * 21846   # the grid has the last batch of the slice sort and the first beyond it


# ---- one byte short: refused before any HIP call
def _refused(name, args, fragment):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.kgat_last_error() or b"").decode()
    assert rc == WORKSPACE, (name, rc, msg)
    assert msg == fragment, (name, msg)


def test_transr_entries_refuse_a_short_workspace():
    lib = _lib.load()
    n_nodes, n_rel, d, k, b = 1000, 41, 64, 64, 65
    need = lib.kgat_transr_workspace_bytes(b, d, k, n_rel)
    _refused("kgat_transr_loss_grad_f32", (n_nodes, n_rel, d, k, b, P, P, P, P, P, P, P, 0.01, P, P, P, P, P, need - 1, None),
             "transr: workspace too small")
    moments = (C.c_void_p * 3)(P, P, P)
    steps = (C.c_int64 * 3)(1, 1, 1)
    need = lib.kgat_transr_step_workspace_bytes(b, d, k, n_rel)
    _refused("kgat_transr_adam_step_f32",
             (n_nodes, n_rel, d, k, b, P, P, P, P, P, P, P, P, C.addressof(moments), C.addressof(moments),
              C.addressof(steps), 1e-3, 0.9, 0.999, 1e-8, 0.01, P, P, 1, P, need - 1, None),
             "transr_adam_step: workspace too small")


def test_bpr_entries_refuse_a_short_workspace():
    lib = _lib.load()
    n_nodes, F, b = 1000, 176, 1366
    need = lib.kgat_bpr_workspace_bytes(b, F)
    _refused("kgat_bpr_loss_f32", (n_nodes, F, P, F, b, P, P, P, 1e-5, P, P, P, need - 1, None),
             "bpr_loss: workspace too small")
    _refused("kgat_bpr_grad_f32", (n_nodes, F, P, F, b, P, P, P, P, 1e-5, None, P, P, need - 1, None),
             "bpr_grad: workspace too small")
