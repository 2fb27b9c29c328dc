"""The wide-K ranking path (kgat_eval_topk_f32 / kgat_eval_metrics_at_ks, metrics.calc_metrics / recommend) without a
GPU: the entries' host-side answers, what the K <= 32 entries still refuse, the refusal of CPU tensors and the example's
--Ks parser."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dgl_kgat_amd import _lib, metrics, ops  # noqa: E402
from dgl_kgat_amd.ops import KGATLibraryError  # noqa: E402


def test_topk_supported_ranges():
    lib = _lib.load()
    assert lib.kgat_eval_topk_supported(176, 100) == 1 and lib.kgat_eval_topk_supported(176, 128) == 1
    assert lib.kgat_eval_topk_supported(176, 129) == 0 and lib.kgat_eval_topk_supported(4000, 20) == 0
    assert lib.kgat_eval_topk_supported(176, 0) == 0 and lib.kgat_eval_topk_supported(0, 20) == 0
    # every K of the old entry, and every width of its register forms at every K
    assert all(lib.kgat_eval_topk_supported(F, K) == 1 for F in (1, 8, 40, 41, 96, 176, 256, 352, 353, 700)
               for K in (1, 20, 32, 33, 64, 65, 128))
    # the rows of the LDS form share the CU's LDS with the buffer: the widest F shrinks as the buffer grows
    assert lib.kgat_eval_topk_supported(1100, 32) == 1 and lib.kgat_eval_topk_supported(1100, 33) == 0
    assert lib.kgat_eval_topk_supported(1000, 64) == 1 and lib.kgat_eval_topk_supported(1000, 65) == 0
    assert ops.eval_topk_supported(176, 100) and not ops.eval_topk_supported(176, 129)


def test_old_entries_keep_their_range():
    lib = _lib.load()
    assert lib.kgat_eval_supported(176, 33) == 0 and lib.kgat_eval_supported(176, 32) == 1
    assert lib.kgat_eval_recall_ndcg_f32(1, None, 10, 176, None, 176, None, None, None, None, None, 40, None, None, 0,
                                         None, None, None, None) == -2


def test_topk_entry_validates_before_device_work():
    lib = _lib.load()
    args = lambda n_items, K, drop: (1, None, n_items, 176, None, 176, None, None, None, K, drop, None, 0, None, None, None)
    assert lib.kgat_eval_topk_f32(*args(1000, 129, 0)) == -2 and b"eval_topk" in lib.kgat_last_error()
    assert lib.kgat_eval_topk_f32(*args(1000, 0, 1)) == -2 and b"eval_topk" in lib.kgat_last_error()
    assert lib.kgat_eval_topk_f32(*args(50, 100, 0)) == -1 and b"fewer items" in lib.kgat_last_error()   # mask: n_items >= K
    assert lib.kgat_eval_topk_f32(*args(50, 100, 1)) == -1 and b"null pointer" in lib.kgat_last_error()  # drop: not the size
    assert lib.kgat_eval_topk_f32(1, None, 1000, 176, None, 100, None, None, None, 100, 0, None, 0, None, None,
                                  None) == -1 and b"bad sizes" in lib.kgat_last_error()                 # stride < F
    assert lib.kgat_eval_topk_f32(0, None, 1000, 176, None, 176, None, None, None, 100, 0, None, 0, None, None, None) == 0


def test_topk_workspace_holds_the_partial_lists():
    lib = _lib.load()
    assert lib.kgat_eval_topk_workspace_bytes(70679, 24915, 176, 100) >= 2 * 70679 * 100 * 4
    # K <= 32 sweeps with the old entry's plan: the same workspace
    assert lib.kgat_eval_topk_workspace_bytes(70679, 24915, 176, 20) == lib.kgat_eval_workspace_bytes(70679, 24915, 176, 20)
    assert lib.kgat_eval_topk_workspace_bytes(0, 24915, 176, 100) == 256


def test_metrics_entry_validates_cutoffs():
    import ctypes
    lib = _lib.load()

    def call(K, ks):
        arr = (ctypes.c_int32 * max(len(ks), 1))(*ks)
        return lib.kgat_eval_metrics_at_ks(0, K, None, None, None, len(ks), ctypes.cast(arr, ctypes.c_void_p), None,
                                           None, None)
    assert call(100, [20, 40, 60, 80, 100]) == 0
    assert call(100, [40, 20]) == -1 and b"eval_metrics_at_ks" in lib.kgat_last_error()
    assert call(100, [20, 20]) == -1 and call(100, [20, 101]) == -1 and call(100, [0, 5]) == -1
    assert call(100, []) == -1 and call(100, list(range(1, 10))) == -1 and call(129, [20]) == -1


def test_python_entries_refuse_cpu_tensors_and_bad_cutoffs():
    emb = torch.zeros((20, 8))
    train, test = {0: np.array([1])}, {0: np.array([2])}
    with pytest.raises(KGATLibraryError):
        metrics.calc_metrics(emb, train, test, np.arange(4, 20), Ks=(5, 10))
    with pytest.raises(KGATLibraryError):
        metrics.recommend(emb, [0, 1], np.arange(4, 20), 5, seen=train)
    with pytest.raises(KGATLibraryError):
        ops.eval_topk(emb, torch.zeros(1, dtype=torch.int32), torch.zeros(16, dtype=torch.int32),
                      torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 5)
    with pytest.raises(KGATLibraryError):
        ops.eval_metrics_at_ks(torch.zeros((1, 5), dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                               torch.zeros(0, dtype=torch.int32), [5])
    for bad in ((40, 20), (20, 20), tuple(range(1, 10)), ()):
        with pytest.raises(ValueError):
            metrics.calc_metrics(emb, train, test, np.arange(4, 20), Ks=bad)
    with pytest.raises(KGATLibraryError):
        metrics.calc_metrics(emb, train, test, np.arange(4, 20), Ks=(20, 129))
    assert "calc_metrics" in metrics.calc_recall_ndcg.__doc__


def _train_kgat():
    spec = importlib.util.spec_from_file_location("_train_kgat_parser_ks", os.path.join(ROOT, "examples", "train_kgat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_parser_takes_cutoffs():
    tk = _train_kgat()
    assert tk.parse_args(["--Ks", "20,40,100"]).Ks == [20, 40, 100]
    assert tk.parse_args([]).Ks == [20]
    for bad in ("40,20", "20,20", "20,129", "0", "1,2,3,4,5,6,7,8,9", "a,b", ""):
        with pytest.raises(SystemExit) as e:
            tk.parse_args(["--Ks", bad])
        assert e.value.code == 2
