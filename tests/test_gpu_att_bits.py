"""The attention logits bit for bit, every MFMA form, against values recorded on an MI355X
(tests/golden/att_bits.npz, written by scripts/record_att_bits.py; the fixture names the commit and the compiler it
was recorded with).  The kernels' tile walks, rings and look-aheads are shared pieces now: a change there that is
meant to be mechanical must leave these bits alone.  A mismatch after a toolchain change, with no change to the
kernels, means re-recording: compare the fixture's `hipcc` entry with the compiler in use first.

Small case (full bit patterns): n = 300, e = 4,000, R = 5, never-scored edges on both sides, an empty relation, one
(head, relation) group of about 600 positions; one-kernel form (= split form) at d = 16, 32, 64, folded form at
d = 16 .. 128 with both product flags, fused form at d = 16 .. 128 with every product form it has, tile caps 64 and
512 (tiles of more than four 64-position chunks), a 37-part cost-balanced split.  The fused form's edge-id-order and
grouped-order outputs are asserted to be the CSR-order values permuted, and the even split to give the same bits.

Ring case (sha-256 only): n = 200,000, e = 1,200,000, R = 3, uniform, no hub - 75,000 edge tiles and about 32,000
group tiles (519,000 groups), i.e. some 24 tiles per wavefront for the one-kernel and split forms (3,072 wavefronts
on 256 CUs) and 16 group tiles per wavefront for the fold-head and fused forms (2,048), so the three-deep rings and
the index look-ahead run in their steady state.  Which wavefront takes which tile does not enter the arithmetic, so
the digests do not depend on the CU count."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("record_att_bits", os.path.join(ROOT, "scripts", "record_att_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN_DIR, "att_bits.npz"))
    return {k: z[k] for k in z.files}


def _where(stored):
    return "recorded at commit %s with %s" % (stored["commit"], stored["hipcc"])


def test_small_case_bit_patterns(rec, stored):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    got = rec.small_case(torch.device("cuda:0"))
    want = {k[len("small/"):]: v for k, v in stored.items() if k.startswith("small/")}
    assert sorted(got) == sorted(want) and len(want) == 23
    for name in sorted(want):
        assert want[name].dtype == np.uint32 and want[name].shape == (4000,)
        diff = np.flatnonzero(got[name] != want[name])
        assert diff.size == 0, "%s: %d of 4000 logits differ, first at CSR position %d (%s)" % (
            name, diff.size, diff[0], _where(stored))


def test_ring_case_digests(rec, stored):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    got = rec.ring_case(torch.device("cuda:0"))
    want = {k[len("ring/"):]: str(v) for k, v in stored.items() if k.startswith("ring/")}
    assert sorted(got) == sorted(want) == ["folded.d128", "folded.d64", "fused.d128", "fused.d64", "groups", "mfma.d64",
                                           "split.d64"]
    for name in sorted(want):
        assert got[name] == want[name], "%s (%s)" % (name, _where(stored))
