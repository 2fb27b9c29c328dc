"""The three fused train-and-step iterations bit for bit against values recorded on an MI355X
(tests/golden/step_bits.npz, written by scripts/record_step_bits.py; the fixture names the commit and the compiler it
was recorded with).  The Adam chunk walk, the row tags, the ordered row sums and the loss mean are shared pieces
(csrc/kgat_step_common.h): a change there that is meant to be mechanical must leave these bits alone.  The fp64 tests
would accept a changed addition order in TransE, whose fused step and two-halves route share the row sum; this does
not.  A mismatch after a toolchain change, with no change to the kernels, means re-recording: compare the fixture's
`hipcc` entry with the compiler in use first.

Every case takes two consecutive steps on one state object, so the second meets the first's (stale) row tags; batch 2
shares about half its entity rows with batch 1.  Compared per case: both losses, every parameter and both moments -
full bit patterns for the losses and the relation tables, sha-256 for the rest.

KG cases (TransR at (d, k) = (64, 64) MFMA partials + the LDS copy of W_r, (20, 12) non-MFMA partials, (128, 64) no LDS
copy; TransE at d = 64, 72, 256: 16, 32 with dead lanes, 64 lanes per sample): n = 300, R = 5 with relation 3 unused,
B = 400, relation 0 on 330 samples (six 64-sample chunks: more than one 4-row look of partials), entity 42 head of 150
samples and tail of 30 (a run of 180 rows).  MF cases: n = 300, F = 16, B = 13 (one-workgroup presort); n = 3000,
F = 32, B = 2731 (slice-sort presort) with user 11 in half of each batch - a run across about 43 windows, several
8-row looks of following pieces."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("record_step_bits", os.path.join(ROOT, "scripts", "record_step_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN_DIR, "step_bits.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_names_every_case(stored):
    cases = {k.split("/")[0] for k in stored if "/" in k}
    assert cases == set(REC.CASES) and len(cases) == 8
    assert str(stored["commit"]) and str(stored["hipcc"])


@pytest.mark.parametrize("name", sorted(REC.CASES))
def test_two_steps_bit_patterns(name, stored):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    where = "recorded at commit %s with %s" % (stored["commit"], stored["hipcc"])
    got = REC.run_case(name, torch.device("cuda:0"))
    want = {k[len(name) + 1:]: v for k, v in stored.items() if k.startswith(name + "/")}
    n_params = {"transr": 3, "transe": 2, "mf": 1}[REC.CASES[name][0]]
    assert sorted(got) == sorted(want) and len(want) == 1 + 3 * n_params
    assert want["losses"].dtype == np.uint32 and want["losses"].shape == (2,)
    for key in sorted(want):
        if want[key].ndim == 0:
            assert got[key] == str(want[key]), "%s %s: digest differs (%s)" % (name, key, where)
            continue
        assert want[key].dtype == np.uint32 and got[key].shape == want[key].shape
        diff = np.flatnonzero(got[key] != want[key])
        assert diff.size == 0, "%s %s: %d of %d values differ, first at %d (%s)" % (
            name, key, diff.size, want[key].size, diff[0], where)
