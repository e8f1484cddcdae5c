"""PairSet.ransac(out_mask=, out_errors=, out_models=, out_index=, out_counts=, stream=, lists=)
(mp_ransac_out_set): ransac's results written into the caller's device arrays by the call itself.

One set per variant 0, 1, 2 with one pair of every size in tests/residuals_worker.py SIZES (either
side of a wave, of a trip of 256 rows and of an item of 4096 rows; sizes 0 and 1 give pairs without
a winner), in every mode of the method.  The reference is the same call without the new keywords;
nothing here has a tolerance.  The device arrays are made with torch, so every check runs in ONE
child process that imports torch first (tests/ransac_out_worker.py); each test asserts its own
check's outcome and prints what the check printed.  Without the feature ransac has none of the
keywords and the library lacks the symbol: every test here fails.

What keeps a check from passing vacuously is asserted and printed per variant and mode: at least
two pairs without a winner, all four pairs of >= 4095 rows with rows both inside and outside the
thresholds, and in the budget=64 mode at least one pair with an accepted final round.  Seed 7
gives all three in every variant (ransac_out_worker.SEED); observed on the MI355X in the budget=64
mode: 2, 2 and 3 pairs without a winner (calibrated, shared focal, two focals), 4 mixed large pairs
in each variant, and 10, 10 and 9 pairs with an accepted round.

Refined focal models: the errors of variants 1 and 2 after final rounds need not equal
residuals(model_row)'s bytes; the number of values that differ is
printed by every check_mode, not asserted."""
import json
import os
import subprocess
import sys

import pytest

import madpose
from tests import ransac_out_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


@pytest.fixture(scope="module")
def worker():
    env = {k: v for k, v in os.environ.items() if not k.startswith("MADPOSE_")}
    r = subprocess.run([sys.executable, "-m", "tests.ransac_out_worker"], env=env, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and len(lines) >= 2, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(lines[-2]), lines[-1], r.stderr


@pytest.mark.parametrize("name", list(W.CHECKS))
def test_device_check(worker, name):
    got = worker[0].get(name)
    assert got is not None, f"the worker did not run {name}"
    print(got["detail"], got["seconds"])
    assert got["ok"], got["detail"]


def test_the_process_exits_cleanly_with_the_sets_open(worker):
    _, last, stderr = worker
    assert last == "DONE with the sets open"
    low = stderr.lower()
    assert "hip" not in low and "error" not in low and "fault" not in low, stderr[-4000:]


def test_the_checks_cover_the_issue():
    names = set(W.CHECKS)
    assert W.VARIANTS == (0, 1, 2) and len(W.MODES) == 10
    for v in W.VARIANTS:
        for m in W.MODES:
            assert f"mode[{v}-{m}]" in names
        assert f"interleaved_with_other_stages_and_repeated[{v}]" in names and f"cut_into_runs[{v}]" in names
    assert {"outputs_last_written_on_another_stream", "bad_device_outputs_are_refused_in_python",
            "short_and_overlapping_buffers_are_refused_by_the_library"} <= names
    assert W.SIZES == (0, 1, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193) and W.GUARD == 64
    assert set(W.SEED) == set(W.VARIANTS) and all(s >= 7 for s in W.SEED.values())
    assert len(set(W.SUBSET)) == len(W.SUBSET) < len(W.SIZES)
