"""PairSet.residuals (mp_residuals_set): for any models on any pairs of a resident set, the three
squared errors and a three-bit inlier mask per correspondence.

One pair of every size in tests/residuals_worker.py SIZES (either side of a wave, of a trip of
256 rows and of an item of 4096 rows) in one set per variant; per pair the synthetic ground
truth, a perturbed ground truth and a model with a NaN entry.  The references are the entries
that existed before: select's inlier lists, score_models(with_errors=True), lsq_fit's num_wide,
ransac's and refine's lists.  Nothing here has a tolerance.  The device-output checks make their
arrays with torch and run in ONE child process that imports torch first
(tests/residuals_worker.py); every test_device_check asserts its own check's outcome.  Without
the feature PairSet has no residuals and every test here fails.

Refined focal models (test_refined_focal_models_differ_in_counted_rows, printed, not asserted):
the lists of ransac's final rounds were formed from the problem-unit model before its focal was
multiplied by norm_scale; residuals divides the returned focal again, and (f * s) / s need not be
f, so a row whose error sits within a rounding of its threshold may differ."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from tests import refine_cases as RC
from tests import residuals_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (0, 1, 2, 3)


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


@pytest.fixture(scope="module")
def sets():
    """one open set per (variant, score type), and the call every test shares (never changed)"""
    made = {}

    def get(variant, score_type=0):
        key = (variant, score_type)
        if key not in made:
            k = W.case(variant, score_type)
            ps = W.open_set(k)
            res = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
            for a in (res.mask, res.errors, res.counts, res.offsets):
                a.flags.writeable = False
            made[key] = (k, ps, res)
        return made[key]
    yield get
    for _, ps, _ in made.values():
        ps.close()


def _bits(mask, t):
    return np.flatnonzero((mask >> t) & 1).astype(np.int32)


def _record(ps, pair):
    out = np.full(L.PAIR_RECORD_VALUES, np.nan)
    L.check(L.lib().mp_debug_pair_set_record(ps._h, pair, out.ctypes.data_as(L.c_double_p)))
    return out


def _same(a, b):
    return (a.offsets.tobytes() == b.offsets.tobytes() and a.counts.tobytes() == b.counts.tobytes()
            and a.mask.tobytes() == b.mask.tobytes()
            and (a.errors is None) == (b.errors is None)
            and (a.errors is None or a.errors.tobytes() == b.errors.tobytes()))


# ---- 1. the lists ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_mask_is_selects_lists(sets, variant):
    k, ps, res = sets(variant)
    assert res.offsets.dtype == np.int64 and res.counts.dtype == np.int32 and res.mask.dtype == np.uint8
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum([W.SIZES[i] for i in k.ids])]).tolist()
    assert res.mask.shape == (int(res.offsets[-1]),) and res.errors.shape == (3, int(res.offsets[-1]))
    assert not np.any(res.mask & 0xF8)
    mixed = 0
    for j, kind in enumerate(W.KINDS):
        entries = [e for e in range(k.ne) if k.kinds[e] == kind]
        assert [k.ids[e] for e in entries] == list(range(len(k.pairs)))
        sel = ps.select([k.rows17[e:e + 1] for e in entries])
        for e, s in zip(entries, sel):
            m = res.mask[res.rows(e)]
            n = W.SIZES[k.ids[e]]
            assert len(m) == n
            if kind == "nan":
                assert not m.any() and res.counts[e].tolist() == [0, 0, 0], (variant, e)
                continue
            assert s.index == 0, (variant, e, kind)
            for t in range(3):
                assert _bits(m, t).tobytes() == s.inlier_indices[t].tobytes(), (variant, e, kind, t)
                assert res.counts[e, t] == len(s.inlier_indices[t])
            if n >= 4095:
                mixed += 0 < int(res.counts[e].sum()) < 3 * n
                print(f"variant {variant} {kind} n {n}: inlier fractions {(res.counts[e] / n).round(3).tolist()}")
    assert mixed >= 4  # (the large pairs have rows inside and outside the thresholds)


# ---- 2. the errors ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_errors_are_score_models_errors(sets, variant):
    k, ps, res = sets(variant)
    norm = ps.norm_scale
    for e in range(k.ne):
        p = k.pairs[k.ids[e]]
        if len(p["depth0"]) == 0:
            continue
        args = RC.pair_args(variant, p)
        m = RC.to_problem_units(variant, k.models[e], norm[k.ids[e]])
        _, err = madpose.score_models(variant, *args[:4], *args[5:], k.o, k.c, [m], with_errors=True)
        got = res.errors[:, res.rows(e)]
        if k.kinds[e] == "nan":
            assert np.array_equal(got, err[0], equal_nan=True), (variant, e)
            assert np.isnan(got).any()
        else:
            assert got.tobytes() == np.ascontiguousarray(err[0]).tobytes(), (variant, e)
            assert np.all(np.isfinite(got))


@pytest.mark.parametrize("score_type", [1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
def test_errors_are_ungated(sets, variant, score_type):
    k0, _, want = sets(variant)
    k, ps, res = sets(variant, score_type)
    assert k.c.score_type == score_type and k0.c.score_type == 0
    for e in range(k.ne):
        a, b = res.errors[:, res.rows(e)], want.errors[:, want.rows(e)]
        if k.kinds[e] == "nan":
            assert np.array_equal(a, b, equal_nan=True)
        else:
            assert a.tobytes() == b.tobytes(), (variant, score_type, e)
    assert res.mask.tobytes() == want.mask.tobytes() and res.counts.tobytes() == want.counts.tobytes()


# ---- 3. the factor ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_factor_counts_are_lsq_fits_wide_counts(sets, variant):
    k, ps, base = sets(variant)
    for factor in (1.5, k.mix):
        res = ps.residuals(k.models, pair_ids=k.ids, factor=factor, errors=True)
        fits = ps.lsq_fit(k.models, 0, factor=factor, pair_ids=k.ids)
        assert res.counts.tolist() == [f.num_wide for f in fits]
        assert res.errors.tobytes() == base.errors.tobytes()  # (the factor moves no error)
        f = np.broadcast_to(np.asarray(factor, dtype=np.float64), (k.ne,))
        for e in range(k.ne):
            if f[e] == 1.0:
                assert res.mask[res.rows(e)].tobytes() == base.mask[base.rows(e)].tobytes()
            assert res.counts[e].tolist() == [len(_bits(res.mask[res.rows(e)], t)) for t in range(3)]
        if variant != 0:
            continue
        # calibrated: the comparison restated in numpy on the record's thresholds
        for e in range(k.ne):
            thr = _record(ps, k.ids[e])[:3]
            assert thr.tolist() == [float(v) for v in RC.thresholds(0, k.o, 1.0)]
            err = res.errors[:, res.rows(e)]
            with np.errstate(invalid="ignore"):
                want = sum(((err[t] < np.float64(thr[t]) * np.float64(f[e])).astype(np.uint8) << t) for t in range(3))
            assert res.mask[res.rows(e)].tobytes() == np.asarray(want, dtype=np.uint8).tobytes(), e
    wide = ps.residuals(k.models, pair_ids=k.ids, factor=1.5)
    assert wide.errors is None and np.all(wide.counts >= base.counts) and np.any(wide.counts > base.counts)


# ---- 4. batch invariance ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_an_entry_does_not_depend_on_its_call(sets, variant):
    k, ps, _ = sets(variant)
    whole = ps.residuals(k.rows17, pair_ids=k.ids, factor=k.mix, errors=True)
    # every entry alone (a pair occurs three times in the call, under different models)
    for e in range(k.ne):
        one = ps.residuals(k.rows17[e:e + 1], pair_ids=[k.ids[e]], factor=k.mix[e], errors=True)
        assert one.offsets.tolist() == [0, W.SIZES[k.ids[e]]]
        assert one.counts[0].tolist() == whole.counts[e].tolist()
        assert one.mask.tobytes() == whole.mask[whole.rows(e)].tobytes()
        assert one.errors.tobytes() == np.ascontiguousarray(whole.errors[:, whole.rows(e)]).tobytes()
    # a permutation of the entries
    perm = np.random.default_rng(variant).permutation(k.ne)
    shuffled = ps.residuals(k.rows17[perm], pair_ids=[k.ids[e] for e in perm], factor=k.mix[perm], errors=True)
    for j, e in enumerate(perm):
        assert shuffled.counts[j].tolist() == whole.counts[e].tolist()
        assert shuffled.mask[shuffled.rows(j)].tobytes() == whole.mask[whole.rows(e)].tobytes()
        assert (np.ascontiguousarray(shuffled.errors[:, shuffled.rows(j)]).tobytes()
                == np.ascontiguousarray(whole.errors[:, whole.rows(e)]).tobytes())
    # pose objects and rows are the same models; pair_ids None is every pair in order
    assert _same(ps.residuals(k.models, pair_ids=k.ids, factor=k.mix, errors=True), whole)
    first = [e for e in range(k.ne) if k.kinds[e] == "truth"]
    assert _same(ps.residuals(k.rows17[first]), ps.residuals(k.rows17[first], pair_ids=list(range(len(k.pairs)))))


def test_the_cut_into_runs_changes_nothing(sets, monkeypatch):
    k, ps, _ = sets(1)
    whole = ps.residuals(k.rows17, pair_ids=k.ids, factor=k.mix, errors=True)
    for rows, entries in ((1, 1 << 15), (5000, 4), (8193, 1 << 15), (1 << 21, 2)):
        monkeypatch.setenv("MADPOSE_RESIDUALS_RUN_ROWS", str(rows))
        monkeypatch.setenv("MADPOSE_RESIDUALS_RUN_ENTRIES", str(entries))
        assert _same(ps.residuals(k.rows17, pair_ids=k.ids, factor=k.mix, errors=True), whole), (rows, entries)
    monkeypatch.setenv("MADPOSE_RESIDUALS_RUN_ROWS", "0")
    with pytest.raises(ValueError, match="MADPOSE_RESIDUALS_RUN_ROWS"):
        ps.residuals(k.rows17, pair_ids=k.ids)


def test_host_outputs_given_by_the_caller(sets):
    k, ps, want = sets(2)
    R = int(want.offsets[-1])
    mask, err = np.full(R, 0xAB, dtype=np.uint8), np.full((3, R), np.nan)
    res = ps.residuals(k.rows17, pair_ids=k.ids, out_mask=mask, out_errors=err)
    assert res.mask is mask and res.errors is err and _same(res, want)
    only = ps.residuals(k.rows17, pair_ids=k.ids, out_errors=err)
    assert only.errors is err and only.mask.tobytes() == want.mask.tobytes()


# ---- 5. host against device (the child process) ----

def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("MADPOSE_")}


@pytest.fixture(scope="module")
def outcomes():
    r = subprocess.run([sys.executable, "-m", "tests.residuals_worker"], env=_env(), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(lines[-1])


@pytest.mark.parametrize("name", list(W.CHECKS))
def test_device_check(outcomes, name):
    got = outcomes.get(name)
    assert got is not None, f"the worker did not run {name}"
    print(got["detail"], got["seconds"])
    assert got["ok"], got["detail"]


def test_the_checks_cover_the_issue():
    names = set(W.CHECKS)
    for v in VARIANTS:
        assert f"device_outputs_equal_host_outputs[{v}]" in names
    assert {"outputs_last_written_on_another_stream", "bad_device_outputs_are_refused_in_python",
            "short_and_overlapping_buffers_are_refused_by_the_library",
            "runs_write_device_outputs_in_place"} <= names
    assert W.SIZES == (0, 1, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193) and W.GUARD == 64


# ---- 6. against ransac and refine ----

def _assert_lists(res, e, lists, what):
    m = res.mask[res.rows(e)]
    for t in range(3):
        assert _bits(m, t).tobytes() == np.asarray(lists[t], dtype=np.int32).tobytes(), (what, e, t)
        assert res.counts[e, t] == len(lists[t])


def test_calibrated_ransac_lists_are_reproduced(sets):
    k, ps, _ = sets(0)
    rs = ps.ransac(budget=64, step=32, lo=1, seed=7)
    won = [i for i, r in enumerate(rs) if r.index >= 0]
    assert len(won) >= 8 and any(r.rounds_accepted > 0 for r in rs)
    res = ps.residuals(np.stack([rs[i].model_row for i in won]), pair_ids=won)
    for e, i in enumerate(won):
        _assert_lists(res, e, rs[i].inlier_indices, "ransac")
    assert sum(len(a) for i in won for a in rs[i].inlier_indices) > 1000


def test_scale_only_refine_lists_are_reproduced(sets):
    k, ps, _ = sets(3)
    starts = [k.models[e] for e in range(k.ne) if k.kinds[e] == "perturbed"]
    rf = ps.refine(starts, rounds=3)
    assert any(r.rounds_accepted > 0 for r in rf)
    res = ps.residuals([r.model for r in rf])
    for e, r in enumerate(rf):
        _assert_lists(res, e, r.inlier_indices, "refine")


@pytest.mark.parametrize("variant", [1, 2])
def test_focal_ransac_lists_without_final_rounds_are_reproduced(sets, variant):
    k, ps, _ = sets(variant)
    rs = ps.ransac(budget=64, seed=7, rounds=0)
    won = [i for i, r in enumerate(rs) if r.index >= 0]
    assert len(won) >= 8
    res = ps.residuals(np.stack([rs[i].model_row for i in won]), pair_ids=won)
    for e, i in enumerate(won):
        _assert_lists(res, e, rs[i].inlier_indices, "ransac rounds=0")


@pytest.mark.parametrize("variant", [1, 2])
def test_refined_focal_models_differ_in_counted_rows(sets, variant):
    """Counted and printed, not asserted (the module docstring says why); measured on the
    MI355X: DESIGN.md 2.12."""
    k, ps, _ = sets(variant)
    rs = ps.ransac(budget=64, step=32, lo=1, seed=7)
    won = [i for i, r in enumerate(rs) if r.index >= 0]
    assert len(won) >= 8
    res = ps.residuals(np.stack([rs[i].model_row for i in won]), pair_ids=won)
    differ = total = 0
    for e, i in enumerate(won):
        m = res.mask[res.rows(e)]
        for t in range(3):
            want = np.zeros(len(m), dtype=bool)
            want[rs[i].inlier_indices[t]] = True
            differ += int(np.sum(want != (((m >> t) & 1) == 1)))
            total += len(m)
    print(f"variant {variant}: {differ} of {total} mask bits differ from the refined models' lists")


# ---- 7. interleaving, a repeated call, exit with the set open ----

def test_interleaved_with_other_stages_and_repeated(sets):
    k, ps, want = sets(0)
    cands = [k.rows17[e:e + 1] for e in range(k.ne) if k.kinds[e] == "perturbed"]
    starts = [k.models[e] for e in range(k.ne) if k.kinds[e] == "perturbed"]
    key = lambda rs: [(r.index, r.score, tuple(a.tobytes() for a in r.inlier_indices)) for r in rs]
    s1 = key(ps.select(cands))
    a = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
    f1 = [RC.result_key(0, r) for r in ps.refine(starts, rounds=2)]
    b = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
    s2 = key(ps.select(cands))
    c = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
    f2 = [RC.result_key(0, r) for r in ps.refine(starts, rounds=2)]
    assert _same(a, want) and _same(b, want) and _same(c, want)
    assert s1 == s2 and f1 == f2
    launches = np.zeros(1, dtype=np.int64)
    L.check(L.lib().mp_debug_residuals_stats(launches.ctypes.data_as(L.c_int64_p), None, 0))
    assert launches[0] >= 3


EXIT_CODE = r"""
import numpy as np
import madpose
from tests import residuals_worker as W
k = W.case(1)
ps = W.open_set(k)
res = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
assert res.mask.any() and res.counts.sum() == sum(int(((res.mask >> t) & 1).sum()) for t in range(3))
print("DONE", len(ps), int(res.offsets[-1]), flush=True)
# forget the handle: the set stays open in the library, whatever the interpreter finalises
ps._h = None
"""


def test_exit_with_the_set_open():
    r = subprocess.run([sys.executable, "-c", EXIT_CODE], env=_env(), capture_output=True, text=True, timeout=240,
                       cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"DONE {len(W.SIZES)} {3 * sum(W.SIZES)}" in r.stdout, r.stdout[-2000:]
    low = r.stderr.lower()
    assert "hip" not in low and "error" not in low and "fault" not in low, r.stderr[-4000:]
