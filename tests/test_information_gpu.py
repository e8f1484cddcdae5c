"""PairSet.information (mp_information_set): per entry the Gauss-Newton system of the estimators'
cost over a model's inliers, and its inverse, from information_kernel and
information_finish_kernel (madpose_amd/csrc/kernels/information.h).

The systems are held to tests/lm_reference.py with the bound of tests/lm_system_cases.py
(check_system, where = 3: (K_ENGINE + rows) 2^-53 S_X per entry, exact zeros on inactive
parameters): small pairs against 50 digits, the sizes either side of a wave, a 256-row trip and
an item of 4096 rows against float64 + fsum.  The block lists of the references are read from
PairSet.residuals; the reference's doubles are SC.engine_doubles with the set's norm_scale and its
focals the user's over norm_scale, the engine's own division.  The covariance is held to the
column-wise backward error of tests/information_worker.column_check on the device's own H.  The
device-output checks run in ONE child process that imports torch first
(tests/information_worker.py).  Without the feature PairSet has no information and every test here
fails."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from tests import information_worker as IW
from tests import lm_system_cases as SC
from tests import refine_cases as RC
from tests import residuals_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (0, 1, 2, 3)

# printed by every run of test_small_pairs_against_50_digits: the device's worst per-term error in
# units of 2^-53 S_X beside the rows' own share, per variant; the reference's float64 yardstick is
# SC.K_REF = 821 and the allowance SC.K_ENGINE = 16 K_REF.  The test passed on an MI355X (every
# figure below the allowance); the figures themselves were not kept from that run, so none is
# recorded here yet (None).  For the same blocks lm_system_kernel measured 296.0 / 250.2 / 801.9
# (tests/test_lm_system_gpu.py DEVICE_WORST_MEASURED).
DEVICE_WORST_MEASURED = {0: None, 1: None, 2: None}

# the config variants of the 50-digit test: LO type 0 / 1 / 2, the depth bound on (no effect on
# the system), and use_shift off (read by the calibrated job only)
CONFIGS = {"lo0": dict(), "lo1": dict(lo_type=1), "lo2": dict(lo_type=2), "mdc": dict(mdc=True),
           "noshift": dict(use_shift=False)}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


@pytest.fixture(scope="module")
def sized():
    """one open set of the size case per variant, its residuals and its information (never changed)"""
    made = {}

    def get(variant):
        if variant not in made:
            k = IW.size_case(variant)
            o, c = IW.config(variant)
            ps = IW.open_set(k, o, c)
            rs = ps.residuals(k.rows17, pair_ids=k.ids)
            res = ps.information(k.rows17, pair_ids=k.ids)
            made[variant] = (k, o, c, ps, rs, res)
        return made[variant]
    yield get
    for entry in made.values():
        entry[3].close()


@pytest.fixture(scope="module")
def small():
    """the small case of a variant under a config: (case, o, c, norm_scale, residuals, information)"""
    made = {}

    def get(variant, name):
        if (variant, name) not in made:
            k = IW.small_case(variant)
            o, c = IW.config(variant, **CONFIGS[name])
            with IW.open_set(k, o, c) as ps:
                made[(variant, name)] = (k, o, c, ps.norm_scale, ps.residuals(k.rows17, pair_ids=k.ids),
                                         ps.information(k.rows17, pair_ids=k.ids))
        return made[(variant, name)]
    return get


def _check_entry(variant, k, o, c, norm, rs, res, e, mode, tag):
    """entry e against LR.system in `mode`; returns check_system's per-term figure"""
    p = k.pairs[k.ids[e]]
    ref = IW.reference(variant, p, o, c, norm[k.ids[e]], k.rows17[e], rs.mask[rs.rows(e)], mode)
    n0, n1, n2 = (len(l) for l in ref["lists"])
    assert res.counts[e].tolist() == rs.counts[e].tolist(), tag
    assert res.rows[e] == 2 * (n0 + n1) + n2 == ref["rows"], tag
    assert res.status[e] == (1 if ref["rows"] else 0), tag
    return SC.check_system(IW.entry(res, e), ref, 3, tag), ref


# ---- 1. against 50 digits ----

@pytest.mark.parametrize("variant", [0, 1, 2])
def test_small_pairs_against_50_digits(small, variant):
    worst = {}
    names = ["lo0", "lo1", "lo2", "mdc"] + (["noshift"] if variant == 0 else [])
    for name in names:
        k, o, c, norm, rs, res = small(variant, name)
        for e in range(k.ne):
            fig, ref = _check_entry(variant, k, o, c, norm, rs, res, e, "mp", (variant, name, e))
            assert res.pd[e] in ((0, 1) if ref["rows"] else (-1,))
            na = 9 + variant
            assert not np.any(res.g[e][na:]) and not np.any(res.col[e][na:])
            worst[name] = max(worst.get(name, 0.0), fig)
        if name == "lo1":
            assert not np.any(res.col[:, 6:9]) and np.all(res.rows == res.counts[:, 2])
        if name == "lo2":
            assert np.all(res.rows == 2 * (res.counts[:, 0] + res.counts[:, 1]))
        if name == "noshift":
            assert not np.any(res.col[:, 7:9]) and np.all(res.col[:, 6] == 1)
    base, mdc = small(variant, "lo0"), small(variant, "mdc")
    for e in range(base[0].ne):  # (the depth bound is not read: nothing is optimised)
        assert IW.entry_bytes(base[5], e) == IW.entry_bytes(mdc[5], e)
    for name in names:
        print(f"variant {variant} {name:8s} worst per-term error {worst[name]:.1f}")
    print(f"variant {variant}: device worst {max(worst.values()):.1f} (recorded {DEVICE_WORST_MEASURED[variant]}); "
          f"K_REF {SC.K_REF}, allowance {SC.K_ENGINE}")


# ---- 2. reduction and item carry ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_reduction_and_item_carry(sized, variant):
    """every size of W.SIZES and the pair of 6000 under the perturbed model (the sizes up to 257
    also under the ground truth) against float64 + fsum; an entry of one block against 50 digits,
    as test_lm_system_gpu.py::test_reduction_and_list_carry does"""
    k, o, c, ps, rs, res = sized(variant)
    norm = ps.norm_scale
    worst, mixed = 0.0, 0
    for e in range(k.ne):
        n = k.sizes[k.ids[e]]
        assert res.counts[e].tolist() == rs.counts[e].tolist()
        if k.kinds[e] == "nan" or n == 0 or (k.kinds[e] == "truth" and n > 257):
            continue
        one = int(rs.counts[e].sum()) == 1
        fig, ref = _check_entry(variant, k, o, c, norm, rs, res, e, "mp" if one else "f64", (variant, n, k.kinds[e]))
        worst = max(worst, fig)
        if n >= IW.ITEM - 1:
            mixed += all(0 < int(rs.counts[e, t]) < n for t in range(3))
            print(f"variant {variant} n {n}: inlier fractions {(rs.counts[e] / n).round(3).tolist()} pd {res.pd[e]}")
    # the large pairs have rows inside and outside each threshold, so gating is exercised
    assert mixed >= 4
    print(f"variant {variant}: worst per-term error {worst:.1f}")


# ---- 3. variant 3 and the cross-check against the one-pair hook ----

@pytest.mark.parametrize("name", ["lo0", "lo1", "lo2"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_system_equals_lm_system_hook(small, variant, name):
    """the same pair, lists and problem-unit model through madpose.lm_system(where = 0): col
    identical and every entry within the sum of the two bounds (each is held to the reference on
    its own); for variant 3 this is the definition, make_lm_job's scale-only job"""
    k, o, c, norm, rs, res = small(variant, name)
    for e in range(k.ne):
        p = k.pairs[k.ids[e]]
        mask = rs.mask[rs.rows(e)]
        lists = [np.flatnonzero((mask >> t) & 1).astype(np.int32) for t in range(3)]
        m = RC.to_problem_units(variant, k.models[e], norm[k.ids[e]])
        hook = madpose.lm_system(variant, *RC.pair_args(variant, p), o, c, [(0, lists, m)], 1e4)
        assert hook["status"][0] == res.status[e]
        if res.status[e] == 0:  # (no block left: the hook reports the set-up's columns, this stage zeros)
            assert hook["pd"][0] == -1 == res.pd[e] and not np.any(res.col[e]) and not np.any(res.H[e])
            continue
        assert hook["col"][0].tolist() == res.col[e].tolist(), (variant, name, e)
        ref = IW.reference(variant, p, o, c, norm[k.ids[e]], k.rows17[e], mask, "f64")
        # on the active parameters (the hook's full layout keeps the raw sums of inactive ones, where
        # this stage has its exact zeros: check_system's where = 0 against where = 3)
        col = np.asarray(res.col[e], bool)
        both = np.array([col[a] and col[b] for a in range(11) for b in range(a, 11)])
        keep = np.r_[True, col, both]
        X = np.r_[res.cost[e], res.g[e], res.H[e]]
        Y = np.r_[hook["cost"][0], hook["g"][0], hook["H"][0]]
        S = np.r_[ref["S_cost"], ref["S_g"], ref["S_H"]]
        assert np.all(np.abs(X - Y)[keep] <= (2 * (SC.K_ENGINE + ref["rows"]) * SC.U * S)[keep]), (variant, name, e)
        assert np.all(X[~keep] == 0.0)
    if variant == 3:
        assert not np.any(res.col[:, 7:]) and (name == "lo1" or np.all(res.col[:, 6] == 1))


# ---- 4. the covariance on the device ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_covariance_columns_on_the_device(sized, small, variant):
    k, o, c, ps, rs, res = sized(variant)
    worst, done = 0.0, 0
    for e in range(k.ne):
        col = np.asarray(res.col[e], bool)
        assert not np.any(res.cov[e][~col, :]) and not np.any(res.cov[e][:, ~col])
        n = k.sizes[k.ids[e]]
        if k.kinds[e] == "truth" and n >= IW.ITEM - 1:
            # the ground truth of a mixed pair (blocks of all three types, test_reduction_and_item_carry)
            assert all(0 < int(res.counts[e, t]) < n for t in range(3)) and res.pd[e] == 1, (variant, n)
        if res.pd[e] != 1:
            assert not np.any(res.cov[e])
            continue
        worst = max(worst, IW.column_check(res.H[e], res.col[e], res.cov[e], (variant, e)))
        done += 1
        C = res.covariance(e, scaled=False)
        assert np.array_equal(C, C.T) and C.shape == (int(col.sum()),) * 2
    assert done >= 12
    # a Sampson-only entry: |t| is a gauge; whatever pd it gets is reported, not asserted
    ks, _, _, _, _, lo1 = small(variant, "lo1")
    print(f"variant {variant}: {done} inverses, worst column backward error {worst:.2f}; Sampson-only pd "
          f"{lo1.pd.tolist()}")
    e = next(e for e in range(k.ne) if k.kinds[e] == "truth" and k.sizes[k.ids[e]] == 8193)
    S = res.covariance(e)
    assert np.all(np.diag(S) > 0)
    without = ps.information(k.rows17, pair_ids=k.ids, covariance=False)
    assert without.cov is None and without.pd.tobytes() == res.pd.tobytes() and without.H.tobytes() == res.H.tobytes()


# ---- 5. independence ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_an_entry_does_not_depend_on_its_call(sized, variant, monkeypatch):
    k, o, c, ps, rs, res = sized(variant)
    again = ps.information(k.rows17, pair_ids=k.ids)
    for e in range(k.ne):
        assert IW.entry_bytes(again, e) == IW.entry_bytes(res, e)
    picks = [e for e in range(k.ne) if k.kinds[e] == "perturbed" and k.sizes[k.ids[e]] in (1, 257, 4097, 8193, IW.BIG)]
    for e in picks:
        alone = ps.information(k.rows17[e:e + 1], pair_ids=[k.ids[e]])
        assert IW.entry_bytes(alone, 0) == IW.entry_bytes(res, e), (variant, e)
        # among 40 others, and twice through repeated pair_ids
        others = np.random.default_rng(e).integers(0, k.ne, 40).tolist()
        order = others[:13] + [e] + others[13:] + [e]
        many = ps.information(k.rows17[order], pair_ids=[k.ids[j] for j in order])
        assert IW.entry_bytes(many, 13) == IW.entry_bytes(res, e) == IW.entry_bytes(many, 41)
    # a factor per entry equals the scalar call
    mix = ps.information(k.rows17, pair_ids=k.ids, factor=k.mix)
    for f in (1.5, 0.75):
        whole = ps.information(k.rows17, pair_ids=k.ids, factor=f)
        for e in np.flatnonzero(k.mix == f):
            assert IW.entry_bytes(whole, e) == IW.entry_bytes(mix, e)
    wide = ps.residuals(k.rows17, pair_ids=k.ids, factor=k.mix)
    assert mix.counts.tobytes() == wide.counts.tobytes()
    # the cut into runs, and host outputs given by the caller
    for rows, entries in ((1, 1 << 13), (5000, 4), (1 << 22, 3)):
        monkeypatch.setenv("MADPOSE_INFORMATION_RUN_ROWS", str(rows))
        monkeypatch.setenv("MADPOSE_INFORMATION_RUN_ENTRIES", str(entries))
        cut = ps.information(k.rows17, pair_ids=k.ids)
        for e in range(k.ne):
            assert IW.entry_bytes(cut, e) == IW.entry_bytes(res, e), (rows, entries, e)
    monkeypatch.delenv("MADPOSE_INFORMATION_RUN_ROWS")
    monkeypatch.delenv("MADPOSE_INFORMATION_RUN_ENTRIES")
    H, cov = np.full((k.ne, 66), np.nan), np.full((k.ne, 11, 11), np.nan)
    given = ps.information(k.rows17, pair_ids=k.ids, out_H=H, out_cov=cov)
    assert given.H is H and given.cov is cov and H.tobytes() == res.H.tobytes() and cov.tobytes() == res.cov.tobytes()
    # pose objects are the same models as their rows
    objs = ps.information(k.models, pair_ids=k.ids)
    assert all(IW.entry_bytes(objs, e) == IW.entry_bytes(res, e) for e in range(k.ne))


# ---- 6. nothing evaluated ----

@pytest.mark.parametrize("variant", VARIANTS)
def test_nothing_evaluated(sized, variant):
    k, o, c, ps, rs, res = sized(variant)

    def nothing(r, e, counts_zero=True):
        assert r.status[e] == 0 and r.pd[e] == -1 and r.rows[e] == 0, (variant, e)
        assert not np.any(r.H[e]) and not np.any(r.g[e]) and r.cost[e] == 0.0 and not np.any(r.cov[e])
        assert not np.any(r.col[e]) and (not counts_zero or not np.any(r.counts[e]))
    seen = set()
    for e in range(k.ne):
        n = k.sizes[k.ids[e]]
        if k.kinds[e] == "nan" or n == 0:
            nothing(res, e)
            seen.add("nan" if n else "empty")
        elif n >= 63:
            assert res.status[e] == 1 and res.pd[e] >= 0 and np.any(res.H[e])  # neighbours are untouched
    assert seen == {"nan", "empty"}
    # a factor so small that no row passes, between two entries that are evaluated
    e = next(e for e in range(k.ne) if k.kinds[e] == "truth" and k.sizes[k.ids[e]] == 4097)
    order = [e, e, e]
    r = ps.information(k.rows17[order], pair_ids=[k.ids[e]] * 3, factor=[1.0, 1e-300, 1.0])
    nothing(r, 1)
    assert IW.entry_bytes(r, 0) == IW.entry_bytes(res, e) == IW.entry_bytes(r, 2)
    # blocks exist but the LO type drops them all: counts are kept, nothing is evaluated
    with pytest.raises(ValueError, match="no covariance"):
        r.covariance(1)


# ---- 7. device outputs (the child process) ----

def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("MADPOSE_")}


@pytest.fixture(scope="module")
def outcomes():
    r = subprocess.run([sys.executable, "-m", "tests.information_worker"], env=_env(), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(lines[-1])


@pytest.mark.parametrize("name", list(IW.CHECKS))
def test_device_check(outcomes, name):
    got = outcomes.get(name)
    assert got is not None, f"the worker did not run {name}"
    print(got["detail"], got["seconds"])
    assert got["ok"], got["detail"]


def test_the_checks_cover_the_issue():
    names = set(IW.CHECKS)
    for v in VARIANTS:
        assert f"device_outputs_equal_host_outputs[{v}]" in names
    assert {"rows_of_other_entries_keep_a_sentinel", "the_sets_lists_are_unchanged",
            "mixed_kinds_and_overlapping_tensors_are_refused", "outputs_last_written_on_another_stream",
            "runs_write_device_outputs_in_place"} <= names
    assert IW.ITEM == 4096 and {1, 63, 64, 65, 255, 256, 257, IW.ITEM - 1, IW.ITEM, IW.ITEM + 1} <= set(W.SIZES)
