"""PairSet.ransac(step=...) on the device (mp_ransac_adaptive_set).  Every comparison is of
bytes against entries that exist without the feature: a pair's adaptive result against
ransac(budget=its num_samples, pair_ids=[that pair]); its stop point against the rule's
Python restatement (tests/ransac_stop_restatement.py) walked over ransac(budget=m_k, rounds=0)
and draw's types.

One set per variant: n = 0, 4, 64 and three pairs of n = 300 with outlier ratios
OUTLIER_RATIOS; example options with min_num_iterations = 8; budget 512 in steps of 48 (48
does not divide 512: the last round has 32 samples)."""
import functools
import os
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import refine_cases as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_stop_restatement as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 4, 64, 300, 300, 300)
OUTLIER_RATIOS = (0.3, 0.3, 0.3, 0.0, 0.3, 0.9)
BUDGET, STEP = 512, 48
SEED = 0xADA9717E5EED0001
ROUNDS = 2
SUBSET = [5, 2, 3, 0]  # a permuted subset
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _pair(variant, i, n, outliers):
    K0 = np.array([[520.0 + 37 * (i % 3), 0, 310.0 + 5 * i], [0, 515.0 + 41 * (i % 2), 236.0 + 3 * i], [0, 0, 1.0]])
    K1 = K0.copy()
    if variant == 2:
        K1[0, 0] = K1[1, 1] = 380.0 + 23 * (i % 4)
        K0[1, 1] = K0[0, 0]
    elif variant == 1:
        K0[1, 1] = K0[0, 0]
        K1 = K0.copy()
    else:
        K1[0, 2] += 7.0
    p = synthetic.make_pair(1300 + i, n=max(n, 8), K0=K0, K1=K1, outlier_ratio=outliers)
    if n < 8:
        for k in ("x0", "x1", "depth0", "depth1", "inlier_mask"):
            p[k] = p[k][:n]
    return p


def key(r, variant):
    """every field of a RansacResult the contract names, as comparable bytes"""
    return (r.num_samples, r.num_candidates, r.index, r.sample, r.slot, r.solver_type,
            np.float64(r.score_selected).tobytes(), np.float64(r.score_initial).tobytes(),
            np.float64(r.score_final).tobytes(), r.rounds_run, r.rounds_accepted, r.status,
            np.float64(r.norm_scale).tobytes(), r.model_row.tobytes(), r.model is None,
            tuple(a.tobytes() for a in r.inlier_indices))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(variant):
    """The set, and what the entries without the feature say: the fixed-budget winners at
    every checkpoint and the drawn types, from which the expected stop points follow."""
    k = Case()
    k.variant = variant
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.o.min_num_iterations = 8
    k.pairs = [_pair(variant, i, n, q) for i, (n, q) in enumerate(zip(SIZES, OUTLIER_RATIOS))]
    k.ps = madpose.PairSet(variant, k.pairs, k.o, k.c)
    k.marks = S.checkpoints(STEP, BUDGET)
    k.fixed = {m: k.ps.ransac(budget=m, seed=SEED, rounds=0) for m in k.marks}
    k.types = [t for t, _ in k.ps.draw(BUDGET, SEED)]
    k.expect = [_walk(k, j, k.marks, BUDGET) for j in range(len(SIZES))]
    return k


def _walk(k, j, marks, budget, fixed=None):
    """(num_samples, stopped) of pair j: the first checkpoint at which the rule holds on the
    fixed-budget winner and the drawn types"""
    fixed = k.fixed if fixed is None else fixed
    n, types = SIZES[j], k.types[j]
    if len(types) == 0:
        return 0, False
    for m in marks:
        r = fixed[m][j]
        assert r.num_samples == m
        counts = [len(a) for a in r.inlier_indices] if r.index >= 0 else None
        req = S.required(k.variant, n, counts, k.o.success_probability, k.o.min_num_iterations,
                         k.o.max_num_iterations_per_solver)
        d1 = int(types[:m].sum())
        if S.stop_reached(req, (m - d1, d1)):
            return m, True
    return budget, False


def test_step_is_the_feature():
    """ransac(step=...) is a TypeError without the feature"""
    k = _case(0)
    out = k.ps.ransac(budget=BUDGET, step=STEP, seed=SEED, rounds=0)
    assert len(out) == len(SIZES) and all(isinstance(r.stopped, bool) for r in out)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_spread_of_the_stop_points(variant):
    """On the fixed-budget results alone (nothing of the code under test): the set has a pair
    that stops at the first checkpoint, one that stops strictly between it and the budget, and
    one that runs to the budget unstopped.

    Outlier ratios of the three n = 300 pairs: 0.0 / 0.3 / 0.9.  (With 0.05 / 0.45 / 0.9 the
    shared-focal set had no pair at the first checkpoint and the middle pair of every set ran
    to 512.)  Observed (num_samples, stopped) of the six pairs on an MI355X:
      calibrated    (0, F) (48, T) (240, T) (96, T) (240, T) (512, F)
      shared focal  (0, F) (512, F) (192, T) (48, T) (288, T) (512, F)
      two focal     (0, F) (512, F) (384, T) (48, T) (288, T) (512, F)"""
    k = _case(variant)
    print("expected stop points", variant, k.expect)
    assert k.expect[0] == (0, False)
    assert any(m == k.marks[0] and s for m, s in k.expect)
    assert any(k.marks[0] < m < BUDGET and s for m, s in k.expect)
    assert any(m == BUDGET and not s for m, s in k.expect)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("rounds", [0, ROUNDS])
def test_bytes_and_stop(variant, rounds):
    k = _case(variant)
    out = k.ps.ransac(budget=BUDGET, step=STEP, seed=SEED, rounds=rounds)
    print("stop points", variant, [(r.num_samples, r.stopped) for r in out])
    # ---- stop: the restatement's checkpoint ----
    assert [(r.num_samples, r.stopped) for r in out] == k.expect
    # ---- bytes: the fixed-budget call of that many samples on that pair alone ----
    for j, r in enumerate(out):
        want, = k.ps.ransac(budget=r.num_samples, seed=SEED, rounds=rounds, pair_ids=[j])
        assert key(r, variant) == key(want, variant), j
        assert want.stopped is False
    if rounds == 0:
        # a pair whose running best dates from a round before its last: its lists were left
        # alone by the later rounds (no sweep item, no write)
        old = [j for j, r in enumerate(out) if r.index >= 0 and r.num_samples > STEP
               and r.sample < STEP * ((r.num_samples - 1) // STEP)]
        assert old, [(r.num_samples, r.sample) for r in out]
        assert any(sum(len(a) for a in out[j].inlier_indices) > 0 for j in old)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_invariance(variant):
    k = _case(variant)
    ps = k.ps
    call = lambda **kw: ps.ransac(budget=BUDGET, step=STEP, seed=SEED, rounds=ROUNDS, **kw)
    keys = lambda rs: [key(r, variant) + (r.stopped,) for r in rs]
    base = keys(call())
    # a permuted subset
    assert keys(call(pair_ids=SUBSET)) == [base[j] for j in SUBSET]
    # no state: repeated, and with a fixed-budget call and a select in between
    ps.ransac(budget=40, seed=SEED + 1, rounds=1)
    cands = ps.candidates(ps.draw(16, SEED + 2))
    ps.select([c[0] for c in cands])
    assert keys(call()) == base
    # slabs that cut through entries, work items and rounds
    assert keys(call(sample_chunk=33, model_chunk=7)) == base
    assert keys(call(sample_chunk=1, model_chunk=1)) == base
    assert keys(call(sample_chunk=0, model_chunk=0)) == base
    # step >= budget: one round, ransac(budget)'s bytes for every pair
    fixed = [key(r, variant) for r in ps.ransac(budget=64, seed=SEED, rounds=ROUNDS)]
    for step in (64, 65, 1 << 30):
        assert [key(r, variant) for r in ps.ransac(budget=64, step=step, seed=SEED, rounds=ROUNDS)] == fixed
    # budget 0: no samples, no winners
    none = ps.ransac(budget=0, step=STEP, seed=SEED, rounds=ROUNDS)
    assert keys(none) == [key(r, variant) + (False,) for r in ps.ransac(budget=0, seed=SEED, rounds=ROUNDS)]
    assert all(r.index == -1 and r.num_samples == 0 and r.model is None for r in none)


def test_rule_options_are_read():
    """min_num_iterations above the budget on the same pairs: nothing stops, every result is
    ransac(512)'s"""
    k = _case(0)
    o, c = synthetic.example_options(RC.KIND[0])
    o.min_num_iterations = BUDGET + 1
    with madpose.PairSet(0, k.pairs, o, c) as ps:
        out = ps.ransac(budget=BUDGET, step=STEP, seed=SEED, rounds=0)
        want = ps.ransac(budget=BUDGET, seed=SEED, rounds=0)
    assert [key(r, 0) for r in out] == [key(r, 0) for r in want]
    assert not any(r.stopped for r in out)
    assert [r.num_samples for r in out] == [0] + [BUDGET] * 5


# ---- the seeded argmin on its own (mp_debug_select_argmin) ----
COUNTS = (0, 1, 63, 64, 65, 200, 200, 65, 1)


def _argmin(moff, scores, prior):
    P = len(moff) - 1
    index = np.full(P, -7, dtype=np.int32)
    score = np.full(P, -7.0)
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
    L.check(L.lib().mp_debug_select_argmin(P, moff.ctypes.data_as(L.c_int64_p), sc.ctypes.data_as(L.c_double_p),
                                           None if pr is None else pr.ctypes.data_as(L.c_double_p),
                                           index.ctypes.data_as(L.c_int32_p), score.ctypes.data_as(L.c_double_p), 0))
    return index, score


def _py_walk(scores, start):
    best, idx = start, -1
    for j, s in enumerate(scores.tolist()):
        if s < best:
            best, idx = s, j
    return idx, best


def test_seeded_argmin():
    rng = np.random.default_rng(77)
    moff = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    scores = rng.uniform(1.0, 1000.0, moff[-1])
    segs = [scores[moff[p]:moff[p + 1]] for p in range(len(COUNTS))]  # (views)
    # equal minima (the first wins), NaN and inf candidates, a pair of NaN only
    segs[5][[150, 20, 199]] = 0.25  # (below every other score)
    segs[6][[0, 3, 64, 128]] = [np.nan, np.inf, np.nan, -np.inf]
    segs[4][:] = np.nan
    segs[3][63] = 0.5          # the minimum in the last lane's only candidate
    segs[2][10] = np.nan
    with np.errstate(invalid="ignore"):
        lo = [np.nanmin(s) if len(s) and not np.isnan(s).all() else 1.0 for s in segs]
    priors = {
        "dbl_max": np.full(len(COUNTS), DBL_MAX),
        "below": np.array([m - 1.0 if np.isfinite(m) else -np.inf for m in lo]),
        "equal": np.array(lo, dtype=np.float64),
        "above_min": np.array([np.nextafter(m, np.inf) if np.isfinite(m) else m for m in lo]),
        "median": np.array([np.nanmedian(s) if len(s) and not np.isnan(s).all() else 5.0 for s in segs]),
        "nan": np.full(len(COUNTS), np.nan),
        "inf": np.full(len(COUNTS), np.inf),
    }
    for name, prior in priors.items():
        index, score = _argmin(moff, scores, prior)
        for p in range(len(COUNTS)):
            idx, best = _py_walk(segs[p], float(prior[p]))
            assert index[p] == idx, (name, p)
            # unchanged: the prior's own bits; else the winner's
            want = prior[p] if idx < 0 else best
            assert np.float64(score[p]).tobytes() == np.float64(want).tobytes(), (name, p)
        if name == "equal":  # strict <: a candidate equal to the prior does not replace it
            assert (index[[1, 2, 3, 5, 7, 8]] == -1).all()
        if name == "above_min":
            assert index[5] == 20 and index[3] == 63
    # the unseeded launch: the walk from DBL_MAX, DBL_MAX without a winner
    index, score = _argmin(moff, scores, None)
    seeded, _ = _argmin(moff, scores, priors["dbl_max"])
    assert (index == seeded).all()
    for p in range(len(COUNTS)):
        idx, best = _py_walk(segs[p], DBL_MAX)
        assert index[p] == idx and score[p] == (best if idx >= 0 else DBL_MAX)
    assert index[0] == -1 and index[4] == -1
