"""Confidence-weighted sampling on the device (PairSet.draw_weights, draw(weights=),
ransac(weights=); mp_draw_weights_create, mp_draw_weighted_set, mp_ransac_weighted_set).

  1. the tables, flags and totals against tests/weighted_draw_restatement.py, for host-given
     weights here and device-given weights in one child process (tests/draw_weighted_worker.py,
     which imports torch first), float32 and float64, pairs either side of every size at which
     the code takes another path;
  2. the drawn bytes against the restatement: over two items and a remainder, under a permuted
     subset, and through ransac with sample_chunk=50;
  3. equal weights against the unweighted calls, byte for byte, in all four modes;
  4. ransac(weights=) against the chain on draw(weights=), and the adaptive modes against their
     existing definitions with the weighted fixed-budget call in the uniform one's place;
  5. masked rows never occur in a winner's sample;
  6. the effect at 70 % outliers with a budget of 32.
Without the feature PairSet has no draw_weights and draw / ransac no weights=: every test fails."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import draw_weighted_worker as W
from tests import lsq_subset_restatement as Z
from tests import ransac_lo_walk as LW

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restatement as D  # noqa: E402
import ransac_stop_restatement as S  # noqa: E402
import test_ransac_adaptive_gpu as A  # noqa: E402  (a set with inliers and outliers, its options and key)
import test_ransac_set_gpu as RS  # noqa: E402  (the chain and the result keys)
import weighted_draw_restatement as WD  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = W.SEED
BUDGET, STEP = 130, 48


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


@functools.lru_cache(maxsize=None)
def _open(variant):
    """the worker's case as an open set with its host-given float64 weights (kept for the module)"""
    k = W.case(variant, "float64")
    ps = madpose.PairSet(variant, k.pairs, k.o, k.c)
    return k, ps, ps.draw_weights(k.weights)


# ---- 1. the table ----

@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_host_given_table_equals_restatement(variant, dtype):
    k = W.case(variant, dtype)
    W.check_case(k)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        with ps.draw_weights(k.weights) as w:
            W.check_object(k, w)
            W.check_draw(k, ps, w)  # (the pairs that fell back draw today's bytes)
        # a mix of float32 and float64 entries is widened, exactly
        mixed = [a if a is None or i % 2 else a.astype(np.float32 if dtype == "float64" else np.float64)
                 for i, a in enumerate(k.weights)]
        km = [None if a is None else WD.table(a) for a in mixed]
        with ps.draw_weights(mixed) as w:
            assert w.total.tolist() == [0 if t is None else int(t[0][-1]) for t in km]
            assert w.positive.tolist() == [0 if t is None else t[1] for t in km]


def test_a_pair_above_65535_takes_no_weights():
    lib = L.lib()
    o, c = synthetic.example_options("calibrated")
    pairs = [W._pair(0, 50, 65536), W._pair(0, 51, 40)]
    with madpose.PairSet(0, pairs, o, c) as ps:
        buf = np.full(65536 + 40, 0.5)
        wh = ctypes.c_void_p()
        byref = ctypes.byref
        mask = np.array([1, 1], dtype=np.uint8)
        mp = lambda m: m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        assert lib.mp_draw_weights_create(ps._h, buf.ctypes.data, 1, 0, mp(mask), None, byref(wh)) == L.MP_EINVAL
        assert b"65535" in lib.mp_last_error() and not wh.value
        assert lib.mp_draw_weights_create(ps._h, buf.ctypes.data, 1, 0, None, None, byref(wh)) == L.MP_EINVAL
        with ps.draw_weights([None, np.full(40, 0.5)]) as w:
            assert w.weighted.tolist() == [False, True] and w.total.tolist() == [0, 40 * 32768]
            got = ps.draw(BUDGET, SEED, weights=w)
            assert W.skey(got) == W.skey(ps.draw(BUDGET, SEED))  # (equal weights; the big pair uniform)
        # a bad value in host-given weights reaches the library only through the C entry: the row is named
        buf[65536 + 7] = np.nan
        buf[65536 + 9] = 2.0
        mask[0] = 0
        assert lib.mp_draw_weights_create(ps._h, buf.ctypes.data, 1, 0, mp(mask), None, byref(wh)) == L.MP_EINVAL
        assert f"weights[{65536 + 7}] (pair 1, correspondence 7)".encode() in lib.mp_last_error()


# ---- the device-given weights: one child process ----

def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("MADPOSE_")}


@pytest.fixture(scope="module")
def outcomes():
    r = subprocess.run([sys.executable, "-m", "tests.draw_weighted_worker"], env=_env(), capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(lines[-1])


@pytest.mark.parametrize("name", list(W.CHECKS))
def test_device_given(outcomes, name):
    got = outcomes.get(name)
    assert got is not None, f"the worker did not run {name}"
    print(got["detail"], got["seconds"])
    assert got["ok"], got["detail"]


def test_the_sizes_cover_the_issue():
    for v in (0, 1, 2):
        k_md, k_pt = D.sizes(v)
        cap = L.DRAW_STAGE_ENTRIES
        assert {2, k_md - 1, k_md, k_pt - 1, k_pt, 63, 64, 65, 300, 65535, cap - 2, cap - 1, cap} <= set(W.sizes(v))
        for d in ("float32", "float64"):
            assert f"device_weights_equal_the_restatement[{v}-{d}]" in W.CHECKS


# ---- 2. the drawn bytes ----

@pytest.mark.parametrize("variant", [0, 1, 2])
def test_draw_equals_restatement(variant):
    k, ps, w = _open(variant)
    W.check_draw(k, ps, w, shares=(0, 256, 128))
    want = W.expected_draw(variant, "float64", 128)
    kk = {0: D.sizes(variant)[0], 1: D.sizes(variant)[1]}
    for i, (T, I) in enumerate(want):  # every index below n, masked ones absent, both types present
        if k.weighted[i]:
            q = np.diff(k.tables[i][0])
            for s in range(len(T)):
                row = I[s, :kk[int(T[s])]]
                assert row.max() < k.sizes[i] and (q[row] > 0).all()
    assert {0, 1} <= set(np.concatenate([T for T, _ in want]).tolist())
    # a subset draws what the whole set draws for its pairs, in any order
    sub = ps.draw(BUDGET, SEED, point_share=128, pair_ids=W.SUBSET, weights=w)
    assert W.skey(sub) == W.skey([want[i] for i in W.SUBSET])
    # through ransac, in slabs of 50 samples that cut through the items: the call on the restatement's samples
    got = ps.ransac(budget=BUDGET, seed=SEED, point_share=128, rounds=0, sample_chunk=50, weights=w)
    ref = ps.ransac(samples=want, rounds=0)
    assert RS._rkeys(variant, got) == RS._rkeys(variant, ref)
    assert sum(r.index >= 0 for r in got) >= 10
    got = ps.ransac(budget=BUDGET, seed=SEED, point_share=128, rounds=0, sample_chunk=50, weights=w, pair_ids=W.SUBSET)
    assert RS._rkeys(variant, got) == RS._rkeys(variant, [ref[i] for i in W.SUBSET])
    # the uniform call is untouched by the handle's existence
    assert W.skey(ps.draw(BUDGET, SEED, point_share=128)) == \
        W.skey([D.draw_pair(variant, n, SEED, 128, i, BUDGET)[:2] for i, n in enumerate(k.sizes)])


# ---- 3. equal weights ----

def _full_key(r, variant):
    return A.key(r, variant) + (r.stopped, r.lo_runs, r.lo_accepted, r.lo_index, r.lo_step, r.lo_stage,
                                r.lo_step_offers, r.lo_step_accepted)


MODES = (dict(), dict(step=STEP), dict(step=STEP, lo=1), dict(step=STEP, lo=1, lo_steps=2))


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("q", [1, 32768, 65535])
def test_equal_weights_are_the_unweighted_calls(variant, q):
    a = A._case(variant)
    value = 1.0 if q == 65535 else q / 65536.0
    with a.ps.draw_weights([np.full(n, value) for n in A.SIZES]) as w:
        assert w.weighted.tolist() == [n >= D.sizes(variant)[0] for n in A.SIZES]
        assert w.total.tolist() == [n * q for n in A.SIZES]
        assert W.skey(a.ps.draw(BUDGET, SEED, weights=w)) == W.skey(a.ps.draw(BUDGET, SEED))
        for mode in MODES if q == 32768 else MODES[:2]:
            got = a.ps.ransac(budget=BUDGET, seed=SEED, rounds=2, weights=w, **mode)
            want = a.ps.ransac(budget=BUDGET, seed=SEED, rounds=2, **mode)
            assert [_full_key(r, variant) for r in got] == [_full_key(r, variant) for r in want], mode
            assert any(r.index >= 0 for r in want)


# ---- 4. the chain ----

@functools.lru_cache(maxsize=None)
def _informed(variant):
    """the adaptive tests' set with confidences 1.0 on the true matches and 0.05 elsewhere"""
    a = A._case(variant)
    return a, a.ps.draw_weights([np.where(p["inlier_mask"], 1.0, 0.05) for p in a.pairs])


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_ransac_equals_the_chain_on_the_weighted_draw(variant):
    a, w = _informed(variant)
    drawn = a.ps.draw(BUDGET, SEED, weights=w)
    assert W.skey(drawn) != W.skey(a.ps.draw(BUDGET, SEED))
    for i, p in enumerate(a.pairs):  # (the draw is the restatement's here too)
        T, I, _ = WD.draw_any(variant, A.SIZES[i], np.where(p["inlier_mask"], 1.0, 0.05), SEED, 128, i, BUDGET)
        assert np.array_equal(drawn[i][0], T) and np.array_equal(drawn[i][1], I), i
    want = RS._chain(a.ps, variant, drawn, 3)
    got = a.ps.ransac(budget=BUDGET, seed=SEED, rounds=3, weights=w)
    assert RS._rkeys(variant, got) == want
    assert any(key[2] >= 0 and key[11] >= 1 for key in want)  # a refinement ran
    sub = a.ps.ransac(budget=BUDGET, seed=SEED, rounds=3, weights=w, pair_ids=A.SUBSET, sample_chunk=37, model_chunk=7)
    assert RS._rkeys(variant, sub) == [want[i] for i in A.SUBSET]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("rounds", [0, 2])
def test_step_equals_the_fixed_budget_call(variant, rounds):
    a, w = _informed(variant)
    out = a.ps.ransac(budget=A.BUDGET, step=STEP, seed=SEED, rounds=rounds, weights=w)
    print("stop points", variant, [(r.num_samples, r.stopped) for r in out])
    for j, r in enumerate(out):
        want, = a.ps.ransac(budget=r.num_samples, seed=SEED, rounds=rounds, pair_ids=[j], weights=w)
        assert A.key(r, variant) == A.key(want, variant), j
    assert any(r.stopped and r.num_samples < A.BUDGET for r in out)
    assert out[0].num_samples == 0 and not out[0].stopped


def _required(a):
    return lambda n, counts: S.required(a.variant, n, counts, a.o.success_probability, a.o.min_num_iterations,
                                        a.o.max_num_iterations_per_solver)


@functools.lru_cache(maxsize=None)
def _weighted_cache(variant):
    """ransac(budget=m, rounds=0, pair_ids=[p], weights=w) for every checkpoint: what the walks of
    tests/ransac_lo_walk.py and tests/lsq_subset_restatement.py read in the uniform call's place"""
    a, w = _informed(variant)
    marks = S.checkpoints(STEP, 240)
    cache = {}
    for m in marks:
        for p, r in enumerate(a.ps.ransac(budget=m, seed=SEED, rounds=0, weights=w)):
            cache[(p, m)] = r
    types = [t for t, _ in a.ps.draw(240, SEED)]  # (word 0's: the same with and without weights)
    assert W.skey([(t, t) for t in types]) == W.skey([(t, t) for t, _ in a.ps.draw(240, SEED, weights=w)])
    return marks, cache, types


def _compare_walk(variant, out, walks, steps):
    bits = lambda x: np.float64(x).tobytes()
    for j, (r, wk) in enumerate(zip(out, walks)):
        m, T = wk.minimal, wk.track
        assert (r.num_samples, r.stopped) == (wk.num_samples, wk.stopped), j
        assert (r.lo_runs, r.lo_accepted, r.lo_index) == (T.lo_runs, T.lo_accepted, T.lo_index), j
        if steps:
            ST = wk.steps
            assert (r.lo_step, r.lo_stage, r.lo_step_offers, r.lo_step_accepted) == (ST.lo_step, ST.lo_stage, ST.offers,
                                                                                    ST.accepted), j
        if m is None:
            assert r.index == -1 and r.model is None and r.num_candidates == 0, j
            continue
        assert (r.num_candidates, r.index, r.sample, r.slot, r.solver_type) == (
            m.num_candidates, m.index, m.sample, m.slot, m.solver_type), j
        assert bits(r.score_selected) == bits(m.score_selected) and bits(r.norm_scale) == bits(m.norm_scale), j
        assert (r.model is None) == (wk.model is None), j
        if wk.model is not None:
            assert RS.RC.model_bytes(variant, r.model) == RS.RC.model_bytes(variant, wk.model), j
        assert bits(r.score_initial) == bits(wk.score_initial) and bits(r.score_final) == bits(wk.score_final), j
        assert (r.rounds_run, r.rounds_accepted, r.status) == (wk.rounds_run, wk.rounds_accepted, wk.status), j
        for t in range(3):
            assert np.array_equal(r.inlier_indices[t], wk.lists[t]), (j, t)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_lo_equals_the_walk(variant):
    a, w = _informed(variant)
    marks, cache, types = _weighted_cache(variant)
    walks = [LW.lo_walk(a.ps, j, A.SIZES[j], types[j], marks, SEED, 1, 2, _required(a), S.stop_reached, cache)
             for j in range(len(A.SIZES))]
    out = a.ps.ransac(budget=240, step=STEP, seed=SEED, rounds=2, lo=1, weights=w)
    _compare_walk(variant, out, walks, False)
    assert any(r.lo_runs > 0 for r in out)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_lo_steps_equal_the_walk(variant):
    a, w = _informed(variant)
    marks, cache, types = _weighted_cache(variant)
    walks = [Z.lo_steps_walk(a.ps, j, A.SIZES[j], types[j], marks, SEED, 1, 2, 2, _required(a), S.stop_reached,
                             cache, int(a.o.num_lsq_iterations), float(a.o.threshold_multiplier),
                             int(a.o.non_min_sample_multiplier)) for j in range(len(A.SIZES))]
    out = a.ps.ransac(budget=240, step=STEP, seed=SEED, rounds=2, lo=1, lo_steps=2, weights=w)
    _compare_walk(variant, out, walks, True)
    assert any(r.lo_step_offers > 0 for r in out)


# ---- 5. masking ----

@pytest.mark.parametrize("variant", [0, 1, 2])
def test_masked_rows_never_reach_a_winner(variant):
    a = A._case(variant)
    masked = [np.flatnonzero(~p["inlier_mask"]) for p in a.pairs]
    with a.ps.draw_weights([np.where(p["inlier_mask"], 0.75, 0.0) for p in a.pairs]) as w:
        assert w.positive.tolist() == [int(p["inlier_mask"].sum()) for p in a.pairs]
        drawn = a.ps.draw(BUDGET, SEED, weights=w)
        winners = 0
        for mode in MODES:
            for j, r in enumerate(a.ps.ransac(budget=BUDGET, seed=SEED, rounds=1, weights=w, **mode)):
                if r.index < 0 or not w.weighted[j]:
                    continue
                k = D.sizes(variant)[r.solver_type]
                assert int(drawn[j][0][r.sample]) == r.solver_type
                assert not np.isin(drawn[j][1][r.sample, :k], masked[j]).any(), (mode, j)
                winners += 1
        assert winners >= 8
        for j in range(len(a.pairs)):  # and no sample at all holds one
            if w.weighted[j]:
                T, I = drawn[j]
                used = np.concatenate([I[s, :D.sizes(variant)[int(T[s])]] for s in range(len(T))])
                assert not np.isin(used, masked[j]).any(), j


# ---- 6. the effect ----

def test_informative_weights_find_better_models_at_a_small_budget():
    """16 calibrated pairs with 70 % outliers, confidences 1.0 on the true matches and 0.05
    elsewhere, 32 samples each, no refinement: the selected scores' sum is lower with the weights.
    An inlier is drawn with probability 0.3 / (0.3 + 0.7 * 0.05) ~ 0.90 instead of 0.3, so a 3-point
    (5-point) sample is all-inlier with probability ~0.72 (~0.58) instead of 0.027 (0.0024)."""
    o, c = synthetic.example_options("calibrated")
    pairs = [synthetic.make_pair(4000 + i, n=300, outlier_ratio=0.7) for i in range(16)]
    with madpose.PairSet(0, pairs, o, c) as ps:
        with ps.draw_weights([np.where(p["inlier_mask"], 1.0, 0.05) for p in pairs]) as w:
            assert w.weighted.all()
            plain = ps.ransac(budget=32, seed=SEED, rounds=0)
            informed = ps.ransac(budget=32, seed=SEED, rounds=0, weights=w)
            clean = []
            for dr in (ps.draw(32, SEED), ps.draw(32, SEED, weights=w)):
                clean.append(sum(any(p["inlier_mask"][I[s, :5 if T[s] else 3]].all() for s in range(32))
                                 for p, (T, I) in zip(pairs, dr)))
    s_plain, s_informed = sum(r.score_selected for r in plain), sum(r.score_selected for r in informed)
    print("pairs with an all-inlier sample among 32: uniform", clean[0], "weighted", clean[1])
    print("sum of score_selected: uniform", s_plain, "weighted", s_informed)
    assert s_informed < s_plain
