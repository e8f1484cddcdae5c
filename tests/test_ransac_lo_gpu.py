"""PairSet.refine(relax=True) and PairSet.ransac(step=, lo=) on the device
(mp_refine_relaxed_set, mp_ransac_lo_set).  Every comparison is of bytes against entries that
exist without the feature, or against compositions of the feature's own public entries:

* the relaxed refinement against tests/ransac_lo_walk.py refine_relaxed_single
  (score_models(with_errors=True), the thresholds times threshold_multiplier, lm_refine_batch);
* the LO loop against lo_walk: ransac(budget=m_k, rounds=0, pair_ids=[p]) at every checkpoint,
  refine(relax=True) where the minimal best changed, the two-track bookkeeping and the
  termination rule restated in Python, refine(rounds) at the end.

The refine set: one pair each of n = 5, 63, 64, 65, 257, 700, start models by
RC.start_model from np.random.default_rng(90 + variant).  These seeds were chosen with the
host's sweep and LM (refine_relaxed_single(on_host=True)): for every variant the n = 63, 65,
257 and 700 pairs have relaxed lists longer than the tight ones in all three terms and accept
rounds 0, 1 and (all but one) 2; n = 5 and n = 64 stop at the size test (too few relaxed
point-term inliers).  The LO set is tests/test_ransac_adaptive_gpu.py's."""
import functools
import os
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import synthetic
from tests import ransac_lo_walk as W
from tests import refine_cases as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_stop_restatement as S  # noqa: E402
import test_ransac_adaptive_gpu as A  # noqa: E402  (the set, its options, budget, step and seed)

pytestmark = pytest.mark.gpu

REFINE_SIZES = (5, 63, 64, 65, 257, 700)
SEED5 = 1
SUBSET = [5, 2, 3, 0]
LO_SUBSET = [5, 2, 4, 0]


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


class Case:
    pass


# ---- refine(relax=True) ----

@functools.lru_cache(maxsize=None)
def _rcase(variant, multiplier=None):
    k = Case()
    k.variant = variant
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    if multiplier is not None:
        k.o.threshold_multiplier = multiplier
    rng = np.random.default_rng(90 + variant)
    k.pairs = [RC.make_pair(variant, SEED5 if n == 5 else 500 + i, n) for i, n in enumerate(REFINE_SIZES)]
    k.models = [RC.start_model(variant, p, rng) for p in k.pairs]
    k.ps = madpose.PairSet(variant, k.pairs, k.o, k.c)
    k.norm = k.ps.norm_scale
    return k


@functools.lru_cache(maxsize=None)
def _expected(variant, rounds):
    k = _rcase(variant)
    return [W.refine_relaxed_single(variant, p, m, k.o, k.c, rounds, float(ns))
            for p, m, ns in zip(k.pairs, k.models, k.norm)]


def _rkeys(variant, rs):
    return [RC.result_key(variant, r) for r in rs]


def test_the_feature_is_there():
    """both are a TypeError without the feature"""
    k = _rcase(0)
    out = k.ps.refine(k.models, relax=True)
    assert len(out) == len(REFINE_SIZES)
    a = A._case(0)
    out = a.ps.ransac(budget=64, step=32, lo=1, seed=A.SEED)
    assert len(out) == len(A.SIZES)
    assert all(isinstance(r.lo_runs, int) and r.lo_runs >= r.lo_accepted >= 0 and r.lo_index >= -1 for r in out)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("rounds", [1, 3])
def test_relaxed_refine_equals_the_single_pair_entries(variant, rounds):
    k = _rcase(variant)
    assert float(k.o.threshold_multiplier) == 5.0
    want = _expected(variant, rounds)
    # ---- the case holds what it is meant to (on the expectation's own values) ----
    print("tight / wide / accepted", variant, rounds, [(e.tight0, e.wide0, e.accepted) for e in want])
    assert any(all(w > t for w, t in zip(e.wide0, e.tight0)) for e in want)
    assert any(0 in e.accepted for e in want)
    if rounds == 3:
        assert any(e.accepted and e.accepted[-1] >= 1 for e in want)
    assert any(e.status == 3 for e in want)  # (below the minimal sample)
    # ---- bytes ----
    got = k.ps.refine(k.models, rounds=rounds, relax=True)
    for i, (g, e) in enumerate(zip(got, want)):
        assert RC.model_bytes(variant, g.model) == RC.model_bytes(variant, e.model), i
        assert np.float64(g.score_initial).tobytes() == np.float64(e.score_initial).tobytes(), i
        assert np.float64(g.score_final).tobytes() == np.float64(e.score_final).tobytes(), i
        assert (g.rounds_run, g.rounds_accepted, g.status) == (e.rounds_run, e.rounds_accepted, e.status), i
        for t in range(3):
            assert g.inlier_indices[t].dtype == np.int32
            assert np.array_equal(g.inlier_indices[t], e.lists[t]), (i, t)
    # the list-buffer accounting: two buffers after a refine, relaxed or not
    assert k.ps.resident_bytes == 120 * sum(REFINE_SIZES)


@pytest.mark.parametrize("variant", [0, 1])
def test_multiplier_one_is_the_plain_refine(variant):
    k = _rcase(variant, 1.0)
    for rounds in (1, 3):
        plain = k.ps.refine(k.models, rounds=rounds)
        assert any(r.rounds_accepted > 0 for r in plain)
        assert _rkeys(variant, k.ps.refine(k.models, rounds=rounds, relax=True)) == _rkeys(variant, plain)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_relaxed_refine_selection_and_neighbours(variant):
    k = _rcase(variant)
    whole = _rkeys(variant, k.ps.refine(k.models, rounds=3, relax=True))
    got = k.ps.refine([k.models[j] for j in SUBSET], rounds=3, relax=True, pair_ids=SUBSET)
    assert _rkeys(variant, got) == [whole[j] for j in SUBSET]
    for j in range(len(REFINE_SIZES)):
        one, = k.ps.refine([k.models[j]], rounds=3, relax=True, pair_ids=[j])
        assert RC.result_key(variant, one) == whole[j], j
    # no state: a plain refine in between, then the same bytes
    k.ps.refine(k.models, rounds=2)
    assert _rkeys(variant, k.ps.refine(k.models, rounds=3, relax=True)) == whole


# ---- ransac(step=, lo=) ----

def _required(a):
    return lambda n, counts: S.required(a.variant, n, counts, a.o.success_probability, a.o.min_num_iterations,
                                        a.o.max_num_iterations_per_solver)


@functools.lru_cache(maxsize=None)
def _walks(variant, lo, rounds):
    """the walk of every pair of the adaptive tests' set (lo None: without local optimisation)"""
    a = A._case(variant)
    if not hasattr(a, "lo_cache"):
        a.lo_cache = {}
    return [W.lo_walk(a.ps, j, A.SIZES[j], a.types[j], a.marks, A.SEED, lo, rounds, _required(a), S.stop_reached,
                      a.lo_cache) for j in range(len(A.SIZES))]


def _bits(x):
    return np.float64(x).tobytes()


def _lo_key(variant, r):
    """every field of a RansacResult, the three new ones, stopped and the lists"""
    return (r.num_samples, r.num_candidates, r.index, r.sample, r.slot, r.solver_type, _bits(r.score_selected),
            _bits(r.score_initial), _bits(r.score_final), r.rounds_run, r.rounds_accepted, r.status,
            _bits(r.norm_scale), None if r.model is None else RC.model_bytes(variant, r.model), r.model_row.tobytes(),
            tuple(a.tobytes() for a in r.inlier_indices), r.stopped, r.lo_runs, r.lo_accepted, r.lo_index)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("lo", [1, 2])
@pytest.mark.parametrize("rounds", [0, 2])
def test_lo_loop_equals_the_walk(variant, lo, rounds):
    a = A._case(variant)
    walks = _walks(variant, lo, rounds)
    out = a.ps.ransac(budget=A.BUDGET, step=A.STEP, seed=A.SEED, rounds=rounds, lo=lo)
    print("walk", variant, lo, rounds, [(w.num_samples, w.stopped, w.track.lo_runs, w.track.lo_accepted,
                                         w.track.lo_index) for w in walks])
    for j, (r, w) in enumerate(zip(out, walks)):
        m, T = w.minimal, w.track
        assert (r.num_samples, r.stopped) == (w.num_samples, w.stopped), j
        assert (r.lo_runs, r.lo_accepted, r.lo_index) == (T.lo_runs, T.lo_accepted, T.lo_index), j
        if m is None:  # no samples: no winner
            assert r.index == -1 and r.model is None and r.num_candidates == 0, j
            continue
        # the minimal track
        assert (r.num_candidates, r.index, r.sample, r.slot, r.solver_type) == (
            m.num_candidates, m.index, m.sample, m.slot, m.solver_type), j
        assert _bits(r.score_selected) == _bits(m.score_selected) and _bits(r.norm_scale) == _bits(m.norm_scale), j
        # the final refinement of the overall best
        assert (r.model is None) == (w.model is None), j
        if w.model is not None:
            assert RC.model_bytes(variant, r.model) == RC.model_bytes(variant, w.model), j
        assert _bits(r.score_initial) == _bits(w.score_initial) and _bits(r.score_final) == _bits(w.score_final), j
        assert (r.rounds_run, r.rounds_accepted, r.status) == (w.rounds_run, w.rounds_accepted, w.status), j
        for t in range(3):
            assert np.array_equal(r.inlier_indices[t], w.lists[t]), (j, t)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("lo", [1, 2])
def test_the_lo_case_is_worth_testing(variant, lo):
    """On the walk's values alone: some pair returns an LO-derived best, some pair ran an LO
    that did not become the overall best, some pair stops at an earlier checkpoint than its
    walk without lo, and some pair runs to the budget unstopped.

    The adaptive tests' outlier ratios (0.0 / 0.3 / 0.9 on the three n = 300 pairs) give all
    four as they are.  Observed (num_samples, stopped, lo_runs, lo_accepted, lo_index) of the six
    pairs on an MI355X, the same for lo = 1 and lo = 2:
      calibrated    (0, F, 0, 0, -1) (48, T, 1, 0, -1) (96, T, 2, 1, 0) (48, T, 1, 1, 2) (96, T, 1, 1, 15) (512, F, 5, 2, 20)
      shared focal  (0, F, 0, 0, -1) (512, F, 1, 0, -1) (144, T, 2, 2, 5) (48, T, 1, 1, 16) (96, T, 1, 1, 6) (512, F, 4, 1, 12)
      two focal     (0, F, 0, 0, -1) (512, F, 0, 0, -1) (192, T, 1, 1, 10) (48, T, 1, 1, 12) (288, T, 1, 1, 4) (512, F, 3, 2, 8)
    against (num_samples, stopped) without lo in tests/test_ransac_adaptive_gpu.py."""
    with_lo, without = _walks(variant, lo, 0), _walks(variant, None, 0)
    print("with lo", variant, lo, [(w.num_samples, w.stopped, w.track.lo_runs, w.track.lo_accepted,
                                    w.track.lo_index, w.trace) for w in with_lo])
    print("without", variant, [(w.num_samples, w.stopped) for w in without])
    assert [(w.num_samples, w.stopped) for w in without] == A._case(variant).expect
    assert any(w.track.lo_index >= 0 for w in with_lo)
    assert any(w.track.lo_runs > w.track.lo_accepted for w in with_lo)
    assert any(w.stopped and w.num_samples < v.num_samples for w, v in zip(with_lo, without))
    assert any(w.num_samples == A.BUDGET and not w.stopped for w in with_lo)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_lo_invariance(variant):
    a = A._case(variant)
    ps = a.ps
    call = lambda **kw: ps.ransac(budget=A.BUDGET, step=A.STEP, seed=A.SEED, rounds=2, lo=2, **kw)
    keys = lambda rs: [_lo_key(variant, r) for r in rs]
    base = keys(call())
    assert keys(call(pair_ids=LO_SUBSET)) == [base[j] for j in LO_SUBSET]
    assert keys(call(sample_chunk=33, model_chunk=7)) == base
    assert keys(call(sample_chunk=1, model_chunk=1)) == base
    # no state: other calls in between
    ps.ransac(budget=40, seed=A.SEED + 1, rounds=1)
    ps.refine([r.model for r in ps.ransac(budget=40, seed=A.SEED, rounds=0, pair_ids=[3, 4])], relax=True,
              pair_ids=[3, 4])
    assert keys(call()) == base
    # rounds = 0: the lists are the overall best's own, whichever track it came from
    base0 = keys(ps.ransac(budget=A.BUDGET, step=A.STEP, seed=A.SEED, rounds=0, lo=2))
    sub0 = keys(ps.ransac(budget=A.BUDGET, step=A.STEP, seed=A.SEED, rounds=0, lo=2, pair_ids=LO_SUBSET))
    assert sub0 == [base0[j] for j in LO_SUBSET]
    # budget 0: no samples, no winners, no LO
    none = ps.ransac(budget=0, step=A.STEP, seed=A.SEED, rounds=2, lo=1)
    assert all(r.index == -1 and r.num_samples == 0 and r.model is None and not r.stopped
               and (r.lo_runs, r.lo_accepted, r.lo_index) == (0, 0, -1) for r in none)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_the_minimal_track_is_untouched(variant):
    """pairs that spent the same num_samples with and without lo have the same minimal fields"""
    a = A._case(variant)
    plain = a.ps.ransac(budget=A.BUDGET, step=A.STEP, seed=A.SEED, rounds=0)
    assert all((r.lo_runs, r.lo_accepted, r.lo_index) == (0, 0, -1) for r in plain)
    same = 0
    for lo in (1, 2):
        out = a.ps.ransac(budget=A.BUDGET, step=A.STEP, seed=A.SEED, rounds=0, lo=lo)
        for j, (r, q) in enumerate(zip(out, plain)):
            # whatever it spent: the minimal track is the fixed-budget call's of that many samples
            f, = a.ps.ransac(budget=r.num_samples, seed=A.SEED, rounds=0, pair_ids=[j])
            for x in (q, f) if r.num_samples == q.num_samples else (f,):
                assert (r.index, r.sample, r.slot, r.solver_type, r.num_candidates) == (
                    x.index, x.sample, x.slot, x.solver_type, x.num_candidates), (lo, j)
                assert _bits(r.score_selected) == _bits(x.score_selected), (lo, j)
            same += r.num_samples == q.num_samples and r.num_samples > 0
    assert same >= 2
