"""PairSet.inlier_mass and PairSet.ransac(weighted_stop=True) on the device (mp_inlier_mass_set,
mp_ransac_weighted_stop_set).  Expected values come from entries that exist without the feature:
the mass of a model is the sum of the restated q (tests/weighted_draw_restatement.py) over the lists
ps.select returns for that single candidate; a loop's result is compared byte for byte with the
fixed-budget call at its stop point and with walks over public entries
(tests/weighted_stop_restatement.py).

The stage: one set per variant with pairs of 4, 63, 64, 65 (either side of a wave), 255, 256, 257
(either side of a block), 513 (three trips), 300 not given weights, 300 that falls back (two
positive weights), 65535 with all weights 1.0 and no outliers (a mass near 2^32), and 65600 not
given weights.  The loop: tests/test_ransac_adaptive_gpu.py's pairs with confidences 1.0 / 0.05."""
import functools
import os
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import synthetic
from tests import refine_cases as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_stop_restatement as S  # noqa: E402
import test_draw_weighted_gpu as DW  # noqa: E402  (_compare_walk, _full_key, _informed)
import test_ransac_adaptive_gpu as A  # noqa: E402  (a set with inliers and outliers, its options and key)
import weighted_stop_restatement as WS  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = DW.SEED
STAGE_SIZES = (4, 63, 64, 65, 255, 256, 257, 513, 300, 300, 65535, 65600)
NOT_GIVEN, FALLS_BACK, FULL, ABOVE = (8, 11), 9, 10, 11
SMALL = tuple(range(10))  # the pairs below 65535
STEP, LO_BUDGET, EQ_BUDGET = 48, 240, 130
MODES = (dict(), dict(lo=1), dict(lo=1, lo_steps=2))


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


# ---- 1. the stage ----

def _stage_weights(i, n, dtype):
    if i in NOT_GIVEN:
        return None
    if i == FULL:
        return np.ones(n, dtype=dtype)
    rng = np.random.default_rng(900 + i)
    w = rng.random(n)
    if i == FALLS_BACK:
        w[:] = 0.0
        w[[7, 200]] = (0.5, 1.0)
        return w.astype(dtype)
    if n > 8:  # exact zeros and exact ones among the values
        w[rng.choice(n, n // 6, replace=False)] = 0.0
        w[rng.choice(n, n // 6, replace=False)] = 1.0
    return w.astype(dtype)


class Stage:
    pass


@functools.lru_cache(maxsize=None)
def _stage(variant, dtype, score_type, pairs_used):
    k = Stage()
    k.variant, k.ids = variant, list(pairs_used)
    o, c = synthetic.example_options(RC.KIND[variant])
    c.score_type = score_type
    k.pairs, k.weights = [], []
    for i, n in enumerate(STAGE_SIZES):
        if i not in pairs_used:
            continue
        p = A._pair(variant, i, n, 0.0 if i == FULL else 0.3)
        k.pairs.append(p)
        k.weights.append(_stage_weights(i, n, dtype))
    k.sizes = [len(p["depth0"]) for p in k.pairs]
    k.ps = madpose.PairSet(variant, k.pairs, o, c)
    k.w = k.ps.draw_weights(k.weights)
    k.pw = [WS.PairWeights(variant, n, w) for n, w in zip(k.sizes, k.weights)]
    # the models of every pair: the recovered true pose (a refined winner), a minimal model out
    # of candidates, a model far from everything, and the true pose with a NaN entry
    won = k.ps.ransac(budget=64, seed=SEED, rounds=1)
    cands = k.ps.candidates(k.ps.draw(6, SEED))
    k.entries = []  # (pair, kind, model)
    cls = (madpose.PoseScaleOffset, madpose.PoseScaleOffsetSharedFocal, madpose.PoseScaleOffsetTwoFocal)[variant]
    for j in range(len(k.pairs)):
        far = cls()
        far.pose = np.hstack([np.diag([-1.0, -1.0, 1.0]), [[1000.0], [0.0], [0.0]]])  # (finite: select scores it)
        far.scale, far.offset0, far.offset1 = 1e6, 0.0, 0.0
        k.entries.append((j, "far", far))
        rows = cands[j][0]
        if len(rows):
            k.entries.append((j, "minimal", madpose.poses_from_models(rows[:1], variant)[0]))
        true = won[j].model
        assert true is not None or k.sizes[j] < 63, j  # (four rows may give no model)
        if true is None:
            continue
        k.entries.append((j, "true", true))
        nan = cls()
        nan.__dict__.update(true.__dict__)
        nan.pose = true.pose.copy()
        nan.pose[0, 0] = float("nan")  # (an entry of R: every one of the three errors reads it)
        k.entries.append((j, "nan", nan))
    return k


def _expected(k, j, m):
    """(mass, count) restated: select's lists and with_counts counts for the single candidate"""
    sr, = k.ps.select([[m]], pair_ids=[j], with_counts=True)
    lists = sr.inlier_indices if sr.index == 0 else [np.zeros(0, dtype=np.int32)] * 3
    mass, count = k.pw[j].mass_of(lists)
    assert tuple(int(c) for c in sr.counts[0]) == count, (j, sr.counts, count)
    return mass, count


def _check_stage(k):
    pair_ids = [j for j, _, _ in k.entries]  # (every pair several times: pair_ids repeat)
    got = k.ps.inlier_mass([m for _, _, m in k.entries], k.w, pair_ids=pair_ids)
    assert len(got) == len(k.entries)
    zero = 0
    for (j, kind, m), g in zip(k.entries, got):
        mass, count = _expected(k, j, m)
        assert (g.mass, g.count) == (mass, count), (j, kind, g, mass, count)
        assert g.weighted == bool(k.w.weighted[j]) == k.pw[j].weighted, (j, kind)
        assert g.total == (int(k.w.total[j]) if g.weighted else k.sizes[j]) == k.pw[j].total, (j, kind)
        assert all(0 <= a <= g.total for a in g.mass)
        if kind == "nan":
            assert g.mass == (0, 0, 0) and g.count == (0, 0, 0), (j, g)
        if kind == "far":
            zero += g.count == (0, 0, 0)
        if kind == "true" and k.sizes[j] >= 63:
            assert min(g.count) > 0, (j, g)
    assert zero >= 1  # a model with no inliers at all
    return got


@pytest.mark.parametrize("variant,dtype", [(0, "float64"), (1, "float64"), (2, "float64"), (0, "float32")])
def test_inlier_mass_equals_the_restated_mass(variant, dtype):
    k = _stage(variant, dtype, 0, tuple(range(len(STAGE_SIZES))))
    assert k.w.weighted.tolist() == [i not in NOT_GIVEN and i != FALLS_BACK for i in range(len(STAGE_SIZES))]
    got = _check_stage(k)
    # the pair of 65535 rows of q = 65535 under its true model: a mass near 2^32 that does not wrap
    full = [g for (j, kind, _), g in zip(k.entries, got) if j == FULL and kind == "true"][0]
    print("the full pair:", full)
    assert full.total == 65535 * 65535 and full.weighted
    assert all(m == 65535 * c for m, c in zip(full.mass, full.count)) and max(full.mass) > 1 << 31
    # the pair above 65535: counts over n
    above = [g for (j, kind, _), g in zip(k.entries, got) if j == ABOVE and kind == "true"][0]
    assert not above.weighted and above.total == 65600 and above.mass == above.count and max(above.count) > 30000


@pytest.mark.parametrize("score_type", [1, 2])
def test_inlier_mass_is_ungated_under_the_score_types(score_type):
    k = _stage(0, "float64", score_type, SMALL)
    got = _check_stage(k)
    # (the lists of all three terms are formed whatever the score reads)
    assert any(min(g.count) > 0 for g in got)


def test_repeated_and_permuted_entries_return_the_same_records():
    k = _stage(0, "float64", 0, SMALL)
    key = lambda g: (g.mass, g.total, g.count, g.weighted)
    base = [key(g) for g in k.ps.inlier_mass([m for _, _, m in k.entries], k.w, pair_ids=[j for j, _, _ in k.entries])]
    order = np.random.default_rng(3).permutation(len(k.entries))[: len(k.entries) // 2].tolist()
    order = order + order[:5] + order[:5]  # a permuted subset with entries repeated
    got = k.ps.inlier_mass([k.entries[e][2] for e in order], k.w, pair_ids=[k.entries[e][0] for e in order])
    assert [key(g) for g in got] == [base[e] for e in order]
    # all pairs in order, without pair_ids
    first = {}
    for e, (j, kind, m) in enumerate(k.entries):
        first.setdefault(j, e)
    got = k.ps.inlier_mass([k.entries[first[j]][2] for j in range(len(k.pairs))], k.w)
    assert [key(g) for g in got] == [base[first[j]] for j in range(len(k.pairs))]
    # a call leaves nothing behind: select's lists afterwards are what they were
    sr0, = k.ps.select([[k.entries[0][2]]], pair_ids=[0])
    k.ps.inlier_mass([k.entries[4][2]] * 3, k.w, pair_ids=[1, 1, 1])
    sr1, = k.ps.select([[k.entries[0][2]]], pair_ids=[0])
    assert all(np.array_equal(a, b) for a, b in zip(sr0.inlier_indices, sr1.inlier_indices))


# ---- 2. the loop ----

def _key(r, variant):
    return DW._full_key(r, variant) + (r.rule_mass, r.rule_total)


def _rules(a, conf):
    return [WS.Rule(a.ps, j, WS.PairWeights(a.variant, A.SIZES[j], conf[j]), a.variant, a.o)
            for j in range(len(A.SIZES))]


def _conf(a):
    return [np.where(p["inlier_mask"], 1.0, 0.05) for p in a.pairs]


@functools.lru_cache(maxsize=None)
def _types(variant):
    a, w = DW._informed(variant)
    return [t for t, _ in a.ps.draw(A.BUDGET, SEED, weights=w)]


@functools.lru_cache(maxsize=None)
def _cache(variant):
    return {}


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("rounds", [0, 2])
def test_step_equals_the_fixed_budget_call_and_the_walk(variant, rounds):
    a, w = DW._informed(variant)
    out = a.ps.ransac(budget=A.BUDGET, step=STEP, seed=SEED, rounds=rounds, weights=w, weighted_stop=True)
    plain = a.ps.ransac(budget=A.BUDGET, step=STEP, seed=SEED, rounds=rounds, weights=w)
    print("stop points, mass rule ", variant, [(r.num_samples, r.stopped) for r in out])
    print("stop points, count rule", variant, [(r.num_samples, r.stopped) for r in plain])
    rules = _rules(a, _conf(a))
    for j, r in enumerate(out):
        want, = a.ps.ransac(budget=r.num_samples, seed=SEED, rounds=rounds, pair_ids=[j], weights=w)
        assert A.key(r, variant) == A.key(want, variant), j
        m, stopped, last = WS.step_walk(a.ps, j, _types(variant)[j], S.checkpoints(STEP, A.BUDGET), SEED, rules[j],
                                        _cache(variant), w)
        assert (r.num_samples, r.stopped) == (m, stopped), j
        assert (r.rule_mass, r.rule_total) == (rules[j].mass, rules[j].pw.total), j
        if rounds == 0 and r.model is not None:
            g, = a.ps.inlier_mass([r.model], w, pair_ids=[j])
            assert g.mass == r.rule_mass and g.total == r.rule_total, j
            assert g.count == tuple(len(x) for x in r.inlier_indices), j
    assert any(r.stopped and r.num_samples < A.BUDGET for r in out)
    assert out[0].num_samples == 0 and not out[0].stopped and out[0].rule_mass == (0, 0, 0)
    assert out[0].rule_total == 0 and out[1].rule_total == int(w.total[1])


@functools.lru_cache(maxsize=None)
def _walks(variant, steps):
    """the walks of every pair with rounds = 0 (the loop does not depend on rounds)"""
    a, w = DW._informed(variant)
    marks, types, rules = S.checkpoints(STEP, LO_BUDGET), _types(variant), _rules(a, _conf(a))
    if steps:
        return [WS.lo_steps_walk(a.ps, j, types[j][:LO_BUDGET], marks, SEED, 1, 2, 0, rules[j], _cache(variant), w,
                                 int(a.o.num_lsq_iterations), float(a.o.threshold_multiplier),
                                 int(a.o.non_min_sample_multiplier)) for j in range(len(A.SIZES))]
    return [WS.lo_walk(a.ps, j, types[j][:LO_BUDGET], marks, SEED, 1, 0, rules[j], _cache(variant), w)
            for j in range(len(A.SIZES))]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("steps", [False, True])
@pytest.mark.parametrize("rounds", [0, 2])
def test_lo_modes_equal_the_walks(variant, steps, rounds):
    a, w = DW._informed(variant)
    mode = dict(lo=1, lo_steps=2) if steps else dict(lo=1)
    out = a.ps.ransac(budget=LO_BUDGET, step=STEP, seed=SEED, rounds=rounds, weights=w, weighted_stop=True, **mode)
    walks = [WS.finish(a.ps, j, wk, rounds) for j, wk in enumerate(_walks(variant, steps))]
    print("stop points", variant, mode, [(r.num_samples, r.stopped) for r in out])
    DW._compare_walk(variant, out, walks, steps)
    for j, (r, wk) in enumerate(zip(out, walks)):
        assert r.rule_mass == wk.rule_mass, j
        if rounds == 0 and r.model is not None:
            g, = a.ps.inlier_mass([r.model], w, pair_ids=[j])
            assert g.mass == r.rule_mass and g.total == r.rule_total, j
            assert g.count == tuple(len(x) for x in r.inlier_indices), j
    assert any(r.lo_runs > 0 for r in out)
    assert any(r.stopped and r.num_samples < LO_BUDGET for r in out)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("q", [1, 1000, 65535])
def test_equal_weights_give_the_count_rules_bytes(variant, q):
    a = A._case(variant)
    value = 1.0 if q == 65535 else q / 65536.0
    with a.ps.draw_weights([np.full(n, value) for n in A.SIZES]) as w:
        assert w.total.tolist() == [n * q for n in A.SIZES]
        for mode in MODES:
            on = a.ps.ransac(budget=EQ_BUDGET, step=STEP, seed=SEED, rounds=2, weights=w, weighted_stop=True, **mode)
            off = a.ps.ransac(budget=EQ_BUDGET, step=STEP, seed=SEED, rounds=2, weights=w, weighted_stop=False, **mode)
            assert [DW._full_key(r, variant) for r in on] == [DW._full_key(r, variant) for r in off], mode
            assert any(r.index >= 0 for r in off)
            assert all(r.rule_mass is None for r in off)
            for j, r in enumerate(on):
                assert r.rule_total == (A.SIZES[j] * q if w.weighted[j] else A.SIZES[j]), (mode, j)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_off_is_the_call_without_the_keyword_and_subsets_are_the_whole_sets(variant):
    a, w = DW._informed(variant)
    for mode in MODES:
        kw = dict(budget=EQ_BUDGET, step=STEP, seed=SEED, rounds=2, weights=w, **mode)
        off, none = a.ps.ransac(weighted_stop=False, **kw), a.ps.ransac(**kw)
        assert [_key(r, variant) for r in off] == [_key(r, variant) for r in none], mode
        whole = a.ps.ransac(weighted_stop=True, **kw)
        sub = a.ps.ransac(weighted_stop=True, pair_ids=A.SUBSET, sample_chunk=37, model_chunk=7, **kw)
        assert [_key(r, variant) for r in sub] == [_key(whole[i], variant) for i in A.SUBSET], mode


# ---- 3. the effect ----

def test_the_mass_rule_stops_informed_pairs_earlier():
    """16 calibrated pairs of 300 correspondences with 70 % outliers, confidences 1.0 on the true
    matches and 0.05 elsewhere, min_num_iterations = 8, budget 512 in steps of 16, no refinement.
    The count rule needs a ratio of 0.456 to stop within 512 MD samples and the true matches are
    30 %, so it runs the budget; their mass ratio is about 0.895, for which the rule asks 8 samples."""
    o, c = synthetic.example_options("calibrated")
    o.min_num_iterations = 8
    pairs = [synthetic.make_pair(4000 + i, n=300, outlier_ratio=0.7) for i in range(16)]
    with madpose.PairSet(0, pairs, o, c) as ps:
        with ps.draw_weights([np.where(p["inlier_mask"], 1.0, 0.05) for p in pairs]) as w:
            assert w.weighted.all()
            off = ps.ransac(budget=512, step=16, seed=SEED, rounds=0, weights=w)
            on = ps.ransac(budget=512, step=16, seed=SEED, rounds=0, weights=w, weighted_stop=True)
    n_off, n_on = [r.num_samples for r in off], [r.num_samples for r in on]
    print("samples, count rule:", n_off, [r.stopped for r in off])
    print("samples, mass rule: ", n_on, [r.stopped for r in on])
    assert sum(n_on) < sum(n_off)
    assert any(a.stopped and a.num_samples < 512 and b.num_samples == 512 and not b.stopped
               for a, b in zip(on, off))
