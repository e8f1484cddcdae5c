"""refine_batch on the device (mp_refine_batch): every pair's result equals, bit for bit,
the composition of the single-pair entries (score_models with errors, the thresholds,
lm_refine_batch kind 0, the acceptance rule); chunking, pair order and neighbours change
nothing; a refined output fed back in is left alone; the lists, decisions and final
costs agree with the CPU oracle's composition; two identical calls return identical
bytes."""
import numpy as np
import pytest

import madpose
import oracle
from madpose_amd import synthetic
from tests import lm_cases as LC
from tests import refine_cases as RC
from tests.helpers import oracle_cfg, oracle_opts

pytestmark = pytest.mark.gpu

SIZES = [5, 63, 64, 65, 257, 700]  # either side of a wave and of the 256-lane block, one below the minimal sample
# seed of the n = 5 pair per variant: the start model has fewer Sampson inliers than the
# point solver's minimal sample on it (calibrated: 5), so the size rule must stop it
SEED5 = {0: 1, 1: 1, 2: 1, 3: 1}


def _case(variant, sizes=SIZES, seed0=100, score_type=0):
    o, c = synthetic.example_options(RC.KIND[variant])
    c.score_type = score_type
    rng = np.random.default_rng(7 + variant)
    pairs, models = [], []
    for k, n in enumerate(sizes):
        p = RC.make_pair(variant, SEED5[variant] if n == 5 else seed0 + k, n)
        pairs.append(p)
        models.append(RC.start_model(variant, p, rng))
    return o, c, pairs, models


def _check_against_single(variant, o, c, pairs, models, rounds):
    res = madpose.refine_batch(variant, pairs, models, o, c, rounds=rounds)
    assert len(res) == len(pairs)
    accepted = 0
    for p, m, r in zip(pairs, models, res):
        n = len(p["depth0"])
        e = RC.refine_single(variant, p, m, o, c, rounds, r.norm_scale)
        what = (variant, n, rounds)
        assert RC.model_bytes(variant, r.model) == RC.model_bytes(variant, e.model), what
        assert r.score_initial == e.score_initial and r.score_final == e.score_final, what
        assert (r.rounds_run, r.rounds_accepted, r.status) == (e.rounds_run, e.rounds_accepted, e.status), what
        for t in range(3):
            assert r.inlier_indices[t].dtype == np.int32
            assert np.array_equal(r.inlier_indices[t], e.lists[t]), (what, t)
            assert np.all(np.diff(r.inlier_indices[t]) > 0)
        assert r.score_final <= r.score_initial
        if n == 5:  # below the minimal sample: untouched, status 3
            assert r.status == 3 and r.rounds_accepted == 0 and r.rounds_run == 1
            assert RC.model_bytes(variant, r.model) == RC.model_bytes(variant, m)
        accepted += r.rounds_accepted
    return res, accepted


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_equals_single_pair_entries(variant, rounds):
    o, c, pairs, models = _case(variant)
    res, accepted = _check_against_single(variant, o, c, pairs, models, rounds)
    # the case exercises the accept path, and with three rounds a later round too
    assert accepted >= 1
    if rounds == 3:
        assert max(r.rounds_run for r in res) >= 2


@pytest.mark.parametrize("score_type", [1, 2])
def test_equals_single_pair_entries_gated_scores(score_type):
    """score_type 1 / 2: the score's gated terms and the lists' ungated errors come from
    one evaluation"""
    o, c, pairs, models = _case(0, sizes=[65, 257], score_type=score_type)
    _check_against_single(0, o, c, pairs, models, 2)


@pytest.mark.parametrize("variant", [0, 1])
def test_chunking_order_and_neighbours(variant):
    o, c, pairs, models = _case(variant)
    key = lambda r: RC.result_key(variant, r)
    base = [key(r) for r in madpose.refine_batch(variant, pairs, models, o, c, rounds=3)]
    for chunk in (1, 2):
        assert [key(r) for r in madpose.refine_batch(variant, pairs, models, o, c, rounds=3, chunk=chunk)] == base
    perm = [4, 0, 5, 2, 1, 3]
    got = madpose.refine_batch(variant, [pairs[i] for i in perm], [models[i] for i in perm], o, c, rounds=3)
    assert [key(r) for r in got] == [base[i] for i in perm]
    for i in range(len(pairs)):
        alone, = madpose.refine_batch(variant, [pairs[i]], [models[i]], o, c, rounds=3)
        assert key(alone) == base[i], i


@pytest.mark.parametrize("variant", [0, 1])
def test_refined_output_is_left_alone(variant):
    """run to the stop (64 rounds at most), feed the output back in: no round is accepted;
    a pair without correspondences sits between two real pairs"""
    o, c, pairs, models = _case(variant, sizes=[257, 0, 700])
    first = madpose.refine_batch(variant, pairs, models, o, c, rounds=64)
    assert all(r.rounds_run < 64 for r in first)
    empty = first[1]
    assert (empty.score_initial, empty.score_final, empty.status, empty.rounds_accepted) == (0.0, 0.0, 3, 0)
    assert all(len(a) == 0 for a in empty.inlier_indices)
    assert RC.model_bytes(variant, empty.model) == RC.model_bytes(variant, models[1])
    assert first[0].rounds_accepted >= 1 and first[2].rounds_accepted >= 1
    again = madpose.refine_batch(variant, pairs, [r.model for r in first], o, c, rounds=64)
    for a, f in zip(again, first):
        assert a.rounds_accepted == 0
        assert RC.model_bytes(variant, a.model) == RC.model_bytes(variant, f.model)
        assert a.score_initial == a.score_final
        if variant == 0:  # (no unit change on the way: the very same model, score and lists)
            assert a.score_initial == f.score_final
            assert all(np.array_equal(x, y) for x, y in zip(a.inlier_indices, f.inlier_indices))


# (variant, seed, n): chosen on the CPU so that the oracle's composition has no error
# within 1e-9 relative of its threshold and takes both rounds, or rejects the first, by
# more than 1e-6 relative -- conditions the test asserts on the oracle's values -- and
# that the same composition through the engine's host sweep and host LM
# (mp_debug_lo_sweep, mp_debug_lm_refine_host) keeps every error 1e-3 relative or more
# away from its threshold
ORACLE_CASES = [(0, 200, 300), (1, 200, 300), (2, 201, 300), (3, 201, 300)]
ORACLE_ROUNDS = 2


def _or_model(variant, m):
    d = dict(R=m.R(), t=m.t(), scale=m.scale, offset0=getattr(m, "offset0", 0.0), offset1=getattr(m, "offset1", 0.0),
             focal0=1.0, focal1=1.0)
    if variant == 1:
        d["focal0"] = d["focal1"] = m.focal
    elif variant == 2:
        d["focal0"], d["focal1"] = m.focal0, m.focal1
    return d


def _or_struct(d):
    m = oracle.OrModel()
    m.R[:] = list(np.asarray(d["R"], dtype=np.float64).reshape(9))
    m.t[:] = list(np.asarray(d["t"], dtype=np.float64).reshape(3))
    for k in ("scale", "offset0", "offset1", "focal0", "focal1"):
        setattr(m, k, float(d[k]))
    return m


def oracle_composition(variant, p, m_user, o, c, rounds):
    """(lists, accepted rounds, final model dict, norm_scale) by the oracle alone, with
    the guard bands asserted."""
    args = RC.pair_args(variant, p)
    oo, oc = oracle_opts(o), oracle_cfg(c)
    _, _, ns = oracle.score_models(variant, *args[:4], *args[5:], oo, oc, [])
    thr = RC.thresholds(variant, o, ns)

    def sweep(d):
        s, err, _ = oracle.score_models(variant, *args[:4], *args[5:], oo, oc, [_or_struct(d)])
        for t in range(3):
            fin = err[0, t][np.isfinite(err[0, t]) & (err[0, t] < 1e300)]
            assert np.all(np.abs(fin - thr[t]) > 1e-9 * thr[t]), "an oracle error lies at its threshold"
        return float(s[0]), [np.flatnonzero(err[0, t] < thr[t]).astype(np.int32) for t in range(3)]

    cur = _or_model(variant, RC.to_problem_units(variant, m_user, ns))
    score, lists = sweep(cur)
    decisions = []
    for _ in range(rounds):
        cand, ran = oracle.least_squares(variant, *args, oo, oc, 0, lists, cur)
        assert ran
        s2, l2 = sweep(cand)
        assert abs(s2 - score) > 1e-6 * score, "an oracle round is decided by less than 1e-6"
        decisions.append(s2 < score)
        if not decisions[-1]:
            break
        cur, score, lists = cand, s2, l2
    assert all(decisions) or decisions == [False], decisions
    return lists, sum(decisions), cur, ns


def _cost(variant, args, o, c, m, lists, ns):
    if variant == 3:  # the scale-only functors: the calibrated ones without offsets
        m = madpose.PoseScaleOffset(m.R(), m.t(), m.scale, 0.0, 0.0)
        variant = 0
    return LC.lm_cost(variant, args, o, c, m, lists, ns)


@pytest.mark.parametrize("variant,seed,n", ORACLE_CASES)
def test_against_oracle(variant, seed, n):
    o, c = synthetic.example_options(RC.KIND[variant])
    p = RC.make_pair(variant, seed, n)
    m0 = RC.start_model(variant, p, np.random.default_rng(seed))
    lists, accepted, ref, ns = oracle_composition(variant, p, m0, o, c, ORACLE_ROUNDS)
    r, = madpose.refine_batch(variant, [p], [m0], o, c, rounds=ORACLE_ROUNDS)
    assert r.rounds_accepted == accepted
    for t in range(3):
        assert np.array_equal(r.inlier_indices[t], lists[t]), t
    args = RC.pair_args(variant, p)
    mk = (lambda d: madpose.PoseAndScale(d["R"], d["t"], d["scale"])) if variant == 3 else (lambda d: LC.model_of(d, variant))
    cr = _cost(variant, args, o, c, mk(ref), lists, ns)
    ce = _cost(variant, args, o, c, RC.to_problem_units(variant, r.model, r.norm_scale), lists, ns)
    print(f"variant {variant}: accepted {accepted}, cost engine {ce:.12g} oracle {cr:.12g}")
    assert abs(ce - cr) <= 2e-6 * max(ce, cr) + 1e-12, (ce, cr)


def test_deterministic_64_pairs():
    o, c = synthetic.example_options("calibrated")
    rng = np.random.default_rng(5)
    sizes = rng.integers(40, 400, 64)
    pairs = [RC.make_pair(0, 300 + k, int(n)) for k, n in enumerate(sizes)]
    models = [RC.start_model(0, p, rng) for p in pairs]
    a = madpose.refine_batch(0, pairs, models, o, c, rounds=3)
    b = madpose.refine_batch(0, pairs, models, o, c, rounds=3)
    assert [RC.result_key(0, r) for r in a] == [RC.result_key(0, r) for r in b]
    assert sum(r.rounds_accepted for r in a) >= 32
