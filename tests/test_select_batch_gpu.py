"""select_batch on the device (mp_select_batch): every candidate's score equals, bit for
bit, what score_models gives for it, its counts are the numbers of score_models' errors
below the thresholds, and every pair's winner is the one a Python walk with the reference's
strict rule finds, with the lists refine_batch would form; chunking, record slabs, pair
order and neighbours change nothing; refine_batch started from the winners
reports the selected score; two identical calls return identical bytes.

Expected values come from entries that existed before select_batch: score_models with
errors on the model in problem units, tests/refine_cases.py's thresholds, a Python walk."""
import functools

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import refine_cases as RC

pytestmark = pytest.mark.gpu

DBL_MAX = float(np.finfo(np.float64).max)
TILE = L.SELECT_TILE
# either side of a wave and of the 256-correspondence trip, an empty pair, one below the minimal sample
SIZES = (0, 5, 63, 64, 65, 255, 256, 257, 700)
SEED5 = 1  # (the n = 5 pair of tests/test_refine_batch_gpu.py)
# candidates per pair, from 0, 1, TILE - 1, TILE, TILE + 1, 37; "nan": max(TILE - 1, 1)
# candidates, every one with a NaN rotation
COUNTS = (TILE + 1, 1, 37, TILE, 37, 0, "nan", 37, 37)
# counts around every work-item size the kernel is built for (the tile test)
TILE_COUNTS = (9, 3, 8, 7, 37, 0, "nan", 5, 16)
WITH_NAN = (65, 700)       # pairs (by n) that hold one NaN model among real ones
WITH_DUP = (65, 257, 700)  # pairs whose last candidate is replaced by a copy of their best


def _turn90(R):
    return np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) @ R


def _candidates(variant, p, n, count, rng):
    """`count` candidates: the far model first, a NaN model second (WITH_NAN), the ground
    truth in the middle, perturbations of it (0.1 to 5 degrees) everywhere else"""
    gt = RC.ground_truth(variant, p)
    if count == "nan":
        return [RC.make_model(variant, np.full((3, 3), np.nan), *gt[1:]) for _ in range(max(TILE - 1, 1))]
    if count == 0:
        return []
    if count == 1:
        return [RC.start_model(variant, p, rng, rot_deg=1.0)]
    out = [None] * count
    out[0] = RC.make_model(variant, _turn90(gt[0]), *gt[1:])
    out[count // 2] = RC.make_model(variant, *gt)
    if n in WITH_NAN and count >= 4:
        out[1] = RC.make_model(variant, np.full((3, 3), np.nan), *gt[1:])
    free = [j for j in range(count) if out[j] is None]
    for j, deg in zip(free, np.linspace(0.1, 5.0, len(free)) if free else []):
        out[j] = RC.start_model(variant, p, rng, rot_deg=float(deg))
    return out


def _walk(scores):
    """GetBestEstimatedModelId: start at DBL_MAX, a candidate is taken only on a strict <"""
    best, idx = DBL_MAX, -1
    for j, s in enumerate(scores):
        if s < best:
            best, idx = float(s), j
    return idx, best


def _score_single(variant, p, o, c, cands, norm_scale):
    """(scores, errors) of one pair's candidates by score_models, in problem units"""
    n = len(p["depth0"])
    if n == 0 or not cands:  # (nothing to sum: every score is 0.0)
        return np.zeros(len(cands)), np.zeros((len(cands), 3, n))
    args = RC.pair_args(variant, p)
    ms = [RC.to_problem_units(variant, m, norm_scale) for m in cands]
    return madpose.score_models(variant, *args[:4], *args[5:], o, c, ms, with_errors=True)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(variant, sizes=SIZES, counts=COUNTS, score_type=0):
    """The pairs, their candidates, select_batch's result and the expected values, computed
    once and shared (nothing below changes them)."""
    k = Case()
    k.variant = variant
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.c.score_type = score_type
    rng = np.random.default_rng(11 + variant)
    k.pairs = [RC.make_pair(variant, SEED5 if n == 5 else 400 + i, n) for i, n in enumerate(sizes)]
    cands = [_candidates(variant, p, n, cnt, rng) for p, n, cnt in zip(k.pairs, sizes, counts)]
    # the normalization scales (make_problem's), then the duplicates: a copy of the pair's
    # best candidate in place of its last one
    first = madpose.select_batch(variant, k.pairs, cands, k.o, k.c)
    k.dup_of = {}
    for i, (p, n) in enumerate(zip(k.pairs, sizes)):
        if n in WITH_DUP and len(cands[i]) >= 4:
            s, _ = _score_single(variant, p, k.o, k.c, cands[i], first[i].norm_scale)
            b, _ = _walk(s)
            assert 0 <= b < len(cands[i]) - 1, "the case needs a best candidate before the last one"
            cands[i] = cands[i][:-1] + [cands[i][b]]
            k.dup_of[i] = b
    k.cands = cands
    k.got = madpose.select_batch(variant, k.pairs, cands, k.o, k.c, with_scores=True, with_counts=True)
    k.exp = []
    for i, p in enumerate(k.pairs):
        e = Case()
        ns = k.got[i].norm_scale
        thr = RC.thresholds(variant, k.o, ns)
        e.scores, err = _score_single(variant, p, k.o, k.c, cands[i], ns)
        e.counts = np.array([[int(np.count_nonzero(err[m, t] < thr[t])) for t in range(3)]
                             for m in range(len(cands[i]))], dtype=np.int32).reshape(-1, 3)
        e.index, e.score = _walk(e.scores)
        e.lists = [np.flatnonzero(err[e.index, t] < thr[t]).astype(np.int32) if e.index >= 0
                   else np.zeros(0, dtype=np.int32) for t in range(3)]
        k.exp.append(e)
    return k


def _key(r):
    """everything a SelectResult holds but the model object, as comparable bytes / numbers"""
    return (r.index, np.float64(r.score).tobytes(), tuple(a.tobytes() for a in r.inlier_indices), r.norm_scale,
            None if r.scores is None else r.scores.tobytes(), None if r.counts is None else r.counts.tobytes())


def _check_case(k, sizes, counts):
    assert len(k.got) == len(k.pairs)
    decided = 0
    for i, (n, cnt, r, e) in enumerate(zip(sizes, counts, k.got, k.exp)):
        what = (k.variant, n, cnt)
        K = len(k.cands[i])
        assert r.scores.dtype == np.float64 and r.scores.shape == (K,), what
        assert r.counts.dtype == np.int32 and r.counts.shape == (K, 3), what
        print(f"variant {k.variant} n {n} candidates {K}: index {r.index} (expected {e.index}) score {r.score!r} "
              f"(expected {e.score!r}) inliers {[len(a) for a in r.inlier_indices]}")
        # scores equal as bits, NaN positions equal
        assert np.array_equal(np.isnan(r.scores), np.isnan(e.scores)), what
        ok = ~np.isnan(e.scores)
        assert np.array_equal(r.scores[ok], e.scores[ok]), (what, r.scores, e.scores)
        assert np.array_equal(r.counts, e.counts), what
        assert r.index == e.index and r.score == e.score, what
        assert r.model is (k.cands[i][e.index] if e.index >= 0 else None), what
        for t in range(3):
            assert r.inlier_indices[t].dtype == np.int32
            assert np.array_equal(r.inlier_indices[t], e.lists[t]), (what, t)
            assert np.all(np.diff(r.inlier_indices[t]) > 0)
            if r.index >= 0:
                assert len(r.inlier_indices[t]) == r.counts[r.index, t], (what, t)
        if cnt == 0 or cnt == "nan":  # no candidates, or none that can win
            assert (r.index, r.score, r.model) == (-1, DBL_MAX, None), what
            assert all(len(a) == 0 for a in r.inlier_indices), what
            if cnt == "nan":
                assert K >= 1 and np.all(np.isnan(r.scores)) and not r.counts.any(), what
        elif n == 0:  # nothing to sum: every score is 0.0 and the first candidate wins
            assert r.index == 0 and r.score == 0.0 and not r.scores.any(), what
        if n in WITH_NAN and K >= 4:  # the NaN model never wins
            assert r.index != 1, what
            if k.c.score_type == 0:
                assert np.isnan(r.scores[1]), what
            else:  # (its gated terms are DBL_MAX and its other comparisons fail: every term at its cap)
                assert np.isnan(r.scores[1]) or r.scores[1] >= np.nanmax(r.scores), what
        if i in k.dup_of:  # the copy ties with the best and sits behind it: it never wins
            assert r.scores[-1] == r.scores[k.dup_of[i]] and r.index == k.dup_of[i] < K - 1, what
        # the accepted path: a finite winner strictly below the far model (candidate 0)
        if cnt == 37 and n >= 63 and np.isfinite(r.score) and r.index > 0 and r.score < r.scores[0]:
            decided += 1
    return decided


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_equals_score_models_and_the_walk(variant):
    k = _case(variant)
    # the case decides something: a test in which every candidate ties or is NaN shows nothing
    assert _check_case(k, SIZES, COUNTS) >= 1
    assert k.dup_of, "no duplicate in the case"


@pytest.mark.parametrize("score_type", [1, 2])
def test_gated_score_types(score_type):
    """score_type 1 / 2: the score's gated terms and the counts' ungated errors come from
    one evaluation"""
    sizes, counts = (65, 257), (37, TILE + 1)
    k = _case(0, sizes, counts, score_type)
    assert _check_case(k, sizes, counts) >= 1


@pytest.mark.parametrize("variant", [0, 1])
def test_chunks_slabs_order_and_neighbours(variant):
    k = _case(variant)
    base = [_key(r) for r in k.got]
    run = lambda pairs, cands, **kw: madpose.select_batch(variant, pairs, cands, k.o, k.c, with_scores=True,
                                                          with_counts=True, **kw)
    for chunk in (1, 2, 0):
        for model_chunk in (1, 3, TILE + 1, 0):
            got = run(k.pairs, k.cands, chunk=chunk, model_chunk=model_chunk)
            assert [_key(r) for r in got] == base, (chunk, model_chunk)
    perm = [4, 0, 8, 5, 2, 7, 1, 6, 3]
    got = run([k.pairs[i] for i in perm], [k.cands[i] for i in perm])
    assert [_key(r) for r in got] == [base[i] for i in perm]
    assert all(g.model is k.got[i].model for g, i in zip(got, perm))
    for i in range(len(k.pairs)):
        alone, = run([k.pairs[i]], [k.cands[i]])
        assert _key(alone) == base[i], i
    assert [_key(r) for r in run(k.pairs, k.cands)] == base
    # without the optional outputs: the same winners, and nothing else comes back
    plain = madpose.select_batch(variant, k.pairs, k.cands, k.o, k.c)
    assert [_key(r)[:4] for r in plain] == [b[:4] for b in base]
    assert all(r.scores is None and r.counts is None for r in plain)


def test_work_item_sizes_of_the_measurement_hook():
    """The kernel is built for 1, 2, 4 and 8 candidates per work item; MP_SELECT_TILE is
    shipped and pinned to score_models' bits, the others exist for the timing record
    (mp_debug_select_tile).  The shipped size set through the hook gives the default's
    bytes.  Another size evaluates the same terms with other fused products: a term is
    min(e, thr) w >= 0 with e from about 60 FP64 operations on pixel-sized values, so the
    sums agree to far better than 1e-9 relative (2^-53 is 1.1e-16), the winners of these
    well-separated cases are the same, and a count can move by one only where an error lies
    within rounding of its threshold."""
    variant = 0
    k = _case(variant, SIZES, TILE_COUNTS)
    assert _check_case(k, SIZES, TILE_COUNTS) >= 1
    base = [_key(r) for r in k.got]
    lib = L.lib()
    try:
        for tile in (1, 2, 4, 8):
            assert lib.mp_debug_select_tile(tile) >= 0
            for model_chunk in (0, 5):
                got = madpose.select_batch(variant, k.pairs, k.cands, k.o, k.c, with_scores=True, with_counts=True,
                                           model_chunk=model_chunk)
                if tile == TILE:
                    assert [_key(r) for r in got] == base, (tile, model_chunk)
                    continue
                for g, r in zip(got, k.got):
                    ok = ~np.isnan(r.scores)
                    assert np.array_equal(np.isnan(g.scores), ~ok), (tile, model_chunk)
                    err = np.abs(g.scores[ok] - r.scores[ok])
                    print(f"tile {tile} model_chunk {model_chunk}: max score difference {err.max() if err.size else 0.0:.3g}")
                    assert np.all(err <= 1e-9 * np.abs(r.scores[ok])), (tile, model_chunk)
                    assert g.index == r.index, (tile, model_chunk)
                    assert np.all(np.abs(g.counts - r.counts) <= 1), (tile, model_chunk)
    finally:
        lib.mp_debug_select_tile(0)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_composes_with_refine_batch(variant):
    """refine_batch started from the winners reports the selected score as score_initial;
    where its round is not accepted, the lists it returns are the model's own (round 0):
    their lengths are the winner's counts"""
    k = _case(variant)
    won = [i for i, r in enumerate(k.got) if r.index >= 0]
    assert len(won) >= 5
    pairs = [k.pairs[i] for i in won]
    ref = madpose.refine_batch(variant, pairs, [k.got[i].model for i in won], k.o, k.c, rounds=1)
    kept = 0
    for i, f in zip(won, ref):
        r = k.got[i]
        assert f.score_initial == r.score, (variant, SIZES[i])
        assert f.norm_scale == r.norm_scale
        if f.rounds_accepted == 0:
            kept += 1
            assert [len(a) for a in f.inlier_indices] == list(r.counts[r.index]), (variant, SIZES[i])
            assert all(np.array_equal(a, b) for a, b in zip(f.inlier_indices, r.inlier_indices))
    assert kept >= 1  # (the pairs with n = 0 and n = 5 are below the solvers' minimal samples)


def test_deterministic_64_pairs():
    o, c = synthetic.example_options("calibrated")
    rng = np.random.default_rng(5)
    sizes = rng.integers(40, 400, 64)
    pairs = [RC.make_pair(0, 300 + i, int(n)) for i, n in enumerate(sizes)]
    cands = [[RC.start_model(0, p, rng, rot_deg=float(d)) for d in rng.uniform(0.1, 5.0, int(rng.integers(0, 12)))]
             for p in pairs]
    a = madpose.select_batch(0, pairs, cands, o, c, with_scores=True, with_counts=True)
    b = madpose.select_batch(0, pairs, cands, o, c, with_scores=True, with_counts=True, model_chunk=7)
    assert [_key(r) for r in a] == [_key(r) for r in b]
    assert sum(r.index >= 0 for r in a) >= 32
