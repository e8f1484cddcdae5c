"""PairSet.draw / candidates / ransac on the device (mp_draw_set, mp_candidates_set,
mp_ransac_set).  Every comparison is of bytes against entries that already exist:
  * draw against the Python restatement of the generator (tests/draw_restatement.py, held to
    the Philox known-answer vectors by tests/test_ransac_set_cpu.py);
  * candidates against the numpy compaction of hypothesize's slot array;
  * ransac against the chain candidates -> select -> refine on the same set.
The pairs: n = 0, 3, 4, 5, 7, 8, 63, 64, 65, 257, 700 in one set -- empty, below and at every
solver's minimum, either side of a wave and of a 256-thread workgroup, several trips -- with
different intrinsics in adjacent positions."""
import functools
import os
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import synthetic
from tests import refine_cases as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restatement as D  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 3, 4, 5, 7, 8, 63, 64, 65, 257, 700)
# samples per pair around the work-item caps of the solve stages and of the sampler (two
# assignments, so that every count meets several pair sizes)
SAMPLE_COUNTS = ((0, 1, 15, 16, 17, 63, 64, 65, 17, 64, 65), (65, 64, 63, 17, 16, 15, 1, 0, 65, 63, 16))
KMD = {0: 3, 1: 4, 2: 4}
KPT = {0: 5, 1: 6, 2: 7}
SEED = 0xC0FFEE1234567890
SUBSET = [9, 2, 10, 4, 0, 7]  # a permuted subset


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


class Case:
    pass


def _pair(variant, i, n):
    """pair i of the set: its own intrinsics (focal and principal point move with i)"""
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
    p = synthetic.make_pair(900 + i, n=max(n, 8), K0=K0, K1=K1)
    if n < 8:
        for k in ("x0", "x1", "depth0", "depth1", "inlier_mask"):
            p[k] = p[k][:n]
    return p


def _samples(variant, counts, rng):
    """(types, idx) per pair: both solver types where the pair is large enough, the unread
    slots holding anything (as tests/test_hypothesize_batch_gpu.py builds them)"""
    out = []
    for n, cnt in zip(SIZES, counts):
        kinds = [t for t, k in ((0, KMD[variant]), (1, KPT[variant])) if n >= k]
        if not kinds:
            cnt = 0
        types = rng.choice(kinds, cnt).astype(np.int32) if cnt else np.zeros(0, dtype=np.int32)
        idx = rng.integers(-9, 900, (cnt, 8)).astype(np.int32)
        for s in range(cnt):
            ks = KPT[variant] if types[s] else KMD[variant]
            idx[s, :ks] = rng.choice(n, ks, replace=False)
        out.append((types, idx))
    return out


@functools.lru_cache(maxsize=None)
def _case(variant, score_type=0):
    k = Case()
    k.variant = variant
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.c.score_type = score_type
    k.pairs = [_pair(variant, i, n) for i, n in enumerate(SIZES)]
    # the n = 3 pair: every model of its samples fails the min-depth filter, which keeps a
    # model with offset0 > -min_depth[0] (calibrated: the only variant whose MD solver runs on
    # three correspondences)
    k.pairs[1]["min_depth"] = np.array([-1e6, -1e6])
    rng = np.random.default_rng(170 + variant)
    k.samples = [_samples(variant, counts, rng) for counts in SAMPLE_COUNTS]
    return k


def _compaction(hyp):
    """the README's one-liner with the tags: per pair (models (K, 17), sample, slot)"""
    out = []
    for m, n in hyp:
        rows = [m[s, :n[s]] for s in range(len(n))] + [np.zeros((0, 17))]
        smp = [np.full(n[s], s, dtype=np.int32) for s in range(len(n))] + [np.zeros(0, dtype=np.int32)]
        slot = [np.arange(n[s], dtype=np.int32) for s in range(len(n))] + [np.zeros(0, dtype=np.int32)]
        out.append((np.concatenate(rows), np.concatenate(smp), np.concatenate(slot)))
    return out


def _ckey(cands):
    return [(m.shape, m.tobytes(), s.tobytes(), t.tobytes()) for m, s, t in cands]


def _chain(ps, variant, samples, rounds, pair_ids=None):
    """candidates -> select -> refine on the pairs with a winner: one comparable key per pair"""
    cands = ps.candidates(samples, pair_ids=pair_ids)
    best = ps.select([c[0] for c in cands], pair_ids=pair_ids)
    ids = list(range(len(samples))) if pair_ids is None else list(pair_ids)
    keep = [j for j, b in enumerate(best) if b.index >= 0]
    refined = {}
    if rounds >= 1 and keep:
        rs = ps.refine([best[j].model for j in keep], rounds=rounds, pair_ids=[ids[j] for j in keep])
        refined = dict(zip(keep, rs))
    keys = []
    for j, b in enumerate(best):
        types = samples[j][0]
        head = (len(types), len(cands[j][0]), b.index, np.float64(b.score).tobytes(), np.float64(b.norm_scale).tobytes())
        if b.index < 0:
            keys.append(head + (-1, -1, -1, None, np.float64(b.score).tobytes(), np.float64(b.score).tobytes(), 0, 0, -1,
                                tuple(a.tobytes() for a in b.inlier_indices)))
            continue
        smp, slot = int(cands[j][1][b.index]), int(cands[j][2][b.index])
        origin = (smp, slot, int(types[smp]))
        if j in refined:
            r = refined[j]
            assert np.float64(r.norm_scale).tobytes() == np.float64(b.norm_scale).tobytes()
            keys.append(head + origin + (RC.model_bytes(variant, r.model), np.float64(r.score_initial).tobytes(),
                                         np.float64(r.score_final).tobytes(), r.rounds_run, r.rounds_accepted, r.status,
                                         tuple(a.tobytes() for a in r.inlier_indices)))
        else:
            keys.append(head + origin + (RC.model_bytes(variant, b.model), np.float64(b.score).tobytes(),
                                         np.float64(b.score).tobytes(), 0, 0, -1,
                                         tuple(a.tobytes() for a in b.inlier_indices)))
    return keys


def _rkeys(variant, results):
    keys = []
    for r in results:
        if r.index < 0:
            assert r.model is None and not r.model_row.any()
        keys.append((r.num_samples, r.num_candidates, r.index, np.float64(r.score_selected).tobytes(),
                     np.float64(r.norm_scale).tobytes(), r.sample, r.slot, r.solver_type,
                     None if r.model is None else RC.model_bytes(variant, r.model),
                     np.float64(r.score_initial).tobytes(), np.float64(r.score_final).tobytes(), r.rounds_run,
                     r.rounds_accepted, r.status, tuple(a.tobytes() for a in r.inlier_indices)))
    return keys


def _skey(dr):
    return [(t.tobytes(), i.tobytes()) for t, i in dr]


# ---- 1. the sampler ----

@pytest.mark.parametrize("variant", [0, 1, 2])
def test_draw_equals_restatement(variant):
    k = _case(variant)
    kmd, kpt = KMD[variant], KPT[variant]
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        for budget in (0, 1, 17, 65):
            for share in ((128, 0, 256) if budget == 17 else (128,)):
                got = ps.draw(budget, SEED, point_share=share)
                assert len(got) == len(SIZES)
                for i, n in enumerate(SIZES):
                    T, I, _ = D.draw_pair(variant, n, SEED, share, i, budget)
                    assert got[i][0].dtype == np.int32 and got[i][1].dtype == np.int32
                    assert got[i][0].shape == T.shape and got[i][1].shape == I.shape, (budget, i)
                    assert np.array_equal(got[i][0], T) and np.array_equal(got[i][1], I), (budget, share, i)
                    if n < kmd:
                        assert len(T) == 0       # too small for the MD solver: no sample
                    else:
                        assert len(T) == budget
                    if n < kpt:
                        assert not T.any()       # too small for the point solver: only type 0
                    if share == 0:
                        assert not T.any()
                    if share == 256 and n >= kpt and budget:
                        assert T.all()
                # a subset draws what the whole set draws for its pairs, in any order
                sub = ps.draw(budget, SEED, point_share=share, pair_ids=SUBSET)
                assert _skey(sub) == _skey([got[i] for i in SUBSET])
        # the default share is the solver type's (hybrid: 128); another seed draws otherwise
        whole = ps.draw(65, SEED, point_share=128)
        assert _skey(ps.draw(65, SEED)) == _skey(whole)
        assert _skey(ps.draw(65, SEED + 1)) != _skey(whole)
        types = np.concatenate([t for t, _ in whole])
        assert {0, 1} <= set(types.tolist())
        # hypothesize accepts the output unchanged
        hyp, _ = ps.hypothesize(whole)
        assert [len(c) for _, c in hyp] == [len(t) for t, _ in whole]
        assert sum(int(c.sum()) for _, c in hyp) > 0


def test_draw_over_several_slabs():
    """more samples than one slab (32768) holds: the items restart in every slab"""
    variant, budget = 0, 3300
    k = _case(variant)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        got = ps.draw(budget, 7)
    assert sum(len(t) for t, _ in got) == 10 * budget > 32768
    for i, n in enumerate(SIZES):
        T, I, _ = D.draw_pair(variant, n, 7, 128, i, budget)
        assert np.array_equal(got[i][0], T) and np.array_equal(got[i][1], I), i


# ---- 2. the hand-over ----

@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("assignment", [0, 1])
def test_candidates_equal_the_compaction_of_hypothesize(variant, assignment):
    k = _case(variant)
    S = k.samples[assignment]
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        hyp, _ = ps.hypothesize(S)
        want = _compaction(hyp)
        assert sum(len(m) for m, _, _ in want) > 0
        got = ps.candidates(S)
        assert _ckey(got) == _ckey(want)
        assert _ckey(ps.candidates(S)) == _ckey(want)  # a repeated call
        for chunk in (16, 37):  # slabs that cut through pairs and through a sample's neighbours
            assert _ckey(ps.candidates(S, sample_chunk=chunk)) == _ckey(want), chunk
        for i in range(len(SIZES)):  # each pair alone
            assert _ckey(ps.candidates([S[i]], pair_ids=[i])) == _ckey([want[i]]), i
        assert _ckey(ps.candidates([S[i] for i in SUBSET], pair_ids=SUBSET, sample_chunk=37)) == \
            _ckey([want[i] for i in SUBSET])
        # the stage it shares with hypothesize still returns hypothesize's bytes afterwards
        again, _ = ps.hypothesize(S)
        assert [(m.tobytes(), c.tobytes()) for m, c in again] == [(m.tobytes(), c.tobytes()) for m, c in hyp]
    if variant == 0:
        assert len(S[1][0]) > 0
        assert len(want[1][0]) == 0  # the n = 3 pair: the min-depth filter rejects every model


# ---- 3. the fused call ----

@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("score_type", [1, 2])
def test_ransac_equals_the_chain(variant, score_type):
    k = _case(variant, score_type)
    S = k.samples[1]
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        for rounds in (0, 1, 3):
            want = _chain(ps, variant, S, rounds)
            got = ps.ransac(samples=S, rounds=rounds)
            assert _rkeys(variant, got) == want, rounds
        # rounds = 3 from here on: the cuts and the selection do not show
        assert _rkeys(variant, ps.ransac(samples=S, sample_chunk=16, model_chunk=7)) == want
        assert _rkeys(variant, ps.ransac(samples=S, sample_chunk=37, model_chunk=1)) == want
        sub = ps.ransac(samples=[S[i] for i in SUBSET], pair_ids=SUBSET)
        assert _rkeys(variant, sub) == [want[i] for i in SUBSET]
        assert _rkeys(variant, sub) == _chain(ps, variant, [S[i] for i in SUBSET], 3, pair_ids=SUBSET)
        # no state: other calls on the set in between leave the bytes unchanged
        ps.select([np.zeros((0, 17))] * len(SIZES))
        ps.refine([RC.make_model(variant, *RC.ground_truth(variant, k.pairs[10]))], rounds=2, pair_ids=[10])
        ps.draw(3, 1)
        assert _rkeys(variant, ps.ransac(samples=S)) == want
    # the case holds what it is meant to
    assert want[0][2] == -1 and want[0][0] == 0          # the empty pair: no sample, no winner
    assert any(key[2] >= 0 and key[11] >= 1 for key in want)  # a refinement ran
    if variant == 0:
        assert want[1][0] > 0 and want[1][1] == 0 and want[1][2] == -1  # samples, but no model
    assert got[0].model is None and got[0].inlier_indices[0].shape == (0,)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_ransac_with_a_budget_equals_the_chain_on_the_draw(variant):
    k = _case(variant, 0)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        for share in (None, 40):
            S = ps.draw(65, SEED, point_share=share)
            want = _chain(ps, variant, S, 3)
            got = ps.ransac(budget=65, seed=SEED, point_share=share)
            assert _rkeys(variant, got) == want, share
            assert _rkeys(variant, ps.ransac(samples=S)) == want
        # share 40 from here on: slabs through pairs, a permuted subset (the draw of a pair is
        # by its index in the set), rounds = 0
        assert _rkeys(variant, ps.ransac(budget=65, seed=SEED, point_share=40, sample_chunk=37, model_chunk=7)) == want
        sub = ps.ransac(budget=65, seed=SEED, point_share=40, pair_ids=SUBSET, sample_chunk=16)
        assert _rkeys(variant, sub) == [want[i] for i in SUBSET]
        assert _rkeys(variant, ps.ransac(budget=65, seed=SEED, point_share=40, rounds=0)) == _chain(ps, variant, S, 0)
        assert all(r.num_samples == 0 and r.index == -1 for r in ps.ransac(budget=0))
    assert sum(key[2] >= 0 for key in want) >= 5
    assert [r.num_samples for r in got] == [65 if n >= KMD[variant] else 0 for n in SIZES]


def test_bad_arguments_on_a_live_set_are_einval():
    """the refusals that need a set with pairs: null required pointers, a repeated pair_ids
    entry, samples a solver cannot take -- MP_EINVAL, and the set works afterwards"""
    import ctypes

    from madpose_amd import _lib as L
    k = _case(0)
    P = len(SIZES)
    lib = L.lib()
    with madpose.PairSet(0, k.pairs, k.o, k.c) as ps:
        h = ps._h
        mods, res = (L.mp_model * P)(), (L.mp_ransac_result * P)()
        twice = (ctypes.c_int32 * 2)(4, 4)
        cnt, ty, ix = (ctypes.c_int32 * P)(), (ctypes.c_int32 * (4 * P))(), (ctypes.c_int32 * (32 * P))()
        nm = ctypes.c_int64(0)
        assert lib.mp_ransac_set(h, P, None, 4, 0, -1, None, None, None, 1, None, res, None, 0, 0) == L.MP_EINVAL
        assert lib.mp_ransac_set(h, P, None, 4, 0, -1, None, None, None, 1, mods, None, None, 0, 0) == L.MP_EINVAL
        assert lib.mp_ransac_set(h, 2, twice, 4, 0, -1, None, None, None, 1, mods, res, None, 0, 0) == L.MP_EINVAL
        assert b"occurs twice" in lib.mp_last_error()
        assert lib.mp_ransac_set(h, P - 1, None, 4, 0, -1, None, None, None, 1, mods, res, None, 0, 0) == L.MP_EINVAL
        assert lib.mp_draw_set(h, P, None, 4, 0, -1, ty, ix, None) == L.MP_EINVAL
        assert lib.mp_draw_set(h, P, None, 4, 0, -1, None, ix, cnt) == L.MP_EINVAL
        assert lib.mp_draw_set(h, 2, twice, 4, 0, -1, ty, ix, cnt) == L.MP_EINVAL
        assert lib.mp_candidates_set(h, P, None, None, None, None, 0, ctypes.byref(nm)) == L.MP_EINVAL
        assert lib.mp_candidates_set(h, 2, twice, None, None, None, 0, ctypes.byref(nm)) == L.MP_EINVAL
        # a point-solver sample on the pair of three correspondences; an index outside the pair
        so = (ctypes.c_int64 * 2)(0, 1)
        one_t, one_i = (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 7)
        pid = (ctypes.c_int32 * 1)(1)
        assert lib.mp_candidates_set(h, 1, pid, so, one_t, one_i, 0, ctypes.byref(nm)) == L.MP_EINVAL
        assert lib.mp_ransac_set(h, 1, pid, -1, 0, -1, so, one_t, one_i, 1, mods, res, None, 0, 0) == L.MP_EINVAL
        one_t[0] = 0
        one_i[2] = 3
        assert lib.mp_ransac_set(h, 1, pid, -1, 0, -1, so, one_t, one_i, 1, mods, res, None, 0, 0) == L.MP_EINVAL
        assert b"outside the pair" in lib.mp_last_error()
        assert lib.mp_candidates_fetch(h, None, so, None, None) == L.MP_EINVAL  # (no result was kept)
        # the set is as good as before
        S = ps.draw(17, SEED)
        assert _rkeys(0, ps.ransac(budget=17, seed=SEED)) == _chain(ps, 0, S, 3)
