"""PairSet on the device (mp_pair_set_*): pairs set up once, and hypothesize / select / refine
on them return, byte for byte, what hypothesize_batch / select_batch / refine_batch return on
the same pairs -- for the whole set, for a permuted subset, in any order of calls, with two
sets open at once.  The calibrated rows derived by the one multi-pair preparation launch equal
the rows of one launch per pair in every bit.

The expected values are the batch entries' own results (pinned by their own tests); the pairs,
start models, candidates and samples are built as tests/test_refine_batch_gpu.py,
tests/test_select_batch_gpu.py and tests/test_hypothesize_batch_gpu.py build theirs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import refine_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# an empty pair, one at the calibrated point solver's minimum, either side of a wave (64
# lanes) and of the 256-thread workgroup, several trips
SIZES = (0, 5, 63, 64, 65, 257, 700)
SEED5 = 1  # (the n = 5 pair of tests/test_refine_batch_gpu.py)
# candidates per pair: none, one, only NaN models ("nan"), many
CAND_COUNTS = (2, 1, 37, 0, 37, "nan", 37)
WITH_NAN = (65, 700)  # pairs (by n) with one NaN model among real ones
WITH_DUP = (65, 700)  # pairs whose last candidate is a copy of their best
# samples per pair, around the work-item caps of the solve stages (two assignments, so that
# every count occurs with seven pairs)
SAMPLE_COUNTS = ((0, 1, 15, 16, 17, 63, 64), (0, 65, 64, 63, 17, 16, 15))
KMD = {0: 3, 1: 4, 2: 4}
KPT = {0: 5, 1: 6, 2: 7}
VARIANT_SCORE = [(v, s) for v in (0, 1, 2, 3) for s in (0, 1, 2)]


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


class Case:
    pass


def _candidates(variant, p, n, count, rng):
    """the far model first, a NaN model second (WITH_NAN), the ground truth in the middle,
    perturbations of it everywhere else (tests/test_select_batch_gpu.py)"""
    gt = RC.ground_truth(variant, p)
    if count == "nan":
        return [RC.make_model(variant, np.full((3, 3), np.nan), *gt[1:])]
    if count == 0:
        return []
    if count == 1:
        return [RC.start_model(variant, p, rng, rot_deg=1.0)]
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = [None] * count
    out[0] = RC.make_model(variant, turn @ gt[0], *gt[1:])
    out[count // 2] = RC.make_model(variant, *gt)
    if n in WITH_NAN and count >= 4:
        out[1] = RC.make_model(variant, np.full((3, 3), np.nan), *gt[1:])
    free = [j for j in range(count) if out[j] is None]
    for j, deg in zip(free, np.linspace(0.1, 5.0, len(free)) if free else []):
        out[j] = RC.start_model(variant, p, rng, rot_deg=float(deg))
    return out


def _samples(variant, sizes, counts, rng):
    """(types, idx) per pair: both solver types where the pair is large enough for them, the
    unread slots holding anything (tests/test_hypothesize_batch_gpu.py)"""
    out = []
    for n, cnt in zip(sizes, counts):
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
def _case(variant, score_type=0, thr_scale=1.0):
    """Pairs, options, two sets of start models, candidates and samples; built once and never
    changed.  The batch entries' results are added by _batch()."""
    k = Case()
    k.variant = variant
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.c.score_type = score_type
    k.o.squared_inlier_thresholds = [float(v) * thr_scale for v in k.o.squared_inlier_thresholds[:2]]
    rng = np.random.default_rng(70 + variant)
    k.pairs = [RC.make_pair(variant, SEED5 if n == 5 else 500 + i, n) for i, n in enumerate(SIZES)]
    k.models_a = [RC.start_model(variant, p, rng) for p in k.pairs]
    k.models_b = [RC.start_model(variant, p, rng, rot_deg=2.0) for p in k.pairs]
    cands = [_candidates(variant, p, n, cnt, rng) for p, n, cnt in zip(k.pairs, SIZES, CAND_COUNTS)]
    first = madpose.select_batch(variant, k.pairs, cands, k.o, k.c)
    k.dups = 0
    for i, n in enumerate(SIZES):
        if n in WITH_DUP and 0 <= first[i].index < len(cands[i]) - 1:
            cands[i] = cands[i][:-1] + [cands[i][first[i].index]]
            k.dups += 1
    k.cands = cands
    if variant != 3:
        k.samples = [_samples(variant, SIZES, counts, rng) for counts in SAMPLE_COUNTS]
    k.batch = {}
    return k


def _batch(k, what, *extra):
    """the batch entry's result on the case's pairs, computed once"""
    key = (what,) + extra
    if key not in k.batch:
        if what == "refine":
            models, rounds = extra
            k.batch[key] = madpose.refine_batch(k.variant, k.pairs, getattr(k, models), k.o, k.c, rounds=rounds)
        elif what == "select":
            k.batch[key] = madpose.select_batch(k.variant, k.pairs, k.cands, k.o, k.c, with_scores=True,
                                                with_counts=True)
        else:
            k.batch[key] = madpose.hypothesize_batch(k.variant, k.pairs, k.samples[extra[0]], k.o, k.c)
    return k.batch[key]


def _rkeys(variant, rs):
    return [RC.result_key(variant, r) for r in rs]


def _skey(r):
    """everything a SelectResult holds but the model object, as comparable bytes / numbers"""
    return (r.index, np.float64(r.score).tobytes(), tuple(a.tobytes() for a in r.inlier_indices),
            np.float64(r.norm_scale).tobytes(), None if r.scores is None else r.scores.tobytes(),
            None if r.counts is None else r.counts.tobytes())


def _skeys(rs):
    return [_skey(r) for r in rs]


def _hkey(res):
    hyp, norm = res
    return ([(m.shape, m.tobytes(), c.tobytes()) for m, c in hyp], np.asarray(norm, dtype=np.float64).tobytes())


# ---- 1. the same bytes as the batch entries ----

@pytest.mark.parametrize("variant,score_type", VARIANT_SCORE)
def test_refine_and_select_equal_the_batch_entries(variant, score_type):
    k = _case(variant, score_type)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        assert len(ps) == len(SIZES) and ps.num_correspondences == sum(SIZES)
        for rounds in (1, 3):
            want = _batch(k, "refine", "models_a", rounds)
            got = ps.refine(k.models_a, rounds=rounds)
            assert _rkeys(variant, got) == _rkeys(variant, want), rounds
        want = _batch(k, "select")
        got = ps.select(k.cands, with_scores=True, with_counts=True)
        assert _skeys(got) == _skeys(want)
        for g, w in zip(got, want):  # (the chosen candidate object itself)
            assert g.model is w.model or (g.model is None and w.model is None)
        assert np.array_equal(ps.norm_scale, [r.norm_scale for r in want])
        # without the optional outputs, and in small record slabs
        plain = ps.select(k.cands, model_chunk=7)
        assert [(r.index, r.score, r.scores, r.counts) for r in plain] == [(r.index, r.score, None, None)
                                                                           for r in want]
    # the case holds what it is meant to: a refinement that moves, no candidates, only NaN
    # candidates, a duplicate of the best
    if score_type == 0:
        assert any(r.rounds_accepted > 0 for r in _batch(k, "refine", "models_a", 3))
        assert want[5].index == -1  # (under the other score types a NaN pose's gated errors sum to a finite score)
    assert want[3].index == -1 and want[6].index >= 0
    assert k.dups >= 1


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("assignment", [0, 1])
def test_hypothesize_equals_the_batch_entry(variant, assignment):
    k = _case(variant)
    want = _batch(k, "hypothesize", assignment)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        got = ps.hypothesize(k.samples[assignment])
        assert _hkey(got) == _hkey(want)
        assert _hkey(ps.hypothesize(k.samples[assignment], sample_chunk=7)) == _hkey(want)
        assert np.array_equal(ps.norm_scale, want[1])
    types = np.concatenate([t for t, _ in k.samples[assignment]])
    assert {0, 1} <= set(types.tolist())
    assert sum(int(c.sum()) for _, c in want[0]) > 0


# ---- 2. the rows of the one-launch preparation ----

def _rows(ps, pair, n):
    out = np.full(12 * max(n, 1), np.nan)
    L.check(L.lib().mp_debug_pair_set_rows(ps._h, pair, out.ctypes.data_as(L.c_double_p)))
    return out[:12 * n].reshape(12, n)


@pytest.mark.parametrize("variant", [0, 3])
def test_prepared_rows_equal_the_per_pair_launches(variant):
    """sizes on either side of the 256-correspondence item in adjacent positions: a write past
    a pair's end would land in its neighbour's rows"""
    sizes = (0, 1, 255, 256, 257, 700, 0, 1)
    o, c = synthetic.example_options("calibrated")
    pairs = []
    for i, n in enumerate(sizes):
        f = 480.0 + 35.0 * i  # (different intrinsics per pair: a record of the wrong pair would show)
        K = np.array([[f, 0.0, 310.0 + 3.0 * i], [0.0, f * 1.01, 235.0 + 2.0 * i], [0.0, 0.0, 1.0]])
        p = synthetic.make_pair(800 + i, n=max(n, 8), K0=K, K1=K * [[1.1], [1.1], [1.0]])
        for key in ("x0", "x1", "depth0", "depth1"):
            p[key] = p[key][:n]
        pairs.append(p)
    lib = L.lib()
    rows = {}
    try:
        for mode in (0, 1):
            assert lib.mp_debug_pair_set_prep(mode) == L.MP_OK
            with madpose.PairSet(variant, pairs, o, c) as ps:
                rows[mode] = [_rows(ps, i, n) for i, n in enumerate(sizes)]
    finally:
        assert lib.mp_debug_pair_set_prep(0) == L.MP_OK
    for i, (p, n) in enumerate(zip(pairs, sizes)):
        a, b = rows[0][i], rows[1][i]
        assert a.shape == b.shape == (12, n)
        assert a.tobytes() == b.tobytes(), (i, n)
        packed = np.stack([p["x0"][:, 0], p["x0"][:, 1], p["x1"][:, 0], p["x1"][:, 1], p["depth0"], p["depth1"]])
        assert a[:6].tobytes() == np.ascontiguousarray(packed, dtype=np.float64).tobytes(), (i, n)
        if n:
            # the derived rows are what they are meant to be: 1 / |K^-1 x| and the rays' xy
            for cam, r, ray in ((0, 6, 8), (1, 7, 10)):
                x = np.c_[p[f"x{cam}"], np.ones(n)] @ np.linalg.inv(p[f"K{cam}"]).T
                assert np.allclose(a[r], 1.0 / np.linalg.norm(x, axis=1), rtol=1e-12, atol=0)
                assert np.allclose(a[ray:ray + 2], x[:, :2].T, rtol=1e-12, atol=1e-15)


# ---- 3. no state between calls ----

@pytest.mark.parametrize("variant", [0, 1])
def test_calls_leave_no_state_in_the_set(variant):
    k = _case(variant)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        first = ps.refine(k.models_a, rounds=3)
        sel = ps.select(k.cands, with_scores=True, with_counts=True)
        hyp = ps.hypothesize(k.samples[0])
        other = ps.refine(k.models_b, rounds=3)
        again = ps.refine(k.models_a, rounds=3)
        sel2 = ps.select(k.cands, with_scores=True, with_counts=True)
    assert _rkeys(variant, again) == _rkeys(variant, first)
    assert _rkeys(variant, first) == _rkeys(variant, _batch(k, "refine", "models_a", 3))
    assert _rkeys(variant, other) == _rkeys(variant, _batch(k, "refine", "models_b", 3))
    assert _skeys(sel) == _skeys(sel2) == _skeys(_batch(k, "select"))
    assert _hkey(hyp) == _hkey(_batch(k, "hypothesize", 0))
    assert _rkeys(variant, other) != _rkeys(variant, first)  # (the call in between was another one)


# ---- 4. selections ----

@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_selection_equals_the_batch_entry_on_those_pairs(variant):
    k = _case(variant)
    ids = [6, 0, 3, 1, 5]  # permuted, with the empty pair, without pairs 2 and 4
    sub = [k.pairs[i] for i in ids]
    pick = lambda xs: [xs[i] for i in ids]
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        got = ps.refine(pick(k.models_a), rounds=3, pair_ids=ids)
        want = madpose.refine_batch(variant, sub, pick(k.models_a), k.o, k.c, rounds=3)
        assert _rkeys(variant, got) == _rkeys(variant, want)
        # (the inlier_idx layout over the selection, through the lists: each list is the
        # list of the same pair in the whole-set call)
        whole = _batch(k, "refine", "models_a", 3)
        assert _rkeys(variant, got) == _rkeys(variant, pick(whole))
        assert sum(len(a) for r in got for a in r.inlier_indices) > 0
        got = ps.select(pick(k.cands), with_scores=True, with_counts=True, pair_ids=ids)
        want = madpose.select_batch(variant, sub, pick(k.cands), k.o, k.c, with_scores=True, with_counts=True)
        assert _skeys(got) == _skeys(want) == _skeys(pick(_batch(k, "select")))
        if variant != 3:
            got = ps.hypothesize(pick(k.samples[1]), pair_ids=np.asarray(ids))
            want = madpose.hypothesize_batch(variant, sub, pick(k.samples[1]), k.o, k.c)
            assert _hkey(got) == _hkey(want)
        # an empty selection
        assert ps.refine([], pair_ids=[]) == [] and ps.select([], pair_ids=[]) == []
        # refused selections and counts, and the set works afterwards
        with pytest.raises(ValueError, match=r"pair_ids\[2\] = 6 occurs twice"):
            ps.refine(pick(k.models_a)[:3], pair_ids=[6, 0, 6])
        with pytest.raises(ValueError, match=r"pair_ids\[1\] = 7 is outside"):
            ps.select(pick(k.cands)[:2], pair_ids=[0, 7])
        with pytest.raises(ValueError, match="one model per selected pair"):
            ps.refine(k.models_a[:3])
        # the library's own check of the same (the Python class checks first)
        lib = L.lib()
        arr = (L.mp_model * 3)()
        res = (L.mp_refine_result * 3)()
        for bad, text in (([6, 0, 6], b"pair_ids[2] = 6 occurs twice"), ([0, 7, 1], b"pair_ids[1] = 7 is outside"),
                          ([0, -1, 1], b"pair_ids[1] = -1 is outside")):
            bad = np.asarray(bad, dtype=np.int32)
            assert lib.mp_refine_set(ps._h, 3, bad.ctypes.data_as(L.c_int32_p), 1, arr, res, None) == L.MP_EINVAL
            assert text in lib.mp_last_error()
        assert lib.mp_refine_set(ps._h, 3, None, 1, arr, res, None) == L.MP_EINVAL  # (NULL: all 7 pairs)
        assert _rkeys(variant, ps.refine(k.models_a, rounds=3)) == _rkeys(variant, whole)


# ---- 5. two sets at once ----

def test_two_sets_interleaved():
    variant = 0
    ka, kb = _case(variant, 1), _case(variant, 2, 0.25)
    assert ka.o.squared_inlier_thresholds[0] != kb.o.squared_inlier_thresholds[0]
    with madpose.PairSet(variant, ka.pairs, ka.o, ka.c) as pa, madpose.PairSet(variant, kb.pairs, kb.o, kb.c) as pb:
        ra = pa.refine(ka.models_a, rounds=3)
        sb = pb.select(kb.cands, with_scores=True, with_counts=True)
        rb = pb.refine(kb.models_a, rounds=3)
        sa = pa.select(ka.cands, with_scores=True, with_counts=True)
        ha = pa.hypothesize(ka.samples[0])
        hb = pb.hypothesize(kb.samples[0])
        ra2 = pa.refine(ka.models_a, rounds=3)
    assert _rkeys(variant, ra) == _rkeys(variant, ra2) == _rkeys(variant, _batch(ka, "refine", "models_a", 3))
    assert _rkeys(variant, rb) == _rkeys(variant, _batch(kb, "refine", "models_a", 3))
    assert _skeys(sa) == _skeys(_batch(ka, "select")) and _skeys(sb) == _skeys(_batch(kb, "select"))
    assert _hkey(ha) == _hkey(_batch(ka, "hypothesize", 0)) and _hkey(hb) == _hkey(_batch(kb, "hypothesize", 0))
    # (the two sets do differ: the same pairs under other thresholds and another score type)
    assert _rkeys(variant, ra) != _rkeys(variant, rb) and _skeys(sa) != _skeys(sb)


# ---- 6. restrictions and lifetime ----

def test_restrictions_and_lifetime():
    """resident_bytes: 96 bytes per correspondence for the rows after creation; the list
    buffers are allocated on first use, 12 bytes per correspondence each -- none for
    hypothesize, one for select, two for refine (120 per correspondence then), and they stay."""
    k3, k0 = _case(3), _case(0)
    T = sum(SIZES)
    smp = k0.samples[0]
    lib = L.lib()
    with madpose.PairSet(3, k3.pairs, k3.o, k3.c) as ps:
        with pytest.raises(ValueError, match="scale only"):
            ps.hypothesize(smp)
        # (the library's own refusal; the Python class checks first)
        soffs = np.zeros(len(SIZES) + 1, dtype=np.int64)
        assert lib.mp_hypothesize_set(ps._h, len(SIZES), None, soffs.ctypes.data_as(L.c_int64_p), None, None, None,
                                      None, 0) == L.MP_EINVAL
        assert b"MP_SCALE_ONLY" in lib.mp_last_error()
        assert _skeys(ps.select(k3.cands, with_scores=True, with_counts=True)) == _skeys(_batch(k3, "select"))
    o_ours, c = synthetic.example_options("calibrated")
    o_ours.use_ours = True
    with madpose.PairSet(0, k0.pairs, o_ours, c) as ps:
        with pytest.raises(ValueError, match="use_ours"):
            ps.hypothesize(smp)
        soffs = np.zeros(len(SIZES) + 1, dtype=np.int64)
        assert lib.mp_hypothesize_set(ps._h, len(SIZES), None, soffs.ctypes.data_as(L.c_int64_p), None, None, None,
                                      None, 0) == L.MP_EINVAL
        assert b"use_ours" in lib.mp_last_error()
        got = ps.select(k0.cands, with_scores=True, with_counts=True)
        want = madpose.select_batch(0, k0.pairs, k0.cands, o_ours, c, with_scores=True, with_counts=True)
        assert _skeys(got) == _skeys(want)
    c_ns = madpose.EstimatorConfig()
    c_ns.use_shift = False
    with madpose.PairSet(0, k0.pairs, k0.o, c_ns) as ps:
        with pytest.raises(ValueError, match="use_shift"):
            ps.hypothesize(smp)
    # resident bytes and the lazy list buffers
    ps = madpose.PairSet(0, k0.pairs, k0.o, k0.c)
    assert ps.num_correspondences == T and ps.resident_bytes == 96 * T
    ps.hypothesize(smp)
    assert ps.resident_bytes == 96 * T
    ps.select(k0.cands)
    assert ps.resident_bytes == 108 * T
    ps.refine(k0.models_a)
    assert ps.resident_bytes == 120 * T
    ps.select(k0.cands)
    assert ps.resident_bytes == 120 * T
    ps.close()
    ps.close()
    for call in (lambda: ps.refine(k0.models_a), lambda: ps.select(k0.cands), lambda: ps.hypothesize(smp),
                 lambda: len(ps), lambda: ps.norm_scale, lambda: ps.resident_bytes):
        with pytest.raises(ValueError, match="closed"):
            call()
    # an empty set, and a set of empty pairs only
    with madpose.PairSet(0, [], k0.o, k0.c) as ps:
        assert len(ps) == 0 and ps.refine([]) == [] and ps.select([]) == [] and ps.resident_bytes == 0
    empties = [k0.pairs[0], k0.pairs[0]]
    with madpose.PairSet(0, empties, k0.o, k0.c) as ps:
        got = ps.refine(k0.models_a[:2])
        assert _rkeys(0, got) == _rkeys(0, madpose.refine_batch(0, empties, k0.models_a[:2], k0.o, k0.c))
        assert ps.resident_bytes == 0 and ps.num_correspondences == 0


# ---- 7. a process that exits with a set open ----

EXIT_CODE = r"""
import numpy as np
import madpose
from madpose_amd import synthetic
from tests import refine_cases as RC
o, c = synthetic.example_options("calibrated")
pairs = [RC.make_pair(0, 900 + i, n) for i, n in enumerate((300, 0, 65))]
rng = np.random.default_rng(3)
models = [RC.start_model(0, p, rng) for p in pairs]
ps = madpose.PairSet(0, pairs, o, c)
keep = madpose.PairSet(0, pairs[:1], o, c)
out = ps.refine(models, rounds=2)
assert len(out) == 3 and out[0].score_final <= out[0].score_initial
print("DONE", len(ps), flush=True)
# forget the handles: both sets stay open in the library, whatever the interpreter finalises
ps._h = keep._h = None
"""


def test_exit_with_an_open_set():
    env = {k: v for k, v in os.environ.items() if not k.startswith("MADPOSE_")}
    r = subprocess.run([sys.executable, "-c", EXIT_CODE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "DONE 3" in r.stdout, r.stdout[-2000:]
    low = r.stderr.lower()
    assert "hip" not in low and "error" not in low and "fault" not in low, r.stderr[-4000:]
