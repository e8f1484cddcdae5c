"""hypothesize_batch on the device (mp_hypothesize_batch): for explicit samples of many pairs,
exactly the models the estimator's MinimalSolver stage forms for them.

* pinned to the estimator: every walked iteration of an estimator run (its solver type and
  sample from MADPOSE_COUNT_DUMP, its models from MADPOSE_MODEL_DUMP) fed back as an
  explicit sample gives the same count and the same 17 doubles per model, byte for byte
  (shared and two focal: the focals are the dump's times norm_scale, one float64 product);
* pinned to the oracle, independently of the estimator: the calibrated models of both
  solver types and the shared / two-focal MD models equal the CPU oracle's own
  (ORACLE_COUNT_DUMP / ORACLE_MODEL_DUMP) to the bit;
* many pairs at once: every pair's result equals that pair run alone, under pair and sample
  permutation, any chunk and sample_chunk, and a repeated call;
* the chain: the models as select_batch's array candidates give the winner, score and lists
  of the same candidates passed as pose objects, and refine_batch starts from that score.
"""
import numpy as np
import pytest

import madpose
import oracle
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests.helpers import oracle_cfg, oracle_opts

pytestmark = pytest.mark.gpu

KIND = {0: "calibrated", 1: "shared_focal", 2: "two_focal"}
KMD = {0: 3, 1: 4, 2: 4}
KPT = {0: 5, 1: 6, 2: 7}
ESTIMATE = {0: "HybridEstimatePoseScaleOffset", 1: "HybridEstimatePoseScaleOffsetSharedFocal",
            2: "HybridEstimatePoseScaleOffsetTwoFocal"}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _cams(p, variant):
    return (p["K0"], p["K1"]) if variant == 0 else (p["pp0"], p["pp1"])


def _read_models(path):
    out = []
    raw = open(path, "rb").read()
    pos = 0
    while pos < len(raw):
        it, n = np.frombuffer(raw, dtype=np.int32, count=2, offset=pos)
        pos += 8
        m = np.frombuffer(raw, dtype=np.float64, count=17 * n, offset=pos).reshape(n, 17)
        pos += 8 * 17 * n
        out.append((int(it), m))
    return out


def _read_counts(path):
    """(iteration, solver type, model count, sample) per line"""
    out = []
    for line in open(path):
        v = [int(x) for x in line.split()]
        out.append((v[0], v[1], v[2], v[3:]))
    return out


def _samples_of(lines):
    types = np.array([ln[1] for ln in lines], dtype=np.int32)
    idx = np.zeros((len(lines), 8), dtype=np.int32)
    for k, ln in enumerate(lines):
        idx[k, :len(ln[3])] = ln[3]
    return types, idx


def _to_user(m, variant, norm):
    """a dump's models (problem units) in user units: the focals times norm_scale"""
    m = m.copy()
    if variant != 0:
        m[:, 15] = m[:, 15] * np.float64(norm)
        m[:, 16] = m[:, 16] * np.float64(norm)
    return m


def _assert_pinned(variant, models, counts, lines, dumped, norm, only_type=None):
    assert len(lines) == len(dumped) == len(counts)
    slots = L.HYPOTHESIZE_SLOTS[variant]
    assert models.shape == (len(lines), slots, 17)
    checked = nm = 0
    for k, ((it, st, cnt, smp), (it2, ref)) in enumerate(zip(lines, dumped)):
        assert it == it2 and cnt == ref.shape[0]
        assert len(smp) == (KMD[variant] if st == 0 else KPT[variant])
        if only_type is not None and st != only_type:
            continue
        assert counts[k] == cnt, (it, st, counts[k], cnt)
        want = _to_user(ref, variant, norm)
        assert models[k, :cnt].tobytes() == want.tobytes(), (it, st, np.abs(models[k, :cnt] - want).max())
        assert not models[k, cnt:].any()
        checked += 1
        nm += cnt
    return checked, nm


@pytest.mark.parametrize("variant,seed,solver", [(0, 11, 0), (0, 12, 0), (0, 13, 1), (0, 14, 2),
                                                 (1, 11, 0), (1, 13, 1), (1, 14, 2),
                                                 (2, 11, 0), (2, 13, 1), (2, 14, 2)])
def test_models_are_the_estimators_to_the_bit(variant, seed, solver, tmp_path, monkeypatch):
    """Every walked iteration of an estimator run (solver_type 0 hybrid, 1 the point solver
    alone, 2 the MD solver alone), fed back as an explicit sample: the same model count and
    the same bytes.  No tolerance."""
    p = synthetic.make_pair(seed, n=300)
    o, c = synthetic.example_options(KIND[variant], iterations=400)
    c.solver_type = solver
    cd, md = str(tmp_path / "counts.txt"), str(tmp_path / "models.bin")
    monkeypatch.setenv("MADPOSE_COUNT_DUMP", cd)
    monkeypatch.setenv("MADPOSE_MODEL_DUMP", md)
    cam0, cam1 = _cams(p, variant)
    getattr(madpose, ESTIMATE[variant])(p["x0"], p["x1"], p["depth0"], p["depth1"], p["min_depth"], cam0, cam1, o, c)
    monkeypatch.delenv("MADPOSE_COUNT_DUMP")
    monkeypatch.delenv("MADPOSE_MODEL_DUMP")
    lines, dumped = _read_counts(cd), _read_models(md)
    assert len(lines) >= 100
    kinds = {ln[1] for ln in lines}
    assert kinds == ({0, 1} if solver == 0 else ({1} if solver == 1 else {0}))
    res, norm = madpose.hypothesize_batch(variant, [p], [_samples_of(lines)], o, c)
    (models, counts), = res
    if variant == 0:
        assert norm[0] == 1.0
    checked, nm = _assert_pinned(variant, models, counts, lines, dumped, norm[0])
    assert checked == len(lines) and nm > 0  # (every iteration compared, and not only empty ones)


@pytest.mark.parametrize("variant,seed,solver", [(0, 11, 0), (0, 12, 0), (0, 13, 1), (0, 14, 1),
                                                 (1, 11, 0), (1, 12, 0), (2, 11, 0), (2, 12, 0)])
def test_models_are_the_oracles_to_the_bit(variant, seed, solver, tmp_path, monkeypatch):
    """Independently of the estimator: the samples and models of the CPU oracle's own run
    (ORACLE_COUNT_DUMP / ORACLE_MODEL_DUMP, oracle/src/ransac.cpp).  Calibrated: both solver
    types equal the oracle's to the bit.  Shared and two focal: the type-0 (MD) iterations
    do; their 6pt / 7pt iterations are pinned by the estimator test above only -- the 6pt
    deflated eigenproblem and the two-focal Bougnoux / recoverPose / cubic are not bitwise
    restatements of the oracle."""
    p = synthetic.make_pair(seed, n=300)
    o, c = synthetic.example_options(KIND[variant], iterations=400)
    c.solver_type = solver
    cd, md = str(tmp_path / "counts.txt"), str(tmp_path / "models.bin")
    monkeypatch.setenv("ORACLE_COUNT_DUMP", cd)
    monkeypatch.setenv("ORACLE_MODEL_DUMP", md)
    cam0, cam1 = _cams(p, variant)
    oracle.estimate(variant, p["x0"], p["x1"], p["depth0"], p["depth1"], p["min_depth"], cam0, cam1, oracle_opts(o),
                    oracle_cfg(c))
    monkeypatch.delenv("ORACLE_COUNT_DUMP")
    monkeypatch.delenv("ORACLE_MODEL_DUMP")
    lines, dumped = _read_counts(cd), _read_models(md)
    # the oracle's dump must be worth comparing with (checked on the CPU for these seeds)
    assert len(lines) >= 100
    kinds = {ln[1] for ln in lines}
    assert kinds == ({0, 1} if solver == 0 else {1})
    assert sum(m.shape[0] for _, m in dumped) > 20
    res, norm = madpose.hypothesize_batch(variant, [p], [_samples_of(lines)], o, c)
    (models, counts), = res
    checked, nm = _assert_pinned(variant, models, counts, lines, dumped, norm[0], only_type=None if variant == 0 else 0)
    assert checked == (len(lines) if variant == 0 else sum(1 for ln in lines if ln[1] == 0))
    assert nm > (20 if variant == 0 else 4)  # (shared / two focal: the MD iterations' models alone)


# ---------------------------------------------------------------------------
COUNTS = (1, 15, 16, 17, 63, 64, 65, 0)  # samples per pair (the last pair has none)


def _many_pairs(variant):
    """Eight pairs with different intrinsics (hence principal points), sizes and min_depth:
    the seven sample counts around the work-item caps and one pair without samples.  Pair 1
    has the point solver's minimum of correspondences, pair 2 MD samples only, pair 3 point
    samples only, the others both types interleaved at random; pair 4's min_depth makes the
    min-depth filter drop MD models."""
    rng = np.random.default_rng(900 + variant)
    sizes = (300, KPT[variant], 40, 57, 211, 128, 300, 33)
    pairs, samples = [], []
    for k, (n, cnt) in enumerate(zip(sizes, COUNTS)):
        f = 500.0 + 40.0 * k
        K = np.array([[f, 0.0, 300.0 + 7.0 * k], [0.0, f, 230.0 + 5.0 * k], [0.0, 0.0, 1.0]])
        p = synthetic.make_pair(1000 + 10 * variant + k, n=n, K0=K, K1=K if variant == 1 else K * [[1.1], [1.1], [1.0]],
                                outlier_ratio=0.1 if k == 4 else 0.3)
        # pair 4: an offset must exceed half a median prior depth to pass the min-depth filter.
        # The true offsets lie within 0.3 median depths / scale, below 0.5 median priors (at
        # least 0.7 median depths / scale), so the models near the truth are dropped
        if k == 4:
            p["min_depth"] = np.array([-0.5 * np.median(p["depth0"]), -0.5 * np.median(p["depth1"])])
        pairs.append(p)
        if k == 2:
            types = np.zeros(cnt, dtype=np.int32)
        elif k == 3:
            types = np.ones(cnt, dtype=np.int32)
        elif k == 4:
            types = (np.arange(cnt) % 2).astype(np.int32)
        else:
            types = rng.integers(0, 2, cnt).astype(np.int32)
        idx = rng.integers(-9, 400, (cnt, 8)).astype(np.int32)  # (the unread slots hold anything)
        for s in range(cnt):
            ks = KPT[variant] if types[s] else KMD[variant]
            idx[s, :ks] = rng.choice(n, ks, replace=False)
        samples.append((types, idx))
    return pairs, samples


def _same(a, b):
    return all(ma.tobytes() == mb.tobytes() and np.array_equal(ca, cb) for (ma, ca), (mb, cb) in zip(a, b))


@pytest.fixture(scope="module")
def many(request):
    out = {}
    for variant in (0, 1, 2):
        pairs, samples = _many_pairs(variant)
        o, c = synthetic.example_options(KIND[variant])
        res, norm = madpose.hypothesize_batch(variant, pairs, samples, o, c)
        out[variant] = (pairs, samples, o, c, res, norm)
    return out


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_many_pairs_equal_each_pair_alone(variant, many):
    pairs, samples, o, c, res, norm = many[variant]
    slots = L.HYPOTHESIZE_SLOTS[variant]
    total = 0
    for k, (p, smp) in enumerate(zip(pairs, samples)):
        models, counts = res[k]
        assert models.shape == (COUNTS[k], slots, 17) and counts.shape == (COUNTS[k],)
        assert counts.dtype == np.int32 and np.all((counts >= 0) & (counts <= slots))
        for s in range(COUNTS[k]):
            assert not models[s, counts[s]:].any()
            assert np.all(np.isfinite(models[s, :counts[s]]))
        alone, norm1 = madpose.hypothesize_batch(variant, [p], [smp], o, c)
        assert _same([res[k]], alone), k
        assert norm1[0] == norm[k]
        total += int(counts.sum())
    assert total > 0
    assert res[7][0].shape == (0, slots, 17)
    # the min-depth filter drops MD models of pair 4; with the constraint off they are kept
    c_off = madpose.EstimatorConfig()
    c_off.min_depth_constraint = False
    off, _ = madpose.hypothesize_batch(variant, [pairs[4]], [samples[4]], o, c_off)
    md = samples[4][0] == 0
    assert res[4][1][md].sum() < off[0][1][md].sum()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_many_pairs_invariances(variant, many):
    pairs, samples, o, c, res, norm = many[variant]
    H = madpose.hypothesize_batch
    # a repeated call
    again, norm2 = H(variant, pairs, samples, o, c)
    assert _same(res, again) and np.array_equal(norm, norm2)
    # pair permutation
    perm = np.random.default_rng(5).permutation(len(pairs))
    got, normp = H(variant, [pairs[i] for i in perm], [samples[i] for i in perm], o, c)
    assert _same([res[i] for i in perm], got) and np.array_equal(norm[perm], normp)
    # sample permutation: the rows follow their samples
    rng = np.random.default_rng(6)
    sperm = [rng.permutation(len(t)) for t, _ in samples]
    got, _ = H(variant, pairs, [(t[q], i[q]) for (t, i), q in zip(samples, sperm)], o, c)
    assert _same([(m[q], n[q]) for (m, n), q in zip(res, sperm)], got)
    # chunk and sample_chunk
    for chunk in (1, 2, 0):
        for sample_chunk in (1, 7, 64, 0):
            if chunk == 0 and sample_chunk == 0:
                continue
            got, normc = H(variant, pairs, samples, o, c, chunk=chunk, sample_chunk=sample_chunk)
            assert _same(res, got), (chunk, sample_chunk)
            assert np.array_equal(norm, normc)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_chain_hypothesize_select_refine(variant, many):
    pairs, samples, o, c, res, _ = many[variant]
    cands = [np.ascontiguousarray(np.concatenate([m[s, :n[s]] for s in range(len(n))] + [np.zeros((0, 17))]))
             for m, n in res]
    assert sum(len(a) for a in cands) > 0
    by_array = madpose.select_batch(variant, pairs, cands, o, c, with_scores=True, with_counts=True)
    by_object = madpose.select_batch(variant, pairs, [madpose.poses_from_models(a, variant) for a in cands], o, c,
                                     with_scores=True, with_counts=True)
    winners, wpairs, wscores = [], [], []
    for k, (a, b) in enumerate(zip(by_array, by_object)):
        assert a.index == b.index and a.score == b.score
        assert np.array_equal(a.scores, b.scores) and np.array_equal(a.counts, b.counts)
        for t in range(3):
            assert np.array_equal(a.inlier_indices[t], b.inlier_indices[t])
        if a.index < 0:
            assert a.model is None and b.model is None
            continue
        assert type(a.model) is type(b.model)
        assert np.array_equal(a.model.R(), b.model.R()) and np.array_equal(a.model.t(), b.model.t())
        assert (a.model.scale, a.model.offset0, a.model.offset1) == (b.model.scale, b.model.offset0, b.model.offset1)
        winners.append(a.model)
        wpairs.append(pairs[k])
        wscores.append(a.score)
    assert len(winners) >= 1 and len(winners) < len(pairs)  # (pair 7 has no candidate, hence no winner)
    # a mixed call: arrays and object sequences side by side
    mixed = madpose.select_batch(variant, pairs[:2], [cands[0], madpose.poses_from_models(cands[1], variant)], o, c)
    assert [r.index for r in mixed] == [r.index for r in by_array[:2]]
    assert [r.score for r in mixed] == [r.score for r in by_array[:2]]
    refined = madpose.refine_batch(variant, wpairs, winners, o, c)
    for r, s in zip(refined, wscores):
        assert r.score_initial == s
