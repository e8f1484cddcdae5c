"""The batched minimal solvers (madpose.solve_scale_and_shift_batch,
solve_scale_shift_pose_batch, relpose_batch) against their yardsticks, bit for bit: every
row of a batch is what the single-sample entry returns for that sample, and for the
default MD solvers also the oracle's result (tests/test_md_exact_cpu.py _oracle,
oracle_poses).  Whole buffers are compared: the slots past a sample's count are zero.
Sample counts sit at the edges of the lane groups (2, 4 and 16 lanes per sample, 64 per
wave), not at workload size."""
import ctypes

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from tests import pt_samples
from tests.test_md_exact_cpu import _oracle, oracle_poses, wide_range_sample

pytestmark = pytest.mark.gpu

W = [4, 5, 6]
K_MD = [3, 4, 4]
K_PT = [5, 6, 7]
EDGES = [1, 3, 4, 5, 15, 16, 17, 33, 65]


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    if madpose.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _same(a, b):
    """bitwise equality of two float64 / int arrays (NaN payloads and zero signs included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _md_random(seed, n, k):
    """the generator of test_device_md_random_bit_exact"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x = np.c_[rng.standard_normal((k, 2)), np.ones(k)]
        y = np.c_[rng.standard_normal((k, 2)), np.ones(k)]
        out.append((x, y, rng.uniform(0.5, 5, k), rng.uniform(0.5, 5, k)))
    return out


def _md_wide(seed, n, k):
    rng = np.random.default_rng(seed)
    return [wide_range_sample(rng, k) for _ in range(n)]


def _md_scene(variant, n):
    """consistent scenes, the generator of tests/test_alt_solvers_gpu.py: the samples on
    which the single-sample alternates (and the default solvers) return models"""
    rng = np.random.default_rng(5 + variant)
    k = K_MD[variant]
    out = []
    for trial in range(n):
        R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        R = R * np.linalg.det(R)
        t = rng.standard_normal(3) * 0.5
        X = np.c_[rng.uniform(-1, 1, (4, 2)), rng.uniform(2, 6, 4)]
        Y = X @ R.T + t
        f0, f1 = rng.uniform(0.5, 3, 2)
        if variant == 0:
            x, y = X / X[:, 2:], Y / np.abs(Y[:, 2:])
        else:
            fy = f0 if variant == 1 else f1
            x = np.c_[f0 * X[:, :2] / X[:, 2:], np.ones(4)]
            y = np.c_[fy * Y[:, :2] / Y[:, 2:], np.ones(4)]
        dx = X[:, 2] + rng.normal(0, 0.0 if trial % 2 == 0 else 1e-2, 4)
        out.append((x[:k].copy(), y[:k].copy(), dx[:k].copy(), Y[:k, 2].copy()))
    return out


def _stack(samples):
    return tuple(np.ascontiguousarray(np.stack([s[i] for s in samples])) for i in range(4))


_MD_CACHE = {}


def _md_batch(variant):
    """601 samples (300 random, 301 wide-range), stacked; computed once per variant"""
    if variant not in _MD_CACHE:
        k = K_MD[variant]
        smp = _md_random(60 + variant, 300, k) + _md_wide(70 + variant, 301, k)
        arrs = _stack(smp)
        for a in arrs:
            a.setflags(write=False)
        _MD_CACHE[variant] = (smp, arrs)
    return _MD_CACHE[variant]


_PT_CACHE = {}


def _pt_samples(kind, which="random", n=65):
    """point samples in the batch layout: unit bearings for kind 0, normalized points else"""
    key = (kind, which, n)
    if key not in _PT_CACHE:
        rng = np.random.default_rng(900 + 10 * kind + ["random", "outlier", "wide"].index(which))
        p0, p1 = getattr(pt_samples, which + "_samples")(rng, n, K_PT[kind])
        if kind == 0:
            p0, p1 = pt_samples.bearings(p0), pt_samples.bearings(p1)
        p0, p1 = np.ascontiguousarray(p0), np.ascontiguousarray(p1)
        p0.setflags(write=False)
        p1.setflags(write=False)
        _PT_CACHE[key] = (p0, p1)
    return _PT_CACHE[key]


_dp = ctypes.POINTER(ctypes.c_double)


def _single_md_poses(variant, alt, x, y, dx, dy):
    """mp_solve_scale_shift_pose{,_alt}'s models of one sample as rows of 17 doubles"""
    c = [np.ascontiguousarray(t, dtype=np.float64) for t in (x, y, dx, dy)]
    out = (L.mp_model * 8)()
    if alt:
        n = L.lib().mp_solve_scale_shift_pose_alt(variant, alt, *[t.ctypes.data_as(_dp) for t in c], out, 8, 0)
    else:
        n = L.lib().mp_solve_scale_shift_pose(variant, *[t.ctypes.data_as(_dp) for t in c], out, 8, 0)
    assert n >= 0, n
    return np.frombuffer(bytes(out), dtype=np.float64).reshape(8, 17)[:min(n, 8)].copy()


def _single_md_sols(variant, x, y, dx, dy):
    c = [np.ascontiguousarray(t, dtype=np.float64) for t in (x, y, dx, dy)]
    out = np.zeros(8 * W[variant])
    n = L.lib().mp_solve_scale_and_shift(variant, *[t.ctypes.data_as(_dp) for t in c], out.ctypes.data_as(_dp), 8, 0)
    assert n >= 0, n
    return out.reshape(8, W[variant])[:min(n, 8)].copy()


def _single_pt(kind, a, b):
    fn = [L.lib().mp_relpose_5pt, L.lib().mp_relpose_6pt_shared_focal, L.lib().mp_relpose_7pt_two_focal][kind]
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = (L.mp_model * 16)()
    n = fn(a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), out, 16, 0)
    assert n >= 0, n
    return np.frombuffer(bytes(out), dtype=np.float64).reshape(16, 17)[:min(n, 16)].copy()


_ALTS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
_POSE = {(0, 0): madpose.solve_scale_shift_pose, (1, 0): madpose.solve_scale_shift_pose_shared_focal,
         (2, 0): madpose.solve_scale_shift_pose_two_focal}
_PT = [madpose.relpose_5pt, madpose.relpose_6pt_shared_focal, madpose.relpose_7pt_two_focal]


def _expect(rows_per_sample, slots, width):
    """padded (B, slots, width) buffer and counts from per-sample row arrays"""
    B = len(rows_per_sample)
    buf, cnt = np.zeros((B, slots, width)), np.zeros(B, dtype=np.int32)
    for b, r in enumerate(rows_per_sample):
        r = np.asarray(r, dtype=np.float64).reshape(-1, width)
        cnt[b] = min(len(r), slots)
        buf[b, :cnt[b]] = r[:slots]
    return buf, cnt


# 1 -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_md_batch_equals_oracle(variant):
    smp, (x, y, dx, dy) = _md_batch(variant)
    assert len(smp) == 601
    sols, ns = madpose.solve_scale_and_shift_batch(variant, x, y, dx, dy)
    models, nm = madpose.solve_scale_shift_pose_batch(variant, x, y, dx, dy)
    es, ens = _expect([_oracle(variant, *s) for s in smp], 8, W[variant])
    em, enm = _expect([oracle_poses(variant, *s) for s in smp], 8, 17)
    assert np.array_equal(ns, ens) and np.array_equal(nm, enm)
    assert ns.sum() > 200 and nm.sum() > 0  # (solutions and models were found and compared)
    assert _same(sols, es)  # zero-filled slots included
    assert _same(models, em)


# 2 -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_md_group_edge_sizes(variant):
    _, arrs = _md_batch(variant)
    full_s = madpose.solve_scale_and_shift_batch(variant, *[a[:65] for a in arrs])
    full_m = madpose.solve_scale_shift_pose_batch(variant, *[a[:65] for a in arrs])
    for B in EDGES:
        s = madpose.solve_scale_and_shift_batch(variant, *[a[:B] for a in arrs])
        m = madpose.solve_scale_shift_pose_batch(variant, *[a[:B] for a in arrs])
        assert _same(s[0], full_s[0][:B]) and _same(s[1], full_s[1][:B]), B
        assert _same(m[0], full_m[0][:B]) and _same(m[1], full_m[1][:B]), B


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_point_group_edge_sizes(kind):
    p0, p1 = _pt_samples(kind)
    full = madpose.relpose_batch(kind, p0, p1)
    assert full[1].sum() > 0
    for B in EDGES:
        m = madpose.relpose_batch(kind, p0[:B], p1[:B])
        assert _same(m[0], full[0][:B]) and _same(m[1], full[1][:B]), B


# 3 -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,alt", _ALTS)
def test_md_batch_equals_single(variant, alt):
    # the first 48 samples of the MD batch, then 48 consistent scenes (on which every
    # solver, the 4p4d included, returns models)
    smp = _md_batch(variant)[0][:48] + _md_scene(variant, 48)
    sub = _stack(smp)
    models, nm = madpose.solve_scale_shift_pose_batch(variant, *sub, alt=alt)
    em, enm = _expect([_single_md_poses(variant, alt, *s) for s in smp], 8, 17)
    assert np.array_equal(nm, enm), (nm, enm)
    assert nm[48:].sum() > 0  # (models were found and compared)
    assert _same(models, em)
    if alt == 0:
        sols, ns = madpose.solve_scale_and_shift_batch(variant, *sub)
        es, ens = _expect([_single_md_sols(variant, *s) for s in smp], 8, W[variant])
        assert np.array_equal(ns, ens), (ns, ens)
        assert _same(sols, es)


@pytest.mark.parametrize("which", ["random", "outlier", "wide"])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_point_batch_equals_single(kind, which):
    p0, p1 = _pt_samples(kind, which, 48)
    models, n = madpose.relpose_batch(kind, p0, p1)
    em, en = _expect([_single_pt(kind, p0[s], p1[s]) for s in range(48)], 16, 17)
    assert np.array_equal(n, en), (n, en)
    assert _same(models, em)


# 4 -----------------------------------------------------------------------------
def test_permutation():
    perm = np.random.default_rng(4).permutation(257)
    _, arrs = _md_batch(1)
    sub = [a[:257] for a in arrs]
    a = madpose.solve_scale_shift_pose_batch(1, *sub)
    b = madpose.solve_scale_shift_pose_batch(1, *[t[perm] for t in sub])
    assert _same(b[0], a[0][perm]) and _same(b[1], a[1][perm])
    a = madpose.solve_scale_and_shift_batch(1, *sub)
    b = madpose.solve_scale_and_shift_batch(1, *[t[perm] for t in sub])
    assert _same(b[0], a[0][perm]) and _same(b[1], a[1][perm])
    for kind in (0, 1):
        p0, p1 = _pt_samples(kind, "random", 257)
        a = madpose.relpose_batch(kind, p0, p1)
        b = madpose.relpose_batch(kind, p0[perm], p1[perm])
        assert _same(b[0], a[0][perm]) and _same(b[1], a[1][perm]), kind


# 5 -----------------------------------------------------------------------------
def test_chunking():
    for variant in (0, 1):
        _, arrs = _md_batch(variant)
        sub = [a[:200] for a in arrs]
        for fn in (madpose.solve_scale_and_shift_batch, madpose.solve_scale_shift_pose_batch):
            a, b = fn(variant, *sub), fn(variant, *sub, chunk=64)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), (variant, fn.__name__)
    p0, p1 = _pt_samples(1, "random", 257)
    a, b = madpose.relpose_batch(1, p0[:200], p1[:200]), madpose.relpose_batch(1, p0[:200], p1[:200], chunk=64)
    assert _same(a[0], b[0]) and _same(a[1], b[1])


def test_default_chunk_crossing():
    _, arrs = _md_batch(0)
    B = L.SOLVE_BATCH_CHUNK + 3
    idx = np.arange(B) % 601
    big = [a[idx] for a in arrs]
    for fn in (madpose.solve_scale_and_shift_batch, madpose.solve_scale_shift_pose_batch):
        a = fn(0, *big)
        b = fn(0, *[t[-8:] for t in big])
        assert _same(a[0][-8:], b[0]) and _same(a[1][-8:], b[1]), fn.__name__
        assert a[1][-8:].sum() > 0


# 6 -----------------------------------------------------------------------------
def test_6pt_past_1024_samples():
    p0, p1 = _pt_samples(1, "random", 48)
    idx = np.arange(1025) % 48
    a = madpose.relpose_batch(1, p0[idx], p1[idx])
    b = madpose.relpose_batch(1, p0, p1)
    assert b[1].sum() > 0
    assert _same(a[0][:48], b[0]) and _same(a[1][:48], b[1])


# 7 -----------------------------------------------------------------------------
def test_poses_from_models():
    def same_pose(p, q):
        for f in ("pose", "scale", "offset0", "offset1", "focal", "focal0", "focal1"):
            assert hasattr(p, f) == hasattr(q, f), f
            if hasattr(p, f):
                assert np.array_equal(np.asarray(getattr(p, f)), np.asarray(getattr(q, f))), f
        assert type(p) is type(q)

    seen = 0
    for variant in (0, 1, 2):
        smp, arrs = _md_batch(variant)
        models, n = madpose.solve_scale_shift_pose_batch(variant, *[a[:16] for a in arrs])
        for b in range(16):
            got = madpose.poses_from_models(models[b, :n[b]], variant)
            ref = _POSE[(variant, 0)](smp[b][0].T, smp[b][1].T, smp[b][2], smp[b][3])
            assert len(got) == len(ref)
            for p, q in zip(got, ref):
                same_pose(p, q)
                seen += 1
    for kind in (0, 1, 2):
        p0, p1 = _pt_samples(kind)
        models, n = madpose.relpose_batch(kind, p0[:16], p1[:16])
        for b in range(16):
            got = madpose.poses_from_models(models[b, :n[b]], kind)
            ref = _PT[kind](p0[b], p1[b])
            assert len(got) == len(ref)
            for p, q in zip(got, ref):
                same_pose(p, q)
                seen += 1
    assert seen > 50
