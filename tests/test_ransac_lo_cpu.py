"""mp_ransac_lo_set / mp_refine_relaxed_set / PairSet.ransac(lo=...) without a device: the
Python argument checks come before any library call; every bad argument of the C entries is
MP_EINVAL on a set whose device does not exist; the two-track bookkeeping
(madpose_amd/csrc/host/ransac_lo_track.h through mp_debug_ransac_lo_track) equals its Python
restatement on random round sequences with equal and NaN scores; and the header passes its
stand-alone check under AddressSanitizer and UBSan (tests/ransac_lo_check.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests.ransac_lo_walk import Track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
DBL_MAX = float(np.finfo(np.float64).max)


def test_symbols_and_header():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in ("mp_ransac_lo_set", "mp_refine_relaxed_set", "mp_debug_ransac_lo_track"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_ransac_result) == 80 and ctypes.sizeof(L.mp_refine_result) == 48
    assert ctypes.sizeof(L.mp_ransac_lo_info) == 16
    r = madpose.RansacResult()
    assert (r.lo_runs, r.lo_accepted, r.lo_index) == (0, 0, -1)
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "ransac_lo_track.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "__global__" not in text  # plain C++


def _fake_set():
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = 0, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = [20, 0, 7, 9, 9]
    ps._norm = np.ones(5)
    return ps


def test_python_checks_before_any_library_call(monkeypatch):
    ps = _fake_set()
    smp = (np.zeros(0, dtype=np.int32), np.zeros((0, 8), dtype=np.int32))

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    for lo in (0, -1, 65, 1.5, True, False, "2"):
        with pytest.raises(ValueError, match="lo must be"):
            ps.ransac(budget=8, step=4, lo=lo)
    with pytest.raises(ValueError, match="lo needs step"):
        ps.ransac(budget=8, lo=1)
    with pytest.raises(ValueError, match="lo needs step"):
        ps.ransac(samples=[smp] * 5, lo=1)
    with pytest.raises(ValueError, match="lo needs step"):
        ps.ransac(samples=[smp] * 5, step=4, lo=1)
    with pytest.raises(ValueError, match="lo needs step"):
        ps.ransac(budget=8, samples=[smp] * 5, step=4, lo=1)
    # the adaptive mode's own checks hold with lo
    with pytest.raises(ValueError, match="step"):
        ps.ransac(budget=8, step=0, lo=1)
    with pytest.raises(ValueError, match="2\\^20"):
        ps.ransac(budget=(1 << 20) + 1, step=4, lo=1)
    with pytest.raises(ValueError, match="2\\^22"):
        ps.ransac(budget=1 << 20, step=(1 << 22) // 5 + 1, lo=1)
    with pytest.raises(ValueError, match="rounds"):
        ps.ransac(budget=8, step=4, lo=1, rounds=65)
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 2 occurs twice"):
        ps.ransac(budget=8, step=4, lo=1, pair_ids=[2, 2])
    assert ps.ransac(budget=8, step=4, lo=64, pair_ids=[]) == []
    # refine(relax=...)
    for relax in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="relax"):
            ps.refine([None] * 5, relax=relax)
    with pytest.raises(ValueError, match="rounds"):
        ps.refine([None] * 5, rounds=0, relax=True)
    with pytest.raises(ValueError, match="one model per selected pair"):
        ps.refine([None] * 4, relax=True)
    assert ps.refine([], pair_ids=[], relax=True) == []


def _empty_set(variant=0, use_shift=True):
    o, c = synthetic.example_options("calibrated")
    c.use_shift = use_shift
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


def test_bad_arguments_are_einval_before_any_device():
    lib = L.lib()
    ps = _empty_set()
    h = ps._h
    mods, res = (L.mp_model * 2)(), (L.mp_ransac_result * 2)()
    stopped = (ctypes.c_int32 * 2)()
    info = (L.mp_ransac_lo_info * 2)()
    ok = lambda **kw: lib.mp_ransac_lo_set(*[kw.get(k, d) for k, d in (
        ("set", h), ("num_sel", 0), ("pair_ids", None), ("budget", 64), ("step", 16), ("seed", 0), ("share", -1),
        ("rounds", 3), ("lo", 1), ("models", mods), ("results", res), ("inl", None), ("stopped", stopped),
        ("info", info), ("sample_chunk", 0), ("model_chunk", 0))])
    assert ok() == L.MP_OK
    assert ok(stopped=None) == L.MP_OK and ok(rounds=0) == L.MP_OK and ok(budget=0) == L.MP_OK
    assert ok(lo=64) == L.MP_OK and ok(info=None) == L.MP_OK  # (no entry: no lo_info read)
    assert ok(budget=1 << 20, step=1 << 30) == L.MP_OK
    assert ok(set=None) == L.MP_EINVAL
    for lo in (0, -1, 65):
        assert ok(lo=lo) == L.MP_EINVAL and b"lo_rounds" in lib.mp_last_error()
    assert ok(num_sel=1, info=None) == L.MP_EINVAL and b"lo_info" in lib.mp_last_error()
    assert ok(step=0) == L.MP_EINVAL and b"step" in lib.mp_last_error()
    assert ok(budget=-1) == L.MP_EINVAL and b"budget" in lib.mp_last_error()
    assert ok(budget=(1 << 20) + 1) == L.MP_EINVAL and b"2^20" in lib.mp_last_error()
    assert ok(rounds=65) == L.MP_EINVAL and b"rounds" in lib.mp_last_error()
    assert ok(rounds=-1) == L.MP_EINVAL
    assert ok(share=257) == L.MP_EINVAL and ok(share=-2) == L.MP_EINVAL
    assert ok(sample_chunk=-1) == L.MP_EINVAL and ok(model_chunk=-1) == L.MP_EINVAL
    assert ok(num_sel=5, budget=1 << 20, step=(1 << 22) // 5 + 1) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    assert ok(num_sel=1) == L.MP_EINVAL  # (the selection, which an empty set refuses)
    # mp_refine_relaxed_set: mp_refine_set's checks
    rres = (L.mp_refine_result * 2)()
    assert lib.mp_refine_relaxed_set(h, 0, None, 1, mods, rres, None) == L.MP_OK
    assert lib.mp_refine_relaxed_set(None, 0, None, 1, mods, rres, None) == L.MP_EINVAL
    for rounds in (0, 65, -1):
        assert lib.mp_refine_relaxed_set(h, 0, None, rounds, mods, rres, None) == L.MP_EINVAL
        assert b"rounds" in lib.mp_last_error()
    assert lib.mp_refine_relaxed_set(h, 1, None, 1, mods, rres, None) == L.MP_EINVAL
    ps.close()


@pytest.mark.parametrize("variant,kw,word", [(3, {}, b"MP_SCALE_ONLY"), (0, dict(use_shift=False), b"use_shift")])
def test_unsupported_sets_are_einval(variant, kw, word):
    lib = L.lib()
    ps = _empty_set(variant, **kw)
    mods, res = (L.mp_model * 1)(), (L.mp_ransac_result * 1)()
    info = (L.mp_ransac_lo_info * 1)()
    assert lib.mp_ransac_lo_set(ps._h, 0, None, 8, 4, 0, -1, 1, 1, mods, res, None, None, info, 0, 0) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    with pytest.raises(ValueError, match="scale only|use_shift"):
        ps.ransac(budget=8, step=4, lo=1)
    ps.close()


def test_empty_set_needs_no_device():
    with _empty_set() as ps:
        assert ps.ransac(budget=8, step=3, lo=2) == []
        assert ps.refine([], relax=True) == []


def _lib_track(rounds):
    """mp_debug_ransac_lo_track over rounds of (min_score, min_counts, candidate, lo_accepted,
    lo_score, lo_counts)"""
    n = len(rounds)
    ms = np.array([r[0] for r in rounds] + [0.0], dtype=np.float64)
    mc = np.array([r[1] for r in rounds] + [(0, 0, 0)], dtype=np.int32).reshape(-1)
    cd = np.array([r[2] for r in rounds] + [0], dtype=np.int32)
    la = np.array([r[3] for r in rounds] + [0], dtype=np.int32)
    ls = np.array([r[4] for r in rounds] + [0.0], dtype=np.float64)
    lc = np.array([r[5] for r in rounds] + [(0, 0, 0)], dtype=np.int32).reshape(-1)
    score = ctypes.c_double(-1.0)
    out = np.full(7, -9, dtype=np.int32)
    p32, pd = (lambda a: a.ctypes.data_as(L.c_int32_p)), (lambda a: a.ctypes.data_as(L.c_double_p))
    assert L.lib().mp_debug_ransac_lo_track(n, pd(ms), p32(mc), p32(cd), p32(la), pd(ls), p32(lc),
                                            ctypes.byref(score), p32(out)) == L.MP_OK
    return score.value, out.tolist()


def test_track_equals_restatement():
    rng = np.random.default_rng(20260)
    assert _lib_track([]) == (DBL_MAX, [0, 0, 0, -1, 0, 0, 0])
    seen = {"minimal": 0, "lo": 0, "equal": 0, "nan": 0, "not_accepted": 0}
    for _ in range(400):
        rounds, T = [], Track()
        for _ in range(int(rng.integers(0, 10))):
            # scores on a small lattice: equal scores are common; one in eight is NaN
            sc = [float("nan") if rng.integers(0, 8) == 0 else float(rng.integers(0, 6)) for _ in range(2)]
            r = (sc[0], tuple(int(v) for v in rng.integers(0, 50, 3)), int(rng.integers(0, 1000)),
                 int(rng.integers(0, 3)), sc[1], tuple(int(v) for v in rng.integers(0, 50, 3)))
            seen["equal"] += (r[0] == T.score) + (r[4] == T.score)
            seen["nan"] += np.isnan(r[0]) + np.isnan(r[4])
            took = T.take_minimal(r[0], r[1])
            seen["minimal"] += took
            assert not (took and (np.isnan(r[0]) or not r[0] < DBL_MAX))
            before = T.score
            took = T.take_refined(r[2], r[3], r[4], r[5])
            seen["lo"] += took
            seen["not_accepted"] += r[3] == 0 and r[4] < before
            assert not (took and (r[3] < 1 or np.isnan(r[4]) or r[4] == before))
            rounds.append(r)
            # (every prefix: the library's walk of the rounds so far)
            assert _lib_track(rounds) == (T.score, list(T.counts) + [T.lo_index, T.lo_runs, T.lo_accepted, T.source])
        assert not np.isnan(T.score)
    assert all(v > 20 for v in seen.values()), seen


def test_track_bad_arguments():
    lib = L.lib()
    score, out = ctypes.c_double(), (ctypes.c_int32 * 7)()
    d, i = (ctypes.c_double * 3)(), (ctypes.c_int32 * 3)()
    assert lib.mp_debug_ransac_lo_track(0, None, None, None, None, None, None, ctypes.byref(score), out) == L.MP_OK
    assert lib.mp_debug_ransac_lo_track(-1, d, i, i, i, d, i, ctypes.byref(score), out) == L.MP_EINVAL
    assert lib.mp_debug_ransac_lo_track(1, None, i, i, i, d, i, ctypes.byref(score), out) == L.MP_EINVAL
    assert lib.mp_debug_ransac_lo_track(1, d, i, i, i, d, i, None, out) == L.MP_EINVAL
    assert lib.mp_debug_ransac_lo_track(1, d, i, i, i, d, i, ctypes.byref(score), None) == L.MP_EINVAL


def test_track_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of ransac_lo_track.h needs ROCm's clang")
    exe = str(tmp_path / "ransac_lo_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "ransac_lo_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
