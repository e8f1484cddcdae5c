"""mp_ransac_adaptive_set / PairSet.ransac(step=...) without a device: the termination rule
(mp_debug_ransac_required, madpose_amd/csrc/host/ransac_stop.h) equals a Python restatement
through the same libm (math.pow / log / ceil are the C library's); every bad argument of the
new entry is MP_EINVAL on a set whose device does not exist; the Python checks come before
any library call; and ransac_stop.h with the planning form that takes a first sample passes
its stand-alone check under AddressSanitizer and UBSan (tests/ransac_stop_check.cpp)."""
import ctypes
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_stop_restatement as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL


def _lib_required(variant, n, counts, opts):
    c = (ctypes.c_int32 * 3)(*counts)
    req = (ctypes.c_uint32 * 2)()
    assert L.lib().mp_debug_ransac_required(variant, n, c, ctypes.byref(opts), req) == L.MP_OK
    return [int(req[0]), int(req[1])]


def _c_options(sp, mn, mx):
    o, _ = synthetic.example_options("calibrated")
    o.success_probability, o.min_num_iterations, o.max_num_iterations_per_solver = sp, mn, mx
    return o._to_c()


def test_symbols_and_header():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in ("mp_ransac_adaptive_set", "mp_debug_ransac_required", "mp_debug_select_argmin"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_ransac_result) == 80
    assert madpose.RansacResult().stopped is False
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "ransac_stop.h")) as f:
        stop = f.read()
    assert "#include <hip" not in stop and "__global__" not in stop  # plain C++


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_required_equals_restatement(variant):
    checked = big = 0
    for sp, mn, mx in itertools.product((0.5, 0.99, 0.999999, 1.0), (0, 8, 100), (50, 10000)):
        opts = _c_options(sp, mn, mx)
        for n in (0, 1, 5, 64, 700):
            lattice = sorted({0, 1, 2, n // 4, n // 2, (4 * n) // 5, n - 1, n} & set(range(n + 1)))
            for counts in itertools.product(lattice, repeat=3):
                want = S.required(variant, n, counts, sp, mn, mx)
                assert _lib_required(variant, n, counts, opts) == want, (sp, mn, mx, n, counts)
                assert all(min(mn, mx) <= w <= max(mn, mx) for w in want)
                checked += 1
    assert checked > 1000
    # Tiny ratios on the point solver must come out as the bound, not as a converted integer:
    # 2 / 700 (on five points `it` is about 2.4e13; on six and seven p_bad is already past
    # 0.99999999999999), and every q / 700 whose `it` is above 2^32 with p_bad below that
    # threshold, so that the clamp in double is what decides
    for mx in (50, 10000):
        opts = _c_options(0.99, 8, mx)
        assert _lib_required(variant, 700, (700, 700, 2), opts)[1] == mx
        for q in range(1, 40):
            p_bad = 1.0 - math.pow(q / 700, float(S.K_PT[variant]))
            if p_bad < 0.99999999999999 and math.log(0.01) / math.log(p_bad) + 0.5 > 2.0 ** 32:
                assert _lib_required(variant, 700, (700, 700, q), opts)[1] == mx, q
                big += 1
    assert big >= 2
    # the issue's example: 80 % inliers on the 5-point solver
    if variant == 0:
        assert _lib_required(0, 300, (240, 240, 240), _c_options(0.99, 8, 10000))[1] == 13


def test_required_bad_arguments():
    lib = L.lib()
    opts = _c_options(0.99, 8, 10000)
    c = (ctypes.c_int32 * 3)(1, 1, 1)
    req = (ctypes.c_uint32 * 2)()
    assert lib.mp_debug_ransac_required(3, 10, c, ctypes.byref(opts), req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required(-1, 10, c, ctypes.byref(opts), req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required(0, -1, c, ctypes.byref(opts), req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required(0, 10, None, ctypes.byref(opts), req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required(0, 10, c, None, req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required(0, 10, c, ctypes.byref(opts), None) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required(0, 0, c, ctypes.byref(opts), req) == L.MP_EINVAL  # counts above n
    c[0] = -1
    assert lib.mp_debug_ransac_required(0, 10, c, ctypes.byref(opts), req) == L.MP_EINVAL


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
    ok = lambda **kw: lib.mp_ransac_adaptive_set(*[kw.get(k, d) for k, d in (
        ("set", h), ("num_sel", 0), ("pair_ids", None), ("budget", 64), ("step", 16), ("seed", 0), ("share", -1),
        ("rounds", 3), ("models", mods), ("results", res), ("inl", None), ("stopped", stopped), ("sample_chunk", 0),
        ("model_chunk", 0))])
    assert ok() == L.MP_OK
    assert ok(stopped=None) == L.MP_OK and ok(rounds=0) == L.MP_OK and ok(budget=0) == L.MP_OK
    assert ok(budget=1 << 20, step=1 << 30) == L.MP_OK
    assert ok(set=None) == L.MP_EINVAL
    assert ok(step=0) == L.MP_EINVAL and b"step" in lib.mp_last_error()
    assert ok(step=-3) == L.MP_EINVAL
    assert ok(budget=-1) == L.MP_EINVAL and b"budget" in lib.mp_last_error()
    assert ok(budget=(1 << 20) + 1) == L.MP_EINVAL and b"2^20" in lib.mp_last_error()
    assert ok(rounds=65) == L.MP_EINVAL and b"rounds" in lib.mp_last_error()
    assert ok(rounds=-1) == L.MP_EINVAL
    assert ok(share=257) == L.MP_EINVAL and ok(share=-2) == L.MP_EINVAL
    assert ok(sample_chunk=-1) == L.MP_EINVAL and ok(model_chunk=-1) == L.MP_EINVAL
    # a round obeys the bound a call obeys: num_sel x min(step, budget) <= 2^22
    assert ok(num_sel=5, budget=1 << 20, step=1 << 20) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    assert ok(num_sel=5, budget=(1 << 22) // 5 + 1, step=1 << 20) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    assert ok(num_sel=5, budget=1 << 20, step=(1 << 22) // 5 + 1) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    # (within the bound the call goes on to the selection, which an empty set refuses)
    assert ok(num_sel=5, budget=1 << 20, step=(1 << 22) // 5) == L.MP_EINVAL and b"2^22" not in lib.mp_last_error()
    assert ok(num_sel=1) == L.MP_EINVAL
    ps.close()


@pytest.mark.parametrize("variant,kw,word", [(3, {}, b"MP_SCALE_ONLY"), (0, dict(use_shift=False), b"use_shift")])
def test_unsupported_sets_are_einval(variant, kw, word):
    lib = L.lib()
    ps = _empty_set(variant, **kw)
    mods, res = (L.mp_model * 1)(), (L.mp_ransac_result * 1)()
    assert lib.mp_ransac_adaptive_set(ps._h, 0, None, 8, 4, 0, -1, 1, mods, res, None, None, 0, 0) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    with pytest.raises(ValueError, match="scale only|use_shift"):
        ps.ransac(budget=8, step=4)
    ps.close()


def test_python_checks_before_any_library_call(monkeypatch):
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = 0, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = [20, 0, 7, 9, 9]
    ps._norm = np.ones(5)
    smp = (np.zeros(0, dtype=np.int32), np.zeros((0, 8), dtype=np.int32))

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    for step in (0, -1, 1.5, True, "4"):
        with pytest.raises(ValueError, match="step"):
            ps.ransac(budget=8, step=step)
    with pytest.raises(ValueError, match="step needs a budget"):
        ps.ransac(step=4)
    with pytest.raises(ValueError, match="step needs a budget"):
        ps.ransac(samples=[smp] * 5, step=4)
    with pytest.raises(ValueError, match="step needs a budget"):
        ps.ransac(budget=8, samples=[smp] * 5, step=4)
    with pytest.raises(ValueError, match="budget"):
        ps.ransac(budget=-1, step=4)
    with pytest.raises(ValueError, match="2\\^20"):
        ps.ransac(budget=(1 << 20) + 1, step=4)
    with pytest.raises(ValueError, match="2\\^22"):
        ps.ransac(budget=1 << 20, step=(1 << 22) // 5 + 1)
    with pytest.raises(ValueError, match="rounds"):
        ps.ransac(budget=8, step=4, rounds=65)
    with pytest.raises(ValueError, match="point_share"):
        ps.ransac(budget=8, step=4, point_share=257)
    with pytest.raises(ValueError, match="seed"):
        ps.ransac(budget=8, step=4, seed=-1)
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 2 occurs twice"):
        ps.ransac(budget=8, step=4, pair_ids=[2, 2])
    assert ps.ransac(budget=8, step=4, pair_ids=[]) == []


def test_empty_set_needs_no_device():
    with _empty_set() as ps:
        assert ps.ransac(budget=8, step=3) == []


def test_stop_rule_and_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of ransac_stop.h needs ROCm's clang")
    exe = str(tmp_path / "ransac_stop_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "ransac_stop_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
