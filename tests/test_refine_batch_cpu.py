"""refine_batch / mp_refine_batch without a device: the C entry rejects bad arguments
with MP_EINVAL before any device call, an empty batch returns MP_OK, the Python wrapper
rejects a model count that differs from the pair count before any library call, and the
chunk planning and packed layout (madpose_amd/csrc/host/refine_plan.h) pass their
stand-alone check under AddressSanitizer and UBSan (tests/refine_plan_check.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


def _args(variant=0, num_pairs=2, rounds=1, chunk=0, sizes=(4, 3)):
    """A well-formed argument list of mp_refine_batch as a dict (arrays kept alive in it)."""
    o, c = synthetic.example_options("calibrated")
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    ncam = 9 if variant in (0, 3) else 2
    a = dict(variant=variant, num_pairs=num_pairs, offsets=offs, x0=np.zeros(2 * n), x1=np.zeros(2 * n),
             d0=np.ones(n), d1=np.ones(n), min_depth=np.zeros(2 * len(sizes)),
             cam0=np.tile(np.eye(3).ravel()[:ncam], len(sizes)), cam1=np.tile(np.eye(3).ravel()[:ncam], len(sizes)),
             options=o._to_c(), config=c._to_c(), rounds=rounds, models=(L.mp_model * len(sizes))(),
             results=(L.mp_refine_result * len(sizes))(), idx=np.zeros(3 * n, dtype=np.int32), chunk=chunk)
    return a


def _call(a, device=0):
    dp = lambda v: None if v is None else v.ctypes.data_as(L.c_double_p)
    return L.lib().mp_refine_batch(
        a["variant"], a["num_pairs"], None if a["offsets"] is None else a["offsets"].ctypes.data_as(L.c_int64_p),
        dp(a["x0"]), dp(a["x1"]), dp(a["d0"]), dp(a["d1"]), dp(a["min_depth"]), dp(a["cam0"]), dp(a["cam1"]),
        None if a["options"] is None else ctypes.byref(a["options"]),
        None if a["config"] is None else ctypes.byref(a["config"]), a["rounds"], a["models"], a["results"],
        None if a["idx"] is None else a["idx"].ctypes.data_as(L.c_int32_p), a["chunk"], device)


def test_symbol_and_struct_layout():
    assert hasattr(L.lib(), "mp_refine_batch")
    assert ctypes.sizeof(L.mp_refine_result) == 3 * 8 + 6 * 4
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        line, = [ln for ln in f if ln.startswith("#define MP_REFINE_RUN_CORRESPONDENCES")]
    assert int(line.split()[2]) == L.REFINE_RUN_CORRESPONDENCES
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "refine_plan.h")) as f:
        assert "kRefineRunCorr = int64_t(1) << 22;" in f.read()
    assert L.REFINE_RUN_CORRESPONDENCES == 1 << 22


@pytest.mark.parametrize("change", [
    dict(num_pairs=-1),
    dict(variant=4),
    dict(variant=-1),
    dict(rounds=0),
    dict(rounds=65),
    dict(rounds=-3),
    dict(chunk=-1),
    dict(offsets=None),
    dict(x0=None),
    dict(x1=None),
    dict(d0=None),
    dict(d1=None),
    dict(min_depth=None),
    dict(cam0=None),
    dict(cam1=None),
    dict(options=None),
    dict(models=None),
    dict(results=None),
    dict(offsets=np.array([0, 4, 3], dtype=np.int64)),   # decreasing
    dict(offsets=np.array([-1, 4, 7], dtype=np.int64)),  # a negative count of values before the first pair
])
def test_bad_arguments_are_einval(change):
    """every one of these is refused before the device is touched: device 10**6 does not
    exist, so a call that reached it would return MP_EDEVICE (or find no device here)"""
    a = _args()
    a.update(change)
    assert _call(a, device=10 ** 6) == L.MP_EINVAL
    assert L.lib().mp_last_error()


def test_bad_options_are_einval():
    a = _args()
    a["options"].squared_inlier_thresholds[0] = 0.0
    assert _call(a, device=10 ** 6) == L.MP_EINVAL
    a = _args()
    a["options"].squared_inlier_thresholds[1] = -1.0
    assert _call(a, device=10 ** 6) == L.MP_EINVAL


def test_empty_batch_is_ok_without_a_device():
    for variant in (0, 1, 2, 3):
        a = _args(variant=variant, num_pairs=0)
        for k in ("offsets", "x0", "x1", "d0", "d1", "min_depth", "cam0", "cam1", "models", "results", "idx"):
            a[k] = None
        assert _call(a, device=10 ** 6) == L.MP_OK
    # a null config means the defaults and the inlier buffer is optional: with pairs, the
    # call gets as far as the device (absent here, or index out of range) -- not EINVAL
    a = _args()
    a["config"] = None
    a["idx"] = None
    assert _call(a, device=10 ** 6) != L.MP_OK
    assert _call(a, device=10 ** 6) in (L.MP_EDEVICE, L.MP_EINVAL)


def test_python_wrapper_checks_before_any_library_call(monkeypatch):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    p = synthetic.make_pair(1, n=20)
    o, c = synthetic.example_options("calibrated")
    m = madpose.PoseScaleOffset(p["R"], p["t"], 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="one model per pair"):
        madpose.refine_batch(0, [p, p], [m], o, c)
    with pytest.raises(ValueError, match="one model per pair"):
        madpose.refine_batch(0, [], [m], o, c)
    with pytest.raises(ValueError, match="rounds"):
        madpose.refine_batch(0, [p], [m], o, c, rounds=0)
    with pytest.raises(ValueError, match="rounds"):
        madpose.refine_batch(0, [p], [m], o, c, rounds=65)
    with pytest.raises(ValueError, match="chunk"):
        madpose.refine_batch(0, [p], [m], o, c, chunk=-1)
    with pytest.raises(ValueError, match="variant"):
        madpose.refine_batch(7, [p], [m], o, c)
    assert madpose.refine_batch(0, [], [], o, c) == []


def test_plan_and_layout_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of refine_plan.h needs ROCm's clang")
    exe = str(tmp_path / "refine_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "refine_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
