"""select_batch / mp_select_batch without a device: the C entry rejects bad arguments with
MP_EINVAL before any device call, an empty batch returns MP_OK, the Python wrapper makes
its checks before any library call, and the slab and work-item planning
(madpose_amd/csrc/host/select_plan.h) passes its stand-alone check under AddressSanitizer
and UBSan (tests/select_plan_check.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


def _args(variant=0, num_pairs=2, sizes=(4, 3), cands=(2, 3), chunk=0, model_chunk=0):
    """A well-formed argument list of mp_select_batch as a dict (arrays kept alive in it)."""
    o, c = synthetic.example_options("calibrated")
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    moffs = np.concatenate([[0], np.cumsum(cands)]).astype(np.int64)
    n, m = int(offs[-1]), int(moffs[-1])
    ncam = 9 if variant in (0, 3) else 2
    return dict(variant=variant, num_pairs=num_pairs, offsets=offs, x0=np.zeros(2 * n), x1=np.zeros(2 * n),
                d0=np.ones(n), d1=np.ones(n), cam0=np.tile(np.eye(3).ravel()[:ncam], len(sizes)),
                cam1=np.tile(np.eye(3).ravel()[:ncam], len(sizes)), options=o._to_c(), config=c._to_c(),
                model_offsets=moffs, models=(L.mp_model * max(m, 1))(), scores=np.zeros(max(m, 1)),
                counts=np.zeros(3 * max(m, 1), dtype=np.int32), results=(L.mp_select_result * len(sizes))(),
                idx=np.zeros(3 * max(n, 1), dtype=np.int32), chunk=chunk, model_chunk=model_chunk)


def _call(a, device=0):
    dp = lambda v: None if v is None else v.ctypes.data_as(L.c_double_p)
    ip = lambda v, t: None if v is None else v.ctypes.data_as(t)
    return L.lib().mp_select_batch(
        a["variant"], a["num_pairs"], ip(a["offsets"], L.c_int64_p), dp(a["x0"]), dp(a["x1"]), dp(a["d0"]),
        dp(a["d1"]), dp(a["cam0"]), dp(a["cam1"]), None if a["options"] is None else ctypes.byref(a["options"]),
        None if a["config"] is None else ctypes.byref(a["config"]), ip(a["model_offsets"], L.c_int64_p), a["models"],
        dp(a["scores"]), ip(a["counts"], L.c_int32_p), a["results"], ip(a["idx"], L.c_int32_p), a["chunk"],
        a["model_chunk"], device)


def test_symbol_struct_layout_and_constants():
    assert hasattr(L.lib(), "mp_select_batch")
    assert ctypes.sizeof(L.mp_select_result) == 32
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    slab, = re.findall(r"^#define MP_SELECT_SLAB_MODELS (\d+)", header, re.M)
    tile, = re.findall(r"^#define MP_SELECT_TILE (\d+)", header, re.M)
    assert int(slab) == L.SELECT_SLAB_MODELS == 65536
    assert int(tile) == L.SELECT_TILE and L.SELECT_TILE in (1, 2, 4, 8)
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "select_plan.h")) as f:
        plan = f.read()
    assert "kSelectSlabModels = int64_t(1) << 16;" in plan
    assert f"kSelectTile = {L.SELECT_TILE};" in plan


@pytest.mark.parametrize("change", [
    dict(num_pairs=-1),
    dict(variant=4),
    dict(variant=-1),
    dict(chunk=-1),
    dict(model_chunk=-1),
    dict(offsets=None),
    dict(model_offsets=None),
    dict(x0=None),
    dict(x1=None),
    dict(d0=None),
    dict(d1=None),
    dict(cam0=None),
    dict(cam1=None),
    dict(options=None),
    dict(models=None),
    dict(results=None),
    dict(offsets=np.array([0, 4, 3], dtype=np.int64)),          # decreasing
    dict(offsets=np.array([-1, 4, 7], dtype=np.int64)),         # negative
    dict(model_offsets=np.array([0, 3, 2], dtype=np.int64)),    # decreasing
    dict(model_offsets=np.array([-2, 0, 3], dtype=np.int64)),   # negative
    dict(model_offsets=np.array([0, 5, (1 << 28) + 1], dtype=np.int64)),  # more than 2^28 candidates
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
        for k in ("offsets", "model_offsets", "x0", "x1", "d0", "d1", "cam0", "cam1", "models", "scores", "counts",
                  "results", "idx"):
            a[k] = None
        assert _call(a, device=10 ** 6) == L.MP_OK
    # a null config means the defaults, the per-candidate outputs and the inlier buffer are
    # optional, and models may be null when no pair has a candidate: with pairs, the call
    # gets as far as the device (absent here, or index out of range) -- not EINVAL
    a = _args(cands=(0, 0))
    for k in ("config", "scores", "counts", "idx", "models"):
        a[k] = None
    assert _call(a, device=10 ** 6) != L.MP_OK
    assert _call(a, device=10 ** 6) in (L.MP_EDEVICE, L.MP_EINVAL)
    assert b"null" not in L.lib().mp_last_error()


def test_tile_hook_accepts_only_the_tiles():
    lib = L.lib()
    assert lib.mp_debug_select_tile(0) == 0  # the default was in force
    try:
        assert lib.mp_debug_select_tile(4) == 0
        assert lib.mp_debug_select_tile(8) == 4
        for bad in (-1, 3, 5, 16):
            assert lib.mp_debug_select_tile(bad) == -1
        assert lib.mp_debug_select_tile(0) == 8  # (a refused value changed nothing)
    finally:
        lib.mp_debug_select_tile(0)


def test_python_wrapper_checks_before_any_library_call(monkeypatch):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    p = synthetic.make_pair(1, n=20)
    o, c = synthetic.example_options("calibrated")
    m = madpose.PoseScaleOffset(p["R"], p["t"], 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="one candidate list per pair"):
        madpose.select_batch(0, [p, p], [[m]], o, c)
    with pytest.raises(ValueError, match="one candidate list per pair"):
        madpose.select_batch(0, [], [[m]], o, c)
    with pytest.raises(ValueError, match="variant"):
        madpose.select_batch(7, [p], [[m]], o, c)
    for bad in (-1, 1.5, "2", None):
        with pytest.raises(ValueError, match="chunk must"):
            madpose.select_batch(0, [p], [[m]], o, c, chunk=bad)
        with pytest.raises(ValueError, match="model_chunk must"):
            madpose.select_batch(0, [p], [[m]], o, c, model_chunk=bad)
    assert madpose.select_batch(0, [], [], o, c) == []


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of select_plan.h needs ROCm's clang")
    exe = str(tmp_path / "select_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "select_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
