"""The batched minimal solvers without a device: argument errors are ValueError before any
library call, an empty batch returns empty arrays of the right shapes, the C entries
reject bad arguments with MP_EINVAL, and the host packing
(madpose_amd/csrc/host/solve_batch_pack.h) passes its stand-alone check under
AddressSanitizer and UBSan (tests/solve_batch_pack_check.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


def _md(B, k):
    return np.zeros((B, k, 3)), np.zeros((B, k, 3)), np.ones((B, k)), np.ones((B, k))


@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test: the errors below are raised before one"""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)


@pytest.mark.parametrize("fn", [madpose.solve_scale_and_shift_batch, madpose.solve_scale_shift_pose_batch])
def test_md_argument_errors(no_library, fn):
    x, y, dx, dy = _md(4, 4)
    with pytest.raises(ValueError):
        fn(1, x, y[:3], dx, dy)  # mismatched B
    with pytest.raises(ValueError):
        fn(1, x, y, dx[:2], dy)
    with pytest.raises(ValueError):
        fn(0, x, y, dx, dy)  # K = 4 arrays for the calibrated solver
    with pytest.raises(ValueError):
        fn(1, x, y[:, :3], dx, dy)  # mismatched K
    with pytest.raises(ValueError):
        fn(1, x, y, dx, dy[:, :3])
    with pytest.raises(ValueError):
        fn(1, x[:, :, :2], y, dx, dy)  # wrong trailing dimension
    with pytest.raises(ValueError):
        fn(1, x, y, dx[..., None], dy)
    with pytest.raises(ValueError):
        fn(3, x, y, dx, dy)  # variant 3
    with pytest.raises(ValueError):
        fn(1, x, y, dx, dy, chunk=-1)
    big = [np.broadcast_to(a[:1], (L.SOLVE_BATCH_MAX + 1,) + a.shape[1:]) for a in (x, y, dx, dy)]
    with pytest.raises(ValueError):
        fn(1, *big)  # B above 2^22 (zero-stride views: nothing is allocated)


def test_alt_errors(no_library):
    for v, k in ((0, 3), (1, 4)):
        with pytest.raises(ValueError):
            madpose.solve_scale_shift_pose_batch(v, *_md(2, k), alt=2)
    with pytest.raises(ValueError):
        madpose.solve_scale_shift_pose_batch(2, *_md(2, 4), alt=3)


def test_relpose_argument_errors(no_library):
    a5, a6 = np.zeros((4, 5, 3)), np.zeros((4, 6, 2))
    with pytest.raises(ValueError):
        madpose.relpose_batch(3, a6, a6)  # kind 3
    with pytest.raises(ValueError):
        madpose.relpose_batch(1, a6, a6[:3])  # mismatched B
    with pytest.raises(ValueError):
        madpose.relpose_batch(2, a6, a6)  # K = 6 arrays for the 7pt solver
    with pytest.raises(ValueError):
        madpose.relpose_batch(0, a5[:, :, :2], a5)  # wrong trailing dimension
    with pytest.raises(ValueError):
        madpose.relpose_batch(1, a5, a5)
    with pytest.raises(ValueError):
        madpose.relpose_batch(1, a6, a6, chunk=-1)
    big = np.broadcast_to(a6[:1], (L.SOLVE_BATCH_MAX + 1, 6, 2))
    with pytest.raises(ValueError):
        madpose.relpose_batch(1, big, big)


def test_poses_from_models_errors(no_library):
    with pytest.raises(ValueError):
        madpose.poses_from_models(np.zeros((2, 16)), 0)
    with pytest.raises(ValueError):
        madpose.poses_from_models(np.zeros((2, 17)), 3)
    assert madpose.poses_from_models(np.zeros((0, 17)), 1) == []
    row = np.arange(17.0)
    p, = madpose.poses_from_models(row[None], 2)
    assert np.array_equal(np.asarray(p.pose)[:, :3].ravel(), row[:9]) and np.array_equal(np.asarray(p.pose)[:, 3], row[9:12])
    assert (p.scale, p.offset0, p.offset1, p.focal0, p.focal1) == (12.0, 13.0, 14.0, 15.0, 16.0)
    q, = madpose.poses_from_models(row[None], 1)
    assert q.focal == 15.0 and type(q).__name__ == "PoseScaleOffsetSharedFocal"
    assert type(madpose.poses_from_models(row[None], 0)[0]).__name__ == "PoseScaleOffset"


def test_empty_batches(no_library):
    for v, k, w in ((0, 3, 4), (1, 4, 5), (2, 4, 6)):
        sols, n = madpose.solve_scale_and_shift_batch(v, *_md(0, k))
        assert sols.shape == (0, 8, w) and sols.dtype == np.float64 and n.shape == (0,) and n.dtype == np.int32
        models, n = madpose.solve_scale_shift_pose_batch(v, *_md(0, k))
        assert models.shape == (0, 8, 17) and models.dtype == np.float64 and n.shape == (0,)
    for kind, tail in ((0, (5, 3)), (1, (6, 2)), (2, (7, 2))):
        models, n = madpose.relpose_batch(kind, np.zeros((0,) + tail), np.zeros((0,) + tail))
        assert models.shape == (0, 16, 17) and n.shape == (0,) and n.dtype == np.int32


def test_c_entries_reject_bad_arguments():
    """MP_EINVAL from the C ABI itself, before any device is opened (ns alone, null data)"""
    lib = L.lib()
    nul_d, nul_i, nul_m = L.c_double_p(), L.c_int32_p(), ctypes.POINTER(L.mp_model)()
    big = L.SOLVE_BATCH_MAX + 1
    assert lib.mp_solve_scale_and_shift_batch(0, big, nul_d, nul_d, nul_d, nul_d, nul_d, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_and_shift_batch(0, -1, nul_d, nul_d, nul_d, nul_d, nul_d, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_and_shift_batch(0, 4, nul_d, nul_d, nul_d, nul_d, nul_d, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_and_shift_batch(3, 0, nul_d, nul_d, nul_d, nul_d, nul_d, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_and_shift_batch(0, 0, nul_d, nul_d, nul_d, nul_d, nul_d, nul_i, -1, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_shift_pose_batch(1, 2, 4, nul_d, nul_d, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_shift_pose_batch(2, 0, big, nul_d, nul_d, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_solve_scale_shift_pose_batch(2, 0, 4, nul_d, nul_d, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_relpose_batch(3, 0, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_relpose_batch(1, big, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_relpose_batch(1, 4, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_EINVAL
    assert lib.mp_relpose_batch(1, 4, nul_d, nul_d, nul_m, nul_i, -1, 0) == L.MP_EINVAL
    # an empty batch is fine, without a device
    for v in (0, 1, 2):
        assert lib.mp_solve_scale_and_shift_batch(v, 0, nul_d, nul_d, nul_d, nul_d, nul_d, nul_i, 0, 0) == L.MP_OK
        assert lib.mp_solve_scale_shift_pose_batch(v, 0, 0, nul_d, nul_d, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_OK
        assert lib.mp_relpose_batch(v, 0, nul_d, nul_d, nul_m, nul_i, 0, 0) == L.MP_OK
    assert L.SOLVE_BATCH_CHUNK <= 65536


def test_default_chunk_matches_header():
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        line, = [ln for ln in f if ln.startswith("#define MP_SOLVE_BATCH_CHUNK")]
    assert int(line.split()[2]) == L.SOLVE_BATCH_CHUNK
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "solve_batch_pack.h")) as f:
        src = f.read()
    assert f"kSolveBatchChunk = {L.SOLVE_BATCH_CHUNK};" in src


def test_host_packing_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of solve_batch_pack.h needs ROCm's clang")
    exe = str(tmp_path / "solve_batch_pack_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "solve_batch_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
