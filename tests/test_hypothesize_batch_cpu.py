"""hypothesize_batch / mp_hypothesize_batch without a device: the symbol and its constants,
the C entry rejects every bad argument with MP_EINVAL before any device call (no kernel may
see an index the host has not range-checked), empty batches return MP_OK, the Python wrapper
makes its checks before any library call, select_batch takes array candidates, and the slab
and work-item planning (madpose_amd/csrc/host/hypothesis_plan.h) passes its stand-alone
check under AddressSanitizer and UBSan (tests/hypothesis_plan_check.cpp)."""
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
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL / MP_OK


def _args(variant=0, sizes=(9, 8), samples=((0, 1), (1, 0, 0)), chunk=0, sample_chunk=0):
    """A well-formed argument list of mp_hypothesize_batch as a dict (arrays kept alive in it):
    sample k of a pair reads the indices k, k + 1, ... (distinct and in range)."""
    o, c = synthetic.example_options("calibrated")
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    soffs = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    n, S = int(offs[-1]), int(soffs[-1])
    ncam = 9 if variant in (0, 3) else 2
    types = np.array([t for s in samples for t in s] or [0], dtype=np.int32)
    idx = np.full((max(S, 1), 8), -7, dtype=np.int32)  # (unused slots hold garbage: they are ignored)
    ksz = (3 if variant in (0, 3) else 4, (5, 6, 7, 5)[variant] if 0 <= variant <= 3 else 5)
    for s in range(S):
        k = ksz[types[s]]
        idx[s, :k] = np.arange(k) + (s % 2)
    slots = L.HYPOTHESIZE_SLOTS[variant] if 0 <= variant <= 2 else 16
    return dict(variant=variant, num_pairs=len(sizes), offsets=offs, x0=np.zeros(2 * n), x1=np.zeros(2 * n),
                d0=np.ones(n), d1=np.ones(n), min_depth=np.zeros(2 * len(sizes)),
                cam0=np.tile(np.eye(3).ravel()[:ncam], len(sizes)), cam1=np.tile(np.eye(3).ravel()[:ncam], len(sizes)),
                options=o._to_c(), config=c._to_c(), sample_offsets=soffs, types=types, idx=idx,
                models=np.zeros((max(S, 1), slots, 17)), counts=np.zeros(max(S, 1), dtype=np.int32),
                norm=np.zeros(len(sizes)), chunk=chunk, sample_chunk=sample_chunk)


def _call(a, device=NO_DEVICE):
    dp = lambda v: None if v is None else v.ctypes.data_as(L.c_double_p)
    ip = lambda v, t: None if v is None else v.ctypes.data_as(t)
    return L.lib().mp_hypothesize_batch(
        a["variant"], a["num_pairs"], ip(a["offsets"], L.c_int64_p), dp(a["x0"]), dp(a["x1"]), dp(a["d0"]),
        dp(a["d1"]), dp(a["min_depth"]), dp(a["cam0"]), dp(a["cam1"]),
        None if a["options"] is None else ctypes.byref(a["options"]),
        None if a["config"] is None else ctypes.byref(a["config"]), ip(a["sample_offsets"], L.c_int64_p),
        ip(a["types"], L.c_int32_p), ip(a["idx"], L.c_int32_p), ip(a["models"], ctypes.POINTER(L.mp_model)),
        ip(a["counts"], L.c_int32_p), dp(a["norm"]), a["chunk"], a["sample_chunk"], device)


def _reaches_device(a):
    """the arguments passed every check: the call got as far as asking for the device, which
    is absent (MP_EDEVICE) or has no such index (the one MP_EINVAL that names the device)"""
    code = _call(a)
    msg = L.lib().mp_last_error()
    return code in (L.MP_EDEVICE, L.MP_EINVAL) and b"device" in msg.lower()


def _einval(a):
    """refused by a check of the arguments, not by the missing device"""
    code = _call(a)
    msg = L.lib().mp_last_error()
    return code == L.MP_EINVAL and msg and b"device" not in msg.lower()


def test_symbol_and_constants():
    assert hasattr(L.lib(), "mp_hypothesize_batch")
    assert hasattr(L.lib(), "mp_debug_hypothesize_timing")
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    slab, = re.findall(r"^#define MP_HYPOTHESIZE_SLAB_SAMPLES (\d+)", header, re.M)
    slots = [int(re.findall(rf"^#define MP_HYPOTHESIZE_SLOTS_{n} (\d+)", header, re.M)[0])
             for n in ("CALIBRATED", "SHARED_FOCAL", "TWO_FOCAL")]
    assert int(slab) == L.HYPOTHESIZE_SLAB_SAMPLES == 32768
    assert tuple(slots) == tuple(L.HYPOTHESIZE_SLOTS) == (10, 16, 4)
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "hypothesis_plan.h")) as f:
        plan = f.read()
    assert f"kHypSlabSamples = {L.HYPOTHESIZE_SLAB_SAMPLES};" in plan
    assert "kHypSamplesMax = int64_t(1) << 22;" in plan and L.HYPOTHESIZE_MAX_SAMPLES == 1 << 22
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "include", "mp_types.h")) as f:
        types = f.read()
    for name, val in zip(("Cal", "SF", "TF"), L.HYPOTHESIZE_SLOTS):
        assert re.search(rf"kMaxModels{name} = {val};", types)
    assert L.HYPOTHESIZE_SAMPLE_STRIDE == 8


def test_well_formed_arguments_pass_the_checks():
    """the fixture itself is valid: with it the call gets as far as the device (absent here,
    or index out of range), so every MP_EINVAL below is the change's doing"""
    for variant in (0, 1, 2):
        a = _args(variant=variant)
        assert _reaches_device(a), L.lib().mp_last_error()


def _idx(a, s, slot, val):
    a["idx"][s, slot] = val
    return a


@pytest.mark.parametrize("change", [
    dict(num_pairs=-1),
    dict(variant=3),      # MP_SCALE_ONLY: not supported
    dict(variant=4),
    dict(variant=-1),
    dict(chunk=-1),
    dict(sample_chunk=-1),
    dict(offsets=None),
    dict(sample_offsets=None),
    dict(x0=None),
    dict(x1=None),
    dict(d0=None),
    dict(d1=None),
    dict(min_depth=None),
    dict(cam0=None),
    dict(cam1=None),
    dict(options=None),
    dict(types=None),
    dict(idx=None),
    dict(models=None),
    dict(counts=None),
    dict(offsets=np.array([0, 9, 8], dtype=np.int64)),           # decreasing
    dict(offsets=np.array([-1, 9, 17], dtype=np.int64)),         # negative
    dict(sample_offsets=np.array([0, 3, 2], dtype=np.int64)),    # decreasing
    dict(sample_offsets=np.array([-2, 0, 3], dtype=np.int64)),   # negative
    dict(sample_offsets=np.array([0, 2, (1 << 22) + 1], dtype=np.int64)),  # more than 2^22 samples
    dict(types=np.array([0, 1, 2, 0, 0], dtype=np.int32)),       # type 2
    dict(types=np.array([0, -1, 1, 0, 0], dtype=np.int32)),
])
def test_bad_arguments_are_einval(change):
    a = _args()
    a.update(change)
    assert _einval(a), L.lib().mp_last_error()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_bad_indices_are_einval(variant):
    ksz = (3 if variant == 0 else 4, (5, 6, 7)[variant])
    # sample 0 is of type 0 on pair 0 (9 correspondences), sample 1 of type 1 on pair 0
    for s, t in ((0, 0), (1, 1)):
        k = ksz[t]
        for slot in (0, k - 1):
            assert _einval(_idx(_args(variant=variant), s, slot, 9))      # equal to n_p
            assert b"outside" in L.lib().mp_last_error()
            assert _einval(_idx(_args(variant=variant), s, slot, -1))     # negative
            assert _einval(_idx(_args(variant=variant), s, slot, 1 << 30))
        a = _args(variant=variant)
        a["idx"][s, k - 1] = a["idx"][s, 0]                                            # repeated
        assert _call(a) == L.MP_EINVAL
        assert b"repeated" in L.lib().mp_last_error()
        # the slots past the solver's sample size are not read: anything may stand there
        a = _args(variant=variant)
        a["idx"][s, k:] = -5
        a["idx"][s, 7] = a["idx"][s, 0]
        assert _reaches_device(a), L.lib().mp_last_error()
    # the second pair's samples are checked against its own size (8), not the first's (9)
    a = _args(variant=variant)
    a["idx"][2, 0] = 8
    assert _call(a) == L.MP_EINVAL
    # a pair too small for the solver of a sample on it
    a = _args(variant=variant, sizes=(9, ksz[1] - 1))
    assert _call(a) == L.MP_EINVAL
    assert b"too few" in L.lib().mp_last_error()
    a = _args(variant=variant, sizes=(ksz[0] - 1, 8), samples=((0,), (1,)))
    assert _call(a) == L.MP_EINVAL


def test_unsupported_configurations_are_einval():
    for variant in (0, 1, 2):
        a = _args(variant=variant)
        a["options"].use_ours = 1
        assert _call(a) == L.MP_EINVAL and b"use_ours" in L.lib().mp_last_error()
        a = _args(variant=variant)
        a["options"].use_4p4d = 1
        assert _call(a) == L.MP_EINVAL and b"use_4p4d" in L.lib().mp_last_error()
        a = _args(variant=variant)
        a["config"].use_shift = 0
        assert _call(a) == L.MP_EINVAL and b"use_shift" in L.lib().mp_last_error()
    a = _args(variant=3)
    assert _call(a) == L.MP_EINVAL and b"MP_SCALE_ONLY" in L.lib().mp_last_error()
    a = _args()
    a["options"].squared_inlier_thresholds[0] = 0.0
    assert _call(a) == L.MP_EINVAL


def test_empty_batches_are_ok_without_a_device():
    keys = ("offsets", "sample_offsets", "x0", "x1", "d0", "d1", "min_depth", "cam0", "cam1", "types", "idx",
            "models", "counts", "norm")
    for variant in (0, 1, 2):
        a = _args(variant=variant)
        a["num_pairs"] = 0
        for k in keys:
            a[k] = None
        assert _call(a) == L.MP_OK
        # pairs, but not one sample: the arguments are checked, the device is not touched; the
        # sample arrays and outputs may be null, the normalisation scales are still given
        a = _args(variant=variant, samples=((), ()))
        for k in ("types", "idx", "models", "counts", "config"):
            a[k] = None
        a["norm"][:] = -1.0
        assert _call(a) == L.MP_OK, L.lib().mp_last_error()
        assert np.all(a["norm"] > 0) and (variant != 0 or np.all(a["norm"] == 1.0))
        a["norm"] = None
        assert _call(a) == L.MP_OK
        a = _args(variant=variant, samples=((), ()))
        a["offsets"] = np.array([0, 9, 8], dtype=np.int64)
        assert _call(a) == L.MP_EINVAL
        a = _args(variant=variant, samples=((), ()))
        a["cam0"] = None
        assert _call(a) == L.MP_EINVAL


def test_timing_hook_needs_an_output():
    assert L.lib().mp_debug_hypothesize_timing(None) == L.MP_EINVAL
    out = np.full(5, -1.0)
    assert L.lib().mp_debug_hypothesize_timing(out.ctypes.data_as(L.c_double_p)) == L.MP_OK
    assert np.all(out >= 0)


def _smp(types, rows):
    idx = np.zeros((len(types), 8), dtype=np.int32)
    for k, r in enumerate(rows):
        idx[k, :len(r)] = r
    return np.asarray(types, dtype=np.int32), idx


def test_python_wrapper_checks_before_any_library_call(monkeypatch):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    p = synthetic.make_pair(1, n=20)
    o, c = synthetic.example_options("calibrated")
    good = _smp([0, 1], [[0, 1, 2], [3, 4, 5, 6, 7]])
    H = madpose.hypothesize_batch
    with pytest.raises(ValueError, match=r"one \(types, idx\) per pair"):
        H(0, [p, p], [good], o, c)
    for bad in (3, 7, -1):
        with pytest.raises(ValueError, match="variant"):
            H(bad, [p], [good], o, c)
    for bad in (-1, 1.5, "2", None):
        with pytest.raises(ValueError, match="chunk must"):
            H(0, [p], [good], o, c, chunk=bad)
        with pytest.raises(ValueError, match="sample_chunk must"):
            H(0, [p], [good], o, c, sample_chunk=bad)
    with pytest.raises(ValueError, match="int32"):
        H(0, [p], [(good[0].astype(np.int64), good[1])], o, c)
    with pytest.raises(ValueError, match="int32"):
        H(0, [p], [(good[0], good[1].astype(np.int64))], o, c)
    with pytest.raises(ValueError, match="shape"):
        H(0, [p], [(good[0], good[1][:, :7])], o, c)
    with pytest.raises(ValueError, match="shape"):
        H(0, [p], [(good[0][:1], good[1])], o, c)
    with pytest.raises(ValueError, match="type must be 0"):
        H(0, [p], [_smp([0, 2], [[0, 1, 2], [3, 4, 5, 6, 7]])], o, c)
    with pytest.raises(ValueError, match="outside"):
        H(0, [p], [_smp([0], [[0, 1, 20]])], o, c)                       # equal to n_p
    with pytest.raises(ValueError, match="outside"):
        H(0, [p], [_smp([1], [[0, 1, 2, 3, -1]])], o, c)                 # negative
    with pytest.raises(ValueError, match="repeats"):
        H(0, [p], [_smp([1], [[0, 1, 2, 3, 1]])], o, c)
    with pytest.raises(ValueError, match="repeats"):
        H(1, [p], [_smp([0], [[5, 1, 2, 5]])], o, c)
    small = synthetic.make_pair(2, n=4)
    with pytest.raises(ValueError, match="too few"):
        H(0, [small], [_smp([1], [[0, 1, 2, 3, 3]])], o, c)
    c2 = madpose.EstimatorConfig()
    c2.use_shift = False
    with pytest.raises(ValueError, match="use_shift"):
        H(0, [p], [good], o, c2)
    o2, _ = synthetic.example_options("calibrated")
    o2.use_ours = True
    with pytest.raises(ValueError, match="use_ours"):
        H(0, [p], [good], o2, c)
    # the slots a solver does not read are not checked
    res, norm = H(0, [], [], o, c)
    assert res == [] and norm.shape == (0,)
    # select_batch's array candidates: shape and type are checked before any library call
    for bad in (np.zeros((2, 16)), np.zeros(17), np.zeros((2, 17), dtype=np.float32)):
        with pytest.raises(ValueError, match="array candidates"):
            madpose.select_batch(0, [p], [bad], o, c)


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of hypothesis_plan.h needs ROCm's clang")
    exe = str(tmp_path / "hypothesis_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "hypothesis_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
