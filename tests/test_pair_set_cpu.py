"""PairSet / mp_pair_set_* without a device: the symbols and constants are there and agree
with madpose_amd/_lib.py, mp_pair_set_create refuses every bad argument with MP_EINVAL
before any array but offsets is read and before the device is touched, an empty set needs
no device, the Python class rejects a wrong model, candidate or sample count before any
library call, and the preparation items and the selection check
(madpose_amd/csrc/host/pair_set_plan.h) pass their stand-alone check under AddressSanitizer
and UBSan (tests/pair_set_plan_check.cpp)."""
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
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
SYMBOLS = ("mp_pair_set_create", "mp_pair_set_destroy", "mp_pair_set_info", "mp_pair_set_norm_scales",
           "mp_refine_set", "mp_select_set", "mp_hypothesize_set", "mp_debug_pair_set_prep",
           "mp_debug_pair_set_rows")


def _args(variant=0, sizes=(4, 3)):
    """A well-formed argument list of mp_pair_set_create as a dict (arrays kept alive in it)."""
    o, c = synthetic.example_options("calibrated")
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    ncam = 9 if variant in (0, 3) else 2
    return dict(variant=variant, num_pairs=len(sizes), offsets=offs, x0=np.zeros(2 * n), x1=np.zeros(2 * n),
                d0=np.ones(n), d1=np.ones(n), min_depth=np.zeros(2 * len(sizes)),
                cam0=np.tile(np.eye(3).ravel()[:ncam], len(sizes)), cam1=np.tile(np.eye(3).ravel()[:ncam], len(sizes)),
                options=o._to_c(), config=c._to_c(), out=ctypes.c_void_p(12345))


def _create(a, device=NO_DEVICE):
    dp = lambda v: None if v is None else v.ctypes.data_as(L.c_double_p)
    return L.lib().mp_pair_set_create(
        a["variant"], a["num_pairs"], None if a["offsets"] is None else a["offsets"].ctypes.data_as(L.c_int64_p),
        dp(a["x0"]), dp(a["x1"]), dp(a["d0"]), dp(a["d1"]), dp(a["min_depth"]), dp(a["cam0"]), dp(a["cam1"]),
        None if a["options"] is None else ctypes.byref(a["options"]),
        None if a["config"] is None else ctypes.byref(a["config"]), device,
        None if a["out"] is None else ctypes.byref(a["out"]))


def test_symbols_and_constants():
    lib = L.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTS, name
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert f"int {name}(" in header, name
    line, = [ln for ln in header.splitlines() if ln.startswith("#define MP_PAIR_SET_MAX_CORRESPONDENCES")]
    assert int(line.split()[2]) == 1 << 26
    assert "typedef struct mp_pair_set mp_pair_set;" in header
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "pair_set_plan.h")) as f:
        plan = f.read()
    assert "kPairSetMaxCorr = int64_t(1) << 26;" in plan
    assert "kPrepItemMax = 256;" in plan
    # 120 bytes resident per correspondence: 12 doubles and two buffers of 3 ints
    assert 12 * 8 + 2 * 3 * 4 == 120
    assert madpose.PairSet is not None


@pytest.mark.parametrize("change", [
    dict(num_pairs=-1),
    dict(variant=4),
    dict(variant=-1),
    dict(offsets=None),
    dict(x0=None),
    dict(x1=None),
    dict(d0=None),
    dict(d1=None),
    dict(min_depth=None),
    dict(cam0=None),
    dict(cam1=None),
    dict(options=None),
    dict(out=None),
    dict(offsets=np.array([0, 4, 3], dtype=np.int64)),             # decreasing
    dict(offsets=np.array([-1, 4, 7], dtype=np.int64)),            # negative
    dict(offsets=np.array([0, 4, 5 + (1 << 28)], dtype=np.int64)),  # a pair above kRefinePairMax
])
def test_bad_create_arguments_are_einval(change):
    a = _args()
    a.update(change)
    assert _create(a) == L.MP_EINVAL
    assert L.lib().mp_last_error()
    if a["out"] is not None:
        assert a["out"].value is None  # (no handle on failure)


def test_too_many_correspondences_is_einval_before_any_read():
    """offsets that claim 2^26 + 1 correspondences over one-element arrays: an entry that read
    the arrays, or reached the device, would fault or return MP_EDEVICE"""
    per = 1 << 24
    sizes = [per] * 4 + [1]
    a = _args(sizes=(1,))
    a["num_pairs"] = len(sizes)
    a["offsets"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert int(a["offsets"][-1]) == (1 << 26) + 1
    a["min_depth"] = np.zeros(2 * len(sizes))
    a["cam0"] = np.tile(np.eye(3).ravel(), len(sizes))
    a["cam1"] = np.tile(np.eye(3).ravel(), len(sizes))
    for k in ("x0", "x1", "d0", "d1"):
        a[k] = np.zeros(1)
    assert _create(a) == L.MP_EINVAL
    assert b"2^26" in L.lib().mp_last_error()
    # exactly the bound passes this check: the call then gets as far as the device
    a["offsets"][-1] -= 1
    for k in ("x0", "x1", "d0", "d1"):
        a[k] = None  # (... which it must not reach with null arrays either)
    assert _create(a) == L.MP_EINVAL
    assert b"null input array" in L.lib().mp_last_error()


def test_bad_options_are_einval():
    a = _args()
    a["options"].squared_inlier_thresholds[0] = 0.0
    assert _create(a) == L.MP_EINVAL
    a = _args()
    a["options"].squared_inlier_thresholds[1] = -1.0
    assert _create(a) == L.MP_EINVAL


def test_well_formed_arguments_reach_the_device():
    """the counterpart of the tests above: nothing but the device is wrong here"""
    a = _args()
    assert _create(a) in (L.MP_EDEVICE, L.MP_EINVAL)  # (EINVAL: "device index out of range")
    assert b"device" in L.lib().mp_last_error().lower()
    a["config"] = None  # (a null config means the defaults)
    assert _create(a) != L.MP_OK


def test_destroy_null_and_prep_switch():
    lib = L.lib()
    assert lib.mp_pair_set_destroy(None) == L.MP_OK
    assert lib.mp_debug_pair_set_prep(2) == L.MP_EINVAL
    assert lib.mp_debug_pair_set_prep(-1) == L.MP_EINVAL
    try:
        assert lib.mp_debug_pair_set_prep(1) == L.MP_OK
    finally:
        assert lib.mp_debug_pair_set_prep(0) == L.MP_OK
    for fn, args in ((lib.mp_pair_set_info, (None, None, None, None, None, None)),
                     (lib.mp_pair_set_norm_scales, (None, None)),
                     (lib.mp_refine_set, (None, 0, None, 1, None, None, None)),
                     (lib.mp_select_set, (None, 0, None, None, None, None, None, None, None, 0)),
                     (lib.mp_hypothesize_set, (None, 0, None, None, None, None, None, None, 0)),
                     (lib.mp_debug_pair_set_rows, (None, 0, None))):
        assert fn(*args) == L.MP_EINVAL


def test_empty_set_needs_no_device():
    lib = L.lib()
    a = _args(sizes=())
    for k in ("offsets", "x0", "x1", "d0", "d1", "min_depth", "cam0", "cam1"):
        a[k] = None
    assert _create(a) == L.MP_OK
    h = a["out"]
    assert h.value
    v, p, dev = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    nc, nb = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.mp_pair_set_info(h, ctypes.byref(v), ctypes.byref(p), ctypes.byref(nc), ctypes.byref(nb),
                                ctypes.byref(dev)) == L.MP_OK
    assert (v.value, p.value, nc.value, nb.value, dev.value) == (0, 0, 0, 0, NO_DEVICE)
    assert lib.mp_refine_set(h, 0, None, 1, None, None, None) == L.MP_OK
    assert lib.mp_select_set(h, 0, None, None, None, None, None, None, None, 0) == L.MP_OK
    assert lib.mp_hypothesize_set(h, 0, None, None, None, None, None, None, 0) == L.MP_OK
    assert lib.mp_refine_set(h, 1, None, 1, None, None, None) == L.MP_EINVAL  # (num_sel != the pair count)
    assert lib.mp_refine_set(h, 0, None, 0, None, None, None) == L.MP_EINVAL  # (rounds)
    assert lib.mp_debug_pair_set_rows(h, 0, None) == L.MP_EINVAL
    assert lib.mp_pair_set_destroy(h) == L.MP_OK
    assert lib.mp_pair_set_destroy(h) == L.MP_EINVAL  # (no longer a live set: refused, not freed twice)
    # the Python class on no pairs
    o, c = synthetic.example_options("calibrated")
    with madpose.PairSet(0, [], o, c, device=NO_DEVICE) as ps:
        assert len(ps) == 0 and ps.num_correspondences == 0 and ps.resident_bytes == 0
        assert ps.norm_scale.shape == (0,)
        assert ps.refine([]) == [] and ps.select([]) == []
        hyp, norm = ps.hypothesize([])
        assert hyp == [] and norm.shape == (0,)
        with pytest.raises(ValueError, match="outside the set"):
            ps.refine([], pair_ids=[0])
    ps.close()
    with pytest.raises(ValueError, match="closed"):
        len(ps)


def test_python_class_checks_before_any_library_call(monkeypatch):
    o, c = synthetic.example_options("calibrated")
    p = synthetic.make_pair(1, n=20)
    m = madpose.PoseScaleOffset(p["R"], p["t"], 1.0, 0.0, 0.0)
    smp = (np.zeros(0, dtype=np.int32), np.zeros((0, 8), dtype=np.int32))
    # a set object as creation leaves it, without the library: three pairs of 20, 0 and 7
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = 0, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = [20, 0, 7]
    ps._norm = np.ones(3)

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    with pytest.raises(ValueError, match="one model per selected pair"):
        ps.refine([m, m])
    with pytest.raises(ValueError, match="one model per selected pair"):
        ps.refine([m, m, m], pair_ids=[0, 2])
    with pytest.raises(ValueError, match="one candidate list per selected pair"):
        ps.select([[m]])
    with pytest.raises(ValueError, match="one candidate list per selected pair"):
        ps.select([[m], [m]], pair_ids=[1])
    with pytest.raises(ValueError, match=r"one \(types, idx\) per selected pair"):
        ps.hypothesize([smp])
    with pytest.raises(ValueError, match=r"one \(types, idx\) per selected pair"):
        ps.hypothesize([smp, smp, smp], pair_ids=[2, 0])
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 2 occurs twice"):
        ps.refine([m, m], pair_ids=[2, 2])
    with pytest.raises(ValueError, match=r"pair_ids\[0\] = 3 is outside"):
        ps.select([[m]], pair_ids=[3])
    with pytest.raises(ValueError, match=r"pair_ids\[0\] = -1 is outside"):
        ps.refine([m], pair_ids=[-1])
    with pytest.raises(ValueError, match="rounds"):
        ps.refine([m, m, m], rounds=0)
    with pytest.raises(ValueError, match="model_chunk"):
        ps.select([[m], [], []], model_chunk=-1)
    with pytest.raises(ValueError, match="sample_chunk"):
        ps.hypothesize([smp, smp, smp], sample_chunk=-1)
    # a sample on a pair too small for its solver, by the selected pair's size (pair 1 is empty)
    one = (np.ones(1, dtype=np.int32), np.arange(8, dtype=np.int32)[None])
    with pytest.raises(ValueError, match="too few"):
        ps.hypothesize([one], pair_ids=[1])
    # an empty selection is answered without the library
    assert ps.refine([], pair_ids=[]) == [] and ps.select([], pair_ids=[]) == []
    hyp, norm = ps.hypothesize([], pair_ids=[])
    assert hyp == [] and norm.shape == (0,)
    # a set that cannot hypothesize says so
    ps._hyp_error = "hypothesize does not support scale only (variant 3)"
    with pytest.raises(ValueError, match="scale only"):
        ps.hypothesize([smp, smp, smp])
    # closed: every method raises, close() stays fine
    ps._h = None
    for call in (lambda: ps.refine([m, m, m]), lambda: ps.select([[], [], []]), lambda: ps.hypothesize([smp] * 3),
                 lambda: len(ps), lambda: ps.norm_scale, lambda: ps.num_correspondences, lambda: ps.resident_bytes,
                 lambda: ps.__enter__()):
        with pytest.raises(ValueError, match="closed"):
            call()
    ps.close()
    ps.close()
    # creation: a bad variant before anything else
    with pytest.raises(ValueError, match="variant"):
        madpose.PairSet(7, [p], o, c)


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of pair_set_plan.h needs ROCm's clang")
    exe = str(tmp_path / "pair_set_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "pair_set_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
