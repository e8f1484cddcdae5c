"""PairSet.ransac's device outputs without a device: the header, the symbol and the ctypes layout;
the output stage's plan (madpose_amd/csrc/host/residuals_plan.h) under AddressSanitizer and UBSan
in its stand-alone check (tests/ransac_out_plan_check.cpp); every Python refusal before any library
call; and mp_ransac_out_set's own refusals on a set whose device does not exist."""
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
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL / MP_OK


def test_symbols_header_and_layout():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in ("mp_ransac_out_set", "mp_debug_ransac_out_stats"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_ransac_out) == 48 and "} mp_ransac_out;" in header
    for i, field in enumerate(("mask", "errors", "models", "index", "counts", "producer_stream")):
        assert getattr(L.mp_ransac_out, field).offset == 8 * i, field
        assert L.mp_ransac_out._fields_[i][0] == field
    assert len(L.EXPORTS["mp_ransac_out_set"][1]) == 25
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "capi.cpp")) as f:
        assert '"ransac out layout"' in f.read()  # (the static_assert on the struct)
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "residuals_plan.h")) as f:
        plan = f.read()
    assert "#include <hip" not in plan and "__global__" not in plan  # plain C++
    assert "ransac_out_items" in plan and "ransac_out_overlap" in plan
    r = madpose.RansacResult()
    assert r.num_inliers == (0, 0, 0) and r.rows is None


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of residuals_plan.h needs ROCm's clang")
    exe = str(tmp_path / "ransac_out_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "ransac_out_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


class _FakeDevice:
    """An object with __cuda_array_interface__ and nothing behind it (never dereferenced here)"""

    def __init__(self, typestr, shape, strides=None, readonly=False, ptr=1 << 20):
        self.__cuda_array_interface__ = {"typestr": typestr, "shape": tuple(shape), "strides": strides,
                                         "data": (ptr, readonly), "version": 3}


def _unopened_set(variant=0, sizes=(20, 0, 7)):
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = variant, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = list(sizes)
    ps._norm = np.ones(len(sizes))
    return ps


def test_python_refusals_before_any_library_call(monkeypatch):
    ps = _unopened_set()
    R, ns = 27, 3

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    M = 1 << 20
    dm, de = _FakeDevice("|u1", (R,), ptr=M), _FakeDevice("<f8", (3, R), ptr=2 * M)
    dmod, di = _FakeDevice("<f8", (ns, 17), ptr=3 * M), _FakeDevice("<i4", (ns,), ptr=4 * M)
    dc = _FakeDevice("<i4", (ns, 3), ptr=5 * M)
    call = lambda **kw: ps.ransac(**{**dict(budget=8, seed=1), **kw})
    # lists
    for bad in (1, 0, None, "no"):
        with pytest.raises(ValueError, match="lists must be a bool"):
            call(lists=bad)
    # numpy arrays are refused, with the way to the host results
    for name, a in (("out_mask", np.zeros(R, dtype=np.uint8)), ("out_errors", np.zeros((3, R))),
                    ("out_models", np.zeros((ns, 17))), ("out_index", np.zeros(ns, dtype=np.int32)),
                    ("out_counts", np.zeros((ns, 3), dtype=np.int32))):
        with pytest.raises(ValueError, match=f"{name} must be a device array.*inlier_indices.*residuals"):
            call(**{name: a})
    with pytest.raises(ValueError, match="out_mask must be a numpy array or a device array"):
        call(out_mask=[0] * R)
    # out_errors needs out_mask
    with pytest.raises(ValueError, match="out_errors needs out_mask"):
        call(out_errors=de)
    with pytest.raises(ValueError, match="out_errors needs out_mask"):
        call(out_errors=de, out_models=dmod)
    # device outputs with lo and rounds = 0
    for out in (dict(out_mask=dm), dict(out_index=di), dict(out_mask=dm, out_errors=de, out_counts=dc)):
        with pytest.raises(ValueError, match="device outputs with lo need rounds >= 1"):
            call(step=4, lo=1, rounds=0, **out)
        with pytest.raises(ValueError, match="device outputs with lo need rounds >= 1"):
            call(step=4, lo=1, lo_steps=2, rounds=0, **out)
    # the stream
    with pytest.raises(ValueError, match="stream goes with device outputs"):
        call(stream=0)
    with pytest.raises(ValueError, match="stream goes with device outputs"):
        call(stream=0, lists=False)
    for bad in (-1, 1.5, True, "0"):
        with pytest.raises(ValueError, match="stream must be None"):
            call(out_mask=dm, stream=bad)
    # shape, dtype, stride, read-only flag, address: every array
    specs = (("out_mask", "|u1", (R,), "|i1", "uint8", (R - 1,), (2,)),
             ("out_errors", "<f8", (3, R), "<f4", "float64", (R, 3), (8, 24)),
             ("out_models", "<f8", (ns, 17), "<f4", "float64", (ns, 16), (8, 8 * ns)),
             ("out_index", "<i4", (ns,), "<i8", "int32", (ns + 1,), (8,)),
             ("out_counts", "<i4", (ns, 3), "<u4", "int32", (ns, 4), (4, 4 * ns)))
    for name, typestr, shape, bad_type, dtype_name, bad_shape, bad_strides in specs:
        base = {} if name == "out_mask" else dict(out_mask=dm)
        with pytest.raises(ValueError, match=f"{name} must be {dtype_name}, got typestr"):
            call(**base, **{name: _FakeDevice(bad_type, shape, ptr=7 * M)})
        with pytest.raises(ValueError, match=f"{name} must have shape"):
            call(**base, **{name: _FakeDevice(typestr, bad_shape, ptr=7 * M)})
        with pytest.raises(ValueError, match=f"{name} must be C-contiguous"):
            call(**base, **{name: _FakeDevice(typestr, shape, strides=bad_strides, ptr=7 * M)})
        with pytest.raises(ValueError, match=f"{name} is read-only"):
            call(**base, **{name: _FakeDevice(typestr, shape, readonly=True, ptr=7 * M)})
        with pytest.raises(ValueError, match=f"{name} has no device address"):
            call(**base, **{name: _FakeDevice(typestr, shape, ptr=0)})
    # the shapes follow the selection
    with pytest.raises(ValueError, match=r"out_mask must have shape \(20,\)"):
        call(out_mask=dm, pair_ids=[0, 1])
    with pytest.raises(ValueError, match=r"out_models must have shape \(2, 17\)"):
        call(out_models=dmod, pair_ids=[2, 0])
    # outputs that overlap one another
    with pytest.raises(ValueError, match="out_mask and out_errors overlap"):
        call(out_mask=dm, out_errors=_FakeDevice("<f8", (3, R), ptr=M + 24))
    with pytest.raises(ValueError, match="out_errors and out_mask overlap"):
        call(out_mask=_FakeDevice("|u1", (R,), ptr=2 * M + 8 * R), out_errors=de)
    with pytest.raises(ValueError, match="out_index and out_counts overlap"):
        call(out_index=di, out_counts=_FakeDevice("<i4", (ns, 3), ptr=4 * M + 8))
    with pytest.raises(ValueError, match="out_counts and out_models overlap"):
        call(out_models=dmod, out_counts=_FakeDevice("<i4", (ns, 3), ptr=3 * M - 4))
    # arrays that only touch do not overlap: the call goes on to the library
    with pytest.raises(AssertionError, match="the library was called"):
        call(out_mask=dm, out_errors=_FakeDevice("<f8", (3, R), ptr=M + 32), out_models=dmod, out_index=di,
             out_counts=dc, lists=False)
    with pytest.raises(AssertionError, match="the library was called"):
        call(lists=False)
    # an empty selection is answered without the library, after the checks
    assert call(pair_ids=[], out_mask=_FakeDevice("|u1", (0,), ptr=0), lists=False) == []
    with pytest.raises(ValueError, match=r"out_index must have shape \(0,\)"):
        call(pair_ids=[], out_index=di)
    # a closed set
    ps._h = None
    with pytest.raises(ValueError, match="closed"):
        call(out_mask=dm)


def _empty_set(variant=0):
    o, c = synthetic.example_options("calibrated")
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_c_refusals_before_any_device(variant):
    lib = L.lib()
    with _empty_set(variant) as ps:
        h = ps._h
        mods, res = (L.mp_model * 2)(), (L.mp_ransac_result * 2)()
        info, sinfo = (L.mp_ransac_lo_info * 2)(), (L.mp_ransac_lo_steps_info * 2)()
        rmass = (L.mp_inlier_mass * 2)()
        idx, stopped = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 2)()
        out = L.mp_ransac_out()
        names = ("set", "weights", "n", "ids", "budget", "step", "seed", "share", "so", "ty", "ix", "rounds", "lo",
                 "lo_steps", "wstop", "models", "results", "idx", "stopped", "info", "sinfo", "sc", "mc", "rmass", "out")
        defaults = dict(set=h, weights=None, n=0, ids=None, budget=8, step=0, seed=1, share=-1, so=None, ty=None,
                        ix=None, rounds=3, lo=0, lo_steps=0, wstop=0, models=mods, results=res, idx=idx,
                        stopped=stopped, info=info, sinfo=sinfo, sc=0, mc=0, rmass=rmass, out=ctypes.byref(out))
        call = lambda **kw: lib.mp_ransac_out_set(*[kw.get(k, defaults[k]) for k in names])
        err = lambda: lib.mp_last_error()
        # no entry is the only legal call on an empty set, and it needs no device: every body
        for kw in (dict(), dict(step=4), dict(step=4, lo=1), dict(step=4, lo=1, lo_steps=2), dict(out=None),
                   dict(idx=None), dict(idx=None, out=None, step=4, lo=1, rounds=0)):
            assert call(**kw) == L.MP_OK, (kw, err())
        assert call(set=None) == L.MP_EINVAL and b"null pair set" in err()
        # errors without mask
        fake = L.mp_ransac_out()
        fake.errors = 1 << 20
        assert call(out=ctypes.byref(fake)) == L.MP_EINVAL and b"errors needs mask" in err()
        # device outputs together with lo_rounds and rounds = 0, whichever array is given
        for field in ("mask", "models", "index", "counts"):
            one = L.mp_ransac_out()
            setattr(one, field, 1 << 20)
            assert call(out=ctypes.byref(one), step=4, lo=1, rounds=0) == L.MP_EINVAL and b"rounds >= 1" in err(), field
            assert call(out=ctypes.byref(one), step=4, lo=1, lo_steps=2, rounds=0) == L.MP_EINVAL
            assert b"rounds >= 1" in err()
            assert call(out=ctypes.byref(one), step=4, lo=1, rounds=1) == L.MP_OK  # (no entry: nothing is read)
            assert call(out=ctypes.byref(one), step=4, rounds=0) == L.MP_OK
        # the union of the entries' arguments
        assert call(step=-1) == L.MP_EINVAL and b"step" in err()
        assert call(lo=-1) == L.MP_EINVAL and call(lo_steps=-1) == L.MP_EINVAL
        assert call(lo=1) == L.MP_EINVAL and b"need step" in err()
        assert call(lo_steps=1) == L.MP_EINVAL and b"need step" in err()
        assert call(step=4, lo_steps=1) == L.MP_EINVAL and b"lo_steps needs lo_rounds" in err()
        assert call(step=4, wstop=1) == L.MP_EINVAL and b"weighted_stop needs draw weights" in err()
        so = (ctypes.c_int64 * 1)(0)
        assert call(step=4, so=so, budget=-1) == L.MP_EINVAL and b"given samples" in err()
        assert call(so=so, budget=8) == L.MP_EINVAL and b"budget must be -1" in err()
        assert call(so=so, budget=-1) == L.MP_OK
        # the chosen body's own refusals
        assert call(rounds=65) == L.MP_EINVAL and b"rounds" in err()
        assert call(step=4, lo=65) == L.MP_EINVAL and b"lo_rounds" in err()
        assert call(step=4, lo=1, lo_steps=65) == L.MP_EINVAL and b"lo_steps" in err()
        assert call(budget=-1) == L.MP_EINVAL and b"budget" in err()
        assert call(sc=-1) == L.MP_EINVAL and call(mc=-1) == L.MP_EINVAL
        for bad in (0, -1, 1):
            ids = (ctypes.c_int32 * 1)(bad)
            assert call(n=1, ids=ids) == L.MP_EINVAL, bad


def test_stats_hook_counts_nothing_without_a_device():
    n, ms = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    assert L.lib().mp_debug_ransac_out_stats(ctypes.byref(n), ctypes.byref(ms), 1) == L.MP_OK
    assert L.lib().mp_debug_ransac_out_stats(ctypes.byref(n), ctypes.byref(ms), 0) == L.MP_OK
    assert n.value == 0 and ms.value == 0.0
    assert L.lib().mp_debug_ransac_out_stats(None, None, 0) == L.MP_OK
