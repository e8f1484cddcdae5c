"""PairSet.residuals without a device: the plan and the output-extent arithmetic
(madpose_amd/csrc/host/residuals_plan.h) pass their stand-alone check under AddressSanitizer and
UBSan (tests/residuals_plan_check.cpp); every Python check comes before any library call; and
mp_residuals_set refuses bad arguments on a set whose device does not exist."""
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
    for name in ("mp_residuals_set", "mp_debug_residuals_stats"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_residuals_out) == 32 and "} mp_residuals_out;" in header
    assert L.mp_residuals_out.errors.offset == 8 and L.mp_residuals_out.on_device.offset == 16
    assert L.mp_residuals_out.producer_stream.offset == 24
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "residuals_plan.h")) as f:
        plan = f.read()
    assert "#include <hip" not in plan and "__global__" not in plan  # plain C++
    assert "kResidItemRows = 4096" in plan
    assert hasattr(madpose.PairSet, "residuals") and hasattr(madpose, "ResidualsResult")


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of residuals_plan.h needs ROCm's clang")
    exe = str(tmp_path / "residuals_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "residuals_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


class _FakeDevice:
    """An object with __cuda_array_interface__ and nothing behind it (never dereferenced here)"""

    def __init__(self, typestr, shape, strides=None, readonly=False, ptr=4096):
        self.__cuda_array_interface__ = {"typestr": typestr, "shape": tuple(shape), "strides": strides,
                                         "data": (ptr, readonly), "version": 3}


def _unopened_set(variant=0, sizes=(20, 0, 7)):
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = variant, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = list(sizes)
    ps._norm = np.ones(len(sizes))
    return ps


def test_python_checks_before_any_library_call(monkeypatch):
    ps = _unopened_set()
    R = 27

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    m = madpose.PoseScaleOffset()
    three = [m, m, m]
    rows = np.zeros((3, 17))
    # the model count, shape and dtype
    with pytest.raises(ValueError, match="one model per pair"):
        ps.residuals([m])
    with pytest.raises(ValueError, match="one model per pair"):
        ps.residuals(np.zeros((2, 17)))
    with pytest.raises(ValueError, match="one model per entry"):
        ps.residuals([m], pair_ids=[0, 0])
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 3 is outside"):
        ps.residuals([m, m], pair_ids=[0, 3])
    with pytest.raises(ValueError, match=r"pair_ids\[0\] = -1 is outside"):
        ps.residuals([m], pair_ids=[-1])
    for bad in (np.zeros((3, 16)), np.zeros(17), np.zeros((3, 17), dtype=np.float32), np.zeros((3, 17, 1))):
        with pytest.raises(ValueError, match="array models must be float64"):
            ps.residuals(bad)
    with pytest.raises(ValueError, match="models must be a sequence"):
        ps.residuals(5)
    # the factor
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf, [1.0, 0.0, 1.0], [1.0, 2.0, np.nan]):
        with pytest.raises(ValueError, match="factor must be finite and positive"):
            ps.residuals(three, factor=bad)
    with pytest.raises(ValueError, match="one factor value per entry"):
        ps.residuals(three, factor=[1.0, 2.0])
    for bad in (True, "2", None):
        with pytest.raises(ValueError, match="factor must be a number"):
            ps.residuals(three, factor=bad)
    with pytest.raises(ValueError, match="errors must be True or False"):
        ps.residuals(three, errors=1)
    # host outputs: dtype, length, contiguity, read-only
    with pytest.raises(ValueError, match="out_mask must be uint8 of shape"):
        ps.residuals(three, out_mask=np.zeros(R - 1, dtype=np.uint8))
    with pytest.raises(ValueError, match="out_mask must be uint8 of shape"):
        ps.residuals(three, out_mask=np.zeros(R, dtype=np.int8))
    with pytest.raises(ValueError, match="out_mask must be C-contiguous"):
        ps.residuals(three, out_mask=np.zeros(2 * R, dtype=np.uint8)[::2])
    ro = np.zeros(R, dtype=np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="out_mask is read-only"):
        ps.residuals(three, out_mask=ro)
    with pytest.raises(ValueError, match="out_errors must be float64 of shape"):
        ps.residuals(three, out_errors=np.zeros((R, 3)))
    with pytest.raises(ValueError, match="out_errors must be float64 of shape"):
        ps.residuals(three, out_errors=np.zeros((3, R), dtype=np.float32))
    with pytest.raises(ValueError, match="out_errors must be C-contiguous"):
        ps.residuals(three, out_errors=np.zeros((R, 3)).T)
    roe = np.zeros((3, R))
    roe.flags.writeable = False
    with pytest.raises(ValueError, match="out_errors is read-only"):
        ps.residuals(three, out_errors=roe)
    with pytest.raises(ValueError, match="out_mask must be a numpy array or a device array"):
        ps.residuals(three, out_mask=[0] * R)
    # device outputs: typestr, shape, contiguity, read-only, address
    dm, de = _FakeDevice("|u1", (R,)), _FakeDevice("<f8", (3, R))
    with pytest.raises(ValueError, match="out_mask must be uint8, got typestr"):
        ps.residuals(three, out_mask=_FakeDevice("|i1", (R,)))
    with pytest.raises(ValueError, match=r"out_mask must have shape \(27,\)"):
        ps.residuals(three, out_mask=_FakeDevice("|u1", (R - 1,)))
    with pytest.raises(ValueError, match="out_mask must be C-contiguous"):
        ps.residuals(three, out_mask=_FakeDevice("|u1", (R,), strides=(2,)))
    with pytest.raises(ValueError, match="out_mask is read-only"):
        ps.residuals(three, out_mask=_FakeDevice("|u1", (R,), readonly=True))
    with pytest.raises(ValueError, match="out_mask has no device address"):
        ps.residuals(three, out_mask=_FakeDevice("|u1", (R,), ptr=0))
    with pytest.raises(ValueError, match="out_errors must be float64, got typestr"):
        ps.residuals(three, out_mask=dm, out_errors=_FakeDevice("<f4", (3, R)))
    with pytest.raises(ValueError, match=r"out_errors must have shape \(3, 27\)"):
        ps.residuals(three, out_mask=dm, out_errors=_FakeDevice("<f8", (R, 3)))
    with pytest.raises(ValueError, match="out_errors must be C-contiguous"):
        ps.residuals(three, out_mask=dm, out_errors=_FakeDevice("<f8", (3, R), strides=(8, 24)))
    with pytest.raises(ValueError, match="out_errors is read-only"):
        ps.residuals(three, out_mask=dm, out_errors=_FakeDevice("<f8", (3, R), readonly=True))
    # kinds
    with pytest.raises(ValueError, match="one kind"):
        ps.residuals(three, out_mask=np.zeros(R, dtype=np.uint8), out_errors=de)
    with pytest.raises(ValueError, match="one kind"):
        ps.residuals(three, out_mask=dm, out_errors=np.zeros((3, R)))
    with pytest.raises(ValueError, match="device outputs"):
        ps.residuals(three, out_errors=de)
    with pytest.raises(ValueError, match="device outputs"):
        ps.residuals(three, out_mask=dm, errors=True)
    # the stream
    with pytest.raises(ValueError, match="stream goes with device outputs"):
        ps.residuals(three, stream=0)
    for bad in (-1, 1.5, True, "0"):
        with pytest.raises(ValueError, match="stream must be None"):
            ps.residuals(three, out_mask=dm, stream=bad)
    # array models pass the checks as pose objects do
    with pytest.raises(ValueError, match="stream goes with device outputs"):
        ps.residuals(rows, stream=0)
    # no row at all: answered without the library
    res = ps.residuals([m, m], pair_ids=[1, 1], errors=True)
    assert res.offsets.tolist() == [0, 0, 0] and res.counts.tolist() == [[0, 0, 0], [0, 0, 0]]
    assert res.mask.shape == (0,) and res.mask.dtype == np.uint8 and res.errors.shape == (3, 0)
    assert res.rows(1) == slice(0, 0)
    res = ps.residuals([], pair_ids=[])
    assert res.offsets.tolist() == [0] and res.counts.shape == (0, 3) and res.errors is None
    # a closed set
    ps._h = None
    with pytest.raises(ValueError, match="closed"):
        ps.residuals(three)


def _empty_set(variant=0):
    o, c = synthetic.example_options("calibrated")
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_c_refusals_before_any_device(variant):
    lib = L.lib()
    with _empty_set(variant) as ps:
        h = ps._h
        mods = (L.mp_model * 2)()
        mask = (ctypes.c_uint8 * 8)()
        errs = (ctypes.c_double * 24)()
        out = L.mp_residuals_out()
        out.mask, out.errors = ctypes.addressof(mask), ctypes.addressof(errs)
        offs, counts = (ctypes.c_int64 * 3)(7, 7, 7), (ctypes.c_int32 * 6)()
        i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
        f64 = lambda *v: (ctypes.c_double * len(v))(*v)
        call = lambda **kw: lib.mp_residuals_set(*[kw.get(k, d) for k, d in (
            ("set", h), ("n", 0), ("ids", None), ("models", mods), ("factors", None), ("out", ctypes.byref(out)),
            ("offs", offs), ("counts", counts))])
        # no entry is the only legal call on an empty set, and it needs no device
        assert call() == L.MP_OK and offs[0] == 0
        assert call(ids=i32(0), factors=f64(2.0)) == L.MP_OK
        assert call(set=None) == L.MP_EINVAL and b"null pair set" in lib.mp_last_error()
        assert call(out=None) == L.MP_EINVAL and b"null out" in lib.mp_last_error()
        assert call(offs=None) == L.MP_EINVAL and b"row_offsets" in lib.mp_last_error()
        assert call(counts=None) == L.MP_EINVAL and b"counts" in lib.mp_last_error()
        nomask = L.mp_residuals_out()
        nomask.errors = ctypes.addressof(errs)
        assert call(out=ctypes.byref(nomask)) == L.MP_EINVAL and b"null mask" in lib.mp_last_error()
        for on_device in (0, 1):  # (the checks do not depend on where the outputs are)
            out.on_device = on_device
            assert call(n=-1) == L.MP_EINVAL and b"num_entries" in lib.mp_last_error()
            assert call(n=(1 << 24) + 1) == L.MP_EINVAL and b"num_entries" in lib.mp_last_error()
            # null pair_ids: the entries are the set's pairs, of which there are none
            assert call(n=1) == L.MP_EINVAL and b"pair count" in lib.mp_last_error()
            for bad in (0, -1, 1):
                assert call(n=1, ids=i32(bad)) == L.MP_EINVAL and b"outside the set" in lib.mp_last_error()
            # (the factors are read before the pair ids, so an empty set reaches their check)
            for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), -float("inf")):
                assert call(n=2, ids=i32(0, 0), factors=f64(1.5, bad)) == L.MP_EINVAL
                assert b"factors[1] must be finite and > 0" in lib.mp_last_error()
            assert call(n=1, ids=i32(0), factors=f64(1.5)) == L.MP_EINVAL and b"outside" in lib.mp_last_error()
        out.on_device = 0
        assert call(n=0, factors=f64(0.0)) == L.MP_OK  # (no entry: no factor is read)


def test_stats_hook_counts_nothing_without_a_device():
    n, ms = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    assert L.lib().mp_debug_residuals_stats(ctypes.byref(n), ctypes.byref(ms), 1) == L.MP_OK
    assert L.lib().mp_debug_residuals_stats(ctypes.byref(n), ctypes.byref(ms), 0) == L.MP_OK
    assert n.value == 0 and ms.value == 0.0
    assert L.lib().mp_debug_residuals_stats(None, None, 0) == L.MP_OK
