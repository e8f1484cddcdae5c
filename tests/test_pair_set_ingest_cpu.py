"""PairSet.from_device / mp_pair_set_create_device without a device: the symbols and constants
are there and agree with madpose_amd/_lib.py; every Python-level refusal (dtype, shape,
contiguity, length against offsets[-1], both depth sources or none) is a ValueError before any
library call, on CPU torch tensors and on stand-in objects with a hand-made
__cuda_array_interface__; every C-level MP_EINVAL that precedes the device is returned on a
device index that does not exist; the empty set is valid; and the item plan, the byte-extent
arithmetic and the record finishing (madpose_amd/csrc/host/ingest_plan.h) pass their stand-alone
check under AddressSanitizer and UBSan (tests/pair_set_ingest_check.cpp)."""
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
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
SYMBOLS = ("mp_pair_set_create_device", "mp_debug_pair_set_record", "mp_debug_ingest_info",
           "mp_debug_device_extent")
FAKE = 0x7F0000001000  # an address no test dereferences


class Dev:
    """a stand-in device array: only __cuda_array_interface__"""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=FAKE):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides,
                                             version=3)


def test_symbols_and_constants():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTS, name
        assert f"int {name}(" in header, name
    for macro, value in (("MP_PAIR_RECORD_VALUES", L.PAIR_RECORD_VALUES), ("MP_INGEST_INFO_VALUES", L.INGEST_INFO_VALUES)):
        line, = [ln for ln in header.splitlines() if ln.startswith(f"#define {macro}")]
        assert int(line.split()[2]) == value
    info = np.zeros(L.INGEST_INFO_VALUES, dtype=np.int32)
    assert lib.mp_debug_ingest_info(info.ctypes.data_as(L.c_int32_p)) == L.MP_OK
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "ingest_plan.h")) as f:
        plan = f.read()
    for name, v in zip(("kIngestBlock", "kIngestChunk", "kIngestSpan"), info.tolist()):
        assert f"constexpr int {name} = {v};" in plan, name
    assert lib.mp_debug_ingest_info(None) == L.MP_EINVAL
    assert lib.mp_debug_pair_set_record(None, 0, None) == L.MP_EINVAL
    assert lib.mp_debug_device_extent(None, 0, None) == L.MP_EINVAL
    # the struct of the binding is the header's: field for field, in order
    body = header.split("typedef struct mp_device_pairs {")[1].split("} mp_device_pairs;")[0]
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f for f, _ in L.mp_device_pairs._fields_], names
    assert hasattr(madpose.PairSet, "from_device")


# ---- the Python layer ----

def _good(P=2, sizes=(4, 3)):
    T = sum(sizes)
    o, c = synthetic.example_options("calibrated")
    return dict(variant=0, x0=Dev((T, 2)), x1=Dev((T, 2)), offsets=np.concatenate([[0], np.cumsum(sizes)]),
                cam0=np.tile(np.eye(3), (P, 1, 1)), cam1=np.tile(np.eye(3), (P, 1, 1)), options=o, est_config=c,
                depth0=Dev((T,)), depth1=Dev((T,)))


def _maps(a, M=2):
    a.update(depth0=None, depth1=None, depth_maps=[Dev((3, 5), "<f4") for _ in range(M)],
             map_ids=np.zeros((2, 2), dtype=np.int64))
    return a


@pytest.mark.parametrize("change,match", [
    (dict(variant=5), "variant"),
    (dict(x0=Dev((7, 2), "<f2")), "x0 must be float32 or float64"),
    (dict(x0=Dev((7, 2), "<i8")), "x0 must be float32 or float64"),
    (dict(x1=Dev((7, 2), "<f4")), "x0 and x1 must have the same dtype"),
    (dict(x0=Dev((6, 2))), r"x0 must have shape \(7, 2\)"),
    (dict(x0=Dev((14,))), r"x0 must have shape \(7, 2\)"),
    (dict(x1=Dev((7, 3))), r"x1 must have shape \(7, 2\)"),
    (dict(x0=Dev((7, 2), strides=(32, 8))), "x0 must be C-contiguous"),
    (dict(x0=Dev((7, 2), strides=(8, 56))), "x0 must be C-contiguous"),
    (dict(x0=np.zeros((7, 2))), "x0 must be a device array"),
    (dict(x0=Dev((7, 2), ptr=0)), "x0 has no device address"),
    (dict(depth0=Dev((5,))), r"depth0 must have shape \(7,\)"),
    (dict(depth1=Dev((7, 1))), r"depth1 must have shape \(7,\)"),
    (dict(depth1=Dev((7,), "<f4")), "depth0 and depth1 must have the same dtype"),
    (dict(depth0=Dev((7,), strides=(16,))), "depth0 must be C-contiguous"),
    (dict(depth1=None), "depth0 and depth1 must both be given"),
    (dict(depth0=None, depth1=None), "no depth source"),
    (dict(depth_maps=[Dev((3, 5))], map_ids=np.zeros((2, 2), dtype=int)), "both depth sources"),
    (dict(map_ids=np.zeros((2, 2), dtype=int)), "both depth sources"),
    (dict(offsets=np.array([0.0, 4.0, 7.0])), "offsets must be a 1-D integer array"),
    (dict(offsets=np.array([0, 4, 3])), "must not decrease"),
    (dict(offsets=np.array([1, 4, 7])), "offsets must start at 0"),
    (dict(offsets=np.array([0, 4, 8])), r"x0 must have shape \(8, 2\)"),
    (dict(cam0=np.eye(3)), "cam0 must hold 9 values for each of the 2 pairs"),
    (dict(min_depth=np.zeros(3)), "min_depth must hold 2 values"),
    (dict(stream="s"), "stream must be None"),
    (dict(stream=-4), "stream must be None"),
    (dict(stream=True), "stream must be None"),
])
def test_python_refusals_come_before_any_library_call(monkeypatch, change, match):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    a = _good()
    a.update(change)
    with pytest.raises(ValueError, match=match):
        madpose.PairSet.from_device(**a)


@pytest.mark.parametrize("change,match", [
    (dict(depth_maps=None), "needs depth_maps and map_ids"),
    (dict(map_ids=None), "needs depth_maps and map_ids"),
    (dict(depth_maps=[]), "depth_maps is empty"),
    (dict(depth_maps=[Dev((3, 5), "<f4"), Dev((3, 5), "<f8")]), "one dtype"),
    (dict(depth_maps=[Dev((15,), "<f4")]), r"depth_maps\[0\] must be a 2-D"),
    (dict(depth_maps=[Dev((3, 5), "<f4"), Dev((0, 5), "<f4")]), r"depth_maps\[1\] must be a 2-D"),
    (dict(depth_maps=[Dev((3, 5), "<f4", strides=(40, 4))]), r"depth_maps\[0\] must be C-contiguous"),
    (dict(depth_maps=[Dev((3, 5), "<i4")]), r"depth_maps\[0\] must be float32 or float64"),
    (dict(map_ids=np.zeros((2, 2))), "map_ids must be an integer array"),
    (dict(map_ids=np.zeros((3, 2), dtype=int)), "map_ids must be an integer array of shape"),
    (dict(map_ids=np.array([[0, 1], [2, 0]])), r"map_ids must lie in 0\.\.1"),
    (dict(map_ids=np.array([[0, -1], [1, 0]])), r"map_ids must lie in 0\.\.1"),
    (dict(image_sizes=np.zeros((2, 2), dtype=int)), "image_sizes must be positive"),
    (dict(image_sizes=np.ones((3, 2), dtype=int)), "image_sizes must be an integer array of shape"),
    (dict(image_sizes=np.ones((2, 2))), "image_sizes must be an integer array"),
])
def test_python_refusals_of_the_map_source(monkeypatch, change, match):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    a = _maps(_good())
    a.update(change)
    with pytest.raises(ValueError, match=match):
        madpose.PairSet.from_device(**a)


def test_cpu_torch_tensors_are_refused(monkeypatch):
    import torch

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    a = _good()
    a["x0"] = torch.zeros(7, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="x0 must be a device array"):
        madpose.PairSet.from_device(**a)
    a = _good()
    a["depth1"] = torch.zeros(7)
    with pytest.raises(ValueError, match="depth1 must be a device array"):
        madpose.PairSet.from_device(**a)


def test_python_accepts_what_the_issue_names(monkeypatch):
    """float32 arrays, unit dimensions with any stride, a stream object, default image sizes:
    the call gets as far as the library (here: a device that does not exist)"""
    class Stream:
        cuda_stream = 0x1234
    a = _good()
    a.update(x0=Dev((7, 2), "<f4", strides=(8, 4)), x1=Dev((7, 2), "<f4"), stream=Stream(), device=NO_DEVICE)
    with pytest.raises((ValueError, RuntimeError), match="(?i)device"):
        madpose.PairSet.from_device(**a)
    a = _maps(_good())
    a.update(device=NO_DEVICE, stream=0)
    with pytest.raises((ValueError, RuntimeError), match="(?i)device"):
        madpose.PairSet.from_device(**a)


# ---- the C entry ----

def _cargs(sizes=(4, 3), maps=False):
    """A well-formed argument list of mp_pair_set_create_device as a dict (arrays kept alive in
    it); the device addresses are never read: the device does not exist."""
    o, c = synthetic.example_options("calibrated")
    P = len(sizes)
    a = dict(variant=0, num_pairs=P, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
             min_depth=np.zeros(2 * P), cam0=np.tile(np.eye(3).ravel(), P), cam1=np.tile(np.eye(3).ravel(), P),
             options=o._to_c(), config=c._to_c(), out=ctypes.c_void_p(12345), inputs=L.mp_device_pairs())
    inp = a["inputs"]
    inp.x0, inp.x1, inp.xy_type = FAKE, FAKE, 1
    if maps:
        a["table"] = (ctypes.c_void_p * 2)(FAKE, FAKE)
        a["dims"] = np.array([[3, 5, 30, 50], [4, 4, 4, 4]], dtype=np.int64)
        a["ids"] = np.zeros((P, 2), dtype=np.int32)
        inp.depth_maps = ctypes.cast(a["table"], ctypes.POINTER(ctypes.c_void_p))
        inp.map_dims = a["dims"].ctypes.data_as(L.c_int64_p)
        inp.map_ids = a["ids"].ctypes.data_as(L.c_int32_p)
        inp.num_maps, inp.map_type = 2, 0
    else:
        inp.d0, inp.d1, inp.depth_type = FAKE, FAKE, 1
    return a


def _ccreate(a, device=NO_DEVICE):
    dp = lambda v: None if v is None else v.ctypes.data_as(L.c_double_p)
    return L.lib().mp_pair_set_create_device(
        a["variant"], a["num_pairs"], None if a["offsets"] is None else a["offsets"].ctypes.data_as(L.c_int64_p),
        None if a["inputs"] is None else ctypes.byref(a["inputs"]), dp(a["min_depth"]), dp(a["cam0"]), dp(a["cam1"]),
        None if a["options"] is None else ctypes.byref(a["options"]),
        None if a["config"] is None else ctypes.byref(a["config"]), device,
        None if a["out"] is None else ctypes.byref(a["out"]))


def _set(field, value):
    def change(a):
        setattr(a["inputs"], field, value)
    return change


def _key(name, value):
    def change(a):
        a[name] = value
    return change


def _ids(value):
    def change(a):
        a["ids"][1, 1] = value
    return change


def _dims(m, j, value):
    def change(a):
        a["dims"][m, j] = value
    return change


@pytest.mark.parametrize("maps,change,text", [
    (False, _key("num_pairs", -1), b"negative pair count"),
    (False, _key("variant", 4), b"variant"),
    (False, _key("variant", -1), b"variant"),
    (False, _key("offsets", None), b"null offsets"),
    (False, _key("min_depth", None), b"null offsets, min_depth or cameras"),
    (False, _key("cam0", None), b"null offsets, min_depth or cameras"),
    (False, _key("cam1", None), b"null offsets, min_depth or cameras"),
    (False, _key("options", None), b"null options"),
    (False, _key("out", None), b"null output"),
    (False, _key("inputs", None), b"null inputs"),
    (False, _key("offsets", np.array([0, 4, 3], dtype=np.int64)), b"must not decrease"),
    (False, _key("offsets", np.array([-1, 4, 7], dtype=np.int64)), b"non-negative"),
    (False, _key("offsets", np.array([0, 4, 5 + (1 << 28)], dtype=np.int64)), b"pair too large"),
    (False, _set("x0", None), b"null input array x0 or x1"),
    (False, _set("x1", None), b"null input array x0 or x1"),
    (False, _set("d0", None), b"null input array d0 or d1"),
    (False, _set("d1", None), b"null input array d0 or d1"),
    (False, _set("xy_type", 2), b"xy_type"),
    (False, _set("xy_type", -1), b"xy_type"),
    (False, _set("depth_type", 2), b"depth_type"),
    (False, _set("num_maps", 1), b"both depth sources"),
    (True, _set("d0", FAKE), b"both depth sources"),
    (True, _set("d1", FAKE), b"both depth sources"),
    (True, _set("map_type", 3), b"map_type"),
    (True, _set("num_maps", 0), b"the map source needs"),
    (True, _set("num_maps", -2), b"the map source needs"),
    (True, _set("map_dims", None), b"the map source needs"),
    (True, _set("map_ids", None), b"the map source needs"),
    (True, _set("depth_maps", None), b"the map source needs"),
    (True, _ids(2), b"map_ids[3] = 2 is outside the 2 maps"),
    (True, _ids(-1), b"map_ids[3] = -1 is outside the 2 maps"),
    (True, _dims(0, 0, 0), b"map_dims[0]"),
    (True, _dims(1, 1, -5), b"map_dims[1]"),
    (True, _dims(1, 2, 0), b"map_dims[1]"),
    (True, _dims(0, 3, -1), b"map_dims[0]"),
])
def test_bad_create_arguments_are_einval(maps, change, text):
    a = _cargs(maps=maps)
    change(a)
    assert _ccreate(a) == L.MP_EINVAL
    assert text in L.lib().mp_last_error(), L.lib().mp_last_error()
    if a["out"] is not None:
        assert a["out"].value is None  # (no handle on failure)


def test_neither_depth_source_is_einval():
    a = _cargs()
    a["inputs"].d0 = a["inputs"].d1 = None
    assert _ccreate(a) == L.MP_EINVAL
    assert b"no depth source" in L.lib().mp_last_error()
    table = (ctypes.c_void_p * 2)(FAKE, None)  # a null entry of the map table
    a = _cargs(maps=True)
    a["inputs"].depth_maps = ctypes.cast(table, ctypes.POINTER(ctypes.c_void_p))
    assert _ccreate(a) == L.MP_EINVAL
    assert b"depth_maps[1] is null" in L.lib().mp_last_error()


def test_bounds_and_options_are_einval_before_any_read():
    per = 1 << 24
    sizes = [per] * 4 + [1]
    a = _cargs(sizes=sizes)
    assert int(a["offsets"][-1]) == (1 << 26) + 1
    assert _ccreate(a) == L.MP_EINVAL
    assert b"2^26" in L.lib().mp_last_error()
    a = _cargs()
    a["options"].squared_inlier_thresholds[0] = 0.0
    assert _ccreate(a) == L.MP_EINVAL
    assert b"squared_inlier_thresholds" in L.lib().mp_last_error()


@pytest.mark.parametrize("maps", [False, True])
def test_well_formed_arguments_reach_the_device(maps):
    """the counterpart of the tests above: nothing but the device is wrong here"""
    a = _cargs(maps=maps)
    assert _ccreate(a) in (L.MP_EDEVICE, L.MP_EINVAL)  # (EINVAL: "device index out of range")
    assert b"device" in L.lib().mp_last_error().lower()
    assert b"device array" not in L.lib().mp_last_error()
    a["config"] = None  # (a null config means the defaults)
    assert _ccreate(a) != L.MP_OK


def test_empty_set_needs_no_device():
    lib = L.lib()
    a = _cargs(sizes=())
    for k in ("offsets", "min_depth", "cam0", "cam1", "inputs"):
        a[k] = None
    assert _ccreate(a) == L.MP_OK
    h = a["out"]
    assert h.value
    p, nc, nb = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.mp_pair_set_info(h, None, ctypes.byref(p), ctypes.byref(nc), ctypes.byref(nb), None) == L.MP_OK
    assert (p.value, nc.value, nb.value) == (0, 0, 0)
    assert lib.mp_debug_pair_set_record(h, 0, np.zeros(L.PAIR_RECORD_VALUES).ctypes.data_as(L.c_double_p)) == L.MP_EINVAL
    assert lib.mp_pair_set_destroy(h) == L.MP_OK
    # the Python class on no pairs: zero-size device arrays have no address
    o, c = synthetic.example_options("shared_focal")
    with madpose.PairSet.from_device(1, Dev((0, 2), ptr=0), Dev((0, 2), ptr=0), [0], np.zeros((0, 2)), np.zeros((0, 2)),
                                     o, c, depth0=Dev((0,), ptr=0), depth1=Dev((0,), ptr=0), device=NO_DEVICE) as ps:
        assert len(ps) == 0 and ps.num_correspondences == 0 and ps.resident_bytes == 0
        assert ps.norm_scale.shape == (0,)
        assert ps.refine([]) == [] and ps.select([]) == []
    with pytest.raises(ValueError, match="closed"):
        len(ps)


def test_plan_extents_and_records_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of ingest_plan.h needs ROCm's clang")
    exe = str(tmp_path / "pair_set_ingest_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "pair_set_ingest_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
