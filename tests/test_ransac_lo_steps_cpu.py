"""mp_lsq_fit_set / mp_ransac_lo_steps_set / PairSet.lsq_fit / PairSet.ransac(lo_steps=...)
without a device: the subset rule's host form (madpose_amd/csrc/include/mp_subset.h through
mp_debug_subset_select_host) and the size rules (mp_debug_lsq_subset_size) equal their Python
restatement (tests/lsq_subset_restatement.py); the plain-C++ headers pass their stand-alone
check under AddressSanitizer and UBSan (tests/lsq_subset_check.cpp); the Python argument checks
come before any library call; and every bad argument of the C entries is MP_EINVAL on a set
whose device does not exist."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import lsq_subset_restatement as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
HOST = os.path.join(ROOT, "madpose_amd", "csrc", "host")


def test_symbols_and_header():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in ("mp_lsq_fit_set", "mp_ransac_lo_steps_set", "mp_debug_subset_select", "mp_debug_subset_select_host",
                 "mp_debug_lsq_subset_size"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_lsq_fit_result) == 48 and ctypes.sizeof(L.mp_ransac_lo_steps_info) == 16
    # no existing struct changed
    assert ctypes.sizeof(L.mp_ransac_result) == 80 and ctypes.sizeof(L.mp_refine_result) == 48
    assert ctypes.sizeof(L.mp_ransac_lo_info) == 16 and ctypes.sizeof(L.mp_select_result) == 32
    r = madpose.RansacResult()
    assert (r.lo_step, r.lo_stage, r.lo_step_offers, r.lo_step_accepted) == (-1, -1, 0, 0)
    assert (r.lo_runs, r.lo_accepted, r.lo_index) == (0, 0, -1)
    for name in ("ransac_lo_steps.h", "lsq_fit_plan.h", os.path.join("..", "include", "mp_subset.h")):
        with open(os.path.join(HOST, name)) as f:
            text = f.read()
        assert "#include <hip" not in text and "__global__" not in text, name  # plain C++
    with open(os.path.join(HOST, "..", "include", "mp_subset.h")) as f:
        text = f.read()
    assert "double" not in text and "float" not in text.replace("floating point", "")  # integer only


# ---- the subset rule and the size rules against the restatement ----

def subset_hook(entry, lists, k, seed, pair, stream, substream, mask, *tail):
    """mp_debug_subset_select_host / mp_debug_subset_select on three ascending lists"""
    offs = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    idx = np.ascontiguousarray(np.concatenate(list(lists) + [np.zeros(1, dtype=np.int32)]).astype(np.int32))
    out = np.full(len(idx), -7, dtype=np.int32)
    sizes = np.full(3, -7, dtype=np.int32)
    L.check(entry(offs.ctypes.data_as(L.c_int64_p), idx.ctypes.data_as(L.c_int32_p), int(k), int(seed), int(pair),
                  int(stream), int(substream), int(mask), out.ctypes.data_as(L.c_int32_p),
                  sizes.ctypes.data_as(L.c_int32_p), *tail))
    got = [out[offs[t]:offs[t] + sizes[t]].copy() for t in range(3)]
    # nothing is written past a subset list
    for t in range(3):
        assert np.all(out[offs[t] + sizes[t]:offs[t + 1]] == -7)
    return got


def subset_cases():
    """(lists, k, mask, seed, pair, stream, substream) over the lengths, sizes and masks of the
    contract; one rng, so the GPU test sees the same cases"""
    rng = np.random.default_rng(2026)
    for lengths in Z.LENGTHS:
        lists = Z.case_lists(lengths, rng)
        for k in Z.case_sizes(sum(lengths)):
            for mask in Z.MASKS:
                yield (lists, k, mask, int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 1000)),
                       int(rng.integers(0, 1 << 31)), int(rng.integers(0, 1 << 30)))


def check_subset(got, lists, k, mask, seed, pair, stream, substream):
    want = Z.subset_select(lists, k, seed, pair, stream, substream, mask)
    M = sum(len(a) for a in lists)
    for t in range(3):
        assert got[t].dtype == np.int32 and np.array_equal(got[t], want[t]), (t, k, hex(mask))
        assert np.all(np.diff(got[t]) > 0) and np.all(np.isin(got[t], lists[t]))
    assert sum(len(a) for a in got) == min(k, M)
    if mask == 0 and k < M:  # the first k elements in (t, i) order
        assert np.array_equal(np.concatenate(got), np.concatenate(lists)[:k])


def test_host_subset_equals_restatement():
    entry = L.lib().mp_debug_subset_select_host
    seen = {"copy": 0, "select": 0, "ties": 0}
    for lists, k, mask, seed, pair, stream, substream in subset_cases():
        check_subset(subset_hook(entry, lists, k, seed, pair, stream, substream, mask), lists, k, mask, seed, pair,
                     stream, substream)
        M = sum(len(a) for a in lists)
        seen["copy" if M <= k else "select"] += 1
        seen["ties"] += mask != Z.MASK_ALL and 0 < k < M
    assert all(v > 30 for v in seen.values()), seen
    # the top-byte mask really ties: 700 elements over 256 key values
    lists = Z.case_lists((700, 0, 0), np.random.default_rng(1))
    keys = Z.subset_keys(5, 1, 2, 3, 0, lists[0]) & np.uint64(Z.MASK_TOP_BYTE)
    assert len(np.unique(keys)) <= 256 < 700


def test_subset_hook_bad_arguments():
    lib = L.lib()
    offs = np.array([0, 2, 2, 3], dtype=np.int64)
    idx = np.array([1, 5, 2], dtype=np.int32)
    out, sizes = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    p64, p32 = (lambda a: a.ctypes.data_as(L.c_int64_p)), (lambda a: a.ctypes.data_as(L.c_int32_p))
    call = lambda o=offs, i=idx, k=1, pair=0, st=0, sub=0: lib.mp_debug_subset_select_host(
        p64(o), p32(i), k, 0, pair, st, sub, Z.MASK_ALL, p32(out), p32(sizes))
    assert call() == L.MP_OK
    assert call(i=np.array([5, 1, 2], dtype=np.int32)) == L.MP_EINVAL and b"ascend" in lib.mp_last_error()
    assert call(i=np.array([1, 1, 2], dtype=np.int32)) == L.MP_EINVAL
    assert call(i=np.array([-1, 1, 2], dtype=np.int32)) == L.MP_EINVAL
    assert call(i=np.array([1, 1 << 28, 2], dtype=np.int32)) == L.MP_EINVAL
    assert call(o=np.array([1, 2, 2, 3], dtype=np.int64)) == L.MP_EINVAL
    assert call(o=np.array([0, 2, 1, 3], dtype=np.int64)) == L.MP_EINVAL
    assert call(k=-1) == L.MP_EINVAL and call(pair=-1) == L.MP_EINVAL and call(st=-1) == L.MP_EINVAL
    assert call(sub=1 << 30) == L.MP_EINVAL and call(sub=(1 << 30) - 1) == L.MP_OK


def lib_size(rule, s, variant, mu, nu, M):
    k, run = ctypes.c_int64(-1), ctypes.c_int32(-1)
    sizes = np.asarray(M, dtype=np.int32)
    L.check(L.lib().mp_debug_lsq_subset_size(L.LSQ_RULES[rule], s, variant, mu, nu, sizes.ctypes.data_as(L.c_int32_p),
                                             ctypes.byref(k), ctypes.byref(run)))
    return bool(run.value), int(k.value)


def test_size_rules_equal_restatement():
    skipped = set()
    lengths = (0, 1, 2, 3, 4, 5, 6, 7, 21, 36, 50, 700)
    for variant, s, rule in itertools.product(range(4), (0, 1), ("lsq", "nonmin")):
        k_md, k_pt = Z.solver_sizes(variant)
        for mu, nu in ((7, 3), (2, 3), (1, 1), (7, 40)):
            for M in itertools.product(lengths, repeat=3):
                want = Z.subset_size(rule, s, variant, mu, nu, M)
                assert lib_size(rule, s, variant, mu, nu, M) == want, (variant, s, rule, mu, nu, M)
                if not want[0]:
                    skipped.add((variant, s))
                    assert rule == "lsq" and (M[2] < k_pt if s else min(M[:2]) < k_md)
                else:
                    assert 0 <= want[1] <= sum(M)
    # the skip occurs for both solver types and all variants; nonmin never skips
    assert skipped == set(itertools.product(range(4), (0, 1)))
    # the defaults' sizes and 64-bit products
    assert [lib_size("lsq", 0, v, 7, 3, (300,) * 3)[1] for v in range(4)] == [294, 392, 392, 294]
    assert [lib_size("lsq", 1, v, 7, 3, (300,) * 3)[1] for v in range(4)] == [245, 294, 343, 245]
    assert [lib_size("lsq", 1, v, 2, 3, (300,) * 3)[1] for v in range(4)] == [20, 24, 28, 20]
    assert [lib_size("lsq", 0, v, 2, 3, (300,) * 3)[1] for v in range(4)] == [24, 32, 32, 24]
    assert [lib_size("nonmin", 0, v, 7, 3, (300,) * 3)[1] for v in range(4)] == [35, 36, 36, 35]
    big = (1 << 28,) * 3
    for rule, mu, nu in (("lsq", (1 << 31) - 1, 3), ("lsq", 1 << 12, 3), ("nonmin", 7, (1 << 31) - 1)):
        assert lib_size(rule, 1, 2, mu, nu, big) == Z.subset_size(rule, 1, 2, mu, nu, big)
    lib = L.lib()
    k, run = ctypes.c_int64(), ctypes.c_int32()
    s3 = (ctypes.c_int32 * 3)(1, 2, 3)
    for bad in ((2, 0, 0), (0, 2, 0), (0, 0, 4), (-1, 0, 0)):
        assert lib.mp_debug_lsq_subset_size(*bad, 7, 3, s3, ctypes.byref(k), ctypes.byref(run)) == L.MP_EINVAL
    assert lib.mp_debug_lsq_subset_size(0, 0, 0, 7, 3, None, ctypes.byref(k), ctypes.byref(run)) == L.MP_EINVAL
    assert lib.mp_debug_lsq_subset_size(0, 0, 0, 7, 3, (ctypes.c_int32 * 3)(1, -2, 3), ctypes.byref(k),
                                        ctypes.byref(run)) == L.MP_EINVAL


def test_step_schedule():
    assert [Z.step_factor(i, 4, 5.0) for i in range(4)] == [5.0, 5.0 - 4.0 / 3.0, 5.0 - 8.0 / 3.0, 1.0]
    assert Z.step_factor(0, 1, 5.0) == 5.0 and Z.step_factor(1, 2, 2.5) == 1.0
    assert Z.step_substream(2, 5) == 517


def test_headers_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of the headers needs ROCm's clang")
    exe = str(tmp_path / "lsq_subset_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", HOST, os.path.join(ROOT, "tests", "lsq_subset_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


# ---- the Python layer ----

def _fake_set():
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = 0, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = [20, 0, 7, 9, 9]
    ps._norm = np.ones(5)
    return ps


def test_python_checks_before_any_library_call(monkeypatch):
    ps = _fake_set()

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    for lo_steps in (0, -1, 65, 1.5, True, False, "2"):
        with pytest.raises(ValueError, match="lo_steps must be"):
            ps.ransac(budget=8, step=4, lo=1, lo_steps=lo_steps)
    with pytest.raises(ValueError, match="lo_steps needs lo"):
        ps.ransac(budget=8, step=4, lo_steps=1)
    with pytest.raises(ValueError, match="lo_steps needs lo"):
        ps.ransac(budget=8, lo_steps=1)
    # lo's own checks hold with lo_steps
    with pytest.raises(ValueError, match="lo needs step"):
        ps.ransac(budget=8, lo=1, lo_steps=1)
    with pytest.raises(ValueError, match="lo must be"):
        ps.ransac(budget=8, step=4, lo=0, lo_steps=1)
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 2 occurs twice"):
        ps.ransac(budget=8, step=4, lo=1, lo_steps=3, pair_ids=[2, 2])
    assert ps.ransac(budget=8, step=4, lo=1, lo_steps=64, pair_ids=[]) == []
    # lsq_fit
    m = madpose.PoseScaleOffset()
    with pytest.raises(ValueError, match="rule"):
        ps.lsq_fit([m] * 5, 0, rule="all")
    with pytest.raises(ValueError, match="one model per pair"):
        ps.lsq_fit([m] * 4, 0)
    with pytest.raises(ValueError, match="one model per entry"):
        ps.lsq_fit([m] * 2, 0, pair_ids=[1, 1, 1])
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 5 is outside"):
        ps.lsq_fit([m] * 2, 0, pair_ids=[1, 5])
    with pytest.raises(ValueError, match="solver_types"):
        ps.lsq_fit([m] * 2, [0, 2], pair_ids=[1, 1])
    with pytest.raises(ValueError, match="solver_types"):
        ps.lsq_fit([m] * 2, [0], pair_ids=[1, 1])
    with pytest.raises(ValueError, match="solver_types"):
        ps.lsq_fit([m] * 2, 0.5, pair_ids=[1, 1])
    for factor in (0.0, -1.0, float("nan"), float("inf"), [1.0, 0.0]):
        with pytest.raises(ValueError, match="factor"):
            ps.lsq_fit([m] * 2, 0, factor=factor, pair_ids=[1, 1])
    with pytest.raises(ValueError, match="streams"):
        ps.lsq_fit([m] * 2, 0, streams=-1, pair_ids=[1, 1])
    with pytest.raises(ValueError, match="streams"):
        ps.lsq_fit([m] * 2, 0, streams=1 << 31, pair_ids=[1, 1])
    with pytest.raises(ValueError, match="substreams"):
        ps.lsq_fit([m] * 2, 0, substreams=[0, 1 << 30], pair_ids=[1, 1])
    with pytest.raises(ValueError, match="seed"):
        ps.lsq_fit([m] * 2, 0, seed=-1, pair_ids=[1, 1])
    with pytest.raises(ValueError, match="entry_chunk"):
        ps.lsq_fit([m] * 2, 0, entry_chunk=-1, pair_ids=[1, 1])
    assert ps.lsq_fit([], 0, pair_ids=[]) == []


class _Recorder:
    """stands in for the library: records every call, answers MP_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return L.MP_OK
        return fn


def test_the_python_layer_calls_the_right_entry(monkeypatch):
    ps = _fake_set()
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    # without lo_steps: mp_ransac_lo_set with today's arguments (16 of them, in today's order)
    ps.ransac(budget=64, step=16, seed=9, rounds=2, lo=3, sample_chunk=5, model_chunk=6)
    (name, args), = rec.calls
    assert name == "mp_ransac_lo_set" and len(args) == 16
    assert args[1] == 5 and args[2] is None and args[3:9] == (64, 16, 9, -1, 2, 3) and args[14:] == (5, 6)
    assert isinstance(args[13], ctypes.Array) and args[13]._type_ is L.mp_ransac_lo_info
    # with it: the new entry, lo_steps after lo_rounds, the steps' info after the lo info
    rec.calls.clear()
    out = ps.ransac(budget=64, step=16, seed=9, rounds=2, lo=3, lo_steps=4, sample_chunk=5, model_chunk=6)
    (name, args), = rec.calls
    assert name == "mp_ransac_lo_steps_set" and len(args) == 18
    assert args[3:10] == (64, 16, 9, -1, 2, 3, 4) and args[16:] == (5, 6)
    assert args[14]._type_ is L.mp_ransac_lo_info and args[15]._type_ is L.mp_ransac_lo_steps_info
    assert len(out) == 5 and all((r.lo_step, r.lo_stage, r.lo_step_offers, r.lo_step_accepted) == (0, 0, 0, 0)
                                 for r in out)  # (the recorder's zeroed structs, read back)
    # the other modes are untouched
    rec.calls.clear()
    ps.ransac(budget=64, step=16)
    ps.ransac(budget=64)
    assert [c[0] for c in rec.calls] == ["mp_ransac_adaptive_set", "mp_ransac_set"]
    # lsq_fit accepts a repeated pair id and passes the entries as given
    rec.calls.clear()
    m = madpose.PoseScaleOffset()
    out = ps.lsq_fit([m] * 4, [0, 1, 1, 0], factor=2.5, rule="nonmin", seed=7, streams=3, substreams=[0, 1, 2, 256],
                     pair_ids=[2, 2, 0, 2], with_subsets=True, entry_chunk=1)
    (name, args), = rec.calls
    assert name == "mp_lsq_fit_set" and len(args) == 13
    assert args[1] == 4 and args[5] == 1 and args[6] == 7 and args[12] == 1
    as_list = lambda p, n: [p[i] for i in range(n)]
    assert as_list(args[2], 4) == [2, 2, 0, 2] and as_list(args[3], 4) == [0, 1, 1, 0]
    assert as_list(args[4], 4) == [2.5] * 4 and as_list(args[7], 4) == [3] * 4
    assert as_list(args[8], 4) == [0, 1, 2, 256]
    assert len(out) == 4 and all(len(r.subsets) == 3 for r in out)
    # the stages that share their list buffers still refuse a repeat
    with pytest.raises(ValueError, match="occurs twice"):
        ps.refine([m] * 2, pair_ids=[2, 2])
    with pytest.raises(ValueError, match="occurs twice"):
        ps.select([[m]] * 2, pair_ids=[2, 2])


def _empty_set(variant=0, use_shift=True, **opts):
    o, c = synthetic.example_options("calibrated")
    for k, v in opts.items():
        setattr(o, k, v)
    c.use_shift = use_shift
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


def test_bad_arguments_are_einval_before_any_device():
    lib = L.lib()
    ps = _empty_set()
    h = ps._h
    mods, res = (L.mp_model * 2)(), (L.mp_ransac_result * 2)()
    stopped = (ctypes.c_int32 * 2)()
    info, sinfo = (L.mp_ransac_lo_info * 2)(), (L.mp_ransac_lo_steps_info * 2)()
    ok = lambda **kw: lib.mp_ransac_lo_steps_set(*[kw.get(k, d) for k, d in (
        ("set", h), ("num_sel", 0), ("pair_ids", None), ("budget", 64), ("step", 16), ("seed", 0), ("share", -1),
        ("rounds", 3), ("lo", 1), ("lo_steps", 3), ("models", mods), ("results", res), ("inl", None),
        ("stopped", stopped), ("info", info), ("sinfo", sinfo), ("sample_chunk", 0), ("model_chunk", 0))])
    assert ok() == L.MP_OK
    assert ok(lo_steps=1) == L.MP_OK and ok(lo_steps=64) == L.MP_OK and ok(sinfo=None) == L.MP_OK
    assert ok(set=None) == L.MP_EINVAL
    for lo_steps in (0, -1, 65):
        assert ok(lo_steps=lo_steps) == L.MP_EINVAL and b"lo_steps" in lib.mp_last_error()
    assert ok(num_sel=1, sinfo=None) == L.MP_EINVAL and b"steps_info" in lib.mp_last_error()
    # mp_ransac_lo_set's checks hold
    assert ok(lo=0) == L.MP_EINVAL and b"lo_rounds" in lib.mp_last_error()
    assert ok(num_sel=1, info=None) == L.MP_EINVAL and b"lo_info" in lib.mp_last_error()
    assert ok(step=0) == L.MP_EINVAL and ok(budget=-1) == L.MP_EINVAL and ok(rounds=65) == L.MP_EINVAL
    assert ok(num_sel=1) == L.MP_EINVAL  # (the selection, which an empty set refuses)
    # mp_lsq_fit_set on the empty set: no entry is the only legal call
    lres = (L.mp_lsq_fit_result * 2)()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)
    fit = lambda **kw: lib.mp_lsq_fit_set(*[kw.get(k, d) for k, d in (
        ("set", h), ("n", 0), ("ids", None), ("types", i32(0, 0)), ("factors", f64(1.0, 1.0)), ("rule", 0),
        ("seed", 0), ("streams", i32(0, 0)), ("substreams", i32(0, 0)), ("models", mods), ("results", lres),
        ("idx", None), ("chunk", 0))])
    assert fit() == L.MP_OK and fit(rule=1, chunk=3) == L.MP_OK
    assert fit(set=None) == L.MP_EINVAL
    assert fit(n=-1) == L.MP_EINVAL and fit(rule=2) == L.MP_EINVAL and fit(rule=-1) == L.MP_EINVAL
    assert fit(chunk=-1) == L.MP_EINVAL and b"entry_chunk" in lib.mp_last_error()
    assert fit(n=1) == L.MP_EINVAL and b"pair count" in lib.mp_last_error()
    assert fit(n=2, ids=i32(0, 0)) == L.MP_EINVAL and b"outside the set" in lib.mp_last_error()
    ps.close()
    with _empty_set(num_lsq_iterations=255) as ps2:
        assert lib.mp_ransac_lo_steps_set(ps2._h, 0, None, 8, 4, 0, -1, 1, 1, 1, mods, res, None, None, info, sinfo, 0,
                                          0) == L.MP_EINVAL
        assert b"num_lsq_iterations" in lib.mp_last_error()


@pytest.mark.parametrize("variant,kw,word", [(3, {}, b"MP_SCALE_ONLY"), (0, dict(use_shift=False), b"use_shift")])
def test_unsupported_sets_are_einval(variant, kw, word):
    lib = L.lib()
    ps = _empty_set(variant, **kw)
    mods, res = (L.mp_model * 1)(), (L.mp_ransac_result * 1)()
    info, sinfo = (L.mp_ransac_lo_info * 1)(), (L.mp_ransac_lo_steps_info * 1)()
    assert lib.mp_ransac_lo_steps_set(ps._h, 0, None, 8, 4, 0, -1, 1, 1, 2, mods, res, None, None, info, sinfo, 0,
                                      0) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    with pytest.raises(ValueError, match="scale only|use_shift"):
        ps.ransac(budget=8, step=4, lo=1, lo_steps=2)
    # lsq_fit has refine's support: these sets take it
    assert ps.lsq_fit([], 0) == []
    ps.close()


def test_empty_set_needs_no_device():
    with _empty_set() as ps:
        assert ps.ransac(budget=8, step=3, lo=2, lo_steps=3) == []
        assert ps.lsq_fit([], [], rule="nonmin") == []
