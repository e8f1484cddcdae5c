"""mp_draw_set / mp_candidates_set / mp_ransac_set (PairSet.draw / candidates / ransac) without
a device: the symbols, constants and header agree with madpose_amd/_lib.py; every bad
argument is MP_EINVAL on a set whose device does not exist, so nothing reached a device; the
host side of madpose_amd/csrc/include/mp_draw.h equals a Python restatement of Philox4x32-10
and the index rule (tests/draw_restatement.py), itself held to the published Philox4x32-10
known-answer vectors; and host/candidates_plan.h passes its stand-alone check under
AddressSanitizer and UBSan (tests/candidates_plan_check.cpp)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restatement as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
SYMBOLS = ("mp_draw_set", "mp_debug_draw_host", "mp_candidates_set", "mp_candidates_fetch", "mp_ransac_set",
           "mp_debug_ransac_timing")
SEED = 0x1234567890ABCDEF


def _options(solver=0, use_shift=True):
    o, c = synthetic.example_options("calibrated")
    c.solver_type = solver
    c.use_shift = use_shift
    return o, c


def _empty_set(variant=0, **kw):
    """An open set of no pairs (needs no device)."""
    o, c = _options(**kw)
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


def _fake_set(variant=0, sizes=(20, 0, 7)):
    """A PairSet object as creation leaves it, without the library (the Python checks)."""
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = variant, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = list(sizes)
    ps._norm = np.ones(len(sizes))
    return ps


def test_symbols_constants_and_header():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTS, name
        assert f"int {name}(" in header, name

    def define(name):
        line, = [ln for ln in header.splitlines() if ln.startswith(f"#define {name} ")]
        return int(line.split()[2])
    assert define("MP_DRAW_BLOCKS") == L.DRAW_BLOCKS == D.BLOCKS == 16
    assert define("MP_DRAW_POINT_SHARE_MAX") == L.DRAW_POINT_SHARE_MAX == 256
    assert define("MP_RANSAC_TIMING_VALUES") == L.RANSAC_TIMING_VALUES
    assert "} mp_ransac_result; /* 80 bytes */" in header
    assert ctypes.sizeof(L.mp_ransac_result) == 80
    # the struct's fields, in the header's order
    body = header[header.index("typedef struct mp_ransac_result {"):header.index("} mp_ransac_result;")]
    names = [w.strip(" ;,").split("[")[0] for ln in body.splitlines()[1:] for w in ln.split(";")[0].split(",")]
    names = [n.split()[-1] for n in names if n]
    assert names == [f[0] for f in L.mp_ransac_result._fields_]
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "include", "mp_draw.h")) as f:
        draw = f.read()
    for const in ("0xD2511F53u", "0xCD9E8D57u", "0x9E3779B9u", "0xBB67AE85u", "kDrawBlocks = 16;", "kDrawShareMax = 256;"):
        assert const in draw, const
    assert "double" not in draw and "float" not in draw.replace("floating point", "")  # integer-only
    assert madpose.RansacResult is not None
    for name in ("draw", "candidates", "ransac"):
        assert callable(getattr(madpose.PairSet, name))


def test_philox_known_answers():
    """The published Philox4x32-10 known-answer vectors (Random123 kat_vectors: counter and
    key all zero, all ones, and the digits of pi)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in D.philox4x32_10(*ctr, *key)) == want


def _host(variant, n, seed, share, pair, s):
    out = (ctypes.c_int32 * 10)()
    assert L.lib().mp_debug_draw_host(variant, n, seed, share, pair, s, out) == L.MP_OK
    return list(out)


def test_host_draw_block0_is_philox():
    """Counter (s, 0, pair, 0), key (seed low, seed high): with n = 2^28 and point_share 256
    the first slot is (word 1 * n) >> 32 and the type bit is word 0's top byte."""
    n = 1 << 28
    for seed, pair, s in ((0, 0, 0), (SEED, 3, 17), ((1 << 64) - 1, 1499, 511)):
        w = [int(x) for x in D.philox4x32_10(s, 0, pair, 0, seed & 0xFFFFFFFF, seed >> 32)]
        for share in (0, 1, 77, 128, 255, 256):
            o = _host(0, n, seed, share, pair, s)
            assert o[0] == (1 if (w[0] >> 24) < share else 0)
            assert o[1] == (w[1] * n) >> 32 and o[2] == (w[2] * n) >> 32 and o[3] == (w[3] * n) >> 32


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_host_draw_equals_restatement(variant):
    k_md, k_pt = D.sizes(variant)
    budget = 4096
    fills = {}
    for k, share in ((k_md, 0), (k_pt, 256), (k_pt, 128)):
        for n in (k, k + 1, 64, 700):
            T, I, F = D.draw_pair(variant, n, SEED, share, 5, budget)
            assert T.shape == (budget,)
            got = np.array([_host(variant, n, SEED, share, 5, s) for s in range(budget)], dtype=np.int32)
            assert (got[:, 0] == T).all()
            assert (got[:, 1:9] == I).all()
            assert (got[:, 9] == F.astype(np.int32)).all()
            kk = np.where(T == 1, k_pt, k_md)
            for s in range(budget):
                row = I[s, :kk[s]]
                assert len(set(row.tolist())) == kk[s] and row.min() >= 0 and row.max() < n
                assert (I[s, kk[s]:] == 0).all()
            if n == k:  # every sample of its type is a permutation of 0 .. k - 1
                for s in np.nonzero(kk == k)[0]:
                    assert sorted(I[s, :k].tolist()) == list(range(k))
            if n < k_pt:
                assert (T == 0).all()
            fills[(k, n)] = int(F.sum())
    if variant == 2:
        assert fills[(7, 7)] >= 1  # the 64-word fallback is covered: n = k = 7
    # a pair too small for the MD solver has no sample
    assert _host(variant, k_md - 1, SEED, 128, 0, 0) == [-1] + [0] * 9
    assert D.draw_pair(variant, k_md - 1, SEED, 128, 0, 8)[0].shape == (0,)


def test_debug_draw_host_bad_arguments():
    out = (ctypes.c_int32 * 10)()
    lib = L.lib()
    assert lib.mp_debug_draw_host(3, 10, 0, 128, 0, 0, out) == L.MP_EINVAL
    assert lib.mp_debug_draw_host(0, -1, 0, 128, 0, 0, out) == L.MP_EINVAL
    assert lib.mp_debug_draw_host(0, 10, 0, 257, 0, 0, out) == L.MP_EINVAL
    assert lib.mp_debug_draw_host(0, 10, 0, -1, 0, 0, out) == L.MP_EINVAL
    assert lib.mp_debug_draw_host(0, 10, 0, 128, -1, 0, out) == L.MP_EINVAL
    assert lib.mp_debug_draw_host(0, 10, 0, 128, 0, 0, None) == L.MP_EINVAL
    assert lib.mp_debug_ransac_timing(None) == L.MP_EINVAL


def test_bad_arguments_are_einval_before_any_device():
    """On an open set whose device is number 10^6: a call that got as far as the device would
    return MP_EDEVICE (or fault), not MP_EINVAL."""
    lib = L.lib()
    ps = _empty_set()
    h = ps._h
    i32 = lambda k: (ctypes.c_int32 * k)()
    i64 = lambda k: (ctypes.c_int64 * k)()
    mods, res = (L.mp_model * 2)(), (L.mp_ransac_result * 2)()
    nm = ctypes.c_int64(-1)
    # null set
    assert lib.mp_draw_set(None, 0, None, 1, 0, -1, i32(8), i32(64), i32(1)) == L.MP_EINVAL
    assert lib.mp_candidates_set(None, 0, None, None, None, None, 0, ctypes.byref(nm)) == L.MP_EINVAL
    assert lib.mp_candidates_fetch(None, None, None, None, None) == L.MP_EINVAL
    assert lib.mp_ransac_set(None, 0, None, 1, 0, -1, None, None, None, 1, mods, res, None, 0, 0) == L.MP_EINVAL
    # the draw's own refusals
    assert lib.mp_draw_set(h, 0, None, -1, 0, -1, i32(8), i32(64), i32(1)) == L.MP_EINVAL       # negative budget
    assert b"budget" in lib.mp_last_error()
    assert lib.mp_draw_set(h, 0, None, 1, 0, 257, i32(8), i32(64), i32(1)) == L.MP_EINVAL       # point_share 257
    assert b"point_share" in lib.mp_last_error()
    assert lib.mp_draw_set(h, 0, None, 1, 0, -2, i32(8), i32(64), i32(1)) == L.MP_EINVAL
    assert lib.mp_draw_set(h, 3, None, (1 << 22) // 3 + 1, 0, -1, None, None, None) == L.MP_EINVAL  # the 2^22 bound
    assert b"2^22" in lib.mp_last_error()
    assert lib.mp_draw_set(h, 1, None, 1, 0, -1, i32(8), i32(64), i32(1)) == L.MP_EINVAL        # num_sel != pair count
    assert lib.mp_draw_set(h, 0, None, 1, 0, -1, None, None, None) == L.MP_OK                    # (no pairs: nothing to do)
    # candidates
    assert lib.mp_candidates_set(h, 0, None, None, None, None, 0, None) == L.MP_EINVAL           # null num_models
    assert lib.mp_candidates_set(h, 0, None, None, None, None, -1, ctypes.byref(nm)) == L.MP_EINVAL
    assert lib.mp_candidates_set(h, 1, None, None, None, None, 0, ctypes.byref(nm)) == L.MP_EINVAL
    assert lib.mp_candidates_fetch(h, None, i64(1), None, None) == L.MP_EINVAL                   # nothing to fetch
    assert b"mp_candidates_set first" in lib.mp_last_error()
    assert lib.mp_candidates_set(h, 0, None, None, None, None, 0, ctypes.byref(nm)) == L.MP_OK and nm.value == 0
    assert lib.mp_candidates_fetch(h, None, None, None, None) == L.MP_EINVAL                     # null model_offsets
    mo = i64(1)
    mo[0] = -7
    assert lib.mp_candidates_fetch(h, None, mo, None, None) == L.MP_OK and mo[0] == 0
    assert lib.mp_candidates_fetch(h, None, mo, None, None) == L.MP_EINVAL                       # fetched: dropped
    # ransac
    ok = lambda **kw: lib.mp_ransac_set(*[kw.get(k, d) for k, d in (
        ("set", h), ("num_sel", 0), ("pair_ids", None), ("budget", 4), ("seed", 0), ("share", -1), ("soff", None),
        ("types", None), ("idx", None), ("rounds", 3), ("models", mods), ("results", res), ("inl", None),
        ("sample_chunk", 0), ("model_chunk", 0))])
    assert ok() == L.MP_OK
    assert ok(rounds=65) == L.MP_EINVAL and b"rounds" in lib.mp_last_error()
    assert ok(rounds=-1) == L.MP_EINVAL
    assert ok(rounds=0) == L.MP_OK
    assert ok(budget=-1) == L.MP_EINVAL                                   # neither a budget nor samples
    assert ok(budget=-2) == L.MP_EINVAL
    assert ok(soff=i64(1)) == L.MP_EINVAL and b"budget must be -1" in lib.mp_last_error()   # both
    assert ok(soff=i64(1), budget=-1) == L.MP_OK
    assert ok(types=i32(1)) == L.MP_EINVAL                                # samples without their offsets
    assert ok(share=257) == L.MP_EINVAL
    assert ok(num_sel=3, budget=(1 << 22) // 3 + 1) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    assert ok(sample_chunk=-1) == L.MP_EINVAL
    assert ok(model_chunk=-1) == L.MP_EINVAL
    assert ok(num_sel=1) == L.MP_EINVAL                                   # num_sel != the pair count
    ids = i32(2)
    assert ok(num_sel=2, pair_ids=ids) == L.MP_EINVAL and b"outside the set" in lib.mp_last_error()
    ps.close()


@pytest.mark.parametrize("variant,kw,word", [(3, {}, b"MP_SCALE_ONLY"), (0, dict(use_shift=False), b"use_shift")])
def test_unsupported_sets_are_einval(variant, kw, word):
    """a scale-only set (and one without the shift) is refused by all three entries, as
    mp_hypothesize_set refuses it"""
    lib = L.lib()
    ps = _empty_set(variant, **kw)
    h = ps._h
    nm = ctypes.c_int64(0)
    mods, res = (L.mp_model * 1)(), (L.mp_ransac_result * 1)()
    assert lib.mp_draw_set(h, 0, None, 1, 0, -1, None, None, None) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    assert lib.mp_candidates_set(h, 0, None, None, None, None, 0, ctypes.byref(nm)) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    assert lib.mp_ransac_set(h, 0, None, 1, 0, -1, None, None, None, 1, mods, res, None, 0, 0) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    for call in (lambda: ps.draw(1, 0), lambda: ps.candidates([]), lambda: ps.ransac(budget=1)):
        with pytest.raises(ValueError, match="scale only|use_shift"):
            call()
    ps.close()


def test_python_checks_before_any_library_call(monkeypatch):
    ps = _fake_set()
    smp = (np.zeros(0, dtype=np.int32), np.zeros((0, 8), dtype=np.int32))

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    with pytest.raises(ValueError, match="exactly one of budget and samples"):
        ps.ransac()
    with pytest.raises(ValueError, match="exactly one of budget and samples"):
        ps.ransac(budget=4, samples=[smp] * 3)
    for rounds in (65, -1, 1.5):
        with pytest.raises(ValueError, match="rounds"):
            ps.ransac(budget=4, rounds=rounds)
    with pytest.raises(ValueError, match="budget"):
        ps.ransac(budget=-1)
    with pytest.raises(ValueError, match="budget"):
        ps.draw(-1, 0)
    with pytest.raises(ValueError, match="2\\^22"):
        ps.draw((1 << 22) // 3 + 1, 0)
    with pytest.raises(ValueError, match="2\\^22"):
        ps.ransac(budget=(1 << 22) // 3 + 1)
    for share in (257, -1, 1.5):
        with pytest.raises(ValueError, match="point_share"):
            ps.draw(4, 0, point_share=share)
        with pytest.raises(ValueError, match="point_share"):
            ps.ransac(budget=4, point_share=share)
    with pytest.raises(ValueError, match="seed"):
        ps.draw(4, -1)
    with pytest.raises(ValueError, match="seed"):
        ps.ransac(budget=4, seed=1 << 64)
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 2 occurs twice"):
        ps.ransac(budget=4, pair_ids=[2, 2])
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 0 occurs twice"):
        ps.draw(4, 0, pair_ids=[0, 0])
    with pytest.raises(ValueError, match=r"pair_ids\[0\] = 3 is outside"):
        ps.candidates([smp], pair_ids=[3])
    with pytest.raises(ValueError, match=r"one \(types, idx\) per selected pair"):
        ps.candidates([smp])
    with pytest.raises(ValueError, match=r"one \(types, idx\) per selected pair"):
        ps.ransac(samples=[smp, smp], pair_ids=[0])
    with pytest.raises(ValueError, match="sample_chunk"):
        ps.candidates([smp] * 3, sample_chunk=-1)
    with pytest.raises(ValueError, match="sample_chunk"):
        ps.ransac(budget=1, sample_chunk=-1)
    with pytest.raises(ValueError, match="model_chunk"):
        ps.ransac(budget=1, model_chunk=-1)
    one = (np.ones(1, dtype=np.int32), np.arange(8, dtype=np.int32)[None])
    with pytest.raises(ValueError, match="too few"):
        ps.ransac(samples=[one], pair_ids=[1])
    assert ps.draw(4, 0, pair_ids=[]) == [] and ps.candidates([], pair_ids=[]) == []
    assert ps.ransac(budget=4, pair_ids=[]) == [] and ps.ransac(samples=[], pair_ids=[]) == []
    ps._h = None
    for call in (lambda: ps.draw(1, 0), lambda: ps.candidates([smp] * 3), lambda: ps.ransac(budget=1)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_empty_set_needs_no_device():
    with _empty_set() as ps:
        assert ps.draw(8, 1) == [] and ps.candidates([]) == []
        assert ps.ransac(budget=8) == [] and ps.ransac(samples=[]) == []


def test_plan_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of candidates_plan.h needs ROCm's clang")
    exe = str(tmp_path / "candidates_plan_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "candidates_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
