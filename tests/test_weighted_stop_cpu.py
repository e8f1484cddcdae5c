"""The weighted stopping rule without a device: mp_debug_ransac_required_mass equals its
restatement (tests/weighted_stop_restatement.py) and, for a pair that is not weighted or has equal
weights, mp_debug_ransac_required; mp_debug_inlier_mass_host equals numpy; ransac_stop.h's new
function and the host gather pass their stand-alone check under AddressSanitizer and UBSan
(tests/weighted_stop_check.cpp); the Python checks come before any library call; and the C entries
refuse a handle of another set, a closed handle and step = 0 on sets whose device does not exist."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weighted_stop_restatement as WS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
BIG = 65535 * 65535
u32p = ctypes.POINTER(ctypes.c_uint32)


def _c_options(sp, mn, mx):
    o, _ = synthetic.example_options("calibrated")
    o.success_probability, o.min_num_iterations, o.max_num_iterations_per_solver = sp, mn, mx
    return o._to_c()


def _lib_required_mass(variant, total, mass, opts):
    m = None if mass is None else (ctypes.c_uint32 * 3)(*mass)
    req = (ctypes.c_uint32 * 2)()
    assert L.lib().mp_debug_ransac_required_mass(variant, total, m, ctypes.byref(opts), req) == L.MP_OK
    return [int(req[0]), int(req[1])]


def _lib_required(variant, n, counts, opts):
    c = (ctypes.c_int32 * 3)(*counts)
    req = (ctypes.c_uint32 * 2)()
    assert L.lib().mp_debug_ransac_required(variant, n, c, ctypes.byref(opts), req) == L.MP_OK
    return [int(req[0]), int(req[1])]


def test_symbols_header_and_layout():
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "madpose_mi355x.h")) as f:
        header = f.read()
    for name in ("mp_inlier_mass_set", "mp_ransac_weighted_stop_set", "mp_debug_ransac_required_mass",
                 "mp_debug_inlier_mass_host", "mp_debug_inlier_mass_stats"):
        assert hasattr(lib, name) and name in L.EXPORTS and f"int {name}(" in header, name
    assert ctypes.sizeof(L.mp_inlier_mass) == 32
    r = madpose.RansacResult()
    assert r.rule_mass is None and r.rule_total == 0
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "host", "ransac_stop.h")) as f:
        stop = f.read()
    assert "#include <hip" not in stop and "__global__" not in stop  # plain C++
    assert "required_samples_mass" in stop


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_required_mass_equals_restatement(variant):
    checked = 0
    for sp, mn, mx in itertools.product((0.5, 0.99, 0.999999, 1.0), (0, 8, 100), (50, 10000)):
        opts = _c_options(sp, mn, mx)
        for total in (0, 1, 5, 300, 65535, 90 * 65535 + 210 * 3276, BIG):
            lattice = sorted(x for x in {0, 1, 2, total // 4, total // 2, (4 * total) // 5, total - 1, total}
                             if 0 <= x <= total)
            for mass in itertools.product(lattice, repeat=3):
                want = WS.required_mass(variant, total, mass, sp, mn, mx)
                assert _lib_required_mass(variant, total, mass, opts) == want, (sp, mn, mx, total, mass)
                assert all(min(mn, mx) <= w <= max(mn, mx) for w in want)
                checked += 1
            # NULL mass: no winner
            assert _lib_required_mass(variant, total, None, opts) == WS.required_mass(variant, total, None, sp, mn, mx)
            assert _lib_required_mass(variant, total, None, opts) == [mx] * 2  # (the bound as it stands)
    assert checked > 5000
    opts = _c_options(0.99, 8, 10000)
    # total = 0 (with any mass the entry accepts: 0), mass = 0, mass = total
    assert _lib_required_mass(variant, 0, (0, 0, 0), opts) == [10000, 10000]
    assert _lib_required_mass(variant, BIG, (0, 0, 0), opts) == [10000, 10000]
    assert _lib_required_mass(variant, BIG, (BIG, BIG, BIG), opts) == [8, 8]
    # mass = 1 of 65535^2: 1 - r^k is 1 in double, the p_bad bound, not a converted integer
    assert _lib_required_mass(variant, BIG, (1, 1, 1), opts) == [10000, 10000]
    assert _lib_required_mass(variant, BIG, (BIG, BIG, 1), opts) == [8, 10000]


def test_the_issues_table():
    """300 correspondences, 90 true matches, confidences 1.0 / 0.05, min_num_iterations = 8"""
    opts = _c_options(0.99, 8, 10000)
    q_in, q_out = 65535, int(np.floor(0.05 * 65536))
    W = 90 * q_in + 210 * q_out
    assert abs(90 * q_in / W - 0.895) < 1e-3
    want = {0: ([6316, 1894], [8, 8]), 1: ([10000, 6316], [10, 8]), 2: ([10000, 10000], [10, 8])}
    for v, (by_count, by_mass) in want.items():
        assert _lib_required(v, 300, (90, 90, 90), opts) == by_count
        assert _lib_required_mass(v, W, (90 * q_in,) * 3, opts) == by_mass


@pytest.mark.parametrize("q", [1, 1000, 65535])
def test_equal_weights_give_the_count_rule(q):
    rng = np.random.default_rng(20 + q)
    for k in range(3000):
        n = int(rng.integers(1, 65536))
        counts = [int(c) for c in rng.integers(0, n + 1, size=3)]
        if k % 10 == 0:
            counts[k % 3] = n
        variant = int(rng.integers(0, 3))
        opts = _c_options((0.99, 0.999999, 0.5)[k % 3], int(rng.integers(0, 20)), int(rng.integers(50, 100000)))
        assert (_lib_required_mass(variant, q * n, [q * c for c in counts], opts)
                == _lib_required(variant, n, counts, opts)), (n, counts, variant)


def test_required_mass_bad_arguments():
    lib = L.lib()
    opts = _c_options(0.99, 8, 10000)
    m = (ctypes.c_uint32 * 3)(1, 1, 1)
    req = (ctypes.c_uint32 * 2)()
    assert lib.mp_debug_ransac_required_mass(3, 10, m, ctypes.byref(opts), req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required_mass(-1, 10, m, ctypes.byref(opts), req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required_mass(0, 10, m, None, req) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required_mass(0, 10, m, ctypes.byref(opts), None) == L.MP_EINVAL
    assert lib.mp_debug_ransac_required_mass(0, 0, m, ctypes.byref(opts), req) == L.MP_EINVAL  # mass above total
    assert lib.mp_debug_ransac_required_mass(0, 10, None, ctypes.byref(opts), req) == L.MP_OK


def _lib_mass(cum, lists):
    n = len(cum) - 1
    cum = np.ascontiguousarray(cum, dtype=np.uint32)
    offs = np.zeros(4, dtype=np.int64)
    for t in range(3):
        offs[t + 1] = offs[t] + len(lists[t])
    idx = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32) for a in lists]).astype(np.int32))
    mass = (ctypes.c_uint32 * 3)(7, 7, 7)
    rc = L.lib().mp_debug_inlier_mass_host(n, cum.ctypes.data_as(u32p), offs.ctypes.data_as(L.c_int64_p),
                                           idx.ctypes.data_as(L.c_int32_p) if len(idx) else None, mass)
    return rc, [int(v) for v in mass]


def test_host_gather_equals_numpy():
    rng = np.random.default_rng(5)
    # empty lists
    cum = np.concatenate([[0], np.cumsum(rng.integers(0, 65536, size=40))])
    assert _lib_mass(cum, [[], [], []]) == (L.MP_OK, [0, 0, 0])
    assert _lib_mass(np.zeros(1), [[], [], []]) == (L.MP_OK, [0, 0, 0])  # n = 0
    # full lists of n = 65535 with all q = 65535: 4294836225, no wrap
    n = 65535
    cum = np.arange(n + 1, dtype=np.int64) * 65535
    full = np.arange(n, dtype=np.int32)
    assert _lib_mass(cum, [full, full, full]) == (L.MP_OK, [4294836225] * 3)
    assert 4294836225 == 65535 * 65535 < 1 << 32
    # random lists
    for k in range(200):
        n = int(rng.integers(1, 900))
        q = rng.integers(0, 65536, size=n)
        q[rng.random(n) < 0.2] = 0
        q[rng.random(n) < 0.1] = 65535
        cum = np.concatenate([[0], np.cumsum(q)])
        lists = [np.flatnonzero(rng.random(n) < f).astype(np.int32) for f in (0.1, 0.5, 0.95)]
        assert _lib_mass(cum, lists) == (L.MP_OK, [int(q[a].sum()) for a in lists]), k


def test_host_gather_bad_arguments():
    cum = np.array([0, 3, 3, 10])
    assert _lib_mass(cum, [[0, 1], [2], []])[0] == L.MP_OK
    assert _lib_mass(cum, [[1, 0], [2], []])[0] == L.MP_EINVAL  # not ascending
    assert _lib_mass(cum, [[0, 0], [2], []])[0] == L.MP_EINVAL  # a row twice
    assert _lib_mass(cum, [[0, 3], [2], []])[0] == L.MP_EINVAL  # outside 0 .. n - 1
    assert _lib_mass(cum, [[-1], [2], []])[0] == L.MP_EINVAL
    assert _lib_mass(np.array([1, 3, 3, 10]), [[0], [], []])[0] == L.MP_EINVAL  # cum[0] != 0
    assert _lib_mass(np.array([0, 3, 2, 10]), [[0], [], []])[0] == L.MP_EINVAL  # falls
    assert _lib_mass(np.array([0, 65536]), [[0], [], []])[0] == L.MP_EINVAL  # a rise above 65535
    mass = (ctypes.c_uint32 * 3)()
    offs = np.zeros(4, dtype=np.int64)
    assert L.lib().mp_debug_inlier_mass_host(65536, None, offs.ctypes.data_as(L.c_int64_p), None, mass) == L.MP_EINVAL


def test_rule_and_gather_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of ransac_stop.h needs ROCm's clang")
    exe = str(tmp_path / "weighted_stop_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "weighted_stop_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")


def test_python_checks_before_any_library_call(monkeypatch):
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = 0, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = [20, 0, 7]
    ps._norm = np.ones(3)
    w = madpose.DrawWeights.__new__(madpose.DrawWeights)
    w._set, w._h = ps, ctypes.c_void_p(2)
    closed = madpose.DrawWeights.__new__(madpose.DrawWeights)
    closed._set, closed._h = ps, None
    other = madpose.DrawWeights.__new__(madpose.DrawWeights)
    other._set, other._h = object(), ctypes.c_void_p(3)

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="weighted_stop must be a bool"):
            ps.ransac(budget=8, step=4, weights=w, weighted_stop=bad)
    with pytest.raises(ValueError, match="weighted_stop needs weights"):
        ps.ransac(budget=8, step=4, weighted_stop=True)
    with pytest.raises(ValueError, match="weighted_stop needs step"):
        ps.ransac(budget=8, weights=w, weighted_stop=True)
    with pytest.raises(ValueError, match="closed"):
        ps.ransac(budget=8, step=4, weights=closed, weighted_stop=True)
    with pytest.raises(ValueError, match="another PairSet"):
        ps.ransac(budget=8, step=4, weights=other, weighted_stop=True)
    assert ps.ransac(budget=8, step=4, weights=w, weighted_stop=True, pair_ids=[]) == []
    m = madpose.PoseScaleOffset()
    with pytest.raises(ValueError, match="one model per pair"):
        ps.inlier_mass([m], w)
    with pytest.raises(ValueError, match="one model per entry"):
        ps.inlier_mass([m], w, pair_ids=[0, 0])
    with pytest.raises(ValueError, match=r"pair_ids\[1\] = 3 is outside"):
        ps.inlier_mass([m, m], w, pair_ids=[0, 3])
    with pytest.raises(ValueError, match="closed"):
        ps.inlier_mass([m], closed, pair_ids=[0])
    with pytest.raises(ValueError, match="weights must be"):
        ps.inlier_mass([m], None, pair_ids=[0])
    assert ps.inlier_mass([], w, pair_ids=[]) == []


def _empty_set():
    o, c = synthetic.example_options("calibrated")
    return madpose.PairSet(0, [], o, c, device=NO_DEVICE)


def test_c_entries_refuse_bad_handles_and_step_zero():
    lib = L.lib()
    with _empty_set() as ps, _empty_set() as ps2:
        w, w2, gone = ps.draw_weights([]), ps2.draw_weights([]), ps.draw_weights([])
        gone_h = gone._h
        gone.close()
        mods, res = (L.mp_model * 2)(), (L.mp_ransac_result * 2)()
        stopped, rm = (ctypes.c_int32 * 2)(), (L.mp_inlier_mass * 2)()
        info, sinfo = (L.mp_ransac_lo_info * 2)(), (L.mp_ransac_lo_steps_info * 2)()
        call = lambda **kw: lib.mp_ransac_weighted_stop_set(*[kw.get(k, d) for k, d in (
            ("set", ps._h), ("handle", w._h), ("num_sel", 0), ("pair_ids", None), ("budget", 64), ("step", 16),
            ("seed", 0), ("share", -1), ("rounds", 3), ("lo", 0), ("lo_steps", 0), ("models", mods), ("results", res),
            ("inl", None), ("stopped", stopped), ("info", info), ("sinfo", sinfo), ("sample_chunk", 0),
            ("model_chunk", 0), ("rule_mass", rm))])
        assert call() == L.MP_OK and call(rule_mass=None) == L.MP_OK
        assert call(lo=1) == L.MP_OK and call(lo=1, lo_steps=2) == L.MP_OK
        assert call(step=0) == L.MP_EINVAL and b"step" in lib.mp_last_error()
        assert call(step=-1) == L.MP_EINVAL
        assert call(handle=None) == L.MP_EINVAL and call(set=None) == L.MP_EINVAL
        assert call(handle=w2._h) == L.MP_EINVAL and b"another pair set" in lib.mp_last_error()
        assert call(handle=gone_h) == L.MP_EINVAL and b"not a live" in lib.mp_last_error()
        # the chosen body's own refusals
        assert call(budget=-1) == L.MP_EINVAL and b"budget" in lib.mp_last_error()
        assert call(rounds=65) == L.MP_EINVAL and call(lo=65) == L.MP_EINVAL
        assert call(lo_steps=2) == L.MP_EINVAL and b"lo_rounds" in lib.mp_last_error()
        assert call(lo=1, lo_steps=65) == L.MP_EINVAL
        assert call(num_sel=1) == L.MP_EINVAL
        # the stage's entry
        mass = lambda **kw: lib.mp_inlier_mass_set(*[kw.get(k, d) for k, d in (
            ("set", ps._h), ("handle", w._h), ("n", 0), ("pair_ids", None), ("models", mods), ("out", rm))])
        assert mass() == L.MP_OK
        assert mass(set=None) == L.MP_EINVAL and mass(handle=None) == L.MP_EINVAL
        assert mass(handle=w2._h) == L.MP_EINVAL and b"another pair set" in lib.mp_last_error()
        assert mass(handle=gone_h) == L.MP_EINVAL and b"not a live" in lib.mp_last_error()
        assert mass(n=-1) == L.MP_EINVAL and mass(n=(1 << 24) + 1) == L.MP_EINVAL
        assert mass(n=1) == L.MP_EINVAL  # (an empty set has no pair 0)
        ids = (ctypes.c_int32 * 1)(0)
        assert mass(n=1, pair_ids=ids) == L.MP_EINVAL and b"outside the set" in lib.mp_last_error()
        assert ps.inlier_mass([], w) == []
        assert ps.ransac(budget=8, step=3, weights=w, weighted_stop=True) == []
        # a destroyed set invalidates its handles for the new entries too
        with _empty_set() as ps3:
            w3 = ps3.draw_weights([])
        assert mass(handle=w3._h) == L.MP_EINVAL and b"destroyed" in lib.mp_last_error()
        assert call(handle=w3._h) == L.MP_EINVAL and b"destroyed" in lib.mp_last_error()
        w.close(), w2.close(), w3.close()


def test_stats_hook_counts_nothing_without_a_device():
    n, ms = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    assert L.lib().mp_debug_inlier_mass_stats(ctypes.byref(n), ctypes.byref(ms), 1) == L.MP_OK
    assert L.lib().mp_debug_inlier_mass_stats(ctypes.byref(n), ctypes.byref(ms), 0) == L.MP_OK
    assert n.value == 0 and ms.value == 0.0
