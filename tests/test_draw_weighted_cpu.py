"""The confidence-weighted draw (mp_draw_weights_*, mp_draw_weighted_set, mp_ransac_weighted_set;
PairSet.draw_weights, draw(weights=), ransac(weights=)) without a device: the symbols and constants
agree between the header, madpose_amd/_lib.py and the library; the host side of the rule
(madpose_amd/csrc/include/mp_draw.h draw_sample_weighted, mp_draw_weights.h draw_quantise, through
mp_debug_draw_weights_host / mp_debug_draw_weighted_host) equals the Python restatement
(tests/weighted_draw_restatement.py) bit for bit; equal weights reproduce the uniform draw; masked
correspondences never appear; the fill is the restatement's; first-slot frequencies follow q_i / W;
every bad argument is MP_EINVAL on a set whose device does not exist; and the Python checks raise
before the library is touched.  The host side of the rule also passes a stand-alone check under
AddressSanitizer and UBSan on tables of exactly n + 1 entries (tests/draw_weighted_check.cpp)."""
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
import weighted_draw_restatement as WD  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
NO_DEVICE = 10 ** 6  # no such device: a call that reached it would not return MP_EINVAL
SEED = 0x1234567890ABCDEF
SYMBOLS = ("mp_draw_weights_create", "mp_draw_weights_info", "mp_draw_weights_destroy", "mp_draw_weighted_set",
           "mp_ransac_weighted_set", "mp_debug_draw_weights_host", "mp_debug_draw_weighted_host")
u32p = ctypes.POINTER(ctypes.c_uint32)


def _empty_set(variant=0, use_shift=True):
    """An open set of no pairs (needs no device)."""
    o, c = synthetic.example_options("calibrated")
    c.use_shift = use_shift
    return madpose.PairSet(variant, [], o, c, device=NO_DEVICE)


def _fake_set(variant=0, sizes=(20, 0, 7)):
    """A PairSet object as creation leaves it, without the library (the Python checks)."""
    ps = madpose.PairSet.__new__(madpose.PairSet)
    ps.variant, ps.device, ps._hyp_error = variant, 0, None
    ps._h = ctypes.c_void_p(1)
    ps._sizes = list(sizes)
    ps._norm = np.ones(len(sizes))
    return ps


def _host_table(weights):
    """(code, cum uint32 (n + 1,), positive) of mp_debug_draw_weights_host"""
    w = np.ascontiguousarray(weights)
    n = w.shape[0]
    cum = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32)
    pos = ctypes.c_int32(-1)
    code = L.lib().mp_debug_draw_weights_host(n, w.ctypes.data, 0 if w.dtype == np.float32 else 1,
                                              cum.ctypes.data_as(u32p), ctypes.byref(pos))
    return code, cum, pos.value


def _host_draw(variant, cum, seed, share, pair, budget):
    """(types, idx, fill) of samples 0 .. budget - 1 through mp_debug_draw_weighted_host"""
    cum = np.ascontiguousarray(cum, dtype=np.uint32)
    out = (ctypes.c_int32 * 10)()
    rows = np.zeros((budget, 10), dtype=np.int32)
    fn = L.lib().mp_debug_draw_weighted_host
    ptr = cum.ctypes.data_as(u32p)
    for s in range(budget):
        assert fn(variant, cum.shape[0] - 1, ptr, seed, share, pair, s, out) == L.MP_OK
        rows[s] = out
    return rows[:, 0], rows[:, 1:9], rows[:, 9].astype(bool)


def _mixed_weights(n, dtype, rng):
    """weights drawn from {0, 2^-17 (q = 0), 2^-16 (q = 1), random, 1.0 (q = 65535)}"""
    w = rng.random(n)
    kind = rng.integers(0, 5, n)
    w[kind == 0] = 0.0
    w[kind == 1] = 2.0 ** -17
    w[kind == 2] = 2.0 ** -16
    w[kind == 4] = 1.0
    return w.astype(dtype)


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
    assert define("MP_DRAW_WEIGHT_MAX_N") == L.DRAW_WEIGHT_MAX_N == WD.MAX_N == 65535
    assert define("MP_DRAW_STAGE_ENTRIES") == L.DRAW_STAGE_ENTRIES
    with open(os.path.join(ROOT, "madpose_amd", "csrc", "include", "mp_draw.h")) as f:
        draw = f.read()
    assert f"kDrawWeightMaxN = {L.DRAW_WEIGHT_MAX_N};" in draw and f"kDrawStageEntries = {L.DRAW_STAGE_ENTRIES};" in draw
    assert madpose.DrawWeights is not None and callable(madpose.PairSet.draw_weights)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_table_equals_restatement(dtype):
    rng = np.random.default_rng(11)
    for n in (1, 3, 4, 5, 7, 64, 65, 1000, 65535):
        w = _mixed_weights(n, dtype, rng)
        code, cum, pos = _host_table(w)
        assert code == L.MP_OK
        want, want_pos = WD.table(w)
        assert (cum.astype(np.int64) == want).all() and pos == want_pos
    # the quantisation's edges, one by one
    edge = np.array([0.0, 2.0 ** -17, 2.0 ** -16, 1.0, 1.0 - 2.0 ** -17, 0.5, np.nextafter(dtype(2.0 ** -16), dtype(0))],
                    dtype=dtype)
    code, cum, pos = _host_table(edge)
    assert code == L.MP_OK and np.diff(cum.astype(np.int64)).tolist() == [0, 0, 1, 65535, 65535, 32768, 0] and pos == 4
    # all ones at the largest size: W = 65535^2 < 2^32
    code, cum, pos = _host_table(np.ones(65535, dtype=dtype))
    assert code == L.MP_OK and int(cum[-1]) == 65535 * 65535 and pos == 65535


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_host_draw_equals_restatement(variant):
    rng = np.random.default_rng(100 + variant)
    k_md, k_pt = D.sizes(variant)
    budget = 300
    for share in (0, 128, 256):
        for n in (k_md, k_pt, 64, 1000):
            w = _mixed_weights(n, np.float64, rng)
            w[rng.permutation(n)[:min(n, k_pt)]] = rng.random(min(n, k_pt)) * 0.5 + 0.25  # enough positive ones
            cum, n_pos = WD.table(w)
            assert WD.is_weighted(variant, n, n_pos)
            T, I, F = WD.draw_pair(variant, cum, SEED, share, 5, budget)
            gT, gI, gF = _host_draw(variant, cum, SEED, share, 5, budget)
            assert (gT == T).all() and (gI == I).all() and (gF == F).all()
            kk = np.where(T == 1, k_pt, k_md)
            q = np.diff(cum)
            for s in range(budget):
                row = I[s, :kk[s]]
                assert len(set(row.tolist())) == kk[s] and row.min() >= 0 and row.max() < n
                assert (q[row] > 0).all() and (I[s, kk[s]:] == 0).all()
            if n < k_pt:
                assert (T == 0).all()


@pytest.mark.parametrize("q", [1, 1000, 65535])
def test_equal_weights_reproduce_the_uniform_draw(q):
    """all q_i = q > 0: i = floor(floor(w n q / 2^32) / q) = floor(w n / 2^32), fill included"""
    out = (ctypes.c_int32 * 10)()
    fills = 0
    for variant in (0, 1, 2):
        k_md, k_pt = D.sizes(variant)
        for n in (k_md, k_pt, 64, 700):
            w = np.full(n, 1.0 if q == 65535 else q / 65536.0)
            code, cum, pos = _host_table(w)
            assert code == L.MP_OK and pos == n and int(cum[-1]) == n * q
            for share in (0, 128, 256):
                # (n = k = 7 needs some thousand samples for the 64 words to run out once)
                budget = 4096 if (variant, n, share) == (2, 7, 256) else 300
                gT, gI, gF = _host_draw(variant, cum, SEED, share, 9, budget)
                for s in range(budget):
                    assert L.lib().mp_debug_draw_host(variant, n, SEED, share, 9, s, out) == L.MP_OK
                    assert [gT[s]] + gI[s].tolist() + [int(gF[s])] == list(out), (variant, n, share, s)
                fills += int(gF.sum())
    assert fills >= 1  # (n = k = 7: the 64-word fallback occurs)


def test_masked_indices_never_appear():
    rng = np.random.default_rng(5)
    n = 200
    w = rng.random(n)
    masked = rng.permutation(n)[:150]
    w[masked[:75]] = 0.0
    w[masked[75:]] = 2.0 ** -17
    cum, n_pos = WD.table(w)
    assert n_pos == 50
    for variant in (0, 1, 2):
        T, I, F = _host_draw(variant, cum, SEED, 128, 2, 300)
        kk = np.where(T == 1, D.sizes(variant)[1], D.sizes(variant)[0])
        used = np.concatenate([I[s, :kk[s]] for s in range(300)])
        assert not np.isin(used, masked).any()


def test_fill_matches_restatement():
    """one weight 1.0 and 299 of 2^-16: nearly every proposal is index 0, so most samples end in
    the ascending fill over the positive weights"""
    w = np.full(300, 2.0 ** -16)
    w[137] = 1.0
    cum, n_pos = WD.table(w)
    assert n_pos == 300 and int(cum[-1]) == 65535 + 299
    for variant in (0, 1, 2):
        T, I, F = WD.draw_pair(variant, cum, SEED, 128, 0, 300)
        gT, gI, gF = _host_draw(variant, cum, SEED, 128, 0, 300)
        assert (gT == T).all() and (gI == I).all() and (gF == F).all()
        assert F.mean() > 0.5
        assert (I[F, 0] == 137).all()
    # with masked ones in between, the fill skips them
    w[:5] = 0.0
    cum, _ = WD.table(w)
    T, I, F = WD.draw_pair(0, cum, SEED, 0, 0, 300)
    gT, gI, gF = _host_draw(0, cum, SEED, 0, 0, 300)
    assert (gI == I).all() and (gF == F).all() and F.any()
    assert I[:, :3].min() >= 5 and (I[F, 1] == 5).any()


def test_first_slot_frequencies():
    """20 000 samples over 16 distinct weights: each index's first-slot count within 5 binomial
    standard deviations of N q_i / W (deterministic under the fixed seed)"""
    n, N = 16, 20000
    w = (np.arange(n) + 1.0) / 20.0
    cum, _ = WD.table(w)
    q = np.diff(cum).astype(np.float64)
    assert len(set(q.tolist())) == n
    p = q / q.sum()
    _, I, _ = _host_draw(0, cum, SEED, 0, 3, N)
    counts = np.bincount(I[:, 0], minlength=n)
    for i in range(n):
        assert abs(counts[i] - N * p[i]) <= 5.0 * np.sqrt(N * p[i] * (1.0 - p[i])), (i, counts[i], N * p[i])


def test_debug_hooks_bad_arguments():
    lib = L.lib()
    cum = np.zeros(11, dtype=np.uint32)
    pos = ctypes.c_int32(0)
    w = np.full(10, 0.5)
    tab = lambda n, ww, dt, c=cum, p=pos: lib.mp_debug_draw_weights_host(
        n, None if ww is None else ww.ctypes.data, dt, None if c is None else c.ctypes.data_as(u32p),
        None if p is None else ctypes.byref(p))
    assert tab(10, w, 1) == L.MP_OK
    assert tab(-1, w, 1) == L.MP_EINVAL
    assert tab(65536, w, 1) == L.MP_EINVAL and b"65535" in lib.mp_last_error()
    assert tab(10, w, 2) == L.MP_EINVAL and b"dtype" in lib.mp_last_error()
    assert tab(10, None, 1) == L.MP_EINVAL
    assert tab(10, w, 1, c=None) == L.MP_EINVAL
    assert tab(10, w, 1, p=None) == L.MP_EINVAL
    for bad in (np.nan, np.inf, -np.inf, -1e-300, np.nextafter(1.0, 2.0), 2.0):
        ww = w.copy()
        ww[7] = bad
        ww[9] = bad
        assert tab(10, ww, 1) == L.MP_EINVAL and b"weights[7]" in lib.mp_last_error(), bad
    w32 = w.astype(np.float32)
    w32[3] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert tab(10, w32, 0) == L.MP_EINVAL and b"weights[3]" in lib.mp_last_error()
    assert tab(10, np.full(10, -0.0), 1) == L.MP_OK and pos.value == 0  # (-0 is 0)

    out = (ctypes.c_int32 * 10)()
    good, _ = WD.table(w)
    good = good.astype(np.uint32)
    drw = lambda v=0, n=10, c=good, share=128, pair=0, s=0, o=out: lib.mp_debug_draw_weighted_host(
        v, n, None if c is None else c.ctypes.data_as(u32p), 0, share, pair, s, o)
    assert drw() == L.MP_OK
    assert drw(v=3) == L.MP_EINVAL
    assert drw(n=-1) == L.MP_EINVAL
    assert drw(n=65536) == L.MP_EINVAL
    assert drw(c=None) == L.MP_EINVAL
    assert drw(share=257) == L.MP_EINVAL and drw(share=-1) == L.MP_EINVAL
    assert drw(pair=-1) == L.MP_EINVAL and drw(s=-1) == L.MP_EINVAL
    assert drw(o=None) == L.MP_EINVAL
    c = good.copy()
    c[0] = 1
    assert drw(c=c) == L.MP_EINVAL and b"cum[0]" in lib.mp_last_error()
    c = good.copy()
    c[5] = c[4] - 1
    assert drw(c=c) == L.MP_EINVAL
    c = good.copy()
    c[10] = c[9] + 65536
    assert drw(c=c) == L.MP_EINVAL
    few, n_pos = WD.table(np.array([0.5, 0, 0, 0.5, 0, 0.5, 0, 0.5, 0, 0]))  # 4 positive of 10: k_pt = 5
    assert n_pos == 4
    assert drw(c=few.astype(np.uint32)) == L.MP_EINVAL and b"not a weighted pair" in lib.mp_last_error()
    assert drw(n=2, c=good[:3].copy()) == L.MP_EINVAL  # a pair too small for the MD solver is never weighted


def test_bad_arguments_are_einval_before_any_device():
    lib = L.lib()
    ps, other = _empty_set(), _empty_set()
    h = ps._h
    i32 = lambda k: (ctypes.c_int32 * k)()
    mods, res = (L.mp_model * 2)(), (L.mp_ransac_result * 2)()
    info, sinfo = (L.mp_ransac_lo_info * 2)(), (L.mp_ransac_lo_steps_info * 2)()
    wh, wo = ctypes.c_void_p(), ctypes.c_void_p()
    # ---- create / info ----
    assert lib.mp_draw_weights_create(None, None, 1, 0, None, None, ctypes.byref(wh)) == L.MP_EINVAL
    assert lib.mp_draw_weights_create(h, None, 1, 0, None, None, None) == L.MP_EINVAL
    assert lib.mp_draw_weights_create(h, None, 2, 0, None, None, ctypes.byref(wh)) == L.MP_EINVAL
    assert b"dtype" in lib.mp_last_error() and not wh.value
    assert lib.mp_draw_weights_create(h, None, 1, 0, None, None, ctypes.byref(wh)) == L.MP_OK and wh.value
    assert lib.mp_draw_weights_create(other._h, None, 0, 1, None, None, ctypes.byref(wo)) == L.MP_OK and wo.value
    assert lib.mp_draw_weights_info(None, None, None, None) == L.MP_EINVAL
    assert lib.mp_draw_weights_info(wh, None, None, None) == L.MP_OK
    assert lib.mp_draw_weights_info(ctypes.c_void_p(12345), None, None, None) == L.MP_EINVAL  # never a handle
    # ---- the draw ----
    draw = lambda s=h, w=wh, ns=0, budget=1, share=-1: lib.mp_draw_weighted_set(s, w, ns, None, budget, 0, share,
                                                                                 i32(8), i32(64), i32(1))
    assert draw() == L.MP_OK
    assert draw(s=None) == L.MP_EINVAL
    assert draw(w=None) == L.MP_EINVAL and b"null draw weights" in lib.mp_last_error()
    assert draw(w=wo) == L.MP_EINVAL and b"another pair set" in lib.mp_last_error()
    assert draw(budget=-1) == L.MP_EINVAL and b"budget" in lib.mp_last_error()
    assert draw(share=257) == L.MP_EINVAL and b"point_share" in lib.mp_last_error()
    assert draw(ns=1) == L.MP_EINVAL
    assert draw(ns=3, budget=(1 << 22) // 3 + 1) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    # ---- ransac: one entry over the four bodies, each with its own refusals ----
    run = lambda **kw: lib.mp_ransac_weighted_set(*[kw.get(k, d) for k, d in (
        ("set", h), ("w", wh), ("num_sel", 0), ("pair_ids", None), ("budget", 4), ("step", 0), ("seed", 0),
        ("share", -1), ("rounds", 3), ("lo", 0), ("lo_steps", 0), ("models", mods), ("results", res), ("inl", None),
        ("stopped", None), ("info", info), ("sinfo", sinfo), ("sample_chunk", 0), ("model_chunk", 0))])
    for mode in (dict(), dict(step=2), dict(step=2, lo=1), dict(step=2, lo=1, lo_steps=2)):
        assert run(**mode) == L.MP_OK, mode
        assert run(set=None, **mode) == L.MP_EINVAL
        assert run(w=None, **mode) == L.MP_EINVAL and b"null draw weights" in lib.mp_last_error()
        assert run(w=wo, **mode) == L.MP_EINVAL and b"another pair set" in lib.mp_last_error()
        assert run(rounds=65, **mode) == L.MP_EINVAL and b"rounds" in lib.mp_last_error()
        assert run(rounds=-1, **mode) == L.MP_EINVAL
        assert run(budget=-1, **mode) == L.MP_EINVAL
        assert run(share=257, **mode) == L.MP_EINVAL
        assert run(sample_chunk=-1, **mode) == L.MP_EINVAL
        assert run(model_chunk=-1, **mode) == L.MP_EINVAL
        assert run(num_sel=1, **mode) == L.MP_EINVAL
    assert run(num_sel=3, budget=(1 << 22) // 3 + 1) == L.MP_EINVAL and b"2^22" in lib.mp_last_error()
    assert run(lo=1) == L.MP_EINVAL and b"need step" in lib.mp_last_error()            # lo without step
    assert run(lo_steps=1) == L.MP_EINVAL
    assert run(step=2, lo_steps=1) == L.MP_EINVAL and b"lo_steps needs lo_rounds" in lib.mp_last_error()
    assert run(step=-1) == L.MP_EINVAL and b"step" in lib.mp_last_error()
    assert run(step=2, budget=(1 << 20) + 1) == L.MP_EINVAL and b"2^20" in lib.mp_last_error()
    assert run(step=2, lo=65) == L.MP_EINVAL and b"lo_rounds" in lib.mp_last_error()
    assert run(step=2, lo=-1) == L.MP_EINVAL
    assert run(step=2, lo=1, num_sel=1, info=None) == L.MP_EINVAL and b"lo_info" in lib.mp_last_error()
    assert run(step=2, lo=1, lo_steps=65) == L.MP_EINVAL and b"lo_steps" in lib.mp_last_error()
    assert run(step=2, lo=1, lo_steps=1, num_sel=1, sinfo=None) == L.MP_EINVAL and b"steps_info" in lib.mp_last_error()
    # ---- lifetime: destroying the set invalidates its handles; destroying them is still fine ----
    ps.close()
    assert lib.mp_draw_weights_info(wh, None, None, None) == L.MP_EINVAL and b"destroyed" in lib.mp_last_error()
    assert draw(s=other._h, w=wh) == L.MP_EINVAL and b"destroyed" in lib.mp_last_error()
    assert run(set=other._h, w=wh) == L.MP_EINVAL
    assert lib.mp_draw_weights_destroy(wh) == L.MP_OK
    assert lib.mp_draw_weights_destroy(wh) == L.MP_EINVAL  # (no longer a handle; nothing is dereferenced)
    assert draw(s=other._h, w=wh) == L.MP_EINVAL
    assert lib.mp_draw_weights_destroy(None) == L.MP_OK
    assert draw(s=other._h, w=wo) == L.MP_OK
    assert lib.mp_draw_weights_destroy(wo) == L.MP_OK
    other.close()


@pytest.mark.parametrize("variant,use_shift,word", [(3, True, b"MP_SCALE_ONLY"), (0, False, b"use_shift")])
def test_unsupported_sets_are_einval(variant, use_shift, word):
    lib = L.lib()
    ps = _empty_set(variant, use_shift)
    wh = ctypes.c_void_p()
    assert lib.mp_draw_weights_create(ps._h, None, 1, 0, None, None, ctypes.byref(wh)) == L.MP_EINVAL
    assert word in lib.mp_last_error()
    with pytest.raises(ValueError, match="scale only|use_shift"):
        ps.draw_weights([])
    ps.close()


def test_python_object_on_an_empty_set():
    ps, other = _empty_set(), _empty_set()
    with ps.draw_weights([]) as w:
        assert w.weighted.shape == w.positive.shape == w.total.shape == (0,)
        assert ps.draw(4, 0, weights=w) == [] and ps.ransac(budget=4, weights=w) == []
        assert ps.ransac(budget=4, step=2, lo=1, lo_steps=1, weights=w) == []
        with pytest.raises(ValueError, match="another PairSet"):
            other.draw(4, 0, weights=w)
    w.close()  # idempotent
    with pytest.raises(ValueError, match="closed"):
        ps.draw(4, 0, weights=w)
    w2 = ps.draw_weights([])
    ps.close()  # the set first, then the weights
    w2.close()
    other.close()


def test_python_checks_before_any_library_call(monkeypatch):
    ps = _fake_set()
    smp = (np.zeros(0, dtype=np.int32), np.zeros((0, 8), dtype=np.int32))
    w = madpose.DrawWeights.__new__(madpose.DrawWeights)
    w._set, w._h = ps, ctypes.c_void_p(2)
    closed = madpose.DrawWeights.__new__(madpose.DrawWeights)
    closed._set, closed._h = ps, None

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "lib", boom)
    good = [np.full(20, 0.5), None, np.full(7, 0.25, dtype=np.float32)]
    bad = lambda i, v: [v if j == i else g for j, g in enumerate(good)]
    with pytest.raises(ValueError, match="one weights entry per pair"):
        ps.draw_weights(good[:2])
    with pytest.raises(ValueError, match="sequence"):
        ps.draw_weights(0.5)
    with pytest.raises(ValueError, match=r"weights\[0\] must be 1-D with the pair's 20 values"):
        ps.draw_weights(bad(0, np.full(19, 0.5)))
    with pytest.raises(ValueError, match=r"weights\[0\] must be 1-D"):
        ps.draw_weights(bad(0, np.full((20, 1), 0.5)))
    with pytest.raises(ValueError, match=r"weights\[2\] must be float32 or float64"):
        ps.draw_weights(bad(2, np.ones(7, dtype=np.int32)))
    with pytest.raises(ValueError, match=r"weights\[2\] must be float32 or float64"):
        ps.draw_weights(bad(2, np.ones(7, dtype=np.float16)))
    with pytest.raises(ValueError, match=r"weights\[0\] must be C-contiguous"):
        ps.draw_weights(bad(0, np.full(40, 0.5)[::2]))
    for v in (np.nan, np.inf, -0.25, 1.5):
        a = np.full(20, 0.5)
        a[11] = v
        a[15] = v
        with pytest.raises(ValueError, match=r"weights\[0\]\[11\]"):
            ps.draw_weights(bad(0, a))
    with pytest.raises(ValueError, match="given and stream go with a device array"):
        ps.draw_weights(good, given=[1, 0, 1])
    big = _fake_set(sizes=(65536,))
    with pytest.raises(ValueError, match="at most 65535"):
        big.draw_weights([np.full(65536, 0.5)])

    class Dev:  # a device array by its interface only
        def __init__(self, shape, typestr="<f8", strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(4096, False), version=2,
                                                 strides=strides)
    with pytest.raises(ValueError, match=r"weights must have shape \(27,\)"):
        ps.draw_weights(Dev((26,)))
    with pytest.raises(ValueError, match="float32 or float64"):
        ps.draw_weights(Dev((27,), "<i4"))
    with pytest.raises(ValueError, match="C-contiguous"):
        ps.draw_weights(Dev((27,), "<f8", (16,)))
    with pytest.raises(ValueError, match="given must hold one bool"):
        ps.draw_weights(Dev((27,)), given=[1, 0])
    with pytest.raises(ValueError, match="stream must be"):
        ps.draw_weights(Dev((27,)), stream="s")
    with pytest.raises(ValueError, match="at most 65535"):
        big.draw_weights(Dev((65536,)))
    # draw / ransac
    with pytest.raises(ValueError, match="weights must be None or the object"):
        ps.draw(4, 0, weights=good)
    with pytest.raises(ValueError, match="closed"):
        ps.draw(4, 0, weights=closed)
    with pytest.raises(ValueError, match="another PairSet"):
        _fake_set().draw(4, 0, weights=w)
    with pytest.raises(ValueError, match="weights go with a budget"):
        ps.ransac(samples=[smp] * 3, weights=w)
    with pytest.raises(ValueError, match="weights must be None or the object"):
        ps.ransac(budget=4, weights=[None] * 3)
    with pytest.raises(ValueError, match="closed"):
        ps.ransac(budget=4, step=2, weights=closed)
    with pytest.raises(ValueError, match="budget"):
        ps.ransac(budget=-1, weights=w)
    with pytest.raises(ValueError, match="lo needs step"):
        ps.ransac(budget=4, lo=1, weights=w)
    with pytest.raises(ValueError, match="rounds"):
        ps.ransac(budget=4, rounds=65, weights=w)
    w._h = closed._h = None
    ps._h = big._h = None  # (nothing to destroy)


def test_rule_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail(f"{CLANG} missing: the host build of mp_draw.h needs ROCm's clang")
    exe = str(tmp_path / "draw_weighted_check")
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "madpose_amd", "csrc", "include"),
           os.path.join(ROOT, "tests", "draw_weighted_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
