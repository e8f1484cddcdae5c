"""The set, the weights and the expectations behind tests/test_draw_weighted_gpu.py, and the
checks of device-given weights, which run in a process of their own.

PairSet.draw_weights takes the weights as per-pair host arrays or as one array that is already
on the device; the tests make the latter with torch, which must be imported before the library
is loaded (tests/pair_set_ingest_worker.py has the full story).  `python -m
tests.draw_weighted_worker` imports torch first, runs every check (or those named on the command
line) and prints one JSON object {name: {"ok": bool, "seconds": s, "detail": text}} as its last
line.  A check is a function that raises AssertionError like a test.

The reference of every check is tests/weighted_draw_restatement.py: the tables, the flags and
the draws are compared with it bit for bit."""
import ctypes
import functools
import os
import sys

import numpy as np

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import refine_cases as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restatement as D  # noqa: E402
import weighted_draw_restatement as WD  # noqa: E402

SEED = 0x5EEDC0DEC0FFEE01
BUDGET = 130  # two 64-sample items and a remainder
CAP = L.DRAW_STAGE_ENTRIES  # the table entries (n + 1) the sampler reads through LDS at most

CHECKS = {}


def check(*params):
    """register a check, once per parameter tuple"""
    def reg(fn):
        name = fn.__name__.replace("check_", "", 1)
        for p in params or [()]:
            CHECKS[name + ("[" + "-".join(str(v) for v in p) + "]" if p else "")] = (fn, p)
        return fn
    return reg


def sizes(variant):
    """n = 2; k_md - 1, k_md, k_pt - 1, k_pt; 63, 64, 65, 300, 65535; tables of CAP - 1, CAP and
    CAP + 1 entries; then the special pairs: 64 (one positive weight short: falls back), 300
    (not given weights), 700 (every weight 0: falls back), 300 (given: neighbours of the rest)"""
    k_md, k_pt = D.sizes(variant)
    return (2, k_md - 1, k_md, k_pt - 1, k_pt, 63, 64, 65, 300, 65535, CAP - 2, CAP - 1, CAP, 64, 300, 700, 300)


SHORT, NOT_GIVEN, ALL_ZERO = 13, 14, 15  # the special pairs' positions
SUBSET = [16, 9, 13, 2, 14, 11, 0, 12]   # a permuted subset


def _pair(variant, i, n):
    p = RC.make_pair(variant, 2100 + i, max(n, 8))
    for key in ("x0", "x1", "depth0", "depth1", "inlier_mask"):
        p[key] = p[key][:n]
    return p


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(variant, dtype="float64"):
    """The pairs (never changed), their weights -- {0, 2^-17 (q = 0), 2^-16, random, 1.0} mixed,
    of `dtype` -- and what the restatement says of them."""
    k = Case()
    k.variant, k.dtype = variant, np.dtype(dtype)
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.sizes = sizes(variant)
    k.pairs = [_pair(variant, i, n) for i, n in enumerate(k.sizes)]
    k_md, k_pt = D.sizes(variant)
    rng = np.random.default_rng(77 + variant)
    k.weights = []
    for i, n in enumerate(k.sizes):
        w = rng.random(n)
        kind = rng.integers(0, 5, n)
        if n == 65535:  # (W above 2^31: the proposal's product needs all 64 bits)
            w = 0.5 + 0.5 * w
        elif n >= 63:
            w[kind == 0] = 0.0
            w[kind == 1] = 2.0 ** -17
            w[kind == 2] = 2.0 ** -16
            w[kind == 4] = 1.0
        w = w.astype(k.dtype)
        if i == SHORT:  # k_max - 1 positive weights
            w[:] = 0
            w[rng.permutation(n)[:k_pt - 1]] = 0.5
        if i == ALL_ZERO:
            w[:] = 0
        k.weights.append(None if i == NOT_GIVEN else w)
    k.tables = [None if w is None else WD.table(w) for w in k.weights]
    k.positive = np.array([0 if t is None else t[1] for t in k.tables])
    k.total = np.array([0 if t is None else int(t[0][-1]) for t in k.tables])
    k.weighted = np.array([t is not None and WD.is_weighted(variant, n, t[1]) for t, n in zip(k.tables, k.sizes)])
    return k


@functools.lru_cache(maxsize=None)
def expected_draw(variant, dtype, share, budget=BUDGET):
    """(types, idx) per pair by the restatement"""
    k = case(variant, dtype)
    out = []
    for i, n in enumerate(k.sizes):
        T, I, _ = WD.draw_any(variant, n, k.weights[i], SEED, share, i, budget)
        out.append((T, I))
    return out


def check_case(k):
    """the case holds what it is meant to (on the restatement alone)"""
    k_md, k_pt = D.sizes(k.variant)
    want = [n >= k_md for n in k.sizes]
    want[SHORT] = want[NOT_GIVEN] = want[ALL_ZERO] = False
    assert k.weighted.tolist() == want, k.weighted.tolist()
    assert k.positive[SHORT] == k_pt - 1 and k.positive[ALL_ZERO] == 0 and k.total[ALL_ZERO] == 0
    assert k.total[9] > 1 << 31  # (the largest pair's W needs all 32 bits)
    assert sum(len(p["depth0"]) for p in k.pairs) == sum(k.sizes)


def check_object(k, w):
    assert w.weighted.dtype == bool and w.weighted.tolist() == k.weighted.tolist()
    assert w.positive.tolist() == k.positive.tolist()
    assert w.total.tolist() == k.total.tolist()


def skey(dr):
    return [(t.tobytes(), i.tobytes()) for t, i in dr]


def check_draw(k, ps, w, shares=(128,)):
    for share in shares:
        want = expected_draw(k.variant, k.dtype.name, share)
        got = ps.draw(BUDGET, SEED, point_share=share, weights=w)
        for i, (g, e) in enumerate(zip(got, want)):
            assert g[0].shape == e[0].shape and g[1].shape == e[1].shape, (share, i)
            assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), (share, i, k.sizes[i])
    # the pairs that fell back, and the one not given weights, draw today's bytes
    plain = ps.draw(BUDGET, SEED, point_share=shares[-1])
    for i in (SHORT, NOT_GIVEN, ALL_ZERO):
        assert skey([got[i]]) == skey([plain[i]]), i
    assert skey(got) != skey(plain)


# ---- the checks of device-given weights (the child process) ----

def _torch():
    import torch
    return torch


def _device_weights(k, fill=0.25):
    """one tensor over the whole set; the rows of the pair not given weights hold `fill`"""
    torch = _torch()
    host = np.concatenate([np.full(n, fill, dtype=k.dtype) if w is None else w for w, n in zip(k.weights, k.sizes)])
    given = np.array([w is not None for w in k.weights])
    return torch.as_tensor(host).to("cuda"), given, host


@check((0, "float32"), (0, "float64"), (1, "float32"), (1, "float64"), (2, "float32"), (2, "float64"))
def check_device_weights_equal_the_restatement(variant, dtype):
    k = case(variant, dtype)
    t, given, host = _device_weights(k)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as ps:
        with ps.draw_weights(t, given=given) as w:
            check_object(k, w)
            check_draw(k, ps, w)
            # the same tables as the host-given ones: the same draws under another share
            with ps.draw_weights(k.weights) as wh:
                assert skey(ps.draw(17, SEED, point_share=40, weights=w)) == \
                    skey(ps.draw(17, SEED, point_share=40, weights=wh))
        assert np.array_equal(t.cpu().numpy(), host)  # only read


@check()
def check_weights_produced_on_another_stream():
    """the weights are written by a kernel queued on a side stream behind a long one; the build
    waits for that stream on the device"""
    torch = _torch()
    k = case(0, "float64")
    _, given, host = _device_weights(k)
    side = torch.cuda.Stream()
    src = torch.as_tensor(host).to("cuda")
    torch.cuda.synchronize()
    with madpose.PairSet(0, k.pairs, k.o, k.c) as ps:
        with torch.cuda.stream(side):
            big = torch.ones(4096, 4096, device="cuda")
            for _ in range(20):
                big = big @ big * 1e-4
            t = torch.zeros_like(src)
            t += src
        with ps.draw_weights(t, stream=side, given=given) as w:
            check_object(k, w)
            check_draw(k, ps, w)
        torch.cuda.synchronize()


@check()
def check_inputs_are_not_referenced_afterwards():
    torch = _torch()
    k = case(0, "float32")
    t, given, _ = _device_weights(k)
    with madpose.PairSet(0, k.pairs, k.o, k.c) as ps:
        w = ps.draw_weights(t, given=given)
        t.fill_(float("nan"))  # (a later change does not reach the tables)
        del t
        torch.cuda.empty_cache()
        check_draw(k, ps, w)
        w.close()


@check()
def check_bad_device_weights_are_refused_by_the_library():
    torch = _torch()
    lib = L.lib()
    k = case(0, "float64")
    t, given, host = _device_weights(k)
    T = host.shape[0]
    with madpose.PairSet(0, k.pairs, k.o, k.c) as ps:
        h = ps._h
        base = (ctypes.c_int64 * 2)()
        L.check(lib.mp_debug_device_extent(t.data_ptr(), 0, base))
        mask = np.ascontiguousarray(given, dtype=np.uint8)
        mp = mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        wh = ctypes.c_void_p()
        # T - 2 elements left in the allocation from this address on
        code = lib.mp_draw_weights_create(h, base[0] + base[1] - 8 * (T - 2), 1, 1, mp, None, ctypes.byref(wh))
        assert code == L.MP_EINVAL and not wh.value and b"weights" in lib.mp_last_error(), lib.mp_last_error()
        # not aligned to the element type; host memory passed as device memory
        assert lib.mp_draw_weights_create(h, t.data_ptr() + 4, 1, 1, mp, None, ctypes.byref(wh)) == L.MP_EINVAL
        assert lib.mp_draw_weights_create(h, host.ctypes.data, 1, 1, mp, None, ctypes.byref(wh)) == L.MP_EINVAL
        assert not wh.value
        # a bad value: the lowest offending row of the set is named, rows of pairs not given are ignored
        off = np.concatenate([[0], np.cumsum(k.sizes)])
        bad = t.clone()
        bad[int(off[NOT_GIVEN]) + 3] = float("nan")
        assert lib.mp_draw_weights_create(h, bad.data_ptr(), 1, 1, mp, None, ctypes.byref(wh)) == L.MP_OK
        assert lib.mp_draw_weights_destroy(wh) == L.MP_OK
        rows = [int(off[9]) + 40000, int(off[5]) + 7, int(off[16]) + 1]
        for r, v in zip(rows, (float("inf"), -0.5, 1.0000001)):
            bad[r] = v
        code = lib.mp_draw_weights_create(h, bad.data_ptr(), 1, 1, mp, None, ctypes.byref(wh))
        assert code == L.MP_EINVAL and f"weights[{min(rows)}]".encode() in lib.mp_last_error(), lib.mp_last_error()
        try:
            ps.draw_weights(bad, given=given)
            raise AssertionError("a bad device weight was accepted")
        except ValueError as e:
            assert f"weights[{min(rows)}]" in str(e) and "pair 5" in str(e)
        # a pair above 65535 correspondences may not be given weights (checked before any launch)
        # -- and the whole array, once more, is taken
        with ps.draw_weights(t, given=given) as w:
            check_object(k, w)


def main(argv):
    import io
    import json
    import time
    import traceback
    from contextlib import redirect_stdout
    torch = _torch()  # before the library is loaded: one HIP runtime in the process
    torch.cuda.init()
    out = {}
    for name in argv or list(CHECKS):
        fn, params = CHECKS[name]
        buf, t0 = io.StringIO(), time.perf_counter()
        try:
            with redirect_stdout(buf):
                fn(*params)
            out[name] = {"ok": True, "detail": buf.getvalue()}
        except Exception as e:
            out[name] = {"ok": False, "detail": buf.getvalue() + traceback.format_exc()[-6000:]}
            stop = not isinstance(e, (AssertionError, ValueError))
        else:
            stop = False
        out[name]["seconds"] = round(time.perf_counter() - t0, 3)
        print(name, "ok" if out[name]["ok"] else "FAILED", out[name]["seconds"], flush=True)
        if stop:  # (a device error: nothing more is started on the GPU after it)
            break
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
