"""The checks of tests/test_pair_set_ingest_gpu.py, run in a process of their own.

PairSet.from_device takes arrays that are already on the device, and the tests make them with
torch.  torch ships a HIP runtime of its own, and a process can drive the GPU through one HIP
runtime only: the library binds to the runtime that is loaded first, so torch must be imported
before the library is loaded.  The pytest process has usually loaded the
library long before this module's tests run, so the checks run here: `python -m
tests.pair_set_ingest_worker` imports torch first, runs every check (or those named on the
command line), and prints one JSON object {name: {"ok": bool, "seconds": s, "detail": text}}
as its last line.  A check is a function that raises AssertionError like a test.

Every check compares against the host-built PairSet of the same numbers; that is the
reference.  The device inputs are torch tensors made from the numpy pairs of
tests/refine_cases.py; the sizes come from the library (mp_debug_ingest_info): either side of
every trip length of the ingest's kernels."""
import ctypes
import functools
import sys

import numpy as np

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import refine_cases as RC

BASE_SIZES = (0, 1, 5, 7, 63, 64, 65, 255, 256, 257, 1100)
SEED = 0x1D6E57ED5EED0001
SPREAD_SEED = 11  # (chosen on the CPU: test_the_sum_order_is_really_tested holds for it)
# mp_debug_pair_set_record: the ray-derived maxima (ea eap exi eb ebp exj eab2) and the margin
# constants computed from them (c0, c1 from eap / ebp; tau2 from exi / exj)
RAY_VALUES = (9, 10, 11, 12, 13, 14, 19, 24, 25, 26, 27, 28)
TIE_SCALE = 7


CHECKS = {}


def check(*params):
    """register a check, once per parameter tuple"""
    def reg(fn):
        name = fn.__name__.replace("check_", "", 1)
        for p in params or [()]:
            CHECKS[name + ("[" + "-".join(str(v) for v in p) + "]" if p else "")] = (fn, p)
        return fn
    return reg


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def ingest_info():
    out = np.zeros(L.INGEST_INFO_VALUES, dtype=np.int32)
    L.check(L.lib().mp_debug_ingest_info(out.ctypes.data_as(L.c_int32_p)))
    assert np.all(out > 0)
    return tuple(int(v) for v in out)


@functools.lru_cache(maxsize=None)
def sizes():
    """the base sizes, and c - 1, c, c + 1, 2 c + 1 for every trip length c of the kernels"""
    out = list(BASE_SIZES)
    for c in ingest_info():
        for n in (c - 1, c, c + 1, 2 * c + 1):
            if n not in out:
                out.append(n)
    return tuple(out)


def _pair(variant, seed, n):
    if n == 0:
        return RC.make_pair(variant, seed, 0)
    p = RC.make_pair(variant, seed, max(n, 8))
    for key in ("x0", "x1", "depth0", "depth1", "inlier_mask"):
        p[key] = p[key][:n]
    return p


def _spread(p, rng):
    """coordinates with radii 1e-2 .. 1e4 pixels around the principal points: the terms of the
    normalization scale's sum span six decades, so its value depends on the order of additions"""
    for x, pp in (("x0", "pp0"), ("x1", "pp1")):
        n = len(p[x])
        r = 10.0 ** rng.uniform(-2.0, 4.0, n)
        a = rng.uniform(0.0, 2.0 * np.pi, n)
        p[x] = np.asarray(p[pp], dtype=np.float64) + np.c_[r * np.cos(a), r * np.sin(a)]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(variant, dtype="float64", spread=False):
    """Pairs of all sizes (never changed), rounded to `dtype` first so that the host path gets
    exactly the numbers the device arrays hold; start models and candidates per pair."""
    k = Case()
    k.variant, k.dtype = variant, np.dtype(dtype)
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.sizes = sizes()
    rng = np.random.default_rng(SPREAD_SEED + 100 * variant)
    k.pairs = []
    for i, n in enumerate(k.sizes):
        p = _pair(variant, 1 if n == 5 else 600 + i, n)
        if spread and variant in (1, 2):
            _spread(p, rng)
        for key in ("x0", "x1", "depth0", "depth1"):
            p[key] = np.asarray(p[key], dtype=k.dtype).astype(np.float64)
        k.pairs.append(p)
    mrng = np.random.default_rng(40 + variant)
    k.models = [RC.start_model(variant, p, mrng) for p in k.pairs]
    k.cands = [[RC.start_model(variant, p, mrng, rot_deg=d) for d in (0.5, 3.0, 1.5)] for p in k.pairs]
    return k


def host_inputs(variant, pairs):
    offs = np.concatenate([[0], np.cumsum([len(p["depth0"]) for p in pairs])]).astype(np.int64)
    cat = lambda key, w: np.concatenate([np.asarray(p[key], dtype=np.float64).reshape(-1, w) for p in pairs])
    cam = [np.stack([np.asarray(RC.cams(variant, p)[s], dtype=np.float64) for p in pairs]) for s in (0, 1)]
    md = np.stack([np.asarray(p.get("min_depth", (0.0, 0.0)), dtype=np.float64).reshape(2) for p in pairs])
    return offs, cat("x0", 2), cat("x1", 2), cat("depth0", 1)[:, 0], cat("depth1", 1)[:, 0], cam[0], cam[1], md


def device_set(variant, pairs, o, c, dtype=np.float64, **kw):
    """from_device on torch tensors of the pairs' numbers; returns (set, tensors, originals)"""
    torch = _torch()
    offs, x0, x1, d0, d1, c0, c1, md = host_inputs(variant, pairs)
    orig = [np.ascontiguousarray(a, dtype=dtype) for a in (x0, x1, d0, d1)]
    ten = [torch.as_tensor(a).to("cuda") for a in orig]
    ps = madpose.PairSet.from_device(variant, ten[0], ten[1], offs, c0, c1, o, c, depth0=ten[2], depth1=ten[3],
                                     min_depth=md, **kw)
    return ps, ten, orig


def rows(ps, pair, n):
    out = np.full(12 * max(n, 1), np.nan)
    L.check(L.lib().mp_debug_pair_set_rows(ps._h, pair, out.ctypes.data_as(L.c_double_p)))
    return out[:12 * n].reshape(12, n)


def record(ps, pair):
    out = np.full(L.PAIR_RECORD_VALUES, np.nan)
    L.check(L.lib().mp_debug_pair_set_record(ps._h, pair, out.ctypes.data_as(L.c_double_p)))
    return out


def assert_same_set(variant, dev, host, ns, what=""):
    """rows 0 .. 5 (and 6 .. 11 of calibrated geometry), norm_scale and the records"""
    nrow = 12 if variant in (0, 3) else 6
    assert len(dev) == len(host) == len(ns)
    assert dev.num_correspondences == host.num_correspondences == sum(ns)
    assert dev.resident_bytes == host.resident_bytes
    assert dev.norm_scale.tobytes() == host.norm_scale.tobytes(), (what, dev.norm_scale, host.norm_scale)
    inexact = 0
    for i, n in enumerate(ns):
        a, b = rows(dev, i, n), rows(host, i, n)
        assert a[:nrow].tobytes() == b[:nrow].tobytes(), (what, i, n)
        ra, rb = record(dev, i), record(host, i)
        exact = [j for j in range(L.PAIR_RECORD_VALUES) if variant in (1, 2) or j not in RAY_VALUES]
        assert ra[exact].tobytes() == rb[exact].tobytes(), (what, i, n, ra, rb)
        # calibrated geometry: the host forms the rays behind these maxima with whatever
        # contraction its compiler chose; each is a three-term sum whose roundings are a few
        # 2^-53 of the absolute sum it is compared with
        for j in RAY_VALUES:
            if ra[j].tobytes() == rb[j].tobytes():
                continue
            inexact += 1
            assert rb[j] * (1 - 1e-14) <= ra[j] <= rb[j] * (1 + 1e-14), (what, i, n, j, ra[j], rb[j])
    return inexact


def digest(variant, r):
    """every field of a result object as comparable bytes"""
    out = []
    for name, v in sorted(vars(r).items()):
        if isinstance(v, np.ndarray):
            v = (v.dtype.str, v.shape, v.tobytes())
        elif isinstance(v, (list, tuple)) and v and isinstance(v[0], np.ndarray):
            v = tuple(a.tobytes() for a in v)
        elif isinstance(v, float):
            v = np.float64(v).tobytes()
        elif hasattr(v, "R") and callable(v.R):
            v = RC.model_bytes(variant, v)
        elif isinstance(v, list):
            v = tuple(v)
        out.append((name, v))
    return tuple(out)


def stage_digests(variant, ps, k, pair_ids=None):
    """the stages of the issue on one set, as digests"""
    pick = (lambda xs: xs) if pair_ids is None else (lambda xs: [xs[i] for i in pair_ids])
    dg = lambda rs: [digest(variant, r) for r in rs]
    out = {}
    if variant != 3:
        out["ransac_lo"] = dg(ps.ransac(budget=64, step=32, lo=1, lo_steps=1, rounds=2, seed=SEED, pair_ids=pair_ids))
        out["ransac"] = dg(ps.ransac(budget=48, seed=SEED, pair_ids=pair_ids))
        out["lsq_fit"] = dg(ps.lsq_fit(pick(k.models), 0, seed=SEED, pair_ids=pair_ids))
    out["select"] = dg(ps.select(pick(k.cands), with_scores=True, with_counts=True, pair_ids=pair_ids))
    out["refine"] = dg(ps.refine(pick(k.models), relax=True, rounds=2, pair_ids=pair_ids))
    return out


# ---- 1. rows, scales and records ----

@check(*[(v, d) for v in (0, 1, 2, 3) for d in ("float32", "float64")])
def check_rows_scales_and_records_equal_the_host_set(variant, dtype):
    k = _case(variant, dtype, spread=True)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as host:
        dev, ten, _ = device_set(variant, k.pairs, k.o, k.c, dtype=k.dtype)
        with dev:
            assert ten[0].dtype == getattr(_torch(), dtype)
            inexact = assert_same_set(variant, dev, host, k.sizes, dtype)
            print(f"variant {variant} {dtype}: {inexact} ray-derived record values differ in their last bits")
            # Byte equality for calibrated geometry too: in the library as it is built
            # (madpose_amd/build.py) the host's make_problem, with pair_magnitudes inlined,
            # holds no fused multiply-add, so host and device round the rays alike.  A host
            # compiler that contracts them would legitimately move these values by a few 2^-53;
            # assert_same_set's 1 +- 1e-14 is the bound for that case, and this line then goes.
            assert inexact == 0
            if variant in (1, 2):
                assert np.all(dev.norm_scale[np.asarray(k.sizes) > 0] != 1.0)


# ---- 2. the order of the sum ----

def check_the_sum_order_is_really_tested(variant, dtype):
    """numpy only: on the pairs of test 1 the sequential sum of make_problem differs from
    np.sum's pairwise sum for at least half of the pairs with n >= 64, so a tree reduction on
    the device cannot give test 1's norm_scale."""
    k = _case(variant, dtype, spread=True)
    differ = total = 0
    for p in k.pairs:
        n = len(p["depth0"])
        if n < 64:
            continue
        a = p["x0"] - np.asarray(p["pp0"], dtype=np.float64)
        b = p["x1"] - np.asarray(p["pp1"], dtype=np.float64)
        terms = np.empty(2 * n)
        terms[0::2] = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
        terms[1::2] = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])
        seq = 0.0
        for t in terms.tolist():
            seq += t
        total += 1
        differ += seq != float(np.sum(terms))
    assert total >= 8 and 2 * differ >= total, (differ, total)


# ---- 4. the stages ----

@check((0,), (1,), (2,), (3,))
def check_stages_return_the_host_sets_bytes(variant):
    k = _case(variant)
    ids = [9, 0, 12, 3, 10, 6, 1]  # a permuted subset, with the empty pair
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as host:
        dev, _, _ = device_set(variant, k.pairs, k.o, k.c)
        with dev:
            want, got = stage_digests(variant, host, k), stage_digests(variant, dev, k)
            assert sorted(got) == sorted(want)
            for stage in want:
                assert got[stage] == want[stage], stage
            want, got = stage_digests(variant, host, k, ids), stage_digests(variant, dev, k, ids)
            for stage in want:
                assert got[stage] == want[stage], (stage, "pair_ids")
    # (the stages did something: a winner and inliers in the large pairs)
    if variant != 3:
        assert sum(1 for r in want["ransac"] if dict(r)["index"] >= 0) >= 3


# ---- 5. depth maps ----

MAP_SHAPES = ((1, 1), (3, 5), (48, 64), (120, 160))
BIG_IMAGE = (968, 1296)  # (factors 48 / 968, 64 / 1296, ...: not representable)


def _map_case(dtype):
    """Maps 0 .. 3: the shapes with the image of the map's own size (factor 1); maps 4 .. 7: the
    same shapes under the large image.  Keypoints of every pair: inside the image, exactly on
    k + 0.5 (factor 1: half-to-even rounding decides), negative, beyond the image."""
    rng = np.random.default_rng(77)
    maps = [rng.uniform(0.5, 9.0, s).astype(dtype) for s in MAP_SHAPES + MAP_SHAPES]
    images = [s for s in MAP_SHAPES] + [BIG_IMAGE] * len(MAP_SHAPES)
    # map 2 serves three pairs: side 0 of pair 0, side 1 of pair 1, side 0 of pair 4
    map_ids = np.array([[2, 3], [0, 2], [1, 5], [6, 7], [2, 4], [7, 1]], dtype=np.int64)
    pairs = []
    for i, (m0, m1) in enumerate(map_ids):
        n = (40, 64, 9, 257, 70, 33)[i]
        p = _pair(0, 700 + i, n)
        for side, m in ((0, m0), (1, m1)):
            ih, iw = images[m]
            x = np.c_[rng.uniform(0, iw, n), rng.uniform(0, ih, n)]
            q = n // 4
            x[:q] = np.floor(x[:q]) + 0.5        # exactly on k + 0.5
            x[q:q + 3] = -x[q:q + 3] - 0.25      # negative
            x[q + 3:q + 6] += (iw, ih)           # beyond the image
            x[q + 6] = (iw - 0.5, ih - 0.5)
            p[f"x{side}"] = x
        pairs.append(p)
    return maps, images, map_ids, pairs


@check(("float32",), ("float64",))
def check_depth_maps_equal_get_depths(dtype):
    torch = _torch()
    variant = 0
    o, c = synthetic.example_options("calibrated")
    maps, images, map_ids, pairs = _map_case(dtype)
    for side in (0, 1):
        got = madpose.get_depths_batch([images[m] for m in map_ids[:, side]], [maps[m] for m in map_ids[:, side]],
                                       [p[f"x{side}"] for p in pairs])
        for p, d in zip(pairs, got):
            assert d.dtype == np.dtype(dtype)
            p[f"depth{side}"] = d.astype(np.float64)
    ns = [len(p["depth0"]) for p in pairs]
    offs, x0, x1, d0, d1, c0, c1, md = host_inputs(variant, pairs)
    tmaps = [torch.as_tensor(m).to("cuda") for m in maps]
    tx0, tx1 = torch.as_tensor(x0).to("cuda"), torch.as_tensor(x1).to("cuda")
    with madpose.PairSet(variant, pairs, o, c) as host:
        with madpose.PairSet.from_device(variant, tx0, tx1, offs, c0, c1, o, c, depth_maps=tmaps, map_ids=map_ids,
                                         image_sizes=np.asarray(images), min_depth=md) as dev:
            for i, n in enumerate(ns):
                r = rows(dev, i, n)
                assert r[4].tobytes() == pairs[i]["depth0"].tobytes(), i
                assert r[5].tobytes() == pairs[i]["depth1"].tobytes(), i
            assert_same_set(variant, dev, host, ns, "maps")
            call = lambda ps: [digest(variant, r) for r in ps.ransac(budget=48, seed=SEED)]
            assert call(dev) == call(host)
        # image_sizes default: each map's own shape (maps 0 .. 3 only are used then)
        own = np.array([[2, 3], [0, 2], [1, 1], [3, 0], [2, 2], [3, 1]])
        pairs2 = [dict(p) for p in pairs]
        for side in (0, 1):
            got = madpose.get_depths_batch([MAP_SHAPES[m] for m in own[:, side]], [maps[m] for m in own[:, side]],
                                           [p[f"x{side}"] for p in pairs2])
            for p, d in zip(pairs2, got):
                p[f"depth{side}"] = d.astype(np.float64)
        with madpose.PairSet(variant, pairs2, o, c) as host2:
            with madpose.PairSet.from_device(variant, tx0, tx1, offs, c0, c1, o, c, depth_maps=tmaps[:4],
                                             map_ids=own, min_depth=md) as dev2:
                assert_same_set(variant, dev2, host2, ns, "own sizes")


# ---- 6. non-finite values ----

@check((0,), (1,))
def check_nan_depth_and_infinite_coordinate(variant):
    k = _case(variant)
    pairs = [dict(p) for p in k.pairs[4:11]]  # n = 63 .. 1100
    ns = [len(p["depth0"]) for p in pairs]
    pairs[1]["depth1"] = pairs[1]["depth1"].copy()
    pairs[1]["depth1"][17] = np.nan
    pairs[4]["x0"] = pairs[4]["x0"].copy()
    pairs[4]["x0"][200, 1] = np.inf
    models, cands = k.models[4:11], k.cands[4:11]
    with madpose.PairSet(variant, pairs, k.o, k.c) as host:
        dev, _, _ = device_set(variant, pairs, k.o, k.c)
        with dev:
            assert_same_set(variant, dev, host, ns, "non-finite")
            ties = [record(dev, i)[TIE_SCALE] for i in range(len(pairs))]
            assert [np.isinf(t) for t in ties] == [i in (1, 4) for i in range(len(pairs))], ties
            for ps_call in (lambda ps: ps.ransac(budget=48, seed=SEED),
                            lambda ps: ps.select(cands, with_scores=True, with_counts=True),
                            lambda ps: ps.refine(models, relax=True, rounds=2)):
                assert [digest(variant, r) for r in ps_call(dev)] == [digest(variant, r) for r in ps_call(host)]


# ---- 7. lifetime: the inputs are neither written nor referenced afterwards ----

@check()
def check_inputs_are_only_read_and_not_referenced_afterwards():
    variant = 1
    k = _case(variant)
    with madpose.PairSet(variant, k.pairs, k.o, k.c) as host:
        want = stage_digests(variant, host, k)
    dev, ten, orig = device_set(variant, k.pairs, k.o, k.c)
    with dev:
        for t, a in zip(ten, orig):  # nothing was written into them
            assert t.cpu().numpy().tobytes() == a.tobytes()
        for t in ten:
            t.zero_()
        _torch().cuda.synchronize()
        got = stage_digests(variant, dev, k)
    assert got == want


# ---- 8. ordering against the producer's stream ----

@check()
def check_inputs_produced_on_another_stream():
    torch = _torch()
    variant = 2
    k = _case(variant)
    offs, x0, x1, d0, d1, c0, c1, md = host_inputs(variant, k.pairs)
    # the inputs as the end of a short chain of device operations on a side stream, every step
    # exact in float64: (x * 4) * 0.25, plus the sum of a large zero buffer that takes a while
    side = torch.cuda.Stream()
    src = [torch.as_tensor(a).to("cuda") for a in (x0, x1, d0, d1)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ballast = torch.zeros(1 << 24, dtype=torch.float64, device="cuda")
        for _ in range(4):
            ballast = ballast * 2.0 + ballast
        made = [(t * 4.0) * 0.25 + ballast[:1].sum() for t in src]
        dev = madpose.PairSet.from_device(variant, made[0], made[1], offs, c0, c1, k.o, k.c, depth0=made[2],
                                          depth1=made[3], min_depth=md, stream=side)
    with dev, madpose.PairSet(variant, k.pairs, k.o, k.c) as host:
        for t, a in zip(made, (x0, x1, d0, d1)):
            assert t.cpu().numpy().tobytes() == a.tobytes()  # (the chain is exact)
        assert_same_set(variant, dev, host, k.sizes, "side stream")


# ---- 9. a short buffer ----

@check()
def check_a_short_buffer_is_refused_by_the_library():
    """The C entry itself, past the Python checks: d1 two elements short of its allocation's
    end (the allocation's range as the runtime reports it, mp_debug_device_extent)."""
    torch = _torch()
    variant = 0
    k = _case(variant)
    offs, x0, x1, d0, d1, c0, c1, md = host_inputs(variant, k.pairs)
    T = int(offs[-1])
    ten = [torch.as_tensor(a).to("cuda") for a in (x0, x1, d0, d1)]
    torch.cuda.synchronize()
    lib = L.lib()
    ext = np.zeros(2, dtype=np.int64)
    L.check(lib.mp_debug_device_extent(ten[3].data_ptr(), 0, ext.ctypes.data_as(L.c_int64_p)))
    base, size = int(ext[0]), int(ext[1])
    assert base <= ten[3].data_ptr() and ten[3].data_ptr() + 8 * T <= base + size
    o, c = k.o._to_c(), k.c._to_c()

    def create(d1_ptr):
        inp = L.mp_device_pairs()
        inp.x0, inp.x1, inp.xy_type = ten[0].data_ptr(), ten[1].data_ptr(), 1
        inp.d0, inp.d1, inp.depth_type = ten[2].data_ptr(), d1_ptr, 1
        h = ctypes.c_void_p()
        code = lib.mp_pair_set_create_device(variant, len(k.pairs), offs.ctypes.data_as(L.c_int64_p),
                                             ctypes.byref(inp), md.ctypes.data_as(L.c_double_p),
                                             c0.ctypes.data_as(L.c_double_p), c1.ctypes.data_as(L.c_double_p),
                                             ctypes.byref(o), ctypes.byref(c), 0, ctypes.byref(h))
        return code, h
    # T - 2 elements left in the allocation from this address on
    code, h = create(base + size - 8 * (T - 2))
    assert code == L.MP_EINVAL and not h.value
    msg = lib.mp_last_error().decode()
    assert "d1" in msg and "shorter" in msg, msg
    # an address that is not aligned to the element type
    code, h = create(ten[3].data_ptr() + 4)
    assert code == L.MP_EINVAL and not h.value and "d1" in lib.mp_last_error().decode()
    # and the same call with the whole array is taken
    code, h = create(ten[3].data_ptr())
    assert code == L.MP_OK and h.value, lib.mp_last_error()
    assert lib.mp_pair_set_destroy(h) == L.MP_OK


# ---- 10. interleaving and teardown ----

@check()
def check_host_and_device_sets_interleaved():
    variant = 0
    ka, kb = _case(0), _case(0, "float32")
    with madpose.PairSet(variant, ka.pairs, ka.o, ka.c) as host:
        dev, _, _ = device_set(variant, kb.pairs, kb.o, kb.c, dtype=np.float32)
        with dev, madpose.PairSet(variant, kb.pairs, kb.o, kb.c) as ref:
            dg = lambda rs: [digest(variant, r) for r in rs]
            a1 = dg(host.refine(ka.models, rounds=2))
            b1 = dg(dev.select(kb.cands, with_scores=True))
            b2 = dg(dev.ransac(budget=48, seed=SEED))
            a2 = dg(host.select(ka.cands, with_scores=True))
            b3 = dg(dev.refine(kb.models, rounds=2))
            a3 = dg(host.refine(ka.models, rounds=2))
            assert a1 == a3
            assert b1 == dg(ref.select(kb.cands, with_scores=True))
            assert b2 == dg(ref.ransac(budget=48, seed=SEED))
            assert b3 == dg(ref.refine(kb.models, rounds=2))
            assert a2 != b1  # (float32-rounded numbers: the two sets do differ)


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
