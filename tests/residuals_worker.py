"""The cases of tests/test_residuals_gpu.py, and its device-output checks run in a process of
their own.

PairSet.residuals can write into arrays that are already on the device, and the tests make
them with torch.  torch ships a HIP runtime of its own, and a process can drive the GPU through
one HIP runtime only: the library binds to the runtime that is loaded first, so torch must be
imported before the library is loaded.  The pytest process has usually loaded
the library long before, so the checks run here: `python -m tests.residuals_worker` imports
torch first, runs every check (or those named on the command line), and prints one JSON object
{name: {"ok": bool, "seconds": s, "detail": text}} as its last line.  A check is a function
that raises AssertionError like a test.

The reference of every check is the same call with host outputs."""
import ctypes
import functools
import sys

import numpy as np

import madpose
from madpose_amd import _lib as L
from madpose_amd import synthetic
from tests import refine_cases as RC

# either side of a wave (64), of a trip (256) and of an item (4096 rows), and three items
SIZES = (0, 1, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
KINDS = ("truth", "perturbed", "nan")
GUARD = 64  # guard bytes (8 guard doubles) on each side of a device buffer
FILL = 0xAB

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


def _pair(variant, seed, n):
    if n == 0:
        return RC.make_pair(variant, seed, 0)
    p = RC.make_pair(variant, seed, max(n, 8))
    for key in ("x0", "x1", "depth0", "depth1", "inlier_mask"):
        p[key] = p[key][:n]
    return p


def model_row(variant, m):
    return np.frombuffer(RC.model_bytes(variant, m), dtype=np.float64).copy()


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(variant, score_type=0):
    """One pair of every size (never changed) and three models per pair: the synthetic ground
    truth, the ground truth perturbed by 0.3 degrees and 1 % (about half of the rows stay inside
    the thresholds: 0.6 / 0.7 / 0.3 of them per term on the calibrated pairs), and the ground
    truth with a NaN translation entry.  Entry 3 k + j is model j of pair k."""
    k = Case()
    k.variant = variant
    k.o, k.c = synthetic.example_options(RC.KIND[variant])
    k.c.score_type = score_type
    k.pairs = [_pair(variant, 1 if n == 5 else 800 + i, n) for i, n in enumerate(SIZES)]
    rng = np.random.default_rng(70 + variant)
    k.models, k.ids, k.kinds = [], [], []
    for i, p in enumerate(k.pairs):
        gt = RC.ground_truth(variant, p)
        bad = list(gt)
        bad[1] = np.array([np.nan, gt[1][1], gt[1][2]])
        for kind, m in zip(KINDS, (RC.make_model(variant, *gt),
                                   RC.start_model(variant, p, rng, rot_deg=0.3, rel=0.01),
                                   RC.make_model(variant, *bad))):
            k.models.append(m)
            k.ids.append(i)
            k.kinds.append(kind)
    k.rows17 = np.stack([model_row(variant, m) for m in k.models])
    k.ne = len(k.models)
    # a per-entry mix of factors: 1 (the tight lists), below 1, and the relaxed range
    k.mix = np.array([(1.0, 1.5, 0.75, 2.0, 1.25)[e % 5] for e in range(k.ne)])
    return k


def open_set(k):
    return madpose.PairSet(k.variant, k.pairs, k.o, k.c)


def guarded(torch, nbytes, lead=0):
    """a device buffer of nbytes + lead between two guards, all bytes FILL; returns (buffer,
    start), the payload at buffer[start : start + nbytes]"""
    buf = torch.full((GUARD + lead + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, GUARD + lead


def assert_guards(buf, start, nbytes):
    h = buf.cpu().numpy()
    assert np.all(h[:start] == FILL) and np.all(h[start + nbytes:] == FILL), "a guard byte was written"


def device_outputs(torch, R, lead=0, errors=True):
    """(mask buffer, mask slice, errors buffer, errors (3, R) view): contiguous slices of guarded
    buffers; the mask slice starts `lead` bytes past the guard"""
    mb, ms = guarded(torch, R, lead)
    mask = mb[ms:ms + R]
    if not errors:
        return mb, mask, None, None
    eb, es = guarded(torch, 24 * R)
    err = eb[es:es + 24 * R].view(torch.float64).view(3, R)
    return mb, mask, eb, err


def same_as_host(k, ps, torch, lead, errors=True, factor=1.0, **kw):
    want = ps.residuals(k.rows17, pair_ids=k.ids, factor=factor, errors=errors)
    R = int(want.offsets[-1])
    mb, mask, eb, err = device_outputs(torch, R, lead, errors)
    assert mask.data_ptr() % 2 == lead % 2 and mask.is_contiguous()
    torch.cuda.synchronize()
    got = ps.residuals(k.rows17, pair_ids=k.ids, factor=factor, out_mask=mask, out_errors=err, **kw)
    assert got.mask is mask and got.errors is err
    assert got.offsets.tobytes() == want.offsets.tobytes() and got.counts.tobytes() == want.counts.tobytes()
    assert mask.cpu().numpy().tobytes() == want.mask.tobytes()
    assert_guards(mb, GUARD + lead, R)
    if errors:
        assert err.cpu().numpy().tobytes() == want.errors.tobytes()
        assert_guards(eb, GUARD, 24 * R)
    return want


# ---- 5. host against device ----

@check((0,), (1,), (2,), (3,))
def check_device_outputs_equal_host_outputs(variant):
    torch = _torch()
    k = case(variant)
    with open_set(k) as ps:
        want = same_as_host(k, ps, torch, lead=0)
        assert int(want.offsets[-1]) == 3 * sum(SIZES) and want.mask.any()
        # a mask slice that starts at an odd byte offset; the per-entry mix of factors
        assert (GUARD + 1) % 2 == 1
        same_as_host(k, ps, torch, lead=1, factor=k.mix)
        # the mask alone
        same_as_host(k, ps, torch, lead=3, errors=False)


@check()
def check_outputs_last_written_on_another_stream():
    """The buffers are filled on a side stream behind work that takes a while; the library's
    writes are ordered after that fill by the event, so the results survive it."""
    torch = _torch()
    k = case(1)
    with open_set(k) as ps:
        want = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
        R = int(want.offsets[-1])
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ballast = torch.zeros(1 << 24, dtype=torch.float64, device="cuda")
            for _ in range(4):
                ballast = ballast * 2.0 + ballast
            mb, mask, eb, err = device_outputs(torch, R, lead=1)
            mb += ballast[:1].sum().to(torch.uint8)  # (adds 0, behind the ballast)
            eb += ballast[:1].sum().to(torch.uint8)
            got = ps.residuals(k.rows17, pair_ids=k.ids, out_mask=mask, out_errors=err, stream=side)
        torch.cuda.synchronize()
        assert mask.cpu().numpy().tobytes() == want.mask.tobytes()
        assert err.cpu().numpy().tobytes() == want.errors.tobytes()
        assert got.counts.tobytes() == want.counts.tobytes()
        assert_guards(mb, GUARD + 1, R)
        assert_guards(eb, GUARD, 24 * R)


class _ReadOnly:
    """a device array's interface with the read-only flag set"""

    def __init__(self, t):
        cai = dict(t.__cuda_array_interface__)
        cai["data"] = (cai["data"][0], True)
        self.__cuda_array_interface__ = cai


@check()
def check_bad_device_outputs_are_refused_in_python():
    torch = _torch()
    k = case(0)
    with open_set(k) as ps:
        R = 3 * sum(SIZES)
        mask = torch.zeros(R, dtype=torch.uint8, device="cuda")
        err = torch.zeros((3, R), dtype=torch.float64, device="cuda")
        call = lambda **kw: ps.residuals(k.rows17, pair_ids=k.ids, **kw)
        for bad, word in ((dict(out_mask=torch.zeros(2 * R, dtype=torch.uint8, device="cuda")[::2]), "out_mask must be C-c"),
                          (dict(out_mask=mask, out_errors=torch.zeros((R, 3), dtype=torch.float64, device="cuda").t()),
                           "out_errors must be C-c"),
                          (dict(out_mask=mask[:R - 1]), "out_mask must have shape"),
                          (dict(out_mask=mask, out_errors=err[:, :R - 1]), "out_errors must have shape"),
                          (dict(out_mask=_ReadOnly(mask)), "out_mask is read-only"),
                          (dict(out_mask=mask, out_errors=_ReadOnly(err)), "out_errors is read-only"),
                          (dict(out_mask=mask.to(torch.int8)), "out_mask must be uint8"),
                          (dict(out_mask=mask, out_errors=err.to(torch.float32)), "out_errors must be float64"),
                          (dict(out_mask=mask, out_errors=np.zeros((3, R))), "one kind"),
                          (dict(out_mask=np.zeros(R, dtype=np.uint8), out_errors=err), "one kind")):
            try:
                call(**bad)
            except ValueError as e:
                assert word in str(e), (word, str(e))
            else:
                raise AssertionError(f"not refused: {word}")
        torch.cuda.synchronize()
        assert not mask.any().item() and not err.any().item()  # nothing was written


@check()
def check_short_and_overlapping_buffers_are_refused_by_the_library():
    """The C entry itself, past the Python checks: outputs one element short of their
    allocation's end (the range as the runtime reports it, mp_debug_device_extent), an
    unaligned errors array, and two ranges that overlap."""
    torch = _torch()
    k = case(0)
    lib = L.lib()
    with open_set(k) as ps:
        want = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
        R = int(want.offsets[-1])
        mask = torch.zeros(R, dtype=torch.uint8, device="cuda")
        err = torch.zeros((3, R), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def extent(t):
            ext = np.zeros(2, dtype=np.int64)
            L.check(lib.mp_debug_device_extent(t.data_ptr(), 0, ext.ctypes.data_as(L.c_int64_p)))
            return int(ext[0]), int(ext[1])
        ids = np.asarray(k.ids, dtype=np.int32)
        rows17 = np.ascontiguousarray(k.rows17)
        offs, counts = np.zeros(k.ne + 1, dtype=np.int64), np.zeros(3 * k.ne, dtype=np.int32)

        def call(mask_ptr, err_ptr):
            out = L.mp_residuals_out()
            out.mask, out.errors, out.on_device = mask_ptr, err_ptr, 1
            code = lib.mp_residuals_set(ps._h, k.ne, ids.ctypes.data_as(L.c_int32_p),
                                        rows17.ctypes.data_as(ctypes.POINTER(L.mp_model)), None, ctypes.byref(out),
                                        offs.ctypes.data_as(L.c_int64_p), counts.ctypes.data_as(L.c_int32_p))
            return code, lib.mp_last_error().decode()
        base, size = extent(mask)
        code, msg = call(base + size - (R - 1), err.data_ptr())  # R - 1 bytes left from here on
        assert code == L.MP_EINVAL and "mask" in msg and "shorter" in msg, msg
        base, size = extent(err)
        code, msg = call(mask.data_ptr(), base + size - 8 * (3 * R - 1))
        assert code == L.MP_EINVAL and "errors" in msg and "shorter" in msg, msg
        code, msg = call(mask.data_ptr(), err.data_ptr() + 4)
        assert code == L.MP_EINVAL and "errors" in msg and "aligned" in msg, msg
        code, msg = call(err.data_ptr() + 8 * R, err.data_ptr())  # the mask inside the errors
        assert code == L.MP_EINVAL and "overlap" in msg, msg
        host = np.zeros(R, dtype=np.uint8)
        code, msg = call(host.ctypes.data, err.data_ptr())
        assert code == L.MP_EINVAL and "mask" in msg, msg
        torch.cuda.synchronize()
        assert not mask.any().item() and not err.any().item()  # nothing was launched
        # and the same call with the whole arrays is taken
        code, msg = call(mask.data_ptr(), err.data_ptr())
        assert code == L.MP_OK, msg
        assert mask.cpu().numpy().tobytes() == want.mask.tobytes()
        assert err.cpu().numpy().tobytes() == want.errors.tobytes()
        assert offs.tobytes() == want.offsets.tobytes() and counts.tobytes() == want.counts.tobytes()


@check()
def check_runs_write_device_outputs_in_place():
    """device outputs cut into many runs: every run writes its rows of the caller's arrays"""
    import os
    torch = _torch()
    k = case(2)
    with open_set(k) as ps:
        want = same_as_host(k, ps, torch, lead=0)
        os.environ["MADPOSE_RESIDUALS_RUN_ROWS"] = "5000"
        os.environ["MADPOSE_RESIDUALS_RUN_ENTRIES"] = "4"
        try:
            again = same_as_host(k, ps, torch, lead=1)
        finally:
            del os.environ["MADPOSE_RESIDUALS_RUN_ROWS"], os.environ["MADPOSE_RESIDUALS_RUN_ENTRIES"]
        assert again.mask.tobytes() == want.mask.tobytes() and again.errors.tobytes() == want.errors.tobytes()


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
