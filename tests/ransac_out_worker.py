"""The device-output checks of tests/test_ransac_out_gpu.py, run in a process of their own.

PairSet.ransac(out_mask=..., out_errors=..., out_models=..., out_index=..., out_counts=...) writes
into arrays that are already on the device, and the tests make them with torch.  A process can
drive the GPU through one HIP runtime only, so torch must be imported before the
library is loaded: `python -m tests.ransac_out_worker` imports torch first, runs every check (or
those named on the command line) and prints one JSON object {name: {"ok": bool, "seconds": s,
"detail": text}} as its last line, as tests/residuals_worker.py does.  A check is a function that
raises AssertionError like a test.  The process ends with a set open in the library.

Inputs: residuals_worker.case(variant) -- one pair of every size in residuals_worker.SIZES, either
side of a wave, of a trip and of an item; sizes 0 and 1 give pairs without a winner.  The
reference of every check is the same call without the new keywords; nothing has a tolerance."""
import ctypes
import functools
import sys

import numpy as np

import madpose
from madpose_amd import _lib as L
from tests import residuals_worker as RW

SIZES, GUARD = RW.SIZES, RW.GUARD
VARIANTS = (0, 1, 2)
P = len(SIZES)
SEED = {0: 7, 1: 7, 2: 7}  # the seed of every mode, per variant (the module docstring of the test says why)
SUBSET = [11, 0, 12, 4, 9, 1]  # a strict subset, not in order: two pairs without a winner among them

MODES = ("budget", "budget_rounds0", "samples", "step", "step_lo", "step_lo_steps", "weights_step_lo",
         "weights_weighted_stop", "reversed", "subset")
FIELDS = ("num_samples", "num_candidates", "stopped", "lo_runs", "lo_accepted", "lo_index", "lo_step", "lo_stage",
          "lo_step_offers", "lo_step_accepted", "rule_mass", "rule_total", "index", "sample", "slot", "solver_type",
          "score_selected", "score_initial", "score_final", "rounds_run", "rounds_accepted", "status", "norm_scale",
          "num_inliers")

CHECKS = {}


def check(*params):
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
def opened(variant):
    """(case, open set, draw weights, thresholds (P, 3)) of a variant; never closed: the process ends
    with the sets open"""
    k = RW.case(variant)
    ps = RW.open_set(k)
    rng = np.random.default_rng(90 + variant)
    w = ps.draw_weights([0.25 + 0.75 * rng.random(n) for n in SIZES])
    thr = np.zeros((P, 3))
    for p in range(P):
        rec = np.full(L.PAIR_RECORD_VALUES, np.nan)
        L.check(L.lib().mp_debug_pair_set_record(ps._h, p, rec.ctypes.data_as(L.c_double_p)))
        thr[p] = rec[:3]
    return k, ps, w, thr


def mode_kwargs(variant, mode):
    k, ps, w, _ = opened(variant)
    seed = SEED[variant]
    return {
        "budget": lambda: dict(budget=64, seed=seed),
        "budget_rounds0": lambda: dict(budget=64, seed=seed, rounds=0),
        "samples": lambda: dict(samples=ps.draw(64, seed)),
        "step": lambda: dict(budget=64, step=32, seed=seed),
        "step_lo": lambda: dict(budget=64, step=32, lo=1, seed=seed),
        "step_lo_steps": lambda: dict(budget=64, step=32, lo=1, lo_steps=2, seed=seed),
        "weights_step_lo": lambda: dict(budget=64, weights=w, step=32, lo=1, seed=seed),
        "weights_weighted_stop": lambda: dict(budget=64, weights=w, step=16, weighted_stop=True, seed=seed),
        "reversed": lambda: dict(budget=64, seed=seed, pair_ids=list(range(P))[::-1]),
        "subset": lambda: dict(budget=64, step=32, lo=1, seed=seed, pair_ids=list(SUBSET)),
    }[mode]()


def same_results(got, want, lists=True):
    """field by field, model_row bytes and lists included"""
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert getattr(a, f) == getattr(b, f), (j, f, getattr(a, f), getattr(b, f))
        assert a.model_row.tobytes() == b.model_row.tobytes(), j
        assert (a.model is None) == (b.model is None), j
        if lists:
            for t in range(3):
                assert a.inlier_indices[t].dtype == np.int32
                assert a.inlier_indices[t].tobytes() == b.inlier_indices[t].tobytes(), (j, t)
        else:
            assert a.inlier_indices is None, j


class Outputs:
    """the five device arrays of a call with ns pairs and R rows, each a contiguous slice of a buffer
    of FILL bytes with GUARD guard bytes on each side; the mask starts at an odd byte address"""

    def __init__(self, torch, ns, R, which=("mask", "errors", "models", "index", "counts")):
        self.ns, self.R = ns, R
        spec = {"mask": (R, 1, torch.uint8, (R,)), "errors": (24 * R, 0, torch.float64, (3, R)),
                "models": (136 * ns, 0, torch.float64, (ns, 17)), "index": (4 * ns, 4, torch.int32, (ns,)),
                "counts": (12 * ns, 4, torch.int32, (ns, 3))}
        self.bufs, self.arr = {}, {}
        for name in which:
            nbytes, lead, dtype, shape = spec[name]
            buf, start = RW.guarded(torch, nbytes, lead)
            self.bufs[name] = (buf, start, nbytes)
            a = buf[start:start + nbytes]
            self.arr[name] = a if dtype == torch.uint8 else a.view(dtype).view(*shape)
        if "mask" in self.arr:
            assert self.arr["mask"].data_ptr() % 2 == 1
        torch.cuda.synchronize()

    def kwargs(self):
        return {"out_" + name: a for name, a in self.arr.items()}

    def host(self):
        """the arrays on the host, after the guards were found intact"""
        for buf, start, nbytes in self.bufs.values():
            RW.assert_guards(buf, start, nbytes)
        return {name: a.cpu().numpy() for name, a in self.arr.items()}


def bits(mask, t):
    return np.flatnonzero((mask >> t) & 1).astype(np.int32)


def assert_outputs(variant, want, ids, H, rounds0):
    """assertions 2 .. 4 of the issue on the host copies H of the outputs of a call whose results
    (lists included) are `want`; returns (pairs without a winner, mixed pairs of >= 4095 rows)"""
    k, ps, _, thr = opened(variant)
    mask, err = H["mask"], H["errors"]
    assert mask.dtype == np.uint8 and not np.any(mask & 0xF8)
    none = mixed = 0
    for j, r in enumerate(want):
        n = SIZES[ids[j]]
        assert r.rows == slice(r.rows.start, r.rows.start + n)
        m, e = mask[r.rows], err[:, r.rows]
        assert H["models"][j].tobytes() == r.model_row.tobytes(), j
        assert H["index"][j] == r.index and H["counts"][j].tolist() == [len(a) for a in r.inlier_indices], j
        assert tuple(H["counts"][j].tolist()) == r.num_inliers
        if r.index < 0:
            none += 1
            assert not m.any() and np.all(np.isnan(e)) and not r.model_row.any(), j
            assert H["counts"][j].tolist() == [0, 0, 0]
            continue
        for t in range(3):
            assert bits(m, t).tobytes() == r.inlier_indices[t].tobytes(), (j, t)
            assert np.array_equal(e[t] < thr[ids[j], t], ((m >> t) & 1) == 1), (j, t)
        if n >= 4095:
            mixed += bool(0 < int(((m & 7) != 0).sum()) and np.any((m & 7) != 7))
    # the errors against residuals on the returned models
    won = [j for j, r in enumerate(want) if r.index >= 0]
    res = ps.residuals(np.stack([want[j].model_row for j in won]), pair_ids=[ids[j] for j in won], errors=True)
    differ = total = 0
    for e_, j in enumerate(won):
        a = np.ascontiguousarray(err[:, want[j].rows])
        b = np.ascontiguousarray(res.errors[:, res.rows(e_)])
        if variant == 0 or rounds0:
            assert a.tobytes() == b.tobytes(), j
        differ += int(np.sum(a.view(np.uint64) != b.view(np.uint64)))
        total += a.size
    print(f"variant {variant}: {differ} of {total} error values differ in their bytes from residuals(model_row)")
    return none, mixed


@check(*[(v, m) for v in VARIANTS for m in MODES])
def check_mode(variant, mode):
    """assertions 1 .. 6 (guards) for one mode: the results equal the call's without the new
    keywords; mask, errors, models, index and counts are the returned lists and rows; lists=False
    changes only inlier_indices, with and without device outputs"""
    torch = _torch()
    k, ps, _, _ = opened(variant)
    kw = mode_kwargs(variant, mode)
    ids = kw.get("pair_ids", list(range(P)))
    ns, R = len(ids), sum(SIZES[i] for i in ids)
    want = ps.ransac(**kw)
    O = Outputs(torch, ns, R)
    got = ps.ransac(**kw, **O.kwargs())
    same_results(got, want)
    offs = np.concatenate([[0], np.cumsum([SIZES[i] for i in ids])])
    for j, r in enumerate(got):
        assert r.rows == slice(int(offs[j]), int(offs[j + 1])), j
        assert want[j].rows is None
    H = O.host()
    none, mixed = assert_outputs(variant, got, ids, H, kw.get("rounds") == 0)
    accepted = sum(r.rounds_accepted >= 1 for r in got)
    print(f"variant {variant} {mode} seed {SEED[variant]}: {none} pairs without a winner, {mixed} mixed pairs of "
          f">= 4095 rows, {accepted} pairs with an accepted round")
    if len(ids) == P:
        assert none >= 2 and mixed >= 4, (none, mixed)
    else:
        assert none >= 2
    if mode == "budget":
        assert accepted >= 1
    # lists=False with the device outputs: the same bytes on the device, no list on the host
    O2 = Outputs(torch, ns, R)
    nolists = ps.ransac(**kw, **O2.kwargs(), lists=False)
    same_results(nolists, want, lists=False)
    H2 = O2.host()
    for name in H:
        assert H2[name].tobytes() == H[name].tobytes(), name
    assert [r.rows for r in nolists] == [r.rows for r in got]
    # ... and without: every other field as today
    plain = ps.ransac(**kw, lists=False)
    same_results(plain, want, lists=False)
    assert all(r.rows is None for r in plain)
    # a subset of the arrays: the mask alone, and the per-pair arrays alone
    O3 = Outputs(torch, ns, R, which=("mask",))
    only = ps.ransac(**kw, **O3.kwargs(), lists=False)
    assert O3.host()["mask"].tobytes() == H["mask"].tobytes() and only[0].rows == got[0].rows
    O4 = Outputs(torch, ns, R, which=("models", "index", "counts"))
    pp = ps.ransac(**kw, **O4.kwargs())
    same_results(pp, want)
    H4 = O4.host()
    assert all(H4[name].tobytes() == H[name].tobytes() for name in H4) and pp[0].rows is None


@check((0,), (1,), (2,))
def check_cut_into_runs(variant):
    """the output stage cut into many runs writes the same bytes"""
    import os
    torch = _torch()
    k, ps, _, _ = opened(variant)
    kw = mode_kwargs(variant, "step_lo")
    R = sum(SIZES)
    O = Outputs(torch, P, R)
    want = ps.ransac(**kw, **O.kwargs())
    H = O.host()
    for rows, entries in (("1", "32768"), ("5000", "4"), ("8193", "2")):
        os.environ["MADPOSE_RESIDUALS_RUN_ROWS"], os.environ["MADPOSE_RESIDUALS_RUN_ENTRIES"] = rows, entries
        try:
            O2 = Outputs(torch, P, R)
            got = ps.ransac(**kw, **O2.kwargs())
        finally:
            del os.environ["MADPOSE_RESIDUALS_RUN_ROWS"], os.environ["MADPOSE_RESIDUALS_RUN_ENTRIES"]
        same_results(got, want)
        H2 = O2.host()
        assert all(H2[name].tobytes() == H[name].tobytes() for name in H), (rows, entries)


@check()
def check_outputs_last_written_on_another_stream():
    """The buffers are filled on a side stream behind work that takes a while; the library's
    writes are ordered after that fill by the event, so the results survive it."""
    torch = _torch()
    k, ps, _, _ = opened(1)
    kw = mode_kwargs(1, "step_lo")
    R = sum(SIZES)
    O = Outputs(torch, P, R)
    want = ps.ransac(**kw, **O.kwargs())
    H = O.host()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ballast = torch.zeros(1 << 24, dtype=torch.float64, device="cuda")
        for _ in range(4):
            ballast = ballast * 2.0 + ballast
        O2 = Outputs.__new__(Outputs)
        O2.bufs, O2.arr = {}, {}
        for name, (buf, start, nbytes) in O.bufs.items():
            b2 = torch.full_like(buf, RW.FILL)
            b2 += ballast[:1].sum().to(torch.uint8)  # (adds 0, behind the ballast)
            O2.bufs[name] = (b2, start, nbytes)
            a = b2[start:start + nbytes]
            O2.arr[name] = a if name == "mask" else a.view(O.arr[name].dtype).view(*O.arr[name].shape)
        got = ps.ransac(**kw, **O2.kwargs(), stream=side)
    torch.cuda.synchronize()
    same_results(got, want)
    H2 = O2.host()
    assert all(H2[name].tobytes() == H[name].tobytes() for name in H)


class _ReadOnly:
    def __init__(self, t):
        cai = dict(t.__cuda_array_interface__)
        cai["data"] = (cai["data"][0], True)
        self.__cuda_array_interface__ = cai


@check()
def check_bad_device_outputs_are_refused_in_python():
    torch = _torch()
    k, ps, _, _ = opened(0)
    R = sum(SIZES)
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    mask, err = z(R, torch.uint8), z((3, R), torch.float64)
    models, index, counts = z((P, 17), torch.float64), z(P, torch.int32), z((P, 3), torch.int32)
    both = z(25 * R, torch.uint8)
    near = (R // 8) * 8 - 8  # (the last aligned place whose eight bytes lie inside the first R)
    for bad, word in (
            (dict(out_mask=z(2 * R, torch.uint8)[::2]), "out_mask must be C-c"),
            (dict(out_mask=mask[:R - 1]), "out_mask must have shape"),
            (dict(out_mask=_ReadOnly(mask)), "out_mask is read-only"),
            (dict(out_mask=mask.to(torch.int8)), "out_mask must be uint8"),
            (dict(out_mask=mask, out_errors=z((R, 3), torch.float64).t()), "out_errors must be C-c"),
            (dict(out_mask=mask, out_errors=err.to(torch.float32)), "out_errors must be float64"),
            (dict(out_errors=err), "out_errors needs out_mask"),
            (dict(out_models=z((P, 16), torch.float64)), "out_models must have shape"),
            (dict(out_models=z((17, P), torch.float64).t()), "out_models must be C-c"),
            (dict(out_index=z(P, torch.int64)), "out_index must be int32"),
            (dict(out_index=z(P + 1, torch.int32)), "out_index must have shape"),
            (dict(out_counts=z((3, P), torch.int32)), "out_counts must have shape"),
            (dict(out_counts=_ReadOnly(counts)), "out_counts is read-only"),
            (dict(out_mask=np.zeros(R, dtype=np.uint8)), "inlier_indices"),
            (dict(out_models=np.zeros((P, 17))), "residuals"),
            (dict(out_mask=both[:R], out_errors=both[near:near + 24 * R].view(torch.float64).view(3, R)), "overlap"),
            (dict(out_index=counts.view(-1)[:P], out_counts=counts), "overlap"),
            (dict(out_mask=mask, lo=1, step=32, rounds=0), "rounds >= 1"),
            (dict(stream=0), "stream goes with device outputs"),
            (dict(out_mask=mask, stream=-1), "stream must be None"),
            (dict(lists=1), "lists must be a bool")):
        try:
            ps.ransac(**{**dict(budget=64, seed=7), **bad})
        except ValueError as e:
            assert word in str(e), (word, str(e))
        else:
            raise AssertionError(f"not refused: {word}")
    torch.cuda.synchronize()
    for a in (mask, err, models, index, counts, both):
        assert not a.any().item()  # nothing was written


@check()
def check_short_and_overlapping_buffers_are_refused_by_the_library():
    """The C entry itself, past the Python checks: outputs one element short of their allocation's
    end (the range as the runtime reports it, mp_debug_device_extent), unaligned arrays, overlapping
    ranges, host memory, and the refused combinations."""
    torch = _torch()
    k, ps, _, _ = opened(0)
    lib = L.lib()
    R = sum(SIZES)
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    T = dict(mask=z(R, torch.uint8), errors=z((3, R), torch.float64), models=z((P, 17), torch.float64),
             index=z(P, torch.int32), counts=z((P, 3), torch.int32))
    torch.cuda.synchronize()
    size = dict(mask=R, errors=24 * R, models=136 * P, index=4 * P, counts=12 * P)

    def extent(t):
        ext = np.zeros(2, dtype=np.int64)
        L.check(lib.mp_debug_device_extent(t.data_ptr(), 0, ext.ctypes.data_as(L.c_int64_p)))
        return int(ext[0]), int(ext[1])
    arr, res = (L.mp_model * P)(), (L.mp_ransac_result * P)()
    idx, stopped = np.zeros(3 * R, dtype=np.int32), np.zeros(P, dtype=np.int32)
    info = (L.mp_ransac_lo_info * P)()

    def call(rounds=3, step=0, lo=0, **ptrs):
        out = L.mp_ransac_out()
        for name in T:
            setattr(out, name, ptrs.get(name, T[name].data_ptr()))
        code = lib.mp_ransac_out_set(ps._h, None, P, None, 64, step, 7, -1, None, None, None, rounds, lo, 0, 0, arr,
                                     res, idx.ctypes.data_as(L.c_int32_p), stopped.ctypes.data_as(L.c_int32_p), info,
                                     None, 0, 0, None, ctypes.byref(out))
        return code, lib.mp_last_error().decode()
    elem = dict(mask=1, errors=8, models=8, index=4, counts=4)
    for name, t in T.items():
        base, total = extent(t)
        code, msg = call(**{name: base + total - (size[name] - elem[name])})  # one element short of the end
        assert code == L.MP_EINVAL and name in msg and "shorter" in msg, (name, msg)
        if elem[name] > 1:
            code, msg = call(**{name: t.data_ptr() + elem[name] // 2})
            assert code == L.MP_EINVAL and name in msg and "aligned" in msg, (name, msg)
    code, msg = call(mask=T["errors"].data_ptr() + 8 * R)  # the mask inside the errors
    assert code == L.MP_EINVAL and "mask and errors overlap" in msg, msg
    code, msg = call(index=T["counts"].data_ptr() + 8 * P)
    assert code == L.MP_EINVAL and "index and counts overlap" in msg, msg
    code, msg = call(models=T["errors"].data_ptr())
    assert code == L.MP_EINVAL and "errors and models overlap" in msg, msg
    host = np.zeros(R, dtype=np.uint8)
    code, msg = call(mask=host.ctypes.data)
    assert code == L.MP_EINVAL and "mask" in msg, msg
    code, msg = call(mask=None)
    assert code == L.MP_EINVAL and "errors needs mask" in msg, msg
    code, msg = call(rounds=0, step=32, lo=1)
    assert code == L.MP_EINVAL and "rounds >= 1" in msg, msg
    torch.cuda.synchronize()
    for t in T.values():
        assert not t.any().item()  # nothing was launched into them
    # and the same call with the whole arrays is taken
    code, msg = call()
    assert code == L.MP_OK, msg
    want = ps.ransac(budget=64, seed=7)
    assert T["index"].cpu().numpy().tolist() == [r.index for r in want]
    assert T["models"].cpu().numpy().tobytes() == np.stack([r.model_row for r in want]).tobytes()
    assert T["mask"].any().item()


@check((0,), (1,), (2,))
def check_interleaved_with_other_stages_and_repeated(variant):
    torch = _torch()
    k, ps, _, _ = opened(variant)
    R = sum(SIZES)
    kw, kw2 = mode_kwargs(variant, "step_lo"), mode_kwargs(variant, "budget_rounds0")
    cands = [k.rows17[e:e + 1] for e in range(k.ne) if k.kinds[e] == "perturbed"]
    starts = [k.models[e] for e in range(k.ne) if k.kinds[e] == "perturbed"]

    def once():
        O, O2 = Outputs(torch, P, R), Outputs(torch, P, R)
        sel = ps.select(cands)
        a = ps.ransac(**kw, **O.kwargs())
        ref = ps.refine(starts, rounds=2)
        res = ps.residuals(k.rows17, pair_ids=k.ids, errors=True)
        b = ps.ransac(**kw2, **O2.kwargs(), lists=False)
        return (a, O.host(), b, O2.host(), [(s.index, s.score) for s in sel],
                [(r.score_final, r.rounds_accepted) for r in ref], res.mask.tobytes() + res.errors.tobytes())
    first = once()
    for _ in range(2):
        again = once()
        same_results(again[0], first[0])
        same_results(again[2], first[2], lists=False)
        for i in (1, 3):
            assert all(again[i][name].tobytes() == first[i][name].tobytes() for name in first[i])
        assert again[4:] == first[4:]
    same_results(first[0], ps.ransac(**kw))
    launches = np.zeros(1, dtype=np.int64)
    L.check(L.lib().mp_debug_ransac_out_stats(launches.ctypes.data_as(L.c_int64_p), None, 0))
    assert launches[0] >= 6


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
    print("DONE with the sets open", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
