"""Measure PairSet.residuals on the ScanNet stand-in: 1500 pairs
(synthetic.scannet_pair, 1500-2500 correspondences each), calibrated, one model per pair (the
winner of a short ps.ransac).

  residuals  ps.residuals over all pairs: the mask alone and with the errors, into host arrays and
             -- when torch can be imported -- into resident device tensors;
  select     for comparison, the only way to the same membership before: ps.select with one
             candidate per pair (it returns index lists on the host);
  kernel     the stage's kernel alone (events around the launch, mp_debug_residuals_stats, while
             profiling is enabled) and the bytes it writes (R mask bytes, plus 24 R with the errors)
             over that time as a fraction of the HBM peak (8 TB/s).

Every time but the kernel's is a host clock around a call that ends in a device synchronise,
median (min - max) of --repeats after a warm-up.  One GPU, one process.  Prints one JSON line per
leg and writes all of them to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # bytes per second


def spread(ts, scale=1e3):
    return {"median_ms": scale * statistics.median(ts), "min_ms": scale * min(ts), "max_ms": scale * max(ts),
            "runs_ms": [round(scale * t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residuals", "residuals_bench.json"))
    a = ap.parse_args()
    try:  # (before the library is loaded: one HIP runtime in the process)
        import torch
        torch.cuda.init()
    except Exception:
        torch = None
    sys.path.insert(0, ROOT)
    import madpose
    from madpose_amd import _lib as L
    from madpose_amd import synthetic
    if madpose.device_count() < 1:
        sys.exit("residuals_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    lib = L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    R = int(sizes.sum())
    o, c = synthetic.example_options("calibrated")
    out = {"tool": "residuals_bench", "pairs": a.pairs, "repeats": a.repeats, "correspondences": R, "legs": {}}

    def report(name, value):
        out["legs"][name] = value
        print(json.dumps({name: value}), flush=True)

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    def kernel_ms(fn):
        """the stage's kernel time per call, from the events around its launches"""
        n, ms = ctypes.c_int64(), ctypes.c_double()
        L.check(lib.mp_profile_enable(1))
        try:
            fn()
            ts = []
            for _ in range(a.repeats):
                L.check(lib.mp_debug_residuals_stats(None, None, 1))
                fn()
                L.check(lib.mp_debug_residuals_stats(ctypes.byref(n), ctypes.byref(ms), 1))
                ts.append(ms.value * 1e-3)
        finally:
            L.check(lib.mp_profile_enable(0))
        return ts, int(n.value)

    with madpose.PairSet(0, pairs, o, c) as ps:
        models = np.stack([r.model_row for r in ps.ransac(budget=64, seed=31)])
        want = ps.residuals(models, errors=True)
        report("inliers", {"fraction_per_term": (want.counts.sum(axis=0) / R).round(4).tolist()})
        leg = {"host_mask": spread(timed(lambda: ps.residuals(models))),
               "host_mask_and_errors": spread(timed(lambda: ps.residuals(models, errors=True)))}
        hm, he = np.zeros(R, dtype=np.uint8), np.zeros((3, R))
        leg["host_mask_and_errors_into_given_arrays"] = spread(
            timed(lambda: ps.residuals(models, out_mask=hm, out_errors=he)))
        if torch is not None:
            dm = torch.zeros(R, dtype=torch.uint8, device="cuda")
            de = torch.zeros((3, R), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ps.residuals(models, out_mask=dm, out_errors=de)
            if dm.cpu().numpy().tobytes() != want.mask.tobytes() or de.cpu().numpy().tobytes() != want.errors.tobytes():
                raise SystemExit("residuals_bench: device outputs differ from host outputs")
            leg["device_mask"] = spread(timed(lambda: ps.residuals(models, out_mask=dm)))
            leg["device_mask_and_errors"] = spread(timed(lambda: ps.residuals(models, out_mask=dm, out_errors=de)))
        report("residuals", leg)
        cands = [models[i:i + 1] for i in range(a.pairs)]
        report("select_one_candidate_per_pair", spread(timed(lambda: ps.select(cands))))
        leg = {}
        for name, fn, nbytes in (("mask", lambda: ps.residuals(models, out_mask=hm), R),
                                 ("mask_and_errors", lambda: ps.residuals(models, out_mask=hm, out_errors=he), 25 * R)):
            ts, launches = kernel_ms(fn)
            s = spread(ts)
            s.update(launches_per_call=launches, bytes_written=nbytes,
                     write_rate_GBps=nbytes / statistics.median(ts) * 1e-9,
                     fraction_of_hbm_peak=nbytes / statistics.median(ts) / HBM_PEAK)
            leg[name] = s
        report("kernel", leg)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
