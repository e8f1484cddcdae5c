"""Measure PairSet.information on the ScanNet stand-in: 1500 pairs
(synthetic.scannet_pair, 1500-2500 correspondences each), calibrated, one model per pair (the
winner of a short ps.ransac).

  information  ps.information over all pairs into host arrays and -- when torch can be imported --
               into resident device tensors, with and without the covariance;
  kernels      the two kernel stages alone (events around the launches,
               mp_debug_information_stats, while profiling is enabled);
  residuals    the yardstick, in the same run: ps.residuals(errors=True) on the same set and
               models -- the same row traffic, no Jacobians;
  hook         the only route to the same numbers before: residuals -> the lists in numpy -> one
               madpose.lm_system(where=0) call per pair, on the first --hook-pairs pairs.

Every time but the kernels' is a host clock around a call that ends in a device synchronise,
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


def spread(ts, scale=1e3):
    return {"median_ms": scale * statistics.median(ts), "min_ms": scale * min(ts), "max_ms": scale * max(ts),
            "runs_ms": [round(scale * t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hook-pairs", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "information", "information_bench.json"))
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
        sys.exit("information_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    lib = L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    R = int(sum(len(p["depth0"]) for p in pairs))
    o, c = synthetic.example_options("calibrated")
    out = {"tool": "information_bench", "pairs": a.pairs, "repeats": a.repeats, "correspondences": R, "legs": {}}

    def report(name, value):
        out["legs"][name] = value
        print(json.dumps({name: value}), flush=True)

    def timed(fn, repeats=None):
        fn()
        ts = []
        for _ in range(repeats or a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    def kernel_ms(fn):
        """the two stages' kernel times per call, from the events around their launches"""
        n, rows, fin = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        L.check(lib.mp_profile_enable(1))
        try:
            fn()
            tr, tf = [], []
            for _ in range(a.repeats):
                L.check(lib.mp_debug_information_stats(None, None, None, 1))
                fn()
                L.check(lib.mp_debug_information_stats(ctypes.byref(n), ctypes.byref(rows), ctypes.byref(fin), 1))
                tr.append(rows.value * 1e-3)
                tf.append(fin.value * 1e-3)
        finally:
            L.check(lib.mp_profile_enable(0))
        return tr, tf, int(n.value)

    with madpose.PairSet(0, pairs, o, c) as ps:
        models = np.stack([r.model_row for r in ps.ransac(budget=64, seed=31)])
        want = ps.information(models)
        report("entries", {"pd": {str(v): int(np.sum(want.pd == v)) for v in (-1, 0, 1)},
                           "rows_mean": float(want.rows.mean()),
                           "inlier_fraction_per_term": (want.counts.sum(axis=0) / R).round(4).tolist()})
        leg = {"host_with_cov": spread(timed(lambda: ps.information(models))),
               "host_without_cov": spread(timed(lambda: ps.information(models, covariance=False)))}
        if torch is not None:
            ne = a.pairs
            d = {n: torch.zeros((ne,) + s, dtype=torch.float64, device="cuda")
                 for n, s in (("H", (66,)), ("g", (11,)), ("cost", ()), ("cov", (11, 11)))}
            torch.cuda.synchronize()
            ps.information(models, out_H=d["H"], out_g=d["g"], out_cost=d["cost"], out_cov=d["cov"])
            for n in d:
                if d[n].cpu().numpy().tobytes() != getattr(want, n).tobytes():
                    raise SystemExit(f"information_bench: device output {n} differs from the host output")
            leg["device_with_cov"] = spread(timed(lambda: ps.information(
                models, out_H=d["H"], out_g=d["g"], out_cost=d["cost"], out_cov=d["cov"])))
            leg["device_without_cov"] = spread(timed(lambda: ps.information(
                models, covariance=False, out_H=d["H"], out_g=d["g"], out_cost=d["cost"])))
        report("information", leg)
        leg = {}
        for name, fn in (("with_cov", lambda: ps.information(models)),
                         ("without_cov", lambda: ps.information(models, covariance=False))):
            tr, tf, launches = kernel_ms(fn)
            leg[name] = {"information_kernel": spread(tr), "information_finish_kernel": spread(tf),
                         "runs_per_call": launches}
        report("kernels", leg)
        report("residuals_errors_yardstick", spread(timed(lambda: ps.residuals(models, errors=True))))
        # the route before: residuals, the lists in numpy, one hook call per pair (each uploads its pair)
        sub = list(range(min(a.hook_pairs, a.pairs)))

        def hook():
            rs = ps.residuals(models[sub], pair_ids=sub)
            for e, i in enumerate(sub):
                p = pairs[i]
                m = rs.mask[rs.rows(e)]
                lists = [np.flatnonzero((m >> t) & 1).astype(np.int32) for t in range(3)]
                pose = madpose.PoseScaleOffset(models[i, :9].reshape(3, 3), models[i, 9:12], models[i, 12],
                                               models[i, 13], models[i, 14])
                madpose.lm_system(0, p["x0"], p["x1"], p["depth0"], p["depth1"], p["min_depth"], p["K0"], p["K1"], o, c,
                                  [(0, lists, pose)], 1e4)
        s = spread(timed(hook, repeats=3))
        s.update(pairs=len(sub), per_pair_ms=s["median_ms"] / len(sub),
                 same_subset_information_ms=spread(timed(lambda: ps.information(models[sub], pair_ids=sub)))["median_ms"])
        report("residuals_then_one_hook_call_per_pair", s)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
