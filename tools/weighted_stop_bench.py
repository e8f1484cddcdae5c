"""Measure the weighted stopping rule on the ScanNet stand-in: 1500 pairs
(synthetic.scannet_pair, 1500-2500 correspondences each), calibrated, with §7's synthetic
confidences: 1.0 on the true matches and 0.05 elsewhere.

  stop     ps.ransac(budget=512, step=64, lo=1, rounds=3, weights=w) with weighted_stop off and on:
           the samples spent (total and per pair), the call's time, the launches of the mass stage
           and their summed time (mp_debug_inlier_mass_stats), and pose AUC@5/10/20;
  default  the default path for the comparison with the parent commit: the same call without the
           keyword, and the unweighted call.  Run the tool in alternating processes with
           --tree <a checkout of the parent> --legs default and without --tree.

--outlier-ratio and --min-iterations change the stand-in's outlier ratio (0.3) and the options'
min_num_iterations (the examples' 100), to find where the mode pays.

Every time is a host clock around a call that ends in a device synchronise, median (min - max) of
--repeats after a warm-up.  One GPU, one process; the process does not import torch (DESIGN.md §7's
measurement trap).  Prints one JSON line per leg and writes all of them to --out."""
import argparse
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
    ap.add_argument("--budget", type=int, default=512)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--outlier-ratio", type=float, default=None)
    ap.add_argument("--min-iterations", type=int, default=None)
    ap.add_argument("--legs", nargs="+", default=["stop", "default"])
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_stop", "weighted_stop_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import madpose
    from madpose_amd import _lib as L
    from madpose_amd import synthetic
    assert "torch" not in sys.modules
    if madpose.device_count() < 1:
        sys.exit("weighted_stop_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    if a.outlier_ratio is None:
        pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    else:
        pairs = [synthetic.make_pair(s, n=synthetic.scannet_size(s), outlier_ratio=a.outlier_ratio)
                 for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    conf = [np.where(p["inlier_mask"], 1.0, 0.05) for p in pairs]
    seed = 31
    o, c = synthetic.example_options("calibrated")
    if a.min_iterations is not None:
        o.min_num_iterations = a.min_iterations
    out = {"tool": "weighted_stop_bench", "tree": os.path.relpath(os.path.abspath(a.tree), ROOT), "pairs": a.pairs,
           "budget": a.budget, "step": a.step, "lo": 1, "rounds": 3, "repeats": a.repeats,
           "correspondences": int(sizes.sum()), "outlier_ratio": 0.3 if a.outlier_ratio is None else a.outlier_ratio,
           "min_num_iterations": int(o.min_num_iterations), "legs": {}}
    kw = dict(budget=a.budget, step=a.step, lo=1, rounds=3, seed=seed)
    T = np.stack([p["T_0to1"] for p in pairs])

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

    def auc(res):
        R = np.stack([r.model.R() if r.model is not None else np.full((3, 3), np.nan) for r in res])
        t = np.stack([r.model.t() if r.model is not None else np.full(3, np.nan) for r in res])
        return madpose.pose_eval_batch(T, R, t, thresholds=(5, 10, 20))[2]

    def samples(res):
        n = np.array([r.num_samples for r in res])
        marks, counts = np.unique(n, return_counts=True)
        return {"total": int(n.sum()), "per_pair_mean": float(n.mean()), "per_pair_median": float(np.median(n)),
                "per_pair_min": int(n.min()), "per_pair_max": int(n.max()),
                "pairs_at_checkpoint": {str(int(m)): int(k) for m, k in zip(marks, counts)},
                "stopped": int(sum(r.stopped for r in res)), "winners": int(sum(r.index >= 0 for r in res))}

    with madpose.PairSet(0, pairs, o, c) as ps:
        w = ps.draw_weights(conf) if hasattr(ps, "draw_weights") else None
        if "default" in a.legs:
            report("call_unweighted", spread(timed(lambda: ps.ransac(**kw))))
            if w is not None:
                report("call_weighted_without_the_keyword", spread(timed(lambda: ps.ransac(weights=w, **kw))))
        if "stop" in a.legs:
            lib = L.lib()
            for name, on in (("weighted_stop_off", False), ("weighted_stop_on", True)):
                call = lambda: ps.ransac(weights=w, weighted_stop=on, **kw)
                leg = spread(timed(call))
                n_runs, ms = L.ctypes.c_int64(0), L.ctypes.c_double(0.0)
                L.check(lib.mp_debug_inlier_mass_stats(None, None, 1))
                res = call()
                L.check(lib.mp_debug_inlier_mass_stats(L.ctypes.byref(n_runs), L.ctypes.byref(ms), 1))
                leg["samples"] = samples(res)
                leg["mass_runs"] = {"launches": int(n_runs.value), "summed_ms": float(ms.value)}
                leg["auc_5_10_20"] = auc(res)
                if on:
                    tot = np.array([r.rule_total for r in res], dtype=np.float64)
                    m = np.array([r.rule_mass for r in res], dtype=np.float64)
                    leg["rule_mass_ratio_median"] = [float(np.median(m[:, t] / tot)) for t in range(3)]
                report(name, leg)
        if w is not None:
            w.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
