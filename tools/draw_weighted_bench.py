"""Measure the confidence-weighted draw on the ScanNet stand-in: 1500 pairs
(synthetic.scannet_pair, 1500-2500 correspondences each), 512 samples per pair, calibrated.  The
confidences are synthetic: 1.0 on the true matches and 0.05 elsewhere.

  draw     the sampler's stage of one profiled ps.ransac(budget=512, rounds=3)
           (mp_debug_ransac_timing's hyp_draw, the stage waited for): unweighted, weighted with the
           tables read from global memory (MADPOSE_DRAW_STAGE=0), weighted with the tables staged
           in LDS (MADPOSE_DRAW_STAGE=1);
  table    ps.draw_weights: per-pair host arrays, and -- when torch can be imported -- one resident
           device tensor;
  call     the unweighted ps.ransac(budget=512, rounds=3), for the comparison with the parent
           commit: run the tool a second time with --tree <a checkout of the parent> --legs call;
  auc      pose AUC@5/10/20 of ps.ransac(budget=B, rounds=3) for B in 32, 128, 512, with and
           without the confidences (reported, not thresholded).

Every time is a host clock around a call that ends in a device synchronise, median (min - max) of
--repeats after a warm-up.  One GPU, one process.  Prints one JSON line per leg and writes all of
them to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# mp_debug_ransac_timing's first values (tools/ransac_set_bench.py)
TIMING = ("call", "hypothesis_stage", "select_stage", "refine_stage", "hyp_plan", "hyp_draw", "hyp_upload",
          "hyp_solve", "hyp_scan_gather", "hyp_copy_back", "select_prepare", "select_upload", "select_score",
          "select_argmin", "select_winners")


def spread(ts, scale=1e3):
    return {"median_ms": scale * statistics.median(ts), "min_ms": scale * min(ts), "max_ms": scale * max(ts),
            "runs_ms": [round(scale * t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="+", default=["draw", "table", "call", "auc"])
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_weighted", "draw_weighted_bench.json"))
    a = ap.parse_args()
    torch = None
    if "table" in a.legs:
        try:  # (before the library is loaded: one HIP runtime in the process)
            import torch
            torch.cuda.init()
        except Exception:
            torch = None
    sys.path.insert(0, os.path.abspath(a.tree))
    import madpose
    from madpose_amd import _lib as L
    from madpose_amd import synthetic
    if madpose.device_count() < 1:
        sys.exit("draw_weighted_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    lib = L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    conf = [np.where(p["inlier_mask"], 1.0, 0.05) for p in pairs]
    K, seed = a.samples, 31
    o, c = synthetic.example_options("calibrated")
    out = {"tool": "draw_weighted_bench", "tree": os.path.relpath(os.path.abspath(a.tree), ROOT),"pairs": a.pairs, "samples_per_pair": K,
           "repeats": a.repeats, "correspondences": int(sizes.sum()), "legs": {}}

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

    def draw_stage(ps, **kw):
        """hyp_draw of a profiled call, ms"""
        v = np.zeros(L.RANSAC_TIMING_VALUES)
        L.check(lib.mp_profile_enable(1))
        try:
            ps.ransac(budget=K, seed=seed, rounds=3, **kw)
            L.check(lib.mp_debug_ransac_timing(v.ctypes.data_as(L.c_double_p)))
        finally:
            L.check(lib.mp_profile_enable(0))
        stages.append([float(x) for x in v[:len(TIMING)]])
        return float(v[5]) * 1e-3

    stages = []  # mp_debug_ransac_timing's stage times of every profiled call, ms

    def stage_medians(rows):
        return {name + "_ms": statistics.median(r[i] for r in rows) for i, name in enumerate(TIMING)}

    with madpose.PairSet(0, pairs, o, c) as ps:
        if "call" in a.legs:
            report("call_unweighted", spread(timed(lambda: ps.ransac(budget=K, seed=seed, rounds=3))))
        w = ps.draw_weights(conf) if hasattr(ps, "draw_weights") else None
        if "draw" in a.legs and w is not None:
            draw_stage(ps)
            del stages[:]
            leg = {"unweighted": spread([draw_stage(ps) for _ in range(a.repeats)])}
            leg["profiled_call_unweighted"] = stage_medians(stages)
            for name, flag in (("weighted_global", "0"), ("weighted_lds", "1")):
                os.environ["MADPOSE_DRAW_STAGE"] = flag
                try:
                    draw_stage(ps, weights=w)
                    del stages[:]
                    leg[name] = spread([draw_stage(ps, weights=w) for _ in range(a.repeats)])
                    leg["profiled_call_" + name] = stage_medians(stages)
                finally:
                    del os.environ["MADPOSE_DRAW_STAGE"]
            leg["weighted_pairs"] = int(w.weighted.sum())
            leg["largest_table_entries"] = int(sizes.max()) + 1
            report("draw_stage", leg)
            report("call_weighted", spread(timed(lambda: ps.ransac(budget=K, seed=seed, rounds=3, weights=w))))
        if "table" in a.legs and w is not None:
            leg = {"host_sequence": spread(timed(lambda: ps.draw_weights(conf).close()))}
            flat = np.concatenate(conf)
            leg["host_concatenation_alone"] = spread(timed(lambda: np.concatenate(conf)))
            if torch is not None:
                for name, arr in (("device_float64", flat), ("device_float32", flat.astype(np.float32))):
                    t = torch.as_tensor(arr).to("cuda")
                    torch.cuda.synchronize()
                    with ps.draw_weights(t) as wd:
                        if wd.total.tolist() != w.total.tolist():
                            raise SystemExit("draw_weighted_bench: device-given tables differ from host-given ones")
                    leg[name] = spread(timed(lambda: ps.draw_weights(t).close()))
            report("table_build", leg)
        if "auc" in a.legs:
            T = np.stack([p["T_0to1"] for p in pairs])
            leg = {}
            for budget in (32, 128, 512):
                for name, kw in (("uniform", {}), ("weighted", {"weights": w})):
                    if name == "weighted" and w is None:
                        continue
                    res = ps.ransac(budget=budget, seed=seed, rounds=3, **kw)
                    R = np.stack([r.model.R() if r.model is not None else np.full((3, 3), np.nan) for r in res])
                    t = np.stack([r.model.t() if r.model is not None else np.full(3, np.nan) for r in res])
                    _, _, aucs = madpose.pose_eval_batch(T, R, t, thresholds=(5, 10, 20))
                    leg[f"budget_{budget}_{name}"] = {"auc_5_10_20": aucs, "winners": int(sum(r.index >= 0 for r in res))}
            report("pose_auc", leg)
        if w is not None:
            w.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
