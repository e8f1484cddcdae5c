"""Time PairSet.ransac with a fixed budget and in the adaptive mode.

Pairs: the ScanNet stand-in of tools/ransac_set_bench.py (synthetic.scannet_pair, 1500-2500
correspondences each).  Per variant (0 calibrated, 1 shared focal, 2 two focal), `--repeats`
runs of each leg after a warm-up, median (min - max) of a host clock around calls that end in
a device synchronise:

  fixed     ps.ransac(budget=B): the call as it was before the adaptive mode (select_run
            with a null prior).  `--legs fixed` runs on a build without the mode, so the same
            tool times a checkout of the parent commit (--label names the build in the record).
  adaptive  ps.ransac(budget=B, step=K) under the example options: the time, the distribution
            of num_samples over the pairs and the share of pairs the rule stopped.
  nostop    the same with min_num_iterations = B, so that no pair stops: B / K rounds against
            one call, the price of the rounds alone.

For fixed and adaptive the pose AUC (pose_eval_batch at 5 / 10 / 20 degrees) of the returned
models against the pairs' ground truth, side by side: recorded, not asserted.  One GPU, one
process.  Prints one JSON line per variant and writes all of them to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import madpose  # noqa: E402
from madpose_amd import api, synthetic  # noqa: E402

NAMES = {0: "calibrated", 1: "shared_focal", 2: "two_focal"}
ROUNDS = 3


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def timed(call, repeats):
    call()  # warm-up
    ts, res = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = call()
        ts.append(time.perf_counter() - t0)
    return spread(ts), res


def auc(pairs, results):
    T = np.stack([p["T_0to1"] for p in pairs])
    rows = np.stack([r.model_row for r in results])
    _, _, aucs = api.pose_eval_batch(T, rows[:, :9], rows[:, 9:12])
    return {"auc_5_10_20": aucs, "winners": int(sum(r.index >= 0 for r in results))}


def sample_stats(results, budget):
    m = np.array([r.num_samples for r in results])
    return {"num_samples_mean": float(m.mean()), "num_samples_min": int(m.min()),
            "num_samples_quartiles": [float(q) for q in np.percentile(m, (25, 50, 75))],
            "num_samples_max": int(m.max()), "samples_total": int(m.sum()),
            "share_of_fixed_budget": float(m.sum() / (budget * len(m))),
            "pairs_stopped_share": float(np.mean([r.stopped for r in results])),
            "histogram_by_checkpoint": {int(v): int(c) for v, c in zip(*np.unique(m, return_counts=True))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--budget", type=int, default=512)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="+", default=["fixed", "adaptive", "nostop"],
                    choices=["fixed", "adaptive", "nostop"])
    ap.add_argument("--label", default="this build", help="what the record says about the library it timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_adaptive", "ransac_adaptive_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("ransac_adaptive_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    B, K = a.budget, a.step
    out = {"tool": "ransac_adaptive_bench", "library": a.label,
           "pairs": a.pairs, "budget": B, "step": K, "rounds": ROUNDS, "repeats": a.repeats,
           "correspondences": int(sizes.sum()),
           "time": "host clock around calls that end in a device synchronise; median (min - max) after a warm-up",
           "runs": []}
    for variant in a.variants:
        seed = 31 + variant
        run = {"variant": NAMES[variant]}
        o, c = synthetic.example_options(NAMES[variant])
        with madpose.PairSet(variant, pairs, o, c) as ps:
            if "fixed" in a.legs:
                t, res = timed(lambda: ps.ransac(budget=B, seed=seed, rounds=ROUNDS), a.repeats)
                run["fixed"] = dict(t, **auc(pairs, res))
            if "adaptive" in a.legs:
                t, res = timed(lambda: ps.ransac(budget=B, step=K, seed=seed, rounds=ROUNDS), a.repeats)
                run["adaptive"] = dict(t, **auc(pairs, res), **sample_stats(res, B),
                                       min_num_iterations=int(o.min_num_iterations))
        if "nostop" in a.legs:
            o.min_num_iterations = B
            with madpose.PairSet(variant, pairs, o, c) as ps:
                t, res = timed(lambda: ps.ransac(budget=B, step=K, seed=seed, rounds=ROUNDS), a.repeats)
                run["nostop"] = dict(t, **sample_stats(res, B), min_num_iterations=B)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
