"""Time PairSet.ransac in the adaptive mode with local optimisation, without and with the LO
steps inside the rounds.

Pairs: the ScanNet stand-in of tools/ransac_set_bench.py (synthetic.scannet_pair, 1500-2500
correspondences each).  Per variant (0 calibrated, 1 shared focal, 2 two focal), `--repeats`
runs of each leg after a warm-up, median (min - max) of a host clock around calls that end in
a device synchronise, under the example options with `--rounds` final rounds:

  fixed          ps.ransac(budget=B)
  adaptive       ps.ransac(budget=B, step=K)
  lo1            ps.ransac(budget=B, step=K, lo=1)
  lo1_steps1, lo1_steps3, lo1_steps10
                 ps.ransac(budget=B, step=K, lo=1, lo_steps=1 / 3 / 10)

Per leg: the time, the share of the B samples per pair that were drawn, the share of pairs the
rule stopped, the mean lo_runs and lo_accepted per pair, the steps' offers and accepted offers
per pair, the share of pairs whose returned start model came from a step, the pose AUC
(pose_eval_batch at 5 / 10 / 20 degrees) of the returned models against the pairs' ground
truth, and a SHA-256 over every result field, model and list -- recorded, not asserted.
`--legs fixed adaptive lo1` runs on a build without the steps, so the same tool times a
checkout of the parent commit (--label names the build in the record) and the digests say
whether the two builds return equal results on the untouched legs.  One GPU, one process.
Prints one JSON line per variant and writes all of them to --out."""
import argparse
import hashlib
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
LEGS = {"fixed": {}, "adaptive": {"step": True}, "lo1": {"step": True, "lo": 1},
        "lo1_steps1": {"step": True, "lo": 1, "lo_steps": 1}, "lo1_steps3": {"step": True, "lo": 1, "lo_steps": 3},
        "lo1_steps10": {"step": True, "lo": 1, "lo_steps": 10}}


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


def stats(results, budget):
    m = np.array([r.num_samples for r in results])
    field = lambda name, default: np.array([getattr(r, name, default) for r in results])
    return {"samples_share_of_budget": float(m.sum() / (budget * len(m))), "num_samples_mean": float(m.mean()),
            "pairs_stopped_share": float(np.mean([r.stopped for r in results])),
            "lo_runs_mean": float(field("lo_runs", 0).mean()), "lo_accepted_mean": float(field("lo_accepted", 0).mean()),
            "start_from_lo_share": float((field("lo_index", -1) >= 0).mean()),
            "step_offers_mean": float(field("lo_step_offers", 0).mean()),
            "step_accepted_mean": float(field("lo_step_accepted", 0).mean()),
            "start_from_step_share": float((field("lo_step", -1) >= 0).mean()),
            "histogram_by_checkpoint": {int(v): int(c) for v, c in zip(*np.unique(m, return_counts=True))}}


def digest(results):
    h = hashlib.sha256()
    for r in results:
        h.update(np.array([r.num_samples, r.num_candidates, r.index, r.sample, r.slot, r.solver_type, r.rounds_run,
                           r.rounds_accepted, r.status, int(r.stopped)], dtype=np.int64).tobytes())
        h.update(np.array([r.score_selected, r.score_initial, r.score_final, r.norm_scale]).tobytes())
        h.update(r.model_row.tobytes())
        for a in r.inlier_indices:
            h.update(np.int64(len(a)).tobytes())
            h.update(a.tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--budget", type=int, default=512)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--label", default="this build", help="what the record says about the library it timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_lo_steps", "ransac_lo_steps_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("ransac_lo_steps_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    B, K = a.budget, a.step
    out = {"tool": "ransac_lo_steps_bench", "library": a.label, "pairs": a.pairs, "budget": B, "step": K,
           "rounds": a.rounds, "repeats": a.repeats, "correspondences": int(sizes.sum()),
           "time": "host clock around calls that end in a device synchronise; median (min - max) after a warm-up",
           "runs": []}
    for variant in a.variants:
        seed = 31 + variant
        run = {"variant": NAMES[variant]}
        o, c = synthetic.example_options(NAMES[variant])
        run["threshold_multiplier"] = float(o.threshold_multiplier)
        run["num_lsq_iterations"] = int(o.num_lsq_iterations)
        run["min_num_iterations"] = int(o.min_num_iterations)
        with madpose.PairSet(variant, pairs, o, c) as ps:
            for leg in a.legs:
                kw = {k: v for k, v in LEGS[leg].items() if k != "step"}
                if LEGS[leg].get("step"):
                    kw["step"] = K
                t, res = timed(lambda: ps.ransac(budget=B, seed=seed, rounds=a.rounds, **kw), a.repeats)
                run[leg] = dict(t, **auc(pairs, res), **stats(res, B), sha256=digest(res))
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
