"""Time refine_batch against the per-pair loops it replaces.

Pairs: the ScanNet stand-in (synthetic.scannet_pair, shared focal, 1500-2500
correspondences each), start models as tests/refine_cases.py perturbs them.  Three legs
at the same `--rounds`, each over the same pairs and starts:

  batch        madpose.refine_batch over all pairs in one call
  loop_device  per pair: score_models(with_errors) + lm_refine_batch on the device LM
               (tests/refine_cases.refine_single, the composition the tests compare with)
  loop_host    the same loop with the host LM hook (on_host=True)

The legs are run alternately `--repeats` times after one warm-up round of each; every
call ends in a device synchronise, so the host clock around it is the call's time.  The
loops run over the first `--loop-pairs` pairs (they take seconds per hundred pairs) and
the figures are reported per pair.  Also checked: the batch results equal loop_device's
bit for bit.  Prints one JSON line and writes it to --out."""
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
from madpose_amd import synthetic  # noqa: E402
from tests import refine_cases as RC  # noqa: E402

VARIANT = 1  # shared focal, as the ScanNet stand-in of bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--loop-pairs", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_batch", "refine_batch_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("refine_batch_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    o, c = synthetic.example_options("shared_focal")
    rng = np.random.default_rng(11)
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    models = [RC.start_model(VARIANT, p, rng) for p in pairs]
    S = min(a.loop_pairs, a.pairs)

    def batch():
        return madpose.refine_batch(VARIANT, pairs, models, o, c, rounds=a.rounds)

    def loop(on_host, scales):
        return [RC.refine_single(VARIANT, pairs[i], models[i], o, c, a.rounds, scales[i], on_host=on_host)
                for i in range(S)]

    # warm-up (code objects, pooled context) and the equality check
    res = batch()
    scales = [r.norm_scale for r in res]
    dev = loop(False, scales)
    loop(True, scales)
    same = all(RC.model_bytes(VARIANT, r.model) == RC.model_bytes(VARIANT, e.model) and
               r.score_final == e.score_final and r.rounds_accepted == e.rounds_accepted and
               all(np.array_equal(x, y) for x, y in zip(r.inlier_indices, e.lists))
               for r, e in zip(res[:S], dev))
    times = {"batch": [], "loop_device": [], "loop_host": []}
    for _ in range(a.repeats):
        for name, fn in (("batch", batch), ("loop_device", lambda: loop(False, scales)),
                         ("loop_host", lambda: loop(True, scales))):
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    per = {"batch": a.pairs, "loop_device": S, "loop_host": S}
    out = {
        "tool": "refine_batch_bench", "variant": "shared_focal", "pairs": a.pairs, "loop_pairs": S,
        "rounds": a.rounds, "repeats": a.repeats,
        "correspondences": int(sum(len(p["depth0"]) for p in pairs)),
        "batch_equals_loop_device": bool(same),
        "rounds_run_total": int(sum(r.rounds_run for r in res)),
        "rounds_accepted_total": int(sum(r.rounds_accepted for r in res)),
        # first-round LM launch: one workgroup per pair that passes the size rule
        "lm_workgroups_round1": int(sum(1 for r in res if not (r.rounds_run == 1 and r.status == 3))),
    }
    for name, ts in times.items():
        out[name] = {
            "median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
            "median_ms_per_pair": 1e3 * statistics.median(ts) / per[name],
            "min_ms_per_pair": 1e3 * min(ts) / per[name], "max_ms_per_pair": 1e3 * max(ts) / per[name],
        }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
