"""Time a fixed-budget RANSAC over a PairSet two ways:

  a  the chain of the set's stages as a caller wrote it before PairSet.ransac: the samples
     drawn in numpy, hypothesize, the models moved to the front by the Python one-liner,
     select, refine with 3 rounds over the pairs with a winner -- timed as a whole and line by
     line (the sampling and the compaction are lines of their own);
  b  ps.ransac(budget=K): one library call, the samples drawn on the device.

Pairs: the ScanNet stand-in (synthetic.scannet_pair, 1500-2500 correspondences each), `--samples`
minimal samples per pair.  Per variant (0 calibrated, 1 shared focal, 2 two focal), `--repeats`
runs of each leg after a warm-up, median (min - max) of a host clock around calls that end in
a device synchronise.  After the timed runs, with profiling on (every stage waited for), the
stage split of one ransac call from mp_debug_ransac_timing, and the bytes its hypothesis stage
copied back beside what the slot array and counts would have been.

Checked, and the tool fails otherwise: ps.ransac(samples=S) on a's samples returns a's results
(the winner's index and score, the refined model, scores, counters, status and inlier lists),
and ps.ransac(budget=K) returns what ps.ransac(samples=ps.draw(K)) returns.  One GPU, one
process.  Prints one JSON line per variant and writes all of them to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

import madpose  # noqa: E402
from hypothesize_batch_bench import draw_samples  # noqa: E402
from madpose_amd import _lib as L  # noqa: E402
from madpose_amd import api, synthetic  # noqa: E402

NAMES = {0: "calibrated", 1: "shared_focal", 2: "two_focal"}
ROUNDS = 3
TIMING = ("call", "hypothesis_stage", "select_stage", "refine_stage", "hyp_plan", "hyp_draw", "hyp_upload",
          "hyp_solve", "hyp_scan_gather", "hyp_copy_back", "select_prepare", "select_upload", "select_score",
          "select_argmin", "select_winners")


def numpy_samples(sizes, K, seed):
    """the caller's sampler: K samples per pair, both solver types, as (types, idx) per pair"""
    rng = np.random.default_rng(seed)
    types = rng.integers(0, 2, len(sizes) * K).astype(np.int32)
    idx = draw_samples(sizes, K, seed + 1)
    return [(types[p * K:(p + 1) * K], idx[p * K:(p + 1) * K]) for p in range(len(sizes))]


def chain(ps, sizes, K, seed, samples=None):
    """the README's chain before PairSet.ransac; (line times, per-pair result keys)"""
    t = {}
    t0 = time.perf_counter()
    if samples is None:
        samples = numpy_samples(sizes, K, seed)
    t["sampling_numpy"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    hyp, _ = ps.hypothesize(samples)
    t["hypothesize"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    cands = [np.concatenate([m[k, :n[k]] for k in range(len(n))] + [np.zeros((0, 17))]) for m, n in hyp]
    t["compaction_python"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    best = ps.select(cands)
    t["select"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    keep = [i for i, b in enumerate(best) if b.index >= 0]
    refined = ps.refine([best[i].model for i in keep], rounds=ROUNDS, pair_ids=keep) if keep else []
    t["refine"] = time.perf_counter() - t0
    done = dict(zip(keep, refined))
    keys = []
    for i, b in enumerate(best):
        r = done.get(i)
        if r is None:
            keys.append((b.index, b.score, None, b.score, 0, 0, -1, tuple(a.tobytes() for a in b.inlier_indices)))
        else:
            keys.append((b.index, b.score, bytes(api._model_to_c(r.model, ps.variant)), r.score_final, r.rounds_run,
                         r.rounds_accepted, r.status, tuple(a.tobytes() for a in r.inlier_indices)))
    return t, keys, samples, int(sum(len(c) for c in cands))


def ransac_keys(variant, results):
    return [(r.index, r.score_selected, None if r.model is None else bytes(api._model_to_c(r.model, variant)),
             r.score_final, r.rounds_run, r.rounds_accepted, r.status, tuple(a.tobytes() for a in r.inlier_indices))
            for r in results]


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_set", "ransac_set_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("ransac_set_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    lib = L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    K = a.samples
    out = {"tool": "ransac_set_bench", "pairs": a.pairs, "samples_per_pair": K, "rounds": ROUNDS,
           "repeats": a.repeats, "correspondences": int(sizes.sum()),
           "time": "host clock around calls that end in a device synchronise; median (min - max) after a warm-up",
           "runs": []}
    for variant in a.variants:
        o, c = synthetic.example_options(NAMES[variant])
        seed = 31 + variant
        with madpose.PairSet(variant, pairs, o, c) as ps:
            # ---- a: the chain ----
            chain(ps, sizes, K, seed)
            rows = []
            for _ in range(a.repeats):
                t, keys_a, samples_a, ncand = chain(ps, sizes, K, seed)
                rows.append(t)
            leg_a = {"chain": spread([sum(r.values()) for r in rows])}
            for name in rows[0]:
                leg_a[name] = spread([r[name] for r in rows])
            # ---- b: the call ----
            ps.ransac(budget=K, seed=seed, rounds=ROUNDS)
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                res_b = ps.ransac(budget=K, seed=seed, rounds=ROUNDS)
                ts.append(time.perf_counter() - t0)
            leg_b = {"call": spread(ts)}
            # the same call on given samples (the upload instead of the device draw)
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                res_s = ps.ransac(samples=samples_a, rounds=ROUNDS)
                ts.append(time.perf_counter() - t0)
            leg_b["call_on_given_samples"] = spread(ts)
            # ---- the split of one call, every stage waited for ----
            L.check(lib.mp_profile_enable(1))
            try:
                splits = {}
                for name, kw in (("budget", dict(budget=K, seed=seed)), ("given_samples", dict(samples=samples_a))):
                    ps.ransac(rounds=ROUNDS, **kw)
                    v = np.zeros(L.RANSAC_TIMING_VALUES)
                    L.check(lib.mp_debug_ransac_timing(v.ctypes.data_as(L.c_double_p)))
                    splits[name] = dict({k + "_ms": float(x) for k, x in zip(TIMING, v)},
                                        hypothesis_bytes_back=int(v[15]), slot_array_bytes=int(v[16]),
                                        host_samples_ms=float(v[17]))
            finally:
                L.check(lib.mp_profile_enable(0))
            # ---- equality ----
            if ransac_keys(variant, res_s) != keys_a:
                raise SystemExit("ransac_set_bench: ransac(samples=S) differs from the chain on S")
            drawn = ps.draw(K, seed)
            if ransac_keys(variant, ps.ransac(samples=drawn, rounds=ROUNDS)) != ransac_keys(variant, res_b):
                raise SystemExit("ransac_set_bench: ransac(budget=K) differs from ransac(samples=draw(K))")
        run = {"variant": NAMES[variant], "samples": int(len(sizes) * K), "candidates_of_a": ncand,
               "winners_b": int(sum(r.index >= 0 for r in res_b)), "equal_to_chain": True,
               "a_chain": leg_a, "b_ransac": leg_b, "split_of_one_profiled_call": splits}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
