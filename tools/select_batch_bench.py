"""Time select_batch against the per-pair loop it replaces.

Pairs: the ScanNet stand-in (synthetic.scannet_pair, 1500-2500 correspondences each).
Candidates: per pair, perturbations of the ground truth (tests/refine_cases.ground_truth)
by 0.1 to 5 degrees and a few percent in the other parameters, built as one array.  For
each of `--variants` (0 calibrated, 1 shared focal) and each of `--candidates` per pair:

  batch   mp_select_batch over all pairs in one call, on the prepared arrays (the C entry:
          the cost of turning Python pose objects into mp_model records is not part of
          it); once more with profiling on for the split between pair setup, host record
          preparation, record upload, select_score, select_argmin and the winners' sweep
          (every stage waited for, so the parts do not overlap as they do in the timed call)
  loop    the only route before select_batch: per pair score_models over its candidates, a
          numpy argmin, and a second score_models(with_errors=True) on the winner for the
          lists -- over the first `--loop-pairs` pairs, reported per pair

Also checked: the batch's winners and scores equal the loop's, bit for bit.  Then the four
work-item sizes (mp_debug_select_tile) on `--tile-pairs` pairs of 2000 correspondences with
512 candidates each: select_score's time from the profiled split.  Every call ends in a
device synchronise, so the host clock around it is the call's time.  Prints one JSON line
and writes it to --out."""
import argparse
import ctypes
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
from madpose_amd import _lib as L  # noqa: E402
from madpose_amd import synthetic  # noqa: E402
from tests import refine_cases as RC  # noqa: E402

NAMES = {0: "calibrated", 1: "shared_focal"}
STAGES = ("pairs_ms", "prepare_ms", "upload_ms", "score_ms", "argmin_ms", "winners_ms")


def candidates_array(variant, p, K, rng):
    """K x 17 doubles in mp_model's layout: perturbed copies of the pair's ground truth"""
    R, t, s, o0, o1, f0, f1 = RC.ground_truth(variant, p)
    ax = rng.standard_normal((K, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.deg2rad(rng.uniform(0.1, 5.0, K))
    X = np.zeros((K, 3, 3))
    X[:, 0, 1], X[:, 0, 2], X[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    X[:, 1, 2], X[:, 2, 0], X[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    dR = np.eye(3) + np.sin(ang)[:, None, None] * X + (1 - np.cos(ang))[:, None, None] * (X @ X)
    j = lambda: 1.0 + 0.03 * rng.standard_normal(K)
    m = np.zeros((K, 17))
    m[:, :9] = (R @ dR).reshape(K, 9)
    m[:, 9:12] = t * (1.0 + 0.03 * rng.standard_normal((K, 3)))
    m[:, 12], m[:, 13], m[:, 14] = s * j(), o0 * j(), o1 * j()
    m[:, 15] = f0 * j() if variant == 1 else 1.0
    m[:, 16] = m[:, 15]
    return m


def model_objects(variant, rows):
    return [RC.make_model(variant, r[:9].reshape(3, 3), r[9:12], r[12], r[13], r[14], r[15], r[16]) for r in rows]


class Batch:
    """The arguments of mp_select_batch for a list of pairs, kept alive"""

    def __init__(self, variant, pairs, K, seed):
        rng = np.random.default_rng(seed)
        self.variant, self.pairs, self.K = variant, pairs, K
        k0, k1 = ("K0", "K1") if variant == 0 else ("pp0", "pp1")
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.float64)
        self.x0, self.x1 = cat([p["x0"].reshape(-1) for p in pairs]), cat([p["x1"].reshape(-1) for p in pairs])
        self.d0, self.d1 = cat([p["depth0"] for p in pairs]), cat([p["depth1"] for p in pairs])
        self.c0, self.c1 = cat([p[k0].reshape(-1) for p in pairs]), cat([p[k1].reshape(-1) for p in pairs])
        self.offsets = np.concatenate([[0], np.cumsum([len(p["depth0"]) for p in pairs])]).astype(np.int64)
        self.model_offsets = (K * np.arange(len(pairs) + 1)).astype(np.int64)
        self.models = np.ascontiguousarray(np.concatenate([candidates_array(variant, p, K, rng) for p in pairs]))
        self.scores = np.zeros(len(self.models))
        self.counts = np.zeros(3 * len(self.models), dtype=np.int32)
        self.results = (L.mp_select_result * len(pairs))()
        self.idx = np.zeros(3 * int(self.offsets[-1]), dtype=np.int32)
        self.o, self.c = synthetic.example_options(NAMES[variant])
        self.oc, self.cc = self.o._to_c(), self.c._to_c()

    def call(self):
        dp = lambda v: v.ctypes.data_as(L.c_double_p)
        L.check(L.lib().mp_select_batch(
            self.variant, len(self.pairs), self.offsets.ctypes.data_as(L.c_int64_p), dp(self.x0), dp(self.x1),
            dp(self.d0), dp(self.d1), dp(self.c0), dp(self.c1), ctypes.byref(self.oc), ctypes.byref(self.cc),
            self.model_offsets.ctypes.data_as(L.c_int64_p), self.models.ctypes.data_as(ctypes.POINTER(L.mp_model)),
            dp(self.scores), self.counts.ctypes.data_as(L.c_int32_p), self.results,
            self.idx.ctypes.data_as(L.c_int32_p), 0, 0, 0))

    def profiled(self):
        madpose.profile_enable(True)
        try:
            self.call()
        finally:
            madpose.profile_enable(False)
        out = np.zeros(6)
        L.check(L.lib().mp_debug_select_timing(out.ctypes.data_as(L.c_double_p)))
        return dict(zip(STAGES, (float(v) for v in out)))

    def loop(self, S):
        """the route before select_batch over the first S pairs: (index, score, list lengths)"""
        got = []
        for i in range(S):
            p = self.pairs[i]
            ns = self.results[i].norm_scale
            rows = self.models[i * self.K:(i + 1) * self.K]
            ms = [RC.to_problem_units(self.variant, m, ns) for m in model_objects(self.variant, rows)]
            args = RC.pair_args(self.variant, p)
            s = madpose.score_models(self.variant, *args[:4], *args[5:], self.o, self.c, ms)
            b = int(np.argmin(s))
            _, err = madpose.score_models(self.variant, *args[:4], *args[5:], self.o, self.c, [ms[b]],
                                          with_errors=True)
            thr = RC.thresholds(self.variant, self.o, ns)
            got.append((b, float(s[b]), [int(np.count_nonzero(err[0, t] < thr[t])) for t in range(3)]))
        return got


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--loop-pairs", type=int, default=60)
    ap.add_argument("--candidates", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tile-pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_batch", "select_batch_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("select_batch_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    S = min(a.loop_pairs, a.pairs)
    out = {"tool": "select_batch_bench", "pairs": a.pairs, "loop_pairs": S, "repeats": a.repeats,
           "correspondences": int(sum(len(p["depth0"]) for p in pairs)), "tile_default": L.SELECT_TILE, "runs": []}
    for variant in a.variants:
        for K in a.candidates:
            B = Batch(variant, pairs, K, seed=17 + variant)
            B.call()  # warm-up (code objects, pooled context)
            ref = B.loop(S)
            same = all((B.results[i].best_index, B.results[i].best_score, list(B.results[i].num_inliers)) ==
                       (b, s, cnt) for i, (b, s, cnt) in enumerate(ref))
            tb, tl = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                B.call()
                tb.append(time.perf_counter() - t0)
            for _ in range(max(1, a.repeats // 2)):
                t0 = time.perf_counter()
                B.loop(S)
                tl.append(time.perf_counter() - t0)
            M = a.pairs * K
            run = {"variant": NAMES[variant], "candidates_per_pair": K, "candidates": M,
                   "batch_equals_loop": bool(same), "batch": spread(tb), "loop": spread(tl),
                   "batch_candidates_per_s": M / statistics.median(tb),
                   "loop_candidates_per_s": S * K / statistics.median(tl),
                   "batch_ms_per_pair": 1e3 * statistics.median(tb) / a.pairs,
                   "loop_ms_per_pair": 1e3 * statistics.median(tl) / S,
                   "split_ms": B.profiled()}
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    # the work-item sizes: pairs of 2000 correspondences, 512 candidates each
    tp = [synthetic.make_pair(9000 + s, n=2000) for s in range(a.tile_pairs)]
    tiles = []
    for variant in a.variants:
        B = Batch(variant, tp, 512, seed=23 + variant)
        B.call()
        base = (B.scores.tobytes(), B.counts.tobytes(), bytes(B.results))
        for tile in (1, 2, 4, 8):
            L.lib().mp_debug_select_tile(tile)
            try:
                B.call()
                # (only the shipped size is pinned to score_models' bits)
                same = (B.scores.tobytes(), B.counts.tobytes(), bytes(B.results)) == base
                ms = [B.profiled()["score_ms"] for _ in range(a.repeats)]
            finally:
                L.lib().mp_debug_select_tile(0)
            tiles.append({"variant": NAMES[variant], "tile": tile, "candidates": len(B.models), "n": 2000,
                          "same_bytes_as_default": bool(same), "select_score_ms_median": statistics.median(ms),
                          "select_score_ms_min": min(ms), "select_score_ms_max": max(ms)})
            print(json.dumps(tiles[-1]), flush=True)
    out["tiles"] = tiles
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
