"""Time hypothesize_batch, and for MD samples the route it replaces.

Pairs: the ScanNet stand-in (synthetic.scannet_pair, 1500-2500 correspondences each), with
`--samples` random minimal samples per pair.  For each of `--variants` (0 calibrated, 1
shared focal, 2 two focal) and each solver type (0 the MD solver, 1 the point solver):

  batch   mp_hypothesize_batch over all pairs in one call, on the prepared arrays (the C
          entry); once more with profiling on for the split between pair setup, host
          planning, uploads, the solve launches and the copies back (every stage waited for)
  route   type 0 only -- what a caller had to do before for the same models: gather the
          samples' points on the host and apply K^-1 (calibrated) or the principal point
          and the normalisation scale (numpy, vectorised over all samples; the scale itself
          is taken from the batch call's output and its cost left out, in the route's
          favour), mp_solve_scale_shift_pose_batch over all samples, then the estimator's
          min-depth filter and offset1 / scale on the host (numpy), the kept models moved
          to the front, the focals to user units.  Checked: the route's models and counts
          equal the batch's, bit for bit.

There is no earlier route for point samples (relpose_batch stops before the depth fit).
Every call ends in a device synchronise, so the host clock around it is the call's time.
Reports the median and range of `--repeats` calls after a warm-up.  Prints one JSON line per
run and writes all of them to --out."""
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

NAMES = {0: "calibrated", 1: "shared_focal", 2: "two_focal"}
STAGES = ("pairs_ms", "plan_ms", "upload_ms", "solve_ms", "download_ms")
KMD = {0: 3, 1: 4, 2: 4}
KPT = {0: 5, 1: 6, 2: 7}


def inv3(K):
    """engine.cpp inv3 (the oracle's), operation for operation on Python floats"""
    K = [float(v) for v in np.asarray(K).reshape(9)]
    d = K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) + K[2] * (K[3] * K[7] - K[4] * K[6])
    return np.array([(K[4] * K[8] - K[5] * K[7]) / d, (K[2] * K[7] - K[1] * K[8]) / d, (K[1] * K[5] - K[2] * K[4]) / d,
                     (K[5] * K[6] - K[3] * K[8]) / d, (K[0] * K[8] - K[2] * K[6]) / d, (K[2] * K[3] - K[0] * K[5]) / d,
                     (K[3] * K[7] - K[4] * K[6]) / d, (K[1] * K[6] - K[0] * K[7]) / d, (K[0] * K[4] - K[1] * K[3]) / d])


def draw_samples(sizes, K, seed):
    """K samples per pair of 8 distinct indices each (S x 8 int32): uniform draws, the rows
    that repeat an index drawn again"""
    if min(sizes) < 8:
        raise ValueError("every pair needs at least 8 correspondences")
    rng = np.random.default_rng(seed)
    n = np.repeat(np.asarray(sizes), K)[:, None]
    idx = np.floor(rng.random((n.shape[0], 8)) * n).astype(np.int32)
    while True:
        srt = np.sort(idx, axis=1)
        bad = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))
        if bad.size == 0:
            return idx
        idx[bad] = np.floor(rng.random((bad.size, 8)) * n[bad]).astype(np.int32)


class Batch:
    """The arguments of mp_hypothesize_batch for a list of pairs and one solver type, kept alive"""

    def __init__(self, variant, pairs, K, stype, idx8):
        self.variant, self.pairs, self.K, self.stype = variant, pairs, K, stype
        k0, k1 = ("K0", "K1") if variant == 0 else ("pp0", "pp1")
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.float64)
        self.x0, self.x1 = cat([p["x0"].reshape(-1) for p in pairs]), cat([p["x1"].reshape(-1) for p in pairs])
        self.d0, self.d1 = cat([p["depth0"] for p in pairs]), cat([p["depth1"] for p in pairs])
        self.c0, self.c1 = cat([p[k0].reshape(-1) for p in pairs]), cat([p[k1].reshape(-1) for p in pairs])
        self.md = cat([np.asarray(p["min_depth"], dtype=np.float64) for p in pairs])
        self.sizes = np.array([len(p["depth0"]) for p in pairs])
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        P = len(pairs)
        self.S = P * K
        self.sample_offsets = (K * np.arange(P + 1)).astype(np.int64)
        self.types = np.full(self.S, stype, dtype=np.int32)
        self.ks = KPT[variant] if stype else KMD[variant]
        self.idx = np.ascontiguousarray(idx8)  # (a solver reads its first ks slots)
        self.slots = L.HYPOTHESIZE_SLOTS[variant]
        self.models = np.zeros((self.S, self.slots, 17))
        self.counts = np.zeros(self.S, dtype=np.int32)
        self.norm = np.ones(P)
        self.o, self.c = synthetic.example_options(NAMES[variant])
        self.oc, self.cc = self.o._to_c(), self.c._to_c()

    def call(self):
        dp = lambda v: v.ctypes.data_as(L.c_double_p)
        ip = lambda v: v.ctypes.data_as(L.c_int32_p)
        L.check(L.lib().mp_hypothesize_batch(
            self.variant, len(self.pairs), self.offsets.ctypes.data_as(L.c_int64_p), dp(self.x0), dp(self.x1),
            dp(self.d0), dp(self.d1), dp(self.md), dp(self.c0), dp(self.c1), ctypes.byref(self.oc),
            ctypes.byref(self.cc), self.sample_offsets.ctypes.data_as(L.c_int64_p), ip(self.types), ip(self.idx),
            self.models.ctypes.data_as(ctypes.POINTER(L.mp_model)), ip(self.counts), dp(self.norm), 0, 0, 0))

    def profiled(self):
        madpose.profile_enable(True)
        try:
            self.call()
        finally:
            madpose.profile_enable(False)
        out = np.zeros(5)
        L.check(L.lib().mp_debug_hypothesize_timing(out.ctypes.data_as(L.c_double_p)))
        return dict(zip(STAGES, (float(v) for v in out)))

    def route(self):
        """the MD models by the earlier route: host gather, the batched raw-sample solver, host filter"""
        v, k, P, K = self.variant, self.ks, len(self.pairs), self.K
        pair_of = np.repeat(np.arange(P), K)
        g = self.offsets[:-1][pair_of][:, None] + self.idx[:, :k]          # S x k global correspondence
        X0, X1 = self.x0.reshape(-1, 2), self.x1.reshape(-1, 2)
        u0, v0, u1, v1 = X0[g, 0], X0[g, 1], X1[g, 0], X1[g, 1]
        x = np.ones((self.S, k, 3))
        y = np.ones((self.S, k, 3))
        if v == 0:
            Ki0 = np.stack([inv3(p["K0"]) for p in self.pairs])[pair_of]   # S x 9
            Ki1 = np.stack([inv3(p["K1"]) for p in self.pairs])[pair_of]
            for r in range(3):  # mv3_exact: (M0 u + M1 v) + M2 1
                x[:, :, r] = Ki0[:, 3 * r, None] * u0 + Ki0[:, 3 * r + 1, None] * v0 + Ki0[:, 3 * r + 2, None] * 1.0
                y[:, :, r] = Ki1[:, 3 * r, None] * u1 + Ki1[:, 3 * r + 1, None] * v1 + Ki1[:, 3 * r + 2, None] * 1.0
        else:
            c0, c1 = self.c0.reshape(-1, 2)[pair_of], self.c1.reshape(-1, 2)[pair_of]
            ns = self.norm[pair_of][:, None]
            x[:, :, 0], x[:, :, 1] = (u0 - c0[:, 0, None]) / ns, (v0 - c0[:, 1, None]) / ns
            y[:, :, 0], y[:, :, 1] = (u1 - c1[:, 0, None]) / ns, (v1 - c1[:, 1, None]) / ns
        dx, dy = self.d0[g], self.d1[g]
        models, counts = madpose.solve_scale_shift_pose_batch(v, x, y, dx, dy)
        # the estimator's filter (hybrid_pose_estimator.cpp:80-85) and offset1 / scale
        md = self.md.reshape(-1, 2)[pair_of]
        live = np.arange(models.shape[1])[None, :] < counts[:, None]
        scale, o0, o1 = models[:, :, 12], models[:, :, 13], models[:, :, 14]
        keep = live & (o0 > -md[:, 0, None]) & (o1 > -md[:, 1, None] * scale)
        with np.errstate(divide="ignore", invalid="ignore"):
            models[:, :, 14] = np.where(keep, o1 / scale, o1)
        if v != 0:
            models[:, :, 15] *= self.norm[pair_of][:, None]
            models[:, :, 16] *= self.norm[pair_of][:, None]
        out = np.zeros((self.S, self.slots, 17))
        n = np.minimum(keep.sum(axis=1), self.slots).astype(np.int32)
        pos = np.cumsum(keep, axis=1) - 1
        s_i, m_i = np.nonzero(keep & (pos < self.slots))
        out[s_i, pos[s_i, m_i]] = models[s_i, m_i]
        return out, n


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hypothesize_batch", "hypothesize_batch_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("hypothesize_batch_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    out = {"tool": "hypothesize_batch_bench", "pairs": a.pairs, "samples_per_pair": a.samples, "repeats": a.repeats,
           "correspondences": int(sum(len(p["depth0"]) for p in pairs)), "runs": []}
    idx8 = draw_samples([len(p["depth0"]) for p in pairs], a.samples, seed=31)
    for variant in a.variants:
        for stype in (0, 1):
            B = Batch(variant, pairs, a.samples, stype, idx8)
            B.call()  # warm-up (code objects, pooled context)
            tb = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                B.call()
                tb.append(time.perf_counter() - t0)
            nm = int(B.counts.sum())
            run = {"variant": NAMES[variant], "solver_type": stype, "samples": B.S, "models": nm, "batch": spread(tb),
                   "batch_samples_per_s": B.S / statistics.median(tb), "batch_models_per_s": nm / statistics.median(tb),
                   "split_ms": B.profiled()}
            if stype == 0:
                rm, rc = B.route()  # warm-up, and the comparison
                run["route_equals_batch"] = bool(np.array_equal(rc, B.counts) and rm.tobytes() == B.models.tobytes())
                tr = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    B.route()
                    tr.append(time.perf_counter() - t0)
                run["route"] = spread(tr)
                run["route_samples_per_s"] = B.S / statistics.median(tr)
                # not slower: the medians compared with the measured run-to-run spread as the only margin
                run["batch_not_slower"] = bool(statistics.median(tb) <= statistics.median(tr) +
                                               (max(tb) - min(tb)) + (max(tr) - min(tr)))
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
