"""Time the chain hypothesize -> select -> refine over the same pairs, through the batch
entries and through a PairSet.

Pairs: the ScanNet stand-in (synthetic.scannet_pair, 1500-2500 correspondences each, as
tools/select_batch_bench.py builds them), `--samples` random minimal samples per pair with
both solver types.  Per variant (0 calibrated, 1 shared focal, 2 two focal) the chain is

  hypothesize  the samples' models;
  select       every pair's models as its candidates;
  refine       3 rounds from the winners, over the pairs that have one,

on the prepared arrays (the C entries).  The hand-over between the stages -- the models moved
to the front as candidate rows, the winners' rows picked -- is host work that is the same in
every leg; it is done outside the timed calls, and a chain's time is the sum of its library
calls.  Four legs, `--repeats` chains each after a warm-up, median (min - max):

  a  the three batch entries of the library given by --parent-lib (the parent commit's
     build), loaded beside this one in the same process;
  b  the three batch entries of this build;
  c  mp_pair_set_create, the three set calls, mp_pair_set_destroy;
  d  the three set calls on a set that already exists.

Checked, and the tool fails otherwise: the result bytes of b equal a's and those of c and d
equal b's (models, counts, select results, refine results, every inlier list).  Also timed:
the setup alone (mp_pair_set_create + destroy) with mp_debug_pair_set_prep 0 and 1, and on
one host thread (MADPOSE_PAIR_SETUP_THREADS=1).  Every call ends in a device synchronise, so the host clock
around it is the call's time.  One GPU, one process.  Prints one JSON line per variant and
writes all of them to --out."""
import argparse
import ctypes
import hashlib
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
from madpose_amd import synthetic  # noqa: E402

NAMES = {0: "calibrated", 1: "shared_focal", 2: "two_focal"}
ROUNDS = 3


def load_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("mp_hypothesize_batch", "mp_select_batch", "mp_refine_batch", "mp_last_error"):
        res, args = L.EXPORTS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def dp(v):
    return v.ctypes.data_as(L.c_double_p)


def ip(v):
    return v.ctypes.data_as(L.c_int32_p)


def lp(v):
    return v.ctypes.data_as(L.c_int64_p)


class Chain:
    """The arrays of the three stages for a list of pairs, kept alive"""

    def __init__(self, variant, pairs, K, seed):
        self.variant, self.P, self.K = variant, len(pairs), K
        k0, k1 = ("K0", "K1") if variant == 0 else ("pp0", "pp1")
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.float64)
        self.x0, self.x1 = cat([p["x0"].reshape(-1) for p in pairs]), cat([p["x1"].reshape(-1) for p in pairs])
        self.d0, self.d1 = cat([p["depth0"] for p in pairs]), cat([p["depth1"] for p in pairs])
        self.c0, self.c1 = cat([p[k0].reshape(-1) for p in pairs]), cat([p[k1].reshape(-1) for p in pairs])
        self.md = cat([np.asarray(p["min_depth"], dtype=np.float64) for p in pairs])
        self.sizes = np.array([len(p["depth0"]) for p in pairs])
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.T = int(self.offsets[-1])
        self.S = self.P * K
        self.sample_offsets = (K * np.arange(self.P + 1)).astype(np.int64)
        rng = np.random.default_rng(seed)
        self.types = rng.integers(0, 2, self.S).astype(np.int32)
        self.idx8 = np.ascontiguousarray(draw_samples(self.sizes, K, seed + 1))
        self.slots = L.HYPOTHESIZE_SLOTS[variant]
        self.o, self.c = synthetic.example_options(NAMES[variant])
        self.oc, self.cc = self.o._to_c(), self.c._to_c()
        self.cand = None  # the candidates of the first chain: every later one forms the same
        # the outputs, allocated and touched once: a fresh array's page faults would fall
        # inside the timed calls.  Every entry writes all slots of models and counts; the
        # inlier buffers are zeroed before each call (outside the timing).
        self.models = np.zeros((self.S, self.slots, 17))
        self.counts = np.zeros(self.S, dtype=np.int32)
        self.sidx = np.zeros(3 * self.T, dtype=np.int32)
        self.ridx = np.zeros(3 * self.T, dtype=np.int32)
        for a in (self.models, self.counts, self.sidx, self.ridx):
            a.fill(0)

    # ---- the hand-over on the host (untimed, the same in every leg) ----
    def candidates(self, models, counts):
        per_pair = counts.reshape(self.P, self.K).sum(axis=1)
        moff = np.concatenate([[0], np.cumsum(per_pair)]).astype(np.int64)
        if self.cand is None:
            keep = np.arange(self.slots)[None, :] < counts[:, None]
            self.cand = (np.ascontiguousarray(models[keep]), counts.copy())
        elif not np.array_equal(self.cand[1], counts):
            raise SystemExit("pair_set_bench: a chain's hypothesize counts differ from the first chain's")
        return moff, self.cand[0]

    def winners(self, moff, cand, results):
        best = np.array([results[p].best_index for p in range(self.P)])
        keep = np.flatnonzero(best >= 0).astype(np.int32)
        rows = np.ascontiguousarray(cand[moff[keep] + best[keep]])
        return keep, rows

    def sub_pairs(self, keep):
        """the batch entries' inputs for the pairs `keep` (the whole arrays when all are kept)"""
        if len(keep) == self.P:
            return self.offsets, self.x0, self.x1, self.d0, self.d1, self.md, self.c0, self.c1
        nc = len(self.c0) // self.P
        sel = np.concatenate([np.arange(self.offsets[p], self.offsets[p + 1]) for p in keep] + [np.zeros(0, int)])
        offs = np.concatenate([[0], np.cumsum(self.sizes[keep])]).astype(np.int64)
        take = lambda a, w: np.ascontiguousarray(a.reshape(-1, w)[sel].reshape(-1))
        per = lambda a, w: np.ascontiguousarray(a.reshape(-1, w)[keep].reshape(-1))
        return (offs, take(self.x0, 2), take(self.x1, 2), take(self.d0, 1), take(self.d1, 1), per(self.md, 2),
                per(self.c0, nc), per(self.c1, nc))

    # ---- the legs ----
    def run_batch(self, lib):
        """(times of the three calls, result bytes) through the batch entries of `lib`"""
        def check(code):
            if code != L.MP_OK:
                raise SystemExit("pair_set_bench: " + lib.mp_last_error().decode(errors="replace"))
        v, P = self.variant, self.P
        models, counts = self.models, self.counts
        counts.fill(-1)
        norm = np.ones(P)
        t0 = time.perf_counter()
        check(lib.mp_hypothesize_batch(v, P, lp(self.offsets), dp(self.x0), dp(self.x1), dp(self.d0), dp(self.d1),
                                       dp(self.md), dp(self.c0), dp(self.c1), ctypes.byref(self.oc),
                                       ctypes.byref(self.cc), lp(self.sample_offsets), ip(self.types), ip(self.idx8),
                                       models.ctypes.data_as(ctypes.POINTER(L.mp_model)), ip(counts), dp(norm), 0, 0,
                                       0))
        t_h = time.perf_counter() - t0
        moff, cand = self.candidates(models, counts)
        sres = (L.mp_select_result * P)()
        sidx = self.sidx
        sidx.fill(0)
        t0 = time.perf_counter()
        check(lib.mp_select_batch(v, P, lp(self.offsets), dp(self.x0), dp(self.x1), dp(self.d0), dp(self.d1),
                                  dp(self.c0), dp(self.c1), ctypes.byref(self.oc), ctypes.byref(self.cc), lp(moff),
                                  cand.ctypes.data_as(ctypes.POINTER(L.mp_model)), None, None, sres, ip(sidx), 0, 0,
                                  0))
        t_s = time.perf_counter() - t0
        keep, rows = self.winners(moff, cand, sres)
        offs, x0, x1, d0, d1, md, c0, c1 = self.sub_pairs(keep)
        rres = (L.mp_refine_result * max(len(keep), 1))()
        ridx = self.ridx[:3 * max(int(offs[-1]), 1)]
        ridx.fill(0)
        t0 = time.perf_counter()
        check(lib.mp_refine_batch(v, len(keep), lp(offs), dp(x0), dp(x1), dp(d0), dp(d1), dp(md), dp(c0), dp(c1),
                                  ctypes.byref(self.oc), ctypes.byref(self.cc), ROUNDS,
                                  rows.ctypes.data_as(ctypes.POINTER(L.mp_model)), rres, ip(ridx), 0, 0))
        t_r = time.perf_counter() - t0
        return (t_h, t_s, t_r), self.key(models, counts, norm, sres, sidx, keep, rows, rres, ridx)

    def create(self):
        h = ctypes.c_void_p()
        L.check(L.lib().mp_pair_set_create(self.variant, self.P, lp(self.offsets), dp(self.x0), dp(self.x1),
                                           dp(self.d0), dp(self.d1), dp(self.md), dp(self.c0), dp(self.c1),
                                           ctypes.byref(self.oc), ctypes.byref(self.cc), 0, ctypes.byref(h)))
        return h

    def run_set(self, h):
        """(times of the three calls, result bytes) through the set `h`"""
        lib, P = L.lib(), self.P
        models, counts = self.models, self.counts
        counts.fill(-1)
        norm = np.ones(P)
        t0 = time.perf_counter()
        L.check(lib.mp_hypothesize_set(h, P, None, lp(self.sample_offsets), ip(self.types), ip(self.idx8),
                                       models.ctypes.data_as(ctypes.POINTER(L.mp_model)), ip(counts), 0))
        t_h = time.perf_counter() - t0
        L.check(lib.mp_pair_set_norm_scales(h, dp(norm)))
        moff, cand = self.candidates(models, counts)
        sres = (L.mp_select_result * P)()
        sidx = self.sidx
        sidx.fill(0)
        t0 = time.perf_counter()
        L.check(lib.mp_select_set(h, P, None, lp(moff), cand.ctypes.data_as(ctypes.POINTER(L.mp_model)), None, None,
                                  sres, ip(sidx), 0))
        t_s = time.perf_counter() - t0
        keep, rows = self.winners(moff, cand, sres)
        rres = (L.mp_refine_result * max(len(keep), 1))()
        ridx = self.ridx[:3 * max(int(self.sizes[keep].sum()), 1)]
        ridx.fill(0)
        t0 = time.perf_counter()
        L.check(lib.mp_refine_set(h, len(keep), None if len(keep) == P else ip(keep), ROUNDS,
                                  rows.ctypes.data_as(ctypes.POINTER(L.mp_model)), rres, ip(ridx)))
        t_r = time.perf_counter() - t0
        return (t_h, t_s, t_r), self.key(models, counts, norm, sres, sidx, keep, rows, rres, ridx)

    @staticmethod
    def key(models, counts, norm, sres, sidx, keep, rows, rres, ridx):
        """a digest of everything the chain returned (the models through one wrapping 64-bit sum
        of the bit patterns per sample: position-sensitive, one pass over the array)"""
        h = hashlib.sha256()
        per_sample = np.add.reduce(models.view(np.uint64).reshape(len(models), -1), axis=1)
        used = bytes(rres)[:ctypes.sizeof(L.mp_refine_result) * len(keep)]
        for part in (per_sample, counts, norm, bytes(sres), sidx, keep, rows, used, ridx):
            h.update(part if isinstance(part, bytes) else np.ascontiguousarray(part).tobytes())
        return h.hexdigest()


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def leg(fn, repeats):
    """warm-up, then `repeats` chains: the spread of the chain time and of each stage, the key"""
    fn()
    rows, keys = [], set()
    for _ in range(repeats):
        ts, key = fn()
        rows.append(ts)
        keys.add(key)
    if len(keys) != 1:
        raise SystemExit("pair_set_bench: two chains of one leg returned different bytes")
    out = {"chain": spread([sum(r.values()) for r in rows])}
    for name in sorted({k for r in rows for k in r}):
        out[name] = spread([r[name] for r in rows])
    return out, keys.pop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", required=True, help="libmadpose_mi355x.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_set", "pair_set_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("pair_set_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    parent = load_parent(a.parent_lib)
    lib = L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    out = {"tool": "pair_set_bench", "pairs": a.pairs, "samples_per_pair": a.samples, "rounds": ROUNDS,
           "repeats": a.repeats, "correspondences": int(sum(len(p["depth0"]) for p in pairs)),
           "time": "sum of the three library calls of a chain (leg c: plus create and destroy), host clock",
           "runs": []}
    for variant in a.variants:
        C = Chain(variant, pairs, a.samples, seed=31 + variant)
        stage = lambda ts: {"hypothesize": ts[0], "select": ts[1], "refine": ts[2]}

        def batch_leg(which):
            ts, key = C.run_batch(which)
            return stage(ts), key

        def set_new():
            t0 = time.perf_counter()
            h = C.create()
            t_c = time.perf_counter() - t0
            ts, key = C.run_set(h)
            t0 = time.perf_counter()
            L.check(lib.mp_pair_set_destroy(h))
            return dict(stage(ts), create=t_c, destroy=time.perf_counter() - t0), key

        la, ka = leg(lambda: batch_leg(parent), a.repeats)
        lb, kb = leg(lambda: batch_leg(lib), a.repeats)
        lc, kc = leg(set_new, a.repeats)
        h = C.create()
        try:
            ld, kd = leg(lambda: (lambda r: (stage(r[0]), r[1]))(C.run_set(h)), a.repeats)
            nb = ctypes.c_int64()
            L.check(lib.mp_pair_set_info(h, None, None, None, ctypes.byref(nb), None))
        finally:
            L.check(lib.mp_pair_set_destroy(h))
        if not (ka == kb == kc == kd):
            raise SystemExit(f"pair_set_bench: result bytes differ between the legs: a {ka[:12]} b {kb[:12]} "
                             f"c {kc[:12]} d {kd[:12]}")

        def setup_alone():
            ts = []
            for _ in range(a.repeats + 1):
                t0 = time.perf_counter()
                hh = C.create()
                ts.append(time.perf_counter() - t0)
                L.check(lib.mp_pair_set_destroy(hh))
            return spread(ts[1:])

        setup = {}
        try:
            for mode in (0, 1):
                L.check(lib.mp_debug_pair_set_prep(mode))
                setup[f"prep_{mode}"] = setup_alone()
        finally:
            L.check(lib.mp_debug_pair_set_prep(0))
        os.environ["MADPOSE_PAIR_SETUP_THREADS"] = "1"
        try:
            setup["prep_0_one_host_thread"] = setup_alone()
        finally:
            del os.environ["MADPOSE_PAIR_SETUP_THREADS"]
        run = {"variant": NAMES[variant], "samples": C.S, "candidates": int(len(C.cand[0])),
               "resident_bytes": int(nb.value), "bytes_equal_a_b_c_d": True,
               "a_parent_batch": la, "b_batch": lb, "c_set_created_per_chain": lc, "d_set_existing": ld,
               "setup_alone": setup}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
