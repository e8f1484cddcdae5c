"""Time the creation of a pair set from host arrays (mp_pair_set_create) and from arrays that
are already on the device (PairSet.from_device / mp_pair_set_create_device) -- DESIGN.md §2.9, §7.

Pairs: the ScanNet stand-in (synthetic.scannet_pair, 1500-2500 correspondences each, the pairs
of tools/pair_set_bench.py), per variant 0 calibrated, 1 shared focal, 2 two focal.  Every
timed call ends in a device synchronise, so the host clock around it is its time.  Each leg:
one warm-up, then `--repeats` runs, median (min - max).

  a  mp_pair_set_create + destroy from float64 numpy arrays, on the library given by
     --parent-lib (the parent commit's build, loaded beside this one) and on this build;
  b  from_device + close from float64 torch tensors that are already resident;
  c  the same from float32 tensors (the host leg of the same numbers is leg a on the widened
     values, timed as a32);
  d  from_device with depth maps (`--maps` maps of 120 x 160 float32 under a 968 x 1296 image, shared by the
     pairs) against get_depths_batch on both sides + mp_pair_set_create;
  e  numpy -> torch.as_tensor(...).cuda() -> from_device: data that starts on the host;
  f  create + ransac(512, step=64, lo=1) + close, from the host arrays and from the tensors.

Checked, and the tool fails otherwise: the digest of a set (its normalization scales and the
device rows of every 97th pair) is the same on the parent's build, on this build and for the
device-built set of the same numbers (b against a, c against a32, d against its host leg), and
leg f returns the same result bytes both ways.  One GPU, one process.  Prints one JSON line per
variant and writes all of them to --out."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library is loaded: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import madpose  # noqa: E402
from madpose_amd import _lib as L  # noqa: E402
from madpose_amd import synthetic  # noqa: E402

NAMES = {0: "calibrated", 1: "shared_focal", 2: "two_focal"}
MAP_SHAPE, IMAGE = (120, 160), (968, 1296)
PARENT_SYMBOLS = ("mp_pair_set_create", "mp_pair_set_destroy", "mp_pair_set_norm_scales", "mp_debug_pair_set_rows",
                  "mp_last_error")


def load_parent(path):
    lib = ctypes.CDLL(path)
    for name in PARENT_SYMBOLS:
        res, args = L.EXPORTS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def dp(v):
    return v.ctypes.data_as(L.c_double_p)


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


class Arrays:
    """The C entries' arrays for a list of pairs (float64), kept alive"""

    def __init__(self, variant, pairs, dtype=np.float64):
        self.variant, self.P = variant, len(pairs)
        k0, k1 = ("K0", "K1") if variant == 0 else ("pp0", "pp1")
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=dtype)
        self.dev = [cat([p["x0"] for p in pairs]), cat([p["x1"] for p in pairs]),
                    cat([p["depth0"] for p in pairs]), cat([p["depth1"] for p in pairs])]
        self.x0, self.x1, self.d0, self.d1 = (np.ascontiguousarray(a, dtype=np.float64) for a in self.dev)
        ncam = 9 if variant == 0 else 2
        self.c0 = np.stack([np.asarray(p[k0], dtype=np.float64).reshape(ncam) for p in pairs])
        self.c1 = np.stack([np.asarray(p[k1], dtype=np.float64).reshape(ncam) for p in pairs])
        self.md = np.stack([np.asarray(p["min_depth"], dtype=np.float64).reshape(2) for p in pairs])
        self.sizes = [len(p["depth0"]) for p in pairs]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.o, self.c = synthetic.example_options(NAMES[variant])
        self.oc, self.cc = self.o._to_c(), self.c._to_c()

    def create(self, lib, d0=None, d1=None):
        h = ctypes.c_void_p()
        code = lib.mp_pair_set_create(self.variant, self.P, self.offsets.ctypes.data_as(L.c_int64_p), dp(self.x0),
                                      dp(self.x1), dp(self.d0 if d0 is None else d0), dp(self.d1 if d1 is None else d1),
                                      dp(self.md), dp(self.c0), dp(self.c1), ctypes.byref(self.oc),
                                      ctypes.byref(self.cc), 0, ctypes.byref(h))
        if code != L.MP_OK:
            raise SystemExit("pair_set_ingest_bench: " + lib.mp_last_error().decode(errors="replace"))
        return h

    def host_set(self):
        """a PairSet object around mp_pair_set_create on the prepared arrays (PairSet(...) itself
        would concatenate the pairs inside the timed call)"""
        ps = madpose.PairSet.__new__(madpose.PairSet)
        ps.variant, ps.device, ps._hyp_error = self.variant, 0, None
        ps._sizes = list(self.sizes)
        ps._h = self.create(L.lib())
        norm = np.ones(self.P)
        L.check(L.lib().mp_pair_set_norm_scales(ps._h, dp(norm)))
        ps._norm = norm
        return ps

    def device_set(self, ten, **kw):
        return madpose.PairSet.from_device(self.variant, ten[0], ten[1], self.offsets, self.c0, self.c1, self.o,
                                           self.c, min_depth=self.md, **kw)

    def digest(self, lib, h):
        norm = np.ones(self.P)
        if lib.mp_pair_set_norm_scales(h, dp(norm)) != L.MP_OK:
            raise SystemExit("pair_set_ingest_bench: norm scales failed")
        d = hashlib.sha256(norm.tobytes())
        for p in range(0, self.P, 97):
            rows = np.zeros(12 * max(self.sizes[p], 1))
            if lib.mp_debug_pair_set_rows(h, p, dp(rows)) != L.MP_OK:
                raise SystemExit("pair_set_ingest_bench: rows failed")
            d.update(rows.tobytes())
        return d.hexdigest()


def timed(make, close, repeats, digest=None):
    """warm-up + repeats of make() (timed) and close() (timed apart); the digests must agree"""
    ts, tc, keys = [], [], set()
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        s = make()
        t1 = time.perf_counter()
        if digest:
            keys.add(digest(s))
        t2 = time.perf_counter()
        close(s)
        t3 = time.perf_counter()
        if r:
            ts.append(t1 - t0)
            tc.append(t3 - t2)
    if len(keys) > 1:
        raise SystemExit("pair_set_ingest_bench: two runs of one leg gave different sets")
    return {"create": spread(ts), "close": spread(tc)}, (keys.pop() if keys else None)


def ransac_key(rs):
    d = hashlib.sha256()
    for r in rs:
        d.update(r.model_row.tobytes())
        d.update(np.float64([r.score_final, r.score_selected, r.norm_scale]).tobytes())
        d.update(np.int64([r.index, r.num_samples, r.num_candidates, r.status, r.lo_runs, r.lo_accepted]).tobytes())
        for a in r.inlier_indices:
            d.update(a.tobytes())
    return d.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maps", type=int, default=100)
    ap.add_argument("--parent-lib", required=True, help="libmadpose_mi355x.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_set_ingest", "pair_set_ingest_bench.json"))
    a = ap.parse_args()
    if madpose.device_count() < 1:
        sys.exit("pair_set_ingest_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    parent, lib = load_parent(a.parent_lib), L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    rng = np.random.default_rng(5)
    maps = [rng.uniform(0.5, 8.0, MAP_SHAPE).astype(np.float32) for _ in range(a.maps)]
    map_ids = rng.integers(0, a.maps, (a.pairs, 2))
    out = {"tool": "pair_set_ingest_bench", "pairs": a.pairs, "repeats": a.repeats,
           "correspondences": int(sum(len(p["depth0"]) for p in pairs)), "maps": a.maps, "map_shape": MAP_SHAPE,
           "time": "host clock around calls that end in a device synchronise; median (min - max) after a warm-up",
           "runs": []}
    cuda = lambda arrs: [torch.as_tensor(v).cuda() for v in arrs]
    for variant in a.variants:
        A = Arrays(variant, pairs)
        A32 = Arrays(variant, pairs, np.float32)
        run = {"variant": NAMES[variant]}
        destroy = lambda l: (lambda h: L.check(l.mp_pair_set_destroy(h)))
        # a: host arrays, the parent's build and this one
        run["a_parent_host"], ka = timed(lambda: A.create(parent), destroy(parent), a.repeats, lambda h: A.digest(parent, h))
        run["a_host"], kb = timed(lambda: A.create(lib), destroy(lib), a.repeats, lambda h: A.digest(lib, h))
        run["a32_host"], kb32 = timed(lambda: A32.create(lib), destroy(lib), a.repeats, lambda h: A32.digest(lib, h))
        # b, c: resident tensors
        t64, t32 = cuda(A.dev), cuda(A32.dev)
        torch.cuda.synchronize()
        close = lambda ps: ps.close()
        run["b_device_f64"], kd = timed(lambda: A.device_set(t64, depth0=t64[2], depth1=t64[3]), close, a.repeats,
                                        lambda ps: A.digest(lib, ps._h))
        run["c_device_f32"], kd32 = timed(lambda: A32.device_set(t32, depth0=t32[2], depth1=t32[3]), close, a.repeats,
                                          lambda ps: A32.digest(lib, ps._h))
        # d: depth maps
        tmaps = cuda(maps)
        torch.cuda.synchronize()
        sizes = np.array([IMAGE] * a.maps)
        kp = [[p[f"x{s}"] for p in pairs] for s in (0, 1)]

        def host_maps():
            d = [np.concatenate(madpose.get_depths_batch([IMAGE] * a.pairs, [maps[m] for m in map_ids[:, s]], kp[s]))
                 .astype(np.float64) for s in (0, 1)]
            return A.create(lib, d[0], d[1])
        run["d_host_get_depths"], km = timed(host_maps, destroy(lib), a.repeats, lambda h: A.digest(lib, h))
        run["d_device_maps"], kdm = timed(lambda: A.device_set(t64, depth_maps=tmaps, map_ids=map_ids,
                                                               image_sizes=sizes), close, a.repeats,
                                          lambda ps: A.digest(lib, ps._h))
        # e: data that starts on the host
        def from_host():
            t = cuda(A.dev)
            return A.device_set(t, depth0=t[2], depth1=t[3])
        run["e_numpy_to_device"], ke = timed(from_host, close, a.repeats, lambda ps: A.digest(lib, ps._h))
        if not (ka == kb == kd == ke and kb32 == kd32 and km == kdm):
            raise SystemExit(f"pair_set_ingest_bench: sets differ: parent {ka[:12]} host {kb[:12]} device {kd[:12]} "
                             f"from-host {ke[:12]}; f32 host {kb32[:12]} device {kd32[:12]}; maps host {km[:12]} "
                             f"device {kdm[:12]}")
        run["digests_equal"] = True
        # f: create + ransac + close
        def chain(make):
            def go():
                t0 = time.perf_counter()
                ps = make()
                rs = ps.ransac(budget=512, step=64, lo=1, seed=11)
                ps.close()
                return time.perf_counter() - t0, ransac_key(rs)
            go()
            got = [go() for _ in range(a.repeats)]
            keys = {k for _, k in got}
            if len(keys) != 1:
                raise SystemExit("pair_set_ingest_bench: two chains returned different bytes")
            return spread([t for t, _ in got]), keys.pop()
        run["f_host_chain"], kf = chain(A.host_set)
        run["f_device_chain"], kfd = chain(lambda: A.device_set(t64, depth0=t64[2], depth1=t64[3]))
        if kf != kfd:
            raise SystemExit("pair_set_ingest_bench: ransac on the device-built set returned other bytes")
        run["ransac_bytes_equal"] = True
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
