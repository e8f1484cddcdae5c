"""Measure PairSet.ransac's device outputs on the ScanNet stand-in: 1500
pairs (synthetic.scannet_pair, 1500-2500 correspondences each), calibrated and shared focal,
ps.ransac(budget=512, step=64, lo=1, seed=31).

  out      (imports torch first: the outputs are torch tensors)
           1 today      the call as before, then what a caller does today to have the results on
                        the device: the masks from the index lists in numpy, np.stack of the model
                        rows, both to the device with .cuda();
           2 device     the call with all five device outputs and lists=False;
           3 device+lists  the same with lists=True;
           4 nolists    lists=False alone;
           5 kernel     the output stage's row kernel alone (events around its launches,
                        mp_debug_ransac_out_stats, while profiling is enabled) and the bytes it
                        writes (25 per row) over that time.
  default  (no torch in the process) the default call, for the comparison with the parent commit:
           run the tool in alternating processes with --tree <a checkout of the parent> --legs
           default and without --tree.

Every time but the kernel's is a host clock around calls that end in a device synchronise, median
(min - max) of --repeats after a warm-up.  One GPU, one process.  Prints one JSON line per leg and
writes all of them to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "calibrated", 1: "shared_focal"}


def spread(ts, scale=1e3):
    return {"median_ms": scale * statistics.median(ts), "min_ms": scale * min(ts), "max_ms": scale * max(ts),
            "runs_ms": [round(scale * t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--budget", type=int, default=512)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--variants", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--legs", nargs="+", default=["out"])
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_out", "ransac_out_bench.json"))
    a = ap.parse_args()
    torch = None
    if "out" in a.legs:  # (before the library is loaded: one HIP runtime in the process)
        import torch
        torch.cuda.init()
    sys.path.insert(0, os.path.abspath(a.tree))
    import madpose
    from madpose_amd import _lib as L
    from madpose_amd import synthetic
    if "out" not in a.legs:
        assert "torch" not in sys.modules
    if madpose.device_count() < 1:
        sys.exit("ransac_out_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    lib = L.lib()
    pairs = [synthetic.scannet_pair(s) for s in range(a.pairs)]
    sizes = np.array([len(p["depth0"]) for p in pairs])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    R, ns = int(sizes.sum()), a.pairs
    kw = dict(budget=a.budget, step=a.step, lo=1, seed=31)
    out = {"tool": "ransac_out_bench", "tree": os.path.relpath(os.path.abspath(a.tree), ROOT), "pairs": a.pairs,
           "call": "ransac(budget=%d, step=%d, lo=1, seed=31)" % (a.budget, a.step), "repeats": a.repeats,
           "correspondences": R, "torch_in_process": torch is not None,
           "time": "host clock around calls that end in a device synchronise; median (min - max) after a warm-up",
           "legs": {}}

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

    for variant in a.variants:
        o, c = synthetic.example_options(NAMES[variant])
        with madpose.PairSet(variant, pairs, o, c) as ps:
            tag = NAMES[variant]
            if "default" in a.legs:
                report(f"{tag}/default_call", spread(timed(lambda: ps.ransac(**kw))))
            if "out" not in a.legs:
                continue

            def today():
                rs = ps.ransac(**kw)
                mask = np.zeros(R, dtype=np.uint8)
                for j, r in enumerate(rs):
                    m = mask[offs[j]:offs[j + 1]]
                    for t in range(3):
                        m[r.inlier_indices[t]] |= np.uint8(1 << t)
                rows = np.stack([r.model_row for r in rs])
                dm, dr = torch.from_numpy(mask).cuda(), torch.from_numpy(rows).cuda()
                torch.cuda.synchronize()
                return rs, dm, dr
            dev = dict(out_mask=torch.zeros(R, dtype=torch.uint8, device="cuda"),
                       out_errors=torch.zeros((3, R), dtype=torch.float64, device="cuda"),
                       out_models=torch.zeros((ns, 17), dtype=torch.float64, device="cuda"),
                       out_index=torch.zeros(ns, dtype=torch.int32, device="cuda"),
                       out_counts=torch.zeros((ns, 3), dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            rs, dm, dr = today()
            got = ps.ransac(**kw, **dev, lists=False)
            if (dev["out_mask"].cpu().numpy().tobytes() != dm.cpu().numpy().tobytes()
                    or dev["out_models"].cpu().numpy().tobytes() != dr.cpu().numpy().tobytes()
                    or [r.num_inliers for r in got] != [tuple(len(x) for x in r.inlier_indices) for r in rs]):
                raise SystemExit("ransac_out_bench: the device outputs differ from the lists")
            report(f"{tag}/winners", {"pairs_with_a_winner": int(sum(r.index >= 0 for r in rs)),
                                      "inlier_fraction_per_term":
                                          (np.sum([r.num_inliers for r in rs], axis=0) / R).round(4).tolist()})
            report(f"{tag}/1_today_call_then_masks_and_rows_to_the_device", spread(timed(today)))
            report(f"{tag}/1a_today_the_call_alone", spread(timed(lambda: ps.ransac(**kw))))
            report(f"{tag}/2_device_outputs_lists_false", spread(timed(lambda: ps.ransac(**kw, **dev, lists=False))))
            report(f"{tag}/3_device_outputs_lists_true", spread(timed(lambda: ps.ransac(**kw, **dev))))
            report(f"{tag}/4_lists_false_alone", spread(timed(lambda: ps.ransac(**kw, lists=False))))
            n, ms = ctypes.c_int64(), ctypes.c_double()
            L.check(lib.mp_profile_enable(1))
            try:
                ps.ransac(**kw, **dev, lists=False)
                ts = []
                for _ in range(a.repeats):
                    L.check(lib.mp_debug_ransac_out_stats(None, None, 1))
                    ps.ransac(**kw, **dev, lists=False)
                    L.check(lib.mp_debug_ransac_out_stats(ctypes.byref(n), ctypes.byref(ms), 1))
                    ts.append(ms.value * 1e-3)
            finally:
                L.check(lib.mp_profile_enable(0))
            s = spread(ts)
            s.update(launches_per_call=int(n.value), bytes_written=25 * R,
                     write_rate_GBps=25 * R / statistics.median(ts) * 1e-9)
            report(f"{tag}/5_kernel_mask_and_errors", s)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
