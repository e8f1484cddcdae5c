#!/usr/bin/env python3
"""Throughput of the batched minimal solvers (madpose.solve_scale_shift_pose_batch,
relpose_batch) beside the single-sample entries, in one process.

For each of the three default MD solvers and the three point solvers: samples/s at
B = 1024 and B = 65536 (wall time over 5 calls after one warm-up, host packing and
copies included), and the per-call wall time of the single-sample entry over 256
samples.  Stops at the first error.

    python tools/solver_batch_bench.py [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import madpose  # noqa: E402
from tests import pt_samples  # noqa: E402

SIZES = (1024, 65536)
CALLS = 5
SINGLES = 256


def md_inputs(variant, n, rng):
    k = 3 if variant == 0 else 4
    x = np.concatenate([rng.standard_normal((n, k, 2)), np.ones((n, k, 1))], axis=2)
    y = np.concatenate([rng.standard_normal((n, k, 2)), np.ones((n, k, 1))], axis=2)
    return x, y, rng.uniform(0.5, 5, (n, k)), rng.uniform(0.5, 5, (n, k))


def pt_inputs(kind, n, rng):
    # 1024 distinct scenes, tiled: the per-sample work does not depend on the neighbours
    base = min(n, 1024)
    p0, p1 = pt_samples.random_samples(rng, base, (5, 6, 7)[kind])
    if kind == 0:
        p0, p1 = pt_samples.bearings(p0), pt_samples.bearings(p1)
    idx = np.arange(n) % base
    return np.ascontiguousarray(p0[idx]), np.ascontiguousarray(p1[idx])


def timed(fn):
    fn()  # warm-up
    t0 = time.perf_counter()
    for _ in range(CALLS):
        out = fn()
    return (time.perf_counter() - t0) / CALLS, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if madpose.device_count() < 1:
        raise SystemExit("no HIP device visible")
    madpose.set_device(a.device)
    rng = np.random.default_rng(7)
    md_single = [madpose.solve_scale_shift_pose, madpose.solve_scale_shift_pose_shared_focal,
                 madpose.solve_scale_shift_pose_two_focal]
    pt_single = [madpose.relpose_5pt, madpose.relpose_6pt_shared_focal, madpose.relpose_7pt_two_focal]
    print(f"{'solver':<14}{'B':>8}{'ms/call':>12}{'samples/s':>14}{'models':>10}   single-sample entry")
    for variant, name in enumerate(("md_cal", "md_sf", "md_tf")):
        x, y, dx, dy = md_inputs(variant, max(SIZES), rng)
        t0 = time.perf_counter()
        for s in range(SINGLES):
            md_single[variant](x[s].T, y[s].T, dx[s], dy[s])
        single = (time.perf_counter() - t0) / SINGLES
        for B in SIZES:
            dt, (_, n) = timed(lambda: madpose.solve_scale_shift_pose_batch(variant, x[:B], y[:B], dx[:B], dy[:B],
                                                                            device=a.device))
            print(f"{name:<14}{B:>8}{dt * 1e3:>12.3f}{B / dt:>14.0f}{int(n.sum()):>10}   "
                  f"{single * 1e6:.1f} us/call = {1 / single:.0f} samples/s ({B / dt * single:.0f}x)", flush=True)
    for kind, name in enumerate(("pt5", "pt6_sf", "pt7_tf")):
        p0, p1 = pt_inputs(kind, max(SIZES), rng)
        t0 = time.perf_counter()
        for s in range(SINGLES):
            pt_single[kind](p0[s], p1[s])
        single = (time.perf_counter() - t0) / SINGLES
        for B in SIZES:
            dt, (_, n) = timed(lambda: madpose.relpose_batch(kind, p0[:B], p1[:B], device=a.device))
            print(f"{name:<14}{B:>8}{dt * 1e3:>12.3f}{B / dt:>14.0f}{int(n.sum()):>10}   "
                  f"{single * 1e6:.1f} us/call = {1 / single:.0f} samples/s ({B / dt * single:.0f}x)", flush=True)


if __name__ == "__main__":
    main()
