#!/usr/bin/env python3
"""Plans friction-limited speed profiles on the GPU (pg_plan_speeds) for a chosen path library x plan-set grid and prints the stats table and the rates.

The paths are committed fixtures (tests/golden/paths; --paths a,b,c; --copies N repeats the list N times; --closed lists the names declared closed, default the three
ovals whose last knot is their first: skidpadoval, newskidpadoval, flidpadoval).  The sets are a grid: --mu-scale 0.5,0.9 x --v-max 20 (every combination), repeated
--set-copies times to fill a batch.  Prints per (path, set) of the first copy t_end, v_min, v_max, usage_max and the limiter counts, then ms per call (host clock around
the synchronous call, --reps calls after one warm-up: uploads and downloads included) and knots planned per second.
Kernel times (k_speed_plan, k_speed_plan_copy) come from running this script under
`rocprofv3 --kernel-trace --stats`; the copy's share of the HBM peak is its bytes written (7 channels of every valid knot and the zero tails, per output) over its time.
usage: tools/gpu_speed_plan.py [--paths skidpadoval,vail] [--copies 1] [--closed skidpadoval] [--mu-scale 0.5,0.9] [--v-max 20] [--set-copies 1] [--precision f64] [--reps 5] [--lanes 0]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ALL = ["EastPaddock", "flidpadoval", "newskidpadoval", "paddockoval", "skidpadoval", "vail", "variable_speed", "westpaddock"]
OVALS = ["skidpadoval", "newskidpadoval", "flidpadoval"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default=",".join(ALL))
    ap.add_argument("--copies", type=int, default=1)
    ap.add_argument("--closed", default=",".join(OVALS))
    ap.add_argument("--mu-scale", default="0.5,0.9")
    ap.add_argument("--v-max", default="20")
    ap.add_argument("--set-copies", type=int, default=1)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=0, choices=[0, 16, 32, 64], help="option speed_plan_lanes: sets per wavefront (0: by the size of the call)")
    a = ap.parse_args()
    pkg = entry._load_pkg()
    names = a.paths.split(",") * a.copies
    closed_names = set(a.closed.split(",")) if a.closed else set()
    paths = [pkg.load_path_fixture(n) for n in names]
    closed = [n in closed_names for n in names]
    grid = [pkg.vehicles.speed_plan(mu_scale=float(mu), V_max=float(v)) for mu in a.mu_scale.split(",") for v in a.v_max.split(",")]
    sets = grid * a.set_copies
    mpc = pkg.BatchedTrajectoryTrackingMPC(paths[0], 8, precision=a.precision)
    mpc.set_option("speed_plan_lanes", a.lanes)
    tubes, stats = mpc.plan_speeds(paths, sets, closed=closed)          # warm-up (loads the code object)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        mpc.plan_speeds(paths, sets, closed=closed)
    ms = (time.perf_counter() - t0) / a.reps * 1e3
    print(f"{'path':16s} {'closed':6s} {'mu_scale':>8s} {'V_max':>6s} {'t_end':>9s} {'v_min':>7s} {'v_max':>7s} {'usage':>7s} {'cap':>5s} {'accel':>5s} {'brake':>5s}")
    for i, n in enumerate(names[:len(names) // a.copies]):
        for j, sp in enumerate(grid):
            s = stats[i * len(sets) + j]
            print(f"{n:16s} {str(closed[i]):6s} {sp['mu_scale']:8.3f} {sp['V_max']:6.1f} {s['t_end']:9.3f} {s['v_min']:7.3f} {s['v_max']:7.3f} {s['usage_max']:7.4f} "
                  f"{s['n_cap']:5d} {s['n_accel']:5d} {s['n_brake']:5d}")
    knots = sum(len(p) for p in paths) * len(sets)
    Lmax = max(len(p) for p in paths)
    elem = 4 if a.precision == "f32" else 8
    copy_bytes = elem * (7 * knots + 10 * sum(Lmax - len(p) for p in paths) * len(sets))
    print(f"{len(paths)} paths x {len(sets)} sets, Lmax {Lmax}: {knots} knots planned; {ms:.3f} ms per call (host clock, transfers included), {knots / ms * 1e3:.3e} knots/s; "
          f"the copy kernel writes {copy_bytes} bytes per call ({mpc.precision})")
    mpc.close()


if __name__ == "__main__":
    main()
