#!/usr/bin/env python3
"""Makes a grid of ovals on the GPU (pg_make_paths), plans their speed profiles (pg_plan_speeds), installs them and drives one instance along each.

The grid is every combination of --radius x --clothoid (m; combinations whose clothoids take the whole half turn are left out) with straights of --straight m, knots --ds m
apart, each oval declared closed.  Prints per oval the stats of pg_make_paths (length, turn, closure_pos, closure_psi, kappa_abs_max, ds) and of the planned profile
(t_end, v_min, v_max, usage_max), then -- the planned library installed, one instance per oval started on its first straight at the planned speed -- the tracking summary
of --steps steps of 0.01 s (max |e|, min Ux, first_exit, the statuses seen).  Last, ms per pg_make_paths call (host clock around the synchronous call, --reps calls after
one warm-up, channels_out = NULL: the kernel, the uploads of specs and segments, the stats download) and knots per second at two shapes: 8 paths x 4000 knots and
4096 paths x 1000 knots (the first oval of the grid at every shape).
Kernel times (k_path_make) come from running this script under `rocprofv3 --kernel-trace --stats`.
usage: tools/gpu_make_paths.py [--radius 8,14.5,40] [--clothoid 0,10,20] [--straight 40] [--ds 0.5] [--mu-scale 0.5] [--v-max 10] [--steps 100] [--precision f64] [--reps 5]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SHAPES = ((8, 4000), (4096, 1000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", default="8,14.5,40")
    ap.add_argument("--clothoid", default="0,10,20")
    ap.add_argument("--straight", type=float, default=40.0)
    ap.add_argument("--ds", type=float, default=0.5)
    ap.add_argument("--mu-scale", type=float, default=0.5)
    ap.add_argument("--v-max", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    grid = [(float(r), float(c)) for r in a.radius.split(",") for c in a.clothoid.split(",") if math.pi - float(c) / abs(float(r)) > 0]
    paths = [V.oval_segments(a.straight, r, c) for r, c in grid]
    n = len(paths)
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), max(n, 8), precision=a.precision)
    mpc.set_option("tracking_summary", 1)
    made, st = mpc.make_paths(paths, ds=a.ds, closed=True)
    tubes, ps = mpc.plan_speeds(made, V.speed_plan(mu_scale=a.mu_scale, V_max=a.v_max), closed=True, install=True)
    # one instance per oval, at knot 10 % of the way along the first straight, at the planned speed
    state = np.zeros((n, 6)); control = np.zeros((n, 3)); t0 = np.zeros(n)
    for b, t in enumerate(tubes):
        k = int(np.argmin(np.abs(t.s - 0.1 * a.straight)))
        state[b] = [t.E[k], t.N[k], t.psi[k], t.V[k], 0.0, t.V[k] * t.kappa[k]]
        t0[b] = t.t[k]
    mpc.set_trajectory_index(np.arange(n, dtype=np.int32))
    mpc.set_inputs(state, control, t0, time_offset=np.zeros(n))
    seen = [set() for _ in range(n)]
    for _ in range(a.steps):
        mpc.simulate_(1, dt=0.01)
        for b, s in enumerate(mpc.solve_info()[0]):
            seen[b].add(int(s))
    summary, steps, first_exit = mpc.tracking_summary()
    print(f"{'radius':>7s} {'cloth':>6s} {'knots':>6s} {'length':>9s} {'turn':>9s} {'clos_pos':>9s} {'clos_psi':>9s} {'k_max':>8s} {'ds':>7s} | {'t_end':>8s} {'v_min':>6s} {'v_max':>6s} "
          f"{'usage':>6s} | {'max|e|':>8s} {'min Ux':>7s} {'exit':>5s} statuses")
    for b, (r, c) in enumerate(grid):
        s, q = st[b], ps[b]
        print(f"{r:7.2f} {c:6.2f} {len(made[b]):6d} {s['length']:9.3f} {s['turn']:9.6f} {s['closure_pos']:9.2e} {s['closure_psi']:9.2e} {s['kappa_abs_max']:8.5f} {s['ds']:7.4f} | "
              f"{q['t_end']:8.3f} {q['v_min']:6.3f} {q['v_max']:6.3f} {q['usage_max']:6.3f} | {summary[b, 0]:8.2e} {summary[b, 4]:7.3f} {first_exit[b]:5d} {sorted(seen[b])}")
    # the rates: the raw call with channels_out = NULL, so that the time is the maker's and not the download's
    for n_path, n_knots in SHAPES:
        specs, segs = mpc.pack_path_specs([paths[0]] * n_path, n_knots, closed=True)
        call = lambda: mpc._chk(mpc.lib.pg_make_paths(mpc.h, n_path, specs, len(segs), segs, n_knots, 0, None, None, None, None), "pg_make_paths")
        call()
        t_0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        ms = (time.perf_counter() - t_0) / a.reps * 1e3
        print(f"{n_path} paths x {n_knots} knots ({mpc.precision}): {ms:.3f} ms per pg_make_paths call (host clock, channels_out = NULL), {n_path * n_knots / ms * 1e3:.3e} knots/s")
    mpc.close()


if __name__ == "__main__":
    main()
