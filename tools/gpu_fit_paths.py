#!/usr/bin/env python3
"""Fits the committed ovals to their own knots thinned to every 1st, 4th and 16th (pg_fit_paths, closed), plans their speed profiles (pg_plan_speeds), installs them and
drives one instance along each.

Prints one table: per (oval, every) the waypoints, the stats of pg_fit_paths (length, turn, closure_psi, kappa_abs_max, chord_min / chord_max, s_err_max), the largest
|psi - file| and |kappa - file| at equal s / total, the planned profile (t_end, v_max, usage_max) and -- the planned library installed, one instance per path started on it at
the planned speed -- the tracking summary of --steps steps of 0.01 s (max |e|, first_exit, the statuses seen).
Then, with --time, the median over --reps calls after one warm-up (host clock around the synchronous call) at two shapes, 8 paths x 1000 waypoints x 1000 knots and 4096
paths x 64 waypoints x 256 knots (circles): pg_fit_paths with channels_out = NULL, the same with the download of channels_out, the same waypoints at 3 knots per path (the
spline alone: chords, recurrences, span lengths), and pg_make_paths at the same output size.  Kernel times (k_path_fit, k_path_make) come from running this script under
`rocprofv3 --kernel-trace --stats`.
usage: tools/gpu_fit_paths.py [--paths skidpadoval,flidpadoval,newskidpadoval] [--every 1,4,16] [--mu-scale 0.5] [--v-max 10] [--steps 100] [--precision f64] [--time] [--reps 9]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SHAPES = ((8, 1000, 1000), (4096, 64, 256))


def median_ms(call, reps):
    call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="skidpadoval,flidpadoval,newskidpadoval")
    ap.add_argument("--every", default="1,4,16")
    ap.add_argument("--mu-scale", type=float, default=0.5)
    ap.add_argument("--v-max", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    names = a.paths.split(","); everys = [int(e) for e in a.every.split(",")]
    files = {n: pkg.load_path_fixture(n) for n in names}
    grid = [(n, e) for n in names for e in everys]
    entries = [dict(waypoints=V.waypoints_from_tube(files[n], e, closed=True), n_knots=len(files[n]), V_ref=6.0, closed=True) for n, e in grid]
    n = len(grid)
    mpc = pkg.BatchedTrajectoryTrackingMPC(files[names[0]], max(n, 8), precision=a.precision)
    mpc.set_option("tracking_summary", 1)
    fitted, closed, st = mpc.fit_paths(entries)
    tubes, ps = mpc.plan_speeds(fitted, V.speed_plan(mu_scale=a.mu_scale, V_max=a.v_max), closed=closed, install=True)
    state = np.zeros((n, 6)); t0 = np.zeros(n)
    for b, t in enumerate(tubes):
        k = len(t) // 10
        state[b] = [t.E[k], t.N[k], t.psi[k], t.V[k], 0.0, t.V[k] * t.kappa[k]]
        t0[b] = t.t[k]
    mpc.set_trajectory_index(np.arange(n, dtype=np.int32))
    mpc.set_inputs(state, np.zeros((n, 3)), t0, time_offset=np.zeros(n))
    seen = [set() for _ in range(n)]
    for _ in range(a.steps):
        mpc.simulate_(1, dt=0.01)
        for b, s in enumerate(mpc.solve_info()[0]):
            seen[b].add(int(s))
    summary, steps, first_exit = mpc.tracking_summary()
    print(f"{'path':>15s} {'every':>5s} {'wps':>5s} {'length':>9s} {'turn':>9s} {'clos_psi':>9s} {'k_max':>8s} {'chord':>13s} {'s_err':>8s} {'d psi':>8s} {'d kappa':>8s} | "
          f"{'t_end':>7s} {'v_max':>6s} {'usage':>6s} | {'max|e|':>8s} {'exit':>5s} statuses")
    for b, (name, e) in enumerate(grid):
        s, q, f, t = st[b], ps[b], files[name], fitted[b]
        at = t.s / t.s[-1] * f.s[-1]
        dpsi = t.psi - np.interp(at, f.s, f.psi); dpsi -= round(float(dpsi[0]) / (2 * math.pi)) * 2 * math.pi
        dk = t.kappa - np.interp(at, f.s, f.kappa)
        print(f"{name:>15s} {e:5d} {len(entries[b]['waypoints']):5d} {s['length']:9.3f} {s['turn']:9.6f} {s['closure_psi']:9.2e} {s['kappa_abs_max']:8.5f} "
              f"{s['chord_min']:6.3f}/{s['chord_max']:6.3f} {s['s_err_max']:8.1e} {np.max(np.abs(dpsi)):8.2e} {np.max(np.abs(dk)):8.2e} | "
              f"{q['t_end']:7.3f} {q['v_max']:6.3f} {q['usage_max']:6.3f} | {summary[b, 0]:8.2e} {first_exit[b]:5d} {sorted(seen[b])}")
    if a.time:
        L = sys.modules["pigeon_jl_amd"]._lib
        for n_path, n_wp, n_knots in SHAPES:
            ring = [V.waypoint(E=50.0 * math.cos(2 * math.pi * k / n_wp), N=50.0 * math.sin(2 * math.pi * k / n_wp)) for k in range(n_wp)]
            specs, wps, _ = mpc.pack_fit_specs([dict(waypoints=ring, n_knots=n_knots, closed=True)])
            many = (L.pg_fit_spec * n_path)(*([specs[0]] * n_path))          # every path reads the one range of waypoints
            few = (L.pg_fit_spec * n_path)(*([specs[0]] * n_path))
            for s in few:
                s.n_knots = 3
            out = np.zeros((n_path, 10, n_knots))
            fit = lambda sp, o: mpc._chk(mpc.lib.pg_fit_paths(mpc.h, n_path, sp, len(wps), wps, n_knots, 0, None, None, None if o is None else o.ctypes.data_as(pkg.mpc.c_dp), None), "pg_fit_paths")
            mspecs, segs = mpc.pack_path_specs([V.circle_segments(50.0)] * n_path, n_knots, closed=True)
            make = lambda: mpc._chk(mpc.lib.pg_make_paths(mpc.h, n_path, mspecs, len(segs), segs, n_knots, 0, None, None, None, None), "pg_make_paths")
            r = dict(fit=median_ms(lambda: fit(many, None), a.reps), fit_down=median_ms(lambda: fit(many, out), a.reps), spline=median_ms(lambda: fit(few, None), a.reps),
                     make=median_ms(make, a.reps))
            print(f"{n_path} paths x {n_wp} waypoints x {n_knots} knots ({mpc.precision}), median of {a.reps} calls, host clock: pg_fit_paths {r['fit']:.3f} ms, with the download of "
                  f"channels_out {r['fit_down']:.3f} ms (the download: {r['fit_down'] - r['fit']:.3f}), at 3 knots per path {r['spline']:.3f} ms, pg_make_paths at the same output size {r['make']:.3f} ms")
    mpc.close()


if __name__ == "__main__":
    main()
