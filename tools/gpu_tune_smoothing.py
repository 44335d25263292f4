#!/usr/bin/env python3
"""Smooths a committed recorded oval to a target rms on the device (pg_tune_smoothing): the weight is searched on the device, the result fitted with pg_fit_paths, and
lambda, its bracket, dev_rms and max |kappa - file| against the file's own k_1pm at equal s / total are printed, next to the interpolated survey's.
Then, with --time, two ways to the same bracket at 8 paths x 1000 waypoints and at 4096 paths x 64 waypoints (closed noisy circles), 3 rounds each, alternated
repetition by repetition after one warm-up of both, host clock around the synchronous calls:
  the device search   one pg_tune_smoothing call, waypoints_out (one block), stats and tune stats downloaded;
  the host loop       what the search replaces: per round one pg_smooth_waypoints call with the ladder's 17 sets, waypoints_out (17 blocks) downloaded, and the
                      narrowing of path 0's bracket on the host from stats.dev_rms (a round has one ladder; the device search narrows every path's own).
Both must end on the same bracket of path 0 (asserted).  Printed: both medians, the spread (max - min) between the host loop's repetitions, and whether the device search's median
is within that spread of the host loop's or below it.  The kernel's own time (k_wp_tune) comes from running this script under `rocprofv3 --kernel-trace --stats`, in a run
of its own.
usage: tools/gpu_tune_smoothing.py [--path skidpadoval] [--target 1.6e-5] [--lambda-lo 1e-4] [--lambda-hi 1e2] [--rounds 3] [--precision f64] [--time] [--reps 9]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def circle(n, seed):
    rng = np.random.RandomState(seed)
    th = np.cumsum(0.5 + rng.rand(n)); th = th / th[-1] * 2.0 * math.pi
    return [dict(E=round(50.0 * math.cos(t), 2), N=round(50.0 * math.sin(t), 2), edge_L=4.0, edge_R=-4.0) for t in th]


def ladder(lo, hi):
    c = [0.0] * 17
    c[0] = lo; c[16] = hi
    half = 8
    while half >= 1:
        for j in range(half, 16, 2 * half):
            c[j] = math.sqrt(c[j - half] * c[j + half])
        half //= 2
    return c


def host_loop(mpc, pkg, specs, wps, n_path, target, lo, hi, rounds):
    """the parent's way: `rounds` calls of pg_smooth_waypoints with 17 sets each, every block downloaded, the choice made here.  All paths share one ladder per round only
    in round 0; afterwards each path has its own bracket, so a round's 17 sets are per path -- 17 sets x n_path paths would smooth every path under every other path's
    ladder.  The loop therefore keeps ONE bracket (path 0's) as a survey's user does who tunes a track and applies the weight to its runs; the device search is given
    the same job: its bracket of path 0 is the one compared."""
    V = pkg.vehicles
    out = (pkg._lib.pg_waypoint * (17 * len(wps)))()
    stats = (pkg._lib.pg_smooth_stats * (n_path * 17))()
    for r in range(rounds):
        c = ladder(lo, hi)
        if r >= 1 and any(a == b for a, b in zip(c, c[1:])):
            break
        arr = mpc.pack_smooths([V.smooth(lam=x) for x in c])
        mpc._chk(mpc.lib.pg_smooth_waypoints(mpc.h, n_path, specs, len(wps), wps, 17, arr, out, stats), "pg_smooth_waypoints")
        f = [stats[j].dev_rms for j in range(17)]                   # path 0
        if r == 0 and (f[0] > target or f[16] <= target):
            return (c[0], c[0]) if f[0] > target else (c[16], c[16])
        j = min(k for k in range(1, 17) if f[k] > target)
        lo, hi = c[j - 1], c[j]
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", default="skidpadoval")
    ap.add_argument("--target", type=float, default=1.6e-5)
    ap.add_argument("--lambda-lo", type=float, default=1e-4)
    ap.add_argument("--lambda-hi", type=float, default=1e2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", a.path + ".npz")))
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture(a.path), 8, precision=a.precision)
    n_knots = len(d["s_m"])
    paths = [dict(waypoints=V.waypoints_from_tube(d, 1, True), closed=True, n_knots=n_knots, V_ref=6.0)]
    t = V.tune(target=a.target, lambda_lo=a.lambda_lo, lambda_hi=a.lambda_hi, rounds=a.rounds)
    sm, st, tn = mpc.tune_smoothing(paths, [t])
    tubes, _, _ = mpc.fit_paths(paths + mpc.smoothed_fit_paths(paths, sm, 0))
    err = [float(np.max(np.abs(tb.kappa - np.interp(tb.s / tb.s[-1], d["s_m"] / d["s_m"][-1], d["k_1pm"])))) for tb in tubes]
    s = tn[0, 0]
    print(f"{a.path}: {len(paths[0]['waypoints'])} waypoints, closed, target {a.target:g} m rms in [{a.lambda_lo:g}, {a.lambda_hi:g}], {a.rounds} rounds ({mpc.precision})")
    print(f"  lambda {float(s['lam'])!r}, bracket [{float(s['lo'])!r}, {float(s['hi'])!r}], dev_rms {st['dev_rms'][0, 0]:.4e} m (at the bracket's upper end {s['rms_hi']:.4e}), verdict {int(s['verdict'])}, "
          f"rounds_done {int(s['rounds_done'])}, monotone {int(s['monotone'])}")
    print(f"  dev_max {st['dev_max'][0, 0]:.3e} m, max |kappa - file| {err[1]:.3e} 1/m smoothed, {err[0]:.3e} interpolated")
    if a.time:
        for n_path, n_wp in ((8, 1000), (4096, 64)):
            ps = [dict(waypoints=circle(n_wp, k % 8), closed=True, n_knots=3) for k in range(n_path)]
            specs, wps, _ = mpc.pack_fit_specs(ps)
            target, lo, hi, rounds = 2e-3, 1e-4, 1e2, 3
            arr = mpc.pack_tunes([V.tune(target=target, lambda_lo=lo, lambda_hi=hi, rounds=rounds)])
            out = (pkg._lib.pg_waypoint * len(wps))()
            stats = (pkg._lib.pg_smooth_stats * n_path)()
            tune = (pkg._lib.pg_tune_stats * n_path)()
            dev = lambda: mpc._chk(mpc.lib.pg_tune_smoothing(mpc.h, n_path, specs, len(wps), wps, 1, arr, out, stats, tune), "pg_tune_smoothing")
            host = lambda: host_loop(mpc, pkg, specs, wps, n_path, target, lo, hi, rounds)
            dev(); bracket = host()                                 # warm-up of both
            assert (tune[0].lo, tune[0].hi) == bracket, ((tune[0].lo, tune[0].hi), bracket)
            td, th = [], []
            for _ in range(a.reps):                                 # alternated
                t0 = time.perf_counter(); dev(); td.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); host(); th.append((time.perf_counter() - t0) * 1e3)
            md, mh, spread = float(np.median(td)), float(np.median(th)), float(max(th) - min(th))
            print(f"{n_path} paths x {n_wp} waypoints, {rounds} rounds ({mpc.precision}), median of {a.reps} alternated repetitions, host clock: pg_tune_smoothing {md:.3f} ms "
                  f"(min {min(td):.3f}, max {max(td):.3f}); the host loop of {rounds} x pg_smooth_waypoints with 17 sets {mh:.3f} ms (min {min(th):.3f}, max {max(th):.3f}, "
                  f"spread {spread:.3f}); path 0's bracket [{bracket[0]!r}, {bracket[1]!r}] on both; the device search is "
                  f"{'within the spread of or below' if md <= mh + spread else 'ABOVE'} the host loop ({mh / md:.2f} x)")
    mpc.close()


if __name__ == "__main__":
    main()
