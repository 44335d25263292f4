#!/usr/bin/env python3
"""Finds the line of least bending energy inside the tube of a committed recorded oval on the device (pg_optimize_line): the file thinned to every --every-th point, one
call under a ladder of rho, then the surveyed line and every optimised one fitted with pg_fit_paths and planned with pg_plan_speeds, and the table: bend before and after,
the largest move, the active waypoints, the two ADMM residuals, the length, max |kappa| and the planned lap time.
Then, with --time, the median over --reps calls after one warm-up (host clock around the synchronous call, waypoints_out downloaded) of pg_optimize_line at 1 pair and at
256 pairs of that path with --iters iterations, against the numpy twin's host loop for one pair (tests/line_opt_numpy.py) and against nothing else, checked bit for bit
against the device.  The kernel's own time (k_line_opt) comes from running this script under `rocprofv3 --kernel-trace --stats`, in a run of its own.
usage: tools/gpu_optimize_line.py [--path skidpadoval] [--every 16] [--iters 1000] [--precision f64] [--time] [--reps 9]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

RHO = (0.01, 0.03, 0.1, 0.3, 1.0)


def median_ms(call, reps):
    call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", default="skidpadoval")
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", a.path + ".npz")))
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture(a.path), 8, precision=a.precision)
    w = V.waypoints_from_tube(d, a.every, True)
    P = np.array([[q["E"], q["N"]] for q in w])
    h_mean = float(np.mean(np.hypot(*(np.roll(P, -1, axis=0) - P).T)))
    paths = [dict(waypoints=w, closed=True, n_knots=400, V_ref=6.0)]
    sets = [V.line(h_mean=h_mean, rho=rho, iters=a.iters) for rho in RHO]
    lines, st = mpc.optimize_line(paths, sets)
    tubes, cl, _ = mpc.fit_paths(paths + [p for k in range(len(RHO)) for p in mpc.smoothed_fit_paths(paths, lines, k)])
    planned, _ = mpc.plan_speeds(tubes, [V.speed_plan()], closed=cl)
    print(f"{a.path}: every {a.every}th point, {len(w)} waypoints, mean chord {h_mean:.3f} m, closed, {a.iters} iterations, fitted at 400 knots ({mpc.precision})")
    print(f"{'rho h^3':>8s} {'bend_in':>8s} {'bend_out':>8s} {'|alpha|max':>10s} {'active':>6s} {'r_prim':>10s} {'r_dual':>10s} {'iters':>5s} {'length':>8s} {'|kappa|max':>10s} {'lap':>8s}")
    print(f"{'surveyed':>8s} {'':8s} {'':8s} {'':10s} {'':6s} {'':10s} {'':10s} {'':5s} {float(tubes[0].s[-1]):8.2f} {float(np.max(np.abs(tubes[0].kappa))):10.4f} {float(planned[0].t[-1]):8.3f}")
    for k, rho in enumerate(RHO):
        s, t = st[0, k], tubes[k + 1]
        print(f"{rho:8g} {s['bend_in']:8.4f} {s['bend_out']:8.4f} {s['alpha_abs_max']:10.3f} {int(s['n_active']):6d} {s['r_prim']:10.2e} {s['r_dual']:10.2e} {int(s['iters_done']):5d} "
              f"{float(t.s[-1]):8.2f} {float(np.max(np.abs(t.kappa))):10.4f} {float(planned[k + 1].t[-1]):8.3f}")
    if a.time:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import line_opt_numpy as twin
        one = V.line(h_mean=h_mean, iters=a.iters)
        t0 = time.perf_counter()
        ref = twin.optimize(w, True, twin.line_set(**one))
        tw = (time.perf_counter() - t0) * 1e3
        for n_path in (1, 256):
            ps = [dict(waypoints=w, closed=True, n_knots=3) for _ in range(n_path)]
            specs, wps, _ = mpc.pack_fit_specs(ps)
            arr = mpc.pack_lines([one])
            out = (pkg._lib.pg_waypoint * len(wps))()
            stats = (pkg._lib.pg_line_stats * n_path)()
            call = lambda: mpc._chk(mpc.lib.pg_optimize_line(mpc.h, n_path, specs, len(wps), wps, 1, arr, out, stats), "pg_optimize_line")
            ms = median_ms(call, a.reps)
            got = np.frombuffer(out, dtype=np.float64).reshape(len(wps), 4)[(n_path - 1) * len(w):]
            same = got.tobytes() == np.stack([ref["E"], ref["N"], ref["edge_L"], ref["edge_R"]], axis=1).tobytes()
            done = int(stats[n_path - 1].iters_done)
            print(f"{n_path} pairs x {len(w)} waypoints, {done} iterations ({mpc.precision}), median of {a.reps} calls, host clock, waypoints_out downloaded: pg_optimize_line "
                  f"{ms:.3f} ms = {ms * 1e3 / done:.2f} us per iteration of the launch; the last pair against the numpy twin: {'bit for bit' if same else 'DIFFERENT'}; the twin's "
                  f"host loop: {tw:.1f} ms per pair, {tw * 1e3 / done:.1f} us per iteration")
            assert same
    mpc.close()


if __name__ == "__main__":
    main()
