#!/usr/bin/env python3
"""Smooths a committed recorded path on the device (pg_smooth_waypoints) under a ladder of lambda in ONE call, fits every smoothed block and the interpolated one with
pg_fit_paths, and prints the lambda table: max |kappa - file| against the file's own k_1pm at equal s / total, and the per-pair stats the caller chooses lambda from
(dev_max, dev_rms, bend, pivot_min).
Then, with --time, the median over --reps calls after one warm-up (host clock around the synchronous call, waypoints_out downloaded) of pg_smooth_waypoints at
8 paths x 1000 waypoints x 16 sets and at 4096 paths x 64 waypoints x 1 set (closed noisy circles), and the numpy twin's time for one pair of each on this host
(tests/wp_smooth_numpy.py), checked bit for bit against the device.  The kernel's own time (k_wp_smooth) comes from running this script under
`rocprofv3 --kernel-trace --stats`, in a run of its own.
usage: tools/gpu_smooth_waypoints.py [--path skidpadoval] [--open] [--precision f64] [--time] [--reps 9]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

LADDER = (0.0, 1e-3, 1e-2, 1e-1, 1.0, 10.0)


def median_ms(call, reps):
    call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def circle(n, seed):
    rng = np.random.RandomState(seed)
    th = np.cumsum(0.5 + rng.rand(n)); th = th / th[-1] * 2.0 * math.pi
    return [dict(E=round(50.0 * math.cos(t), 2), N=round(50.0 * math.sin(t), 2), edge_L=4.0, edge_R=-4.0) for t in th]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", default="skidpadoval")
    ap.add_argument("--open", action="store_true", help="the file is an open path (vail): keep its last knot")
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", a.path + ".npz")))
    closed = not a.open
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture(a.path), 8, precision=a.precision)
    n_knots = len(d["s_m"])
    paths = [dict(waypoints=V.waypoints_from_tube(d, 1, closed), closed=closed, n_knots=n_knots, V_ref=6.0)]
    sm, st = mpc.smooth_waypoints(paths, [V.smooth(lam=lam) for lam in LADDER])
    tubes, _, _ = mpc.fit_paths([p for k in range(len(LADDER)) for p in mpc.smoothed_fit_paths(paths, sm, k)])
    print(f"{a.path}: {len(paths[0]['waypoints'])} waypoints, {'closed' if closed else 'open'}, fitted at {n_knots} knots ({mpc.precision})")
    print(f"{'lambda':>8s} {'|kappa - file|':>14s} {'dev_max':>10s} {'dev_rms':>10s} {'i_dev_max':>9s} {'bend':>10s} {'n_outside':>9s} {'pivot_min':>10s}")
    for k, (lam, t) in enumerate(zip(LADDER, tubes)):
        ref = np.interp(t.s / t.s[-1], d["s_m"] / d["s_m"][-1], d["k_1pm"])
        s = st[0, k]
        print(f"{lam:8g} {float(np.max(np.abs(t.kappa - ref))):14.3e} {s['dev_max']:10.3e} {s['dev_rms']:10.3e} {int(s['i_dev_max']):9d} {s['bend']:10.3e} {int(s['n_outside']):9d} "
              f"{s['pivot_min']:10.3e}")
    if a.time:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import wp_smooth_numpy as twin
        for n_path, n_wp, n_sets in ((8, 1000, 16), (4096, 64, 1)):
            ps = [dict(waypoints=circle(n_wp, k % 8), closed=True, n_knots=3) for k in range(n_path)]
            specs, wps, _ = mpc.pack_fit_specs(ps)
            lams = [0.1 * (j + 1) for j in range(n_sets)]
            arr = mpc.pack_smooths([V.smooth(lam=lam) for lam in lams])
            out = (pkg._lib.pg_waypoint * (n_sets * len(wps)))()
            stats = (pkg._lib.pg_smooth_stats * (n_path * n_sets))()
            call = lambda: mpc._chk(mpc.lib.pg_smooth_waypoints(mpc.h, n_path, specs, len(wps), wps, n_sets, arr, out, stats), "pg_smooth_waypoints")
            ms = median_ms(call, a.reps)
            t0 = time.perf_counter()
            ref = twin.smooth(ps[0]["waypoints"], True, twin.smooth_set(lam=lams[-1]))
            tw = (time.perf_counter() - t0) * 1e3
            got = np.frombuffer(out, dtype=np.float64).reshape(n_sets, len(wps), 4)[n_sets - 1, :n_wp]
            same = got.tobytes() == np.stack([ref["E"], ref["N"], ref["edge_L"], ref["edge_R"]], axis=1).tobytes()
            print(f"{n_path} paths x {n_wp} waypoints x {n_sets} sets ({mpc.precision}), median of {a.reps} calls, host clock, waypoints_out downloaded: pg_smooth_waypoints "
                  f"{ms:.3f} ms; pair (0, {n_sets - 1}) against the numpy twin: {'bit for bit' if same else 'DIFFERENT'}; the twin on this host: {tw:.1f} ms per pair, "
                  f"{tw * n_path * n_sets / 1e3:.2f} s for the same call")
            assert same
    mpc.close()


if __name__ == "__main__":
    main()
