#!/usr/bin/env python3
"""Refines the recorded vail track and a coarse straight (pg_refine_paths): knots every --ds metres everywhere, knots for a lane change (vehicles.refine_for) and knots
round a cone the coarse straight does not see (vehicles.refine_around on the report of pg_clip_tubes), then offsets and clips the refined straight.

Prints one table: per (path, set) the stats of pg_refine_paths (knots in and out, m_max, ds_min / ds_max, closure_pos_max, closure_psi_max, kappa_abs_max); then the length
error of the lane change and the cone's report on the coarse and on the refined straight.
Then, with --time, the median over --reps calls after one warm-up (host clock around the synchronous call) of pg_refine_paths at 8 paths x 64 sets x 500 knots (circles
of R = 50 m; the identity, ds alone, one window and two overlapping windows in turn; Lmax_out = the largest L_out) with channels_out = NULL and with its download, and
--twin-pairs of the same pairs checked against the numpy twin (tests/path_refine_numpy.py) on this host: the exact channels bit for bit, E and N within the header's bar.
The kernel's own time (k_path_refine) comes from running this script under `rocprofv3 --kernel-trace --stats`.
usage: tools/gpu_refine_paths.py [--ds 1.0] [--knots 10] [--precision f64] [--time] [--reps 9] [--twin-pairs 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def median_ms(call, reps):
    call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ds", type=float, default=1.0)
    ap.add_argument("--knots", type=int, default=10)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--twin-pairs", type=int, default=3)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    vail = pkg.load_path_fixture("vail")
    mpc = pkg.BatchedTrajectoryTrackingMPC(vail, 8, precision=a.precision)
    line, _ = mpc.make_paths([V.line_segments(390.0)], n_knots=40, V_ref=6.0)
    lane = V.lane_change(0.0, 1.5, 212.0, 217.0)
    cone = V.obstacle_at(line[0], 214.0, 0.3, 1.5)
    _, _, rep = mpc.clip_tubes(line, [V.obstacle_set([cone])])
    sets = [V.refine(), V.refine(ds=a.ds), V.refine_for(lane, knots=a.knots), V.refine_around(rep[0, 0], line[0], 0.5, 2.0, radius=1.5)]
    labels = ["identity", f"ds {a.ds:g}", "for the lane change", "round the cone"]
    names = ["vail", "line"]
    t0 = time.perf_counter()
    tubes, st = mpc.refine_paths([vail, line[0]], sets)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"pg_refine_paths: 2 paths x {len(sets)} sets, Lmax {len(vail)}, Lmax_out {max(len(t) for t in tubes)}, {ms:.3f} ms (host clock, sizing and download included)")
    print(f"{'path':>5s} {'set':>20s} {'L':>5s} {'L_out':>6s} {'m_max':>5s} {'ds_min':>8s} {'ds_max':>8s} {'closure_pos':>11s} {'closure_psi':>11s} {'k_max':>8s}")
    for k, t in enumerate(tubes):
        s = st[k]
        print(f"{names[k // len(sets)]:>5s} {labels[k % len(sets)]:>20s} {len(t) - s['n_added']:5d} {len(t):6d} {s['m_max']:5d} {s['ds_min']:8.4f} {s['ds_max']:8.4f} "
              f"{s['closure_pos_max']:11.3e} {s['closure_psi_max']:11.3e} {s['kappa_abs_max']:8.5f}")
    for label, src in (("coarse", line[0]), ("refined for the lane change", tubes[len(sets) + 2]), ("refined round the cone", tubes[len(sets) + 3])):
        _, ost = mpc.offset_paths([src], [lane])
        _, cst, crep = mpc.clip_tubes([src], [V.obstacle_set([cone])])
        print(f"  the straight, {label}: {len(src)} knots; the lane change adds {ost['length'][0] - 390.0:.12f} m; the cone: side {crep[0, 0]['side']}, "
              f"seen by the knots {crep[0, 0]['k_first']} .. {crep[0, 0]['k_last']}")
    if a.time:
        n_path, n_sets, n_knots = 8, 64, 500
        src, _ = mpc.make_paths([V.circle_segments(50.0)] * n_path, n_knots=n_knots, closed=True)
        L, ch, cl = mpc.pack_paths(src, closed=True)
        kinds = [V.refine(), V.refine(ds=0.2), V.refine(windows=[(40.0, 70.0, 0.05)]), V.refine(windows=[(10.0, 120.0, 0.3), (100.0, 160.0, 0.1)])]
        arr = mpc.pack_refines([kinds[j % len(kinds)] for j in range(n_sets)])
        Lo = mpc.refined_lengths(L, ch, arr)
        Lmax_out = int(Lo.max())
        out = np.zeros((n_path * n_sets, 10, Lmax_out))
        p = pkg.mpc._p; c_i32p = pkg.mpc.c_i32p
        call = lambda o: mpc._chk(mpc.lib.pg_refine_paths(mpc.h, n_path, n_knots, p(L, c_i32p), p(cl, c_i32p), p(ch), n_sets, arr, Lmax_out, 0, None, None, p(o), None), "pg_refine_paths")
        r = dict(call=median_ms(lambda: call(None), a.reps), down=median_ms(lambda: call(out), a.reps))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import path_refine_numpy as twin
        t0 = time.perf_counter()
        worst = 0.0
        for j in range(1, 1 + a.twin_pairs):
            S = twin.refine_set(ds=arr[j].ds, windows=[(arr[j].s_lo[q], arr[j].s_hi[q], arr[j].ds_w[q]) for q in range(4)])
            ref = twin.refine(ch[0], S)
            n = len(ref["s"])
            assert n == Lo[j], (j, n, Lo[j])
            if a.precision == "f64":
                for c, name in enumerate(twin.CHANNELS):
                    if name in ("E", "N"):
                        d = float(np.max(np.abs(out[j, c, :n] - ref[name]))); worst = max(worst, d)
                        assert np.all(np.abs(out[j, c, :n] - ref[name]) <= 8.0 * 2.0 ** -52 * (np.abs(ref[name]) + float(np.max(np.diff(ch[0, 1]))))), (j, name, d)
                    else:
                        assert out[j, c, :n].tobytes() == ref[name].tobytes(), (j, name)
        tw = (time.perf_counter() - t0) * 1e3 / max(a.twin_pairs, 1)
        print(f"{n_path} paths x {n_sets} sets x {n_knots} knots -> Lmax_out {Lmax_out}, {int(Lo.sum())} knots in all ({mpc.precision}), median of {a.reps} calls, host clock: "
              f"pg_refine_paths {r['call']:.3f} ms, with the download of channels_out {r['down']:.3f} ms (the download: {r['down'] - r['call']:.3f}); {a.twin_pairs} pairs against "
              f"the numpy twin: exact channels bit for bit, worst |E or N - twin| {worst:.3e} m; the twin on this host: {tw:.1f} ms per pair, {tw * n_path * n_sets / 1e3:.1f} s for the same call")
    mpc.close()


if __name__ == "__main__":
    main()
