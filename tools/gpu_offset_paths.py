#!/usr/bin/env python3
"""Offsets the clothoid oval (pg_make_paths) and the recorded vail track into lanes and into a pass-by (pg_offset_paths), re-plans their speed profiles for the new
curvature (pg_plan_speeds), installs them and runs a short rollout in which a route event hands every second instance over from the centre line to the pass-by.

Prints one table: per (path, set) the stats of pg_offset_paths (length, ds_min / ds_max, kappa_abs_max, x_min, d_abs_max, closure_pos, n_outside) and the planned profile
(t_end, v_min, v_max); then per instance of the rollout the trajectory it ends on, its largest |e| and first_exit.
Then, with --time, the median over --reps calls after one warm-up (host clock around the synchronous call) of pg_offset_paths at 8 paths x 512 sets x 1000 knots (circles
of R = 50 m; lanes, lane changes and pass-bys in turn) with channels_out = NULL and with its download, and the numpy twin (tests/path_offset_numpy.py) on --twin-pairs of
the same pairs on this host.  The kernel's own time (k_path_offset) comes from running this script under `rocprofv3 --kernel-trace --stats`.
usage: tools/gpu_offset_paths.py [--lane 1.5] [--pass-by 2.0,20,35,45,60] [--mu-scale 0.5] [--steps 120] [--event-step 40] [--precision f64] [--time] [--reps 9] [--twin-pairs 3]"""
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
    ap.add_argument("--lane", type=float, default=1.5)
    ap.add_argument("--pass-by", default="2.0,20,35,45,60")
    ap.add_argument("--mu-scale", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--event-step", type=int, default=40)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--twin-pairs", type=int, default=3)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    vail = pkg.load_path_fixture("vail")
    B = 8
    mpc = pkg.BatchedTrajectoryTrackingMPC(vail, B, precision=a.precision)
    mpc.set_option("tracking_summary", 1)
    oval, _ = mpc.make_paths([V.oval_segments(40.0, 14.5, 15.0)], n_knots=400, closed=True)
    names = ["oval", "vail"]; closed = [1, 0]
    pb = [float(x) for x in a.pass_by.split(",")]
    sets = [V.lane(0.0), V.lane(a.lane), V.lane(-a.lane), V.pass_by(*pb)]
    labels = ["lane 0", f"lane {a.lane:+g}", f"lane {-a.lane:+g}", "pass-by"]
    ns = len(sets)
    t0 = time.perf_counter()
    lanes, st = mpc.offset_paths([oval[0], vail], sets, closed=closed)
    ms = (time.perf_counter() - t0) * 1e3
    tubes, ps = mpc.plan_speeds(lanes, V.speed_plan(mu_scale=a.mu_scale), closed=np.repeat(closed, ns), install=True)
    print(f"pg_offset_paths: 2 paths x {ns} sets, Lmax {max(len(oval[0]), len(vail))}, {ms:.3f} ms (host clock, download included)")
    print(f"{'path':>5s} {'set':>10s} {'length':>9s} {'ds_min':>8s} {'ds_max':>8s} {'k_max':>8s} {'x_min':>6s} {'d_max':>6s} {'closure':>8s} {'outside':>7s} | {'t_end':>7s} {'v_min':>6s} {'v_max':>6s}")
    for k in range(2 * ns):
        s, q = st[k], ps[k]
        print(f"{names[k // ns]:>5s} {labels[k % ns]:>10s} {s['length']:9.3f} {s['ds_min']:8.4f} {s['ds_max']:8.4f} {s['kappa_abs_max']:8.5f} {s['x_min']:6.3f} {s['d_abs_max']:6.2f} "
              f"{s['closure_pos']:8.1e} {s['n_outside']:7d} | {q['t_end']:7.3f} {q['v_min']:6.3f} {q['v_max']:6.3f}")
    # the rollout, on the oval: instance b starts on the centre line 5 + b metres in; every second pair is handed over to the pass-by at --event-step
    home = np.zeros(B, dtype=np.int32)
    mpc.set_trajectory_index(home)
    routes = [V.route(), V.route(V.route_event(a.event_step, ns - 1, "project", relative=True))]
    mpc.set_routes(routes, np.array([(b // 2) % 2 for b in range(B)], dtype=np.int32))
    state = np.zeros((B, 6)); t_in = np.zeros(B)
    for b in range(B):
        t = tubes[home[b]]
        k = int(np.searchsorted(t.s - t.s[0], 5.0 + b))
        state[b] = [t.E[k], t.N[k], t.psi[k], t.V[k], 0.0, t.V[k] * t.kappa[k]]
        t_in[b] = t.t[k]
    mpc.set_inputs(state, np.zeros((B, 3)), t_in, time_offset=np.zeros(B))
    mpc.simulate_(a.steps, dt=0.01)
    summary, steps, first_exit = mpc.tracking_summary()
    rs = mpc.route_state()
    print(f"rollout of {a.steps} steps, route event at step {a.event_step}:")
    for b in range(B):
        print(f"  instance {b}: home {home[b]} ({names[home[b] // ns]}), ends on trajectory {rs['traj'][b]} ({labels[rs['traj'][b] % ns]}), events fired {rs['fired'][b]}, "
              f"max |e| {summary[b, 0]:.3f} m, s of the last step {summary[b, 5]:.2f} m, first_exit {first_exit[b]}")
    if a.time:
        n_path, n_sets, n_knots = 8, 512, 1000
        src, _ = mpc.make_paths([V.circle_segments(50.0)] * n_path, n_knots=n_knots, closed=True)
        L, ch, cl = mpc.pack_paths(src, closed=True)
        kinds = [V.lane(0.0), V.lane(3.5), V.lane(-3.5), V.pass_by(3.0, 40.0, 70.0, 120.0, 160.0), V.pass_by(-2.0, 10.0, 20.0, 20.0, 30.0), V.lane(2.0, edge_mode=1)]
        arr = mpc.pack_offsets([kinds[j % len(kinds)] for j in range(n_sets)])
        out = np.zeros((n_path * n_sets, 10, n_knots))
        p = pkg.mpc._p; c_i32p = pkg.mpc.c_i32p
        call = lambda o: mpc._chk(mpc.lib.pg_offset_paths(mpc.h, n_path, n_knots, p(L, c_i32p), p(cl, c_i32p), p(ch), n_sets, arr, 0, None, None, p(o), None), "pg_offset_paths")
        r = dict(call=median_ms(lambda: call(None), a.reps), down=median_ms(lambda: call(out), a.reps))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import path_offset_numpy as twin
        t0 = time.perf_counter()
        for j in range(a.twin_pairs):
            twin.offset(ch[0], {n: getattr(arr[j + 1], n) for n, _ in arr[0]._fields_}, True)
        tw = (time.perf_counter() - t0) * 1e3 / a.twin_pairs
        print(f"{n_path} paths x {n_sets} sets x {n_knots} knots ({mpc.precision}), median of {a.reps} calls, host clock: pg_offset_paths {r['call']:.3f} ms, with the download of "
              f"channels_out {r['down']:.3f} ms (the download: {r['down'] - r['call']:.3f}); the numpy twin on this host: {tw:.1f} ms per pair, {tw * n_path * n_sets / 1e3:.1f} s for the same call")
    mpc.close()


if __name__ == "__main__":
    main()
