#!/usr/bin/env python3
"""Clips a straight made by pg_make_paths round a cone and a parked car (pg_clip_tubes): the sets "cone", "car" and "both", as a user would sweep them.  For every obstacle
that a knot sees, vehicles.pass_by_around proposes the pass-by that goes round it, and pg_offset_paths on the CLIPPED tube says whether the proposal stays inside
(n_outside).

Prints per set the stats of pg_clip_tubes (width_min and where, the clipped, blocked and centre-out knots, the obstacles seen and ignored), per obstacle its report
(closest knot, side, the seeing knots, what is left on either side) and the proposal with its n_outside next to the identity's.
Then, with --time, the median over --reps calls after one warm-up (host clock around the synchronous call) of pg_clip_tubes at 8 paths x 512 sets of 4 obstacles x 1000
knots (circles of R = 50 m, the discs spread along them, every second set with a taper) with channels_out = NULL and with its download, and the numpy twin
(tests/tube_clip_numpy.py) on --twin-pairs of the same pairs on this host.  The kernel's own time (k_tube_clip) comes from running this script under
`rocprofv3 --kernel-trace --stats`.
usage: tools/gpu_clip_tubes.py [--cone 80,0.5,0.3] [--car 140,2.2,1.1] [--margin 1.0] [--taper 0.25] [--ramp 30] [--precision f64] [--time] [--reps 9] [--twin-pairs 3]"""
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
    ap.add_argument("--cone", default="80,0.5,0.3", help="arc length, metres to the left, radius")
    ap.add_argument("--car", default="140,2.2,1.1")
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--taper", type=float, default=0.25)
    ap.add_argument("--ramp", type=float, default=30.0)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--twin-pairs", type=int, default=3)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 8, precision=a.precision)
    src, _ = mpc.make_paths([V.line_segments(250.0)], n_knots=251, V_ref=10.0)
    cone = V.obstacle_at(src[0], *[float(x) for x in a.cone.split(",")])
    car = V.obstacle_at(src[0], *[float(x) for x in a.car.split(",")])
    kw = dict(margin=a.margin, taper=a.taper, min_width=2.0)
    names = ["cone", "car", "both"]
    members = [[cone], [car], [cone, car]]
    t0 = time.perf_counter()
    tubes, st, rep = mpc.clip_tubes(src, [V.obstacle_set(m, **kw) for m in members])
    ms = (time.perf_counter() - t0) * 1e3
    print(f"pg_clip_tubes: 1 path x 3 sets, Lmax {len(src[0])}, {ms:.3f} ms (host clock, download included)")
    for k, name in enumerate(names):
        s = st[k]
        print(f"{name:>5s}: width_min {s['width_min']:.3f} m at u = {s['u_width_min']:.1f} m, clipped knots L / R {s['n_clip_L']} / {s['n_clip_R']}, blocked {s['n_blocked']}, "
              f"centre out {s['n_centre_out']}, seen {s['n_seen']}, ignored {s['n_ignored']}")
        for j in range(len(members[k])):
            r = rep[k, j]
            print(f"       obstacle {j}: closest knot {r['k_at']} (u {r['u_at']:.1f} m, {r['dist_at']:.3f} m away, a {r['a_at']:+.3f}, h {r['h_at']:.3f}), side {r['side']:+d}, "
                  f"seen by knots {r['k_first']} .. {r['k_last']}, free left {r['free_left']:.3f} / right {r['free_right']:.3f} m")
            if r["side"] == 0:
                continue
            try:
                pb = V.pass_by_around(r, src[0], a.ramp)
            except ValueError as e:
                print(f"         no proposal: {e}")
                continue
            _, ost = mpc.offset_paths([tubes[k]], [V.offset(), pb])
            print(f"         proposal: pass_by({pb['d1']:+.3f}, {pb['s_a']:.1f}, {pb['s_b']:.1f}, {pb['s_c']:.1f}, {pb['s_d']:.1f}): n_outside {ost['n_outside'][1]} "
                  f"(the centre line: {ost['n_outside'][0]}), kappa_abs_max {ost['kappa_abs_max'][1]:.4f} 1/m")
    if a.time:
        n_path, n_sets, n_knots, per_set = 8, 512, 1000, 4
        circ, _ = mpc.make_paths([V.circle_segments(50.0)] * n_path, n_knots=n_knots, closed=True)
        L, ch, cl = mpc.pack_paths(circ, closed=True)
        length = float(circ[0].s[-1] - circ[0].s[0])
        sets = []
        for j in range(n_sets):
            discs = [V.obstacle_at(circ[0], (0.05 + 0.9 * ((j * per_set + i) % 97) / 97.0) * length, ((j + i) % 7 - 3) * 0.9, 0.4 + 0.1 * (i % 3)) for i in range(per_set)]
            sets.append(V.obstacle_set(discs, margin=1.0, taper=0.25 if j % 2 else float("inf"), min_width=2.0, policy=j % 4))
        arr, obs, n_obs = mpc.pack_obstacle_sets(sets)
        out = np.zeros((n_path * n_sets, 10, n_knots))
        p = pkg.mpc._p; c_i32p = pkg.mpc.c_i32p
        call = lambda o: mpc._chk(mpc.lib.pg_clip_tubes(mpc.h, n_path, n_knots, p(L, c_i32p), p(cl, c_i32p), p(ch), n_sets, arr, n_obs, obs, 0, None, None, p(o), None, None), "pg_clip_tubes")
        r = dict(call=median_ms(lambda: call(None), a.reps), down=median_ms(lambda: call(out), a.reps))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import tube_clip_numpy as twin
        ob = [(o.E, o.N, o.radius) for o in obs]
        t0 = time.perf_counter()
        for j in range(a.twin_pairs):
            S = twin.obstacle_set(first=arr[j + 1].first, count=arr[j + 1].count, margin=arr[j + 1].margin, taper=arr[j + 1].taper, min_width=arr[j + 1].min_width, policy=arr[j + 1].policy)
            twin.clip(ch[0], S, ob, True)
        tw = (time.perf_counter() - t0) * 1e3 / max(a.twin_pairs, 1)
        print(f"{n_path} paths x {n_sets} sets of {per_set} obstacles x {n_knots} knots ({mpc.precision}), median of {a.reps} calls, host clock: pg_clip_tubes {r['call']:.3f} ms, with the "
              f"download of channels_out {r['down']:.3f} ms (the download: {r['down'] - r['call']:.3f}); the numpy twin on this host: {tw:.1f} ms per pair, "
              f"{tw * n_path * n_sets / 1e3:.1f} s for the same call")
    mpc.close()


if __name__ == "__main__":
    main()
