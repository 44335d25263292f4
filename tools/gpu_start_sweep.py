#!/usr/bin/env python3
"""A start sweep on a made library: ovals from pg_make_paths, their speed profiles from pg_plan_speeds (installed), the batch placed on them by pg_make_starts, a rollout
and the tracking summary -- the planned channels never come to the host (pg_plan_speeds is called with channels_out = NULL; the geometry it is handed is the one
pg_make_paths returned, which that call takes from the host), and no channel is read on the host to place a car.

The grid is every combination of --radius x --mu-scale; instance b runs on tube b % n_tubes under start set (b // n_tubes) % n_sets, the sets being --offsets lateral
windows +-x m around the centre line (with the ranges of vehicles.start_config2 otherwise), along the first nine tenths of the tube (s_mode 1, [0, 0.9]).  Prints per (tube, set) the instances,
max |e|, the rms of e, min Ux, the exits of --steps steps of 0.01 s and the instances whose sum of e^2 is not finite (left out of the rms), then the wall time of make_starts (host clock around the synchronous call, install, every output
NULL; --reps calls after one warm-up) next to that of synthetic.config2_inputs + set_inputs + synchronize for the same B (on the host copy of tube 0 as pg_make_paths
returned it): a measurement, for EXPERIMENTS.md.
usage: tools/gpu_start_sweep.py [--radius 14.5,40] [--mu-scale 0.5,0.8] [--offsets 0.25,1.0] [--batch 4096] [--steps 50] [--precision f64] [--reps 5]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", default="14.5,40")
    ap.add_argument("--mu-scale", default="0.5,0.8")
    ap.add_argument("--offsets", default="0.25,1.0")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    B = a.batch
    paths = [V.oval_segments(40.0, float(r), 10.0) for r in a.radius.split(",")]
    plans = [V.speed_plan(mu_scale=float(x), V_max=10.0) for x in a.mu_scale.split(",")]
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), B, precision=a.precision, phase_timing=False)
    mpc.set_option("tracking_summary", 1)
    made, _ = mpc.make_paths(paths, ds=0.5, closed=True)
    L, ch, cl = mpc.pack_paths(made, True)
    arr = mpc.pack_speed_plans(plans)
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    mpc._chk(mpc.lib.pg_plan_speeds(mpc.h, len(L), ch.shape[2], p32(L), p32(cl), ch.ctypes.data_as(C.POINTER(C.c_double)), len(arr), arr, None, 1, None, None), "pg_plan_speeds")
    n_tubes = len(paths) * len(plans)
    offsets = [float(x) for x in a.offsets.split(",")]
    sets = [dict(V.start_config2(), s_hi=0.9, e_lo=-x, e_hi=x) for x in offsets]      # (the tube ends at its last knot: a car that passes it has no projection)
    b = np.arange(B)
    tube, which = (b % n_tubes).astype(np.int32), ((b // n_tubes) % len(sets)).astype(np.int32)
    mpc.set_trajectory_index(tube)
    mpc.make_starts(sets, index=which, seed=2024)
    mpc.simulate_(a.steps, dt=0.01)
    summary, steps, first_exit = mpc.tracking_summary()
    print(f"{'radius':>7s} {'mu':>5s} {'+-e':>5s} {'n':>6s} {'max|e|':>8s} {'rms e':>8s} {'min Ux':>7s} {'exits':>6s} {'no e':>6s}")
    for k in range(n_tubes):
        for j, x in enumerate(offsets):
            sel = (tube == k) & (which == j)
            if not sel.any():
                continue
            fin = sel & np.isfinite(summary[:, 1])                    # (an instance with a step that found no projection carries a NaN sum: counted, not averaged)
            rms = np.sqrt(np.sum(summary[fin, 1]) / max(1, int(np.sum(steps[fin]))))
            print(f"{a.radius.split(',')[k // len(plans)]:>7s} {a.mu_scale.split(',')[k % len(plans)]:>5s} {x:5.2f} {int(sel.sum()):6d} {np.nanmax(summary[sel, 0]):8.3f} {rms:8.4f} "
                  f"{np.nanmin(summary[sel, 4]):7.3f} {int(np.sum(first_exit[sel] >= 0)):6d} {int(sel.sum() - fin.sum()):6d}")
    # the two wall times, same B: the device call against the host's interpolation + draws + upload
    sarr = mpc.pack_starts(sets)
    on_device = lambda: mpc._chk(mpc.lib.pg_make_starts(mpc.h, B, len(sarr), sarr, p32(which), C.c_uint64(2024), None, 1, None, None, None, None, None, None), "pg_make_starts")

    def on_host():
        state, control, t0, toff = pkg.synthetic.config2_inputs(made[0], B, seed=2024, s_range=(0.0, float(made[0].s[-1])))
        mpc.set_inputs(state, control, t0, time_offset=toff)
        mpc.synchronize()
    for name, call in (("make_starts (install, outputs NULL)", on_device), ("config2_inputs + set_inputs + synchronize", on_host)):
        call()
        t_0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        print(f"B = {B} ({mpc.precision}): {(time.perf_counter() - t_0) / a.reps * 1e3:.3f} ms per {name} (host clock)")
    mpc.close()


if __name__ == "__main__":
    main()
