#!/usr/bin/env python3
"""A hand-over sweep: "the planner hands over a lane change at step k", for a sweep of k crossed with a tuning library, in ONE batch and one rollout call.

The trajectory library is made on the device (pg_make_paths): tube 0 a straight, tube 1 the same straight with a lane change of --offset m over --length m that begins
--lead m down the road.  Every instance starts on tube 0 (its home); instance b runs under route set b % n_steps -- one PROJECT event "at clock step k go to tube 1, joined
where the car is" per --event-steps entry, plus the identity set -- and under tuning (b // n_sets) % n_tunings (--q-e: the lateral-error weight Q_e of the control-parameter
library).  Prints per (event step, tuning) the tracking summary on the trajectory each instance ended on -- instances, max |e|, rms e, min Ux, exits --, the largest
lateral offset at the join and how far to the left of the straight the cars ended (the lane change: --offset for those handed over, 0 for the others).  With the defaults
the cars start 2 to 10 m down the road at 6 m/s, the lane change runs from 15 to 55 m, and the hand-overs come before it (step 50), at its start (150) and inside it (250:
the car is then up to a metre beside the new tube); 900 steps carry every car past its end.

--cost: instead, the cost of the feature for EXPERIMENTS.md: ms per step of simulate_ (pg_simulate_dev) at --batch, fp64, median of --reps alternating runs of --steps
steps, for (a) no route library, (b) a library of eventless sets, (c) a PROJECT event on every instance at one step of the run.
usage: tools/gpu_route_sweep.py [--event-steps 50,150,250] [--q-e 0.5,1,2] [--offset 3.5] [--length 40] [--lead 15] [--batch 4096] [--steps 900] [--precision f64] [--cost] [--reps 5]"""
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
    ap.add_argument("--event-steps", default="50,150,250")
    ap.add_argument("--q-e", default="0.5,1,2")
    ap.add_argument("--offset", type=float, default=3.5)
    ap.add_argument("--length", type=float, default=40.0)
    ap.add_argument("--lead", type=float, default=15.0)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=900)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    V = pkg.vehicles
    B = a.batch
    total = a.lead + a.length + 120.0
    paths = [V.line_segments(total), V.line_segments(a.lead) + V.lane_change_segments(a.offset, a.length) + V.line_segments(120.0)]
    mpc = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), B, precision=a.precision, phase_timing=False)
    made, _ = mpc.make_paths(paths, ds=0.5, V_ref=6.0, install=True)
    mpc.set_trajectory_index(np.zeros(B, dtype=np.int32))
    state, control, t0, toff = pkg.synthetic.config2_inputs(made[0], B, seed=2024, s_range=(2.0, 10.0))

    if a.cost:
        k_ev = a.steps // 2
        variants = {"no route library": None, "eventless sets": [V.route()], "PROJECT on every instance at one step": [V.route(V.route_event(k_ev, 1, "project"))]}
        ms = {name: [] for name in variants}
        for rep in range(a.reps + 1):                            # (the first round warms up and is dropped)
            for name, sets in variants.items():
                mpc.clear_routes() if sets is None else mpc.set_routes(sets)
                mpc.reset(); mpc.set_inputs(state, control, t0, time_offset=toff); mpc.synchronize()
                t_0 = time.perf_counter()
                mpc.lib.pg_simulate_dev(mpc.h, a.steps, C.c_double(0.01), None, None); mpc.synchronize()
                if rep:
                    ms[name].append((time.perf_counter() - t_0) / a.steps * 1e3)
        for name, v in ms.items():
            print(f"B = {B} ({mpc.precision}), {a.steps} steps: {np.median(v):.5f} ms per step (median of {len(v)}; {min(v):.5f} .. {max(v):.5f})  {name}")
        print(f"k_route launches: {int(mpc.get_option('stat_route_steps'))}")
        mpc.close()
        return

    ev_steps = [int(x) for x in a.event_steps.split(",")]
    tunings = [float(x) for x in a.q_e.split(",")]
    sets = [V.route()] + [V.route(V.route_event(k, 1, "project")) for k in ev_steps]
    b = np.arange(B)
    which, tune = (b % len(sets)).astype(np.int32), ((b // len(sets)) % len(tunings)).astype(np.int32)
    mpc.set_routes(sets, which)
    mpc.set_control_params([{"Q_e": q} for q in tunings], tune)
    mpc.set_option("tracking_summary", 1)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    final = mpc.simulate_(a.steps, dt=0.01)[0]
    # the straight starts at made[0]'s first knot with heading psi (from North): its left normal is (-cos psi, -sin psi)
    E0, N0, psi0 = float(made[0].E[0]), float(made[0].N[0]), float(made[0].psi[0])
    left = -(final[:, 0] - E0) * np.cos(psi0) - (final[:, 1] - N0) * np.sin(psi0)
    summary, steps, first_exit = mpc.tracking_summary()
    st = mpc.route_state()
    print(f"{'event':>6s} {'Q_e':>5s} {'n':>6s} {'on tube 1':>9s} {'max|e|':>8s} {'rms e':>8s} {'min Ux':>7s} {'exits':>6s} {'e at join':>9s} {'left (m)':>9s}")
    for j in range(len(sets)):
        for q, Q in enumerate(tunings):
            sel = (which == j) & (tune == q)
            if not sel.any():
                continue
            fin = sel & np.isfinite(summary[:, 1])
            rms = np.sqrt(np.sum(summary[fin, 1]) / max(1, int(np.sum(steps[fin]))))
            ej = np.nanmax(np.abs(st["e_at"][sel])) if j else float("nan")
            print(f"{'none' if j == 0 else ev_steps[j - 1]:>6} {Q:5.2f} {int(sel.sum()):6d} {int(np.sum(st['traj'][sel] == 1)):9d} {np.nanmax(summary[sel, 0]):8.3f} {rms:8.4f} "
                  f"{np.nanmin(summary[sel, 4]):7.3f} {int(np.sum(first_exit[sel] >= 0)):6d} {ej:9.3f} {np.mean(left[sel]):9.3f}")
    print(f"k_route launches: {int(mpc.get_option('stat_route_steps'))} of {a.steps} steps")
    mpc.close()


if __name__ == "__main__":
    main()
