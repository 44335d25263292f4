#!/usr/bin/env python3
"""Disturbance sweep in ONE batch: G gust levels x W friction windows x 2 tunings x M starts on `skidpadoval` through one closed-loop rollout.  The plant of instance b
integrates the body model plus w_k of disturbance set d[b] (pg_set_disturbance_sets + pg_set_disturbance_index): a side gust of standard deviation sigma_Fy acting
1 m ahead of the CG with a correlation time of 0.3 s, and the plant's mu scaled inside the window [step_on, step_off).  The controller never sees any of it.  The figures
come back through the device's tracking summary (option "tracking_summary"): max |e| and the first step outside the tube, per cell.
--time: ms per rollout step of pg_simulate_dev and pg_simulate_safety_dev at --batch (default 4096), fp64, without a library, with the identity set and with a four-set
library (tracking summary off), alternated in one process.
usage: tools/gpu_disturbance_sweep.py [--starts 32] [--steps 200] [--half-width 0.5] [--seed 1] [--time] [--batch 4096]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SIGMAS = (0.0, 400.0, 800.0, 1600.0)                             # sigma_Fy, N
WINDOWS = ((1.0, 0, -1), (0.7, 50, 150), (0.55, 50, 150), (0.4, 50, 150))      # (mu_scale, step_on, step_off)


def timed(run, mpc, inputs, steps):
    mpc.reset(); mpc.set_inputs(*inputs)                    # (cold: the previous case's warm starts belong to another closed loop)
    run(10); mpc.synchronize()                              # (first launches; the instances are warm from here on)
    t = time.perf_counter()
    run(steps); mpc.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def timing(pkg, traj, B, steps):
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=7)
    inputs = (state, control, t0, pkg.synthetic.other_cars(state), toff)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    four = [pkg.disturbance(), pkg.disturbance(Fy=2000.0, x_cp=1.0, sigma_Fy=800.0, tau_gust=0.3, step_on=3, step_off=9), pkg.disturbance(mu_scale=0.55, step_on=2),
            pkg.disturbance(Fx=-1000.0, sigma_Fx=500.0)]
    idx = (np.arange(B) % 4).astype(np.int32)
    cases = {"none": lambda: mpc.clear_disturbances(), "identity": lambda: mpc.set_disturbances(pkg.disturbance()), "four sets": lambda: mpc.set_disturbances(four, idx, seed=1)}
    runs = {"pg_simulate_dev": lambda n: mpc.simulate_(n), "pg_simulate_safety_dev": lambda n: mpc.simulate_safety_(n, use_HJI_policy=False)}
    for name, run in runs.items():
        ms = {c: [] for c in cases}
        for _ in range(5):                                   # alternated: all see the same clocks and the same neighbours
            for c, install in cases.items():
                install()
                ms[c].append(timed(run, mpc, inputs, steps))
        print(f"{name} at B = {B}, ms per step (warm, {steps} steps, median of 5): " + ", ".join(f"{c} {np.median(v):.4f}" for c, v in ms.items())
              + f"; identity - none = {1e3 * (np.median(ms['identity']) - np.median(ms['none'])):+.1f} us (all: "
              + " | ".join(", ".join(f"{x:.4f}" for x in v) for v in ms.values()) + ")")
    print(f"disturbance steps so far {int(mpc.get_option('stat_disturbance_steps'))}")
    mpc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=32); ap.add_argument("--steps", type=int, default=200); ap.add_argument("--half-width", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=1); ap.add_argument("--time", action="store_true"); ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    d = traj.data.copy(); d[10] = a.half_width; d[11] = -a.half_width      # the tube the exits are counted against
    traj = pkg.TrajectoryTube(*d)
    cp = pkg.CoupledControlParams()
    tunings = [cp, dict(cp, Q_e=2.0 * cp["Q_e"])]
    sets = [pkg.disturbance(sigma_Fy=sg, x_cp=1.0, tau_gust=0.3) for sg in SIGMAS for _ in WINDOWS]
    for k, (mu, on, off) in enumerate(WINDOWS * len(SIGMAS)):
        if mu != 1.0:      # one window per set: the gust is confined to it too, so the rows with mu_scale = 1 carry the gust over the whole run
            sets[k].update(mu_scale=mu, step_on=on, step_off=off)
    M, T = a.starts, len(tunings)
    B = len(sets) * T * M
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    state, control, t0, toff = (np.tile(x, (len(sets) * T,) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1))      # the same M starts in every cell
    di = np.repeat(np.arange(len(sets)), T * M).astype(np.int32)
    ti = np.tile(np.repeat(np.arange(T), M), len(sets)).astype(np.int32)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    mpc.set_control_params(tunings, ti)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    mpc.set_disturbances(sets, di, seed=a.seed, streams=np.tile(np.arange(M), len(sets) * T))      # (the same gust for a start in every cell)
    mpc.set_option("tracking_summary", 1)
    t = time.perf_counter()
    mpc.simulate_(a.steps); mpc.synchronize()
    wall = time.perf_counter() - t
    sm, n, fx = mpc.tracking_summary()
    print(f"one batch: {len(SIGMAS)} gust levels x {len(WINDOWS)} friction windows x {T} tunings x {M} starts = {B} instances, {a.steps} steps: {wall * 1e3:.1f} ms (first launches included)")
    print("  sigma_Fy   mu window            Q_e     max |e|   left the tube   first exit (median step)")
    for k, s in enumerate(sets):
        for j in range(T):
            sel = (di == k) & (ti == j)
            out = fx[sel][fx[sel] >= 0]
            win = "none" if s["mu_scale"] == 1.0 else f"x{s['mu_scale']:.2f} [{s['step_on']}, {s['step_off']})"
            print(f"  {s['sigma_Fy']:7.0f} N  {win:19s}  {tunings[j]['Q_e']:5.2f}  {sm[sel, 0].max():8.3f} m  {out.size:4d} of {M:<4d}    {'-' if out.size == 0 else int(np.median(out))}")
    mpc.close()
    if a.time:
        timing(pkg, traj, a.batch, a.steps)


if __name__ == "__main__":
    main()
