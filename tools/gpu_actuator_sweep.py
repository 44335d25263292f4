#!/usr/bin/env python3
"""Actuator sweep in ONE batch: D transport delays x L steering lags x both `feedback` values x M starts on `skidpadoval` through one closed-loop rollout.  The plant of
instance b integrates a_k = actuator(c_{k - delay}, a_{k-1}) under actuator set a[b] (pg_set_actuator_sets + pg_set_actuator_index); with feedback = 0 the controller
linearises and rate-limits about the command it last sent (the deployed node, ros_integration.jl:52), with feedback = 1 about the actuator's position (the commented-out
line :51).  The figures come back through the device's tracking summary (option "tracking_summary").
--time: ms per rollout step of pg_simulate_dev and pg_simulate_safety_dev at --batch (default 4096), fp64, without a library, with the identity set and with a six-set
library (tracking summary off), alternated in one process.
usage: tools/gpu_actuator_sweep.py [--delays 9] [--starts 32] [--steps 200] [--half-width 0.5] [--time] [--batch 4096]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

TAUS = (0.0, 0.05, 0.1, 0.2)                                     # tau_delta, s


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
    six = [pkg.actuator(), pkg.actuator(delay_steps=3), pkg.actuator(delay_steps=16), pkg.actuator(tau_delta=0.05, tau_fx=0.05),
           pkg.actuator(rate_delta=0.2, rate_fx=5e3, delay_steps=1), pkg.actuator(delay_steps=2, tau_delta=0.1, feedback=1)]
    idx = (np.arange(B) % 6).astype(np.int32)
    cases = {"none": lambda: mpc.clear_actuators(), "identity": lambda: mpc.set_actuators(pkg.actuator()), "six sets": lambda: mpc.set_actuators(six, idx)}
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
    print(f"actuator steps so far {int(mpc.get_option('stat_actuator_steps'))}")
    mpc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--delays", type=int, default=9); ap.add_argument("--starts", type=int, default=32); ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--half-width", type=float, default=0.5); ap.add_argument("--time", action="store_true"); ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    d = traj.data.copy(); d[10] = a.half_width; d[11] = -a.half_width      # the tube the exits are counted against
    traj = pkg.TrajectoryTube(*d)
    D, L, M = a.delays, len(TAUS), a.starts
    sets = [pkg.actuator(delay_steps=dl, tau_delta=tau, feedback=fb) for dl in range(D) for tau in TAUS for fb in (0, 1)]
    B = len(sets) * M
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    state, control, t0, toff = (np.tile(x, (len(sets),) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1))      # the same M starts under every set
    ai = np.repeat(np.arange(len(sets)), M).astype(np.int32)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    mpc.set_actuators(sets, ai)
    mpc.set_option("tracking_summary", 1)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    t = time.perf_counter()
    mpc.simulate_(a.steps); mpc.synchronize()
    wall = time.perf_counter() - t
    sm, n, fx = mpc.tracking_summary()
    print(f"one batch: {D} delays x {L} steering lags x 2 feedback choices x {M} starts = {B} instances, {a.steps} steps: {wall * 1e3:.1f} ms (first launches included)")
    for k, s in enumerate(sets):
        sel = ai == k
        print(f"  delay {s['delay_steps']} steps, tau_delta {s['tau_delta']:.2f} s, controller sees the {'position' if s['feedback'] else 'command '}: "
              f"max |e| = {sm[sel, 0].max():.3f} m, RMS e = {np.sqrt(sm[sel, 1].sum() / n[sel].sum()):.3f} m, max |r| = {sm[sel, 3].max():.3f} rad/s, "
              f"left the +-{a.half_width} m tube: {int(np.sum(fx[sel] >= 0))} of {M}")
    mpc.close()
    if a.time:
        timing(pkg, traj, a.batch, a.steps)


if __name__ == "__main__":
    main()
