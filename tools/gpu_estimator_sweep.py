#!/usr/bin/env python3
"""Estimator sweep in ONE batch: G gains x S sensors x P plants x M starts on `skidpadoval` through one closed-loop rollout.  The controller of instance b reads the estimate
of a fixed-gain observer, prior + gain (measured - prior) with the controller's own model as the prior (pg_set_estimator_sets + pg_set_estimator_index), on top of sensor
set s[b] (pg_set_sensor_sets), and its plant is vehicle p[b] (pg_set_plant_sets); the figures come back through the device's tracking summary (option
"tracking_summary"), which describes the TRUE state.  Gain 1 is the identity: the raw measurement, as without a library.
--time: ms per rollout step of pg_simulate_dev and pg_simulate_safety_dev at --batch (default 4096), fp64, without a library, with the identity set and with the four
sets of tests/estimator_numpy.py, and with gain 0.2 and the model on every lane and an exact sensor (the estimate equals the truth: the RK4's cost alone; tracking summary off), alternated in one process.
usage: tools/gpu_estimator_sweep.py [--gains 1,0.5,0.2,0.05] [--sensors 3] [--plants 2] [--starts 128] [--steps 100] [--half-width 0.5] [--seed 1] [--no-model] [--time] [--batch 4096]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SIGMA = np.array([0.05, 0.05, 0.005, 0.1, 0.05, 0.01])          # (E, N, psi, Ux, Uy, r): a GPS / INS estimate of moderate quality


def timed(run, mpc, inputs, steps):
    mpc.set_inputs(*inputs)
    run(3); mpc.synchronize()                               # (first launches; the instances are warm from here on)
    t = time.perf_counter()
    run(steps); mpc.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def timing(pkg, traj, B, steps):
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=7)
    inputs = (state, control, t0, pkg.synthetic.other_cars(state), toff)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    E = pkg.estimator
    four = [E(), E(gain=0.2), E(gain=0.5, predict=0), E(gain=[1, 1, 0.2, 0.2, 0, 0.2])]
    idx = (np.arange(B) % 4).astype(np.int32)
    runs = {"pg_simulate_dev": lambda n: mpc.simulate_(n), "pg_simulate_safety_dev": lambda n: mpc.simulate_safety_(n, use_HJI_policy=False)}
    for name, run in runs.items():
        ms = {"none": [], "identity": [], "observer": [], "four": []}
        for _ in range(5):                                   # alternated: all see the same clocks and the same neighbours
            mpc.clear_estimators()
            ms["none"].append(timed(run, mpc, inputs, steps))
            mpc.set_estimators(E())
            ms["identity"].append(timed(run, mpc, inputs, steps))
            mpc.set_estimators(E(gain=0.2))                  # (no sensor library: an exact model on an exact measurement predicts what it is shown, so the closed loop is
            ms["observer"].append(timed(run, mpc, inputs, steps))      #  the one without a library and the difference is k_estimate's RK4 alone)
            mpc.set_estimators(four, idx)
            ms["four"].append(timed(run, mpc, inputs, steps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(f"{name} at B = {B}, ms per step (warm, {steps} steps, median of 5): no library {med['none']:.4f}, identity set {med['identity']:.4f} "
              f"({(med['identity'] - med['none']) * 1e3:+.1f} us), gain 0.2 with the model on every lane {med['observer']:.4f} ({(med['observer'] - med['none']) * 1e3:+.1f} us), four sets {med['four']:.4f} ({(med['four'] - med['none']) * 1e3:+.1f} us) "
              f"(all: {' | '.join(', '.join(f'{x:.4f}' for x in v) for v in ms.values())})")
    print(f"estimator steps so far {int(mpc.get_option('stat_estimator_steps'))}")
    mpc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gains", default="1,0.5,0.2,0.05"); ap.add_argument("--sensors", type=int, default=3); ap.add_argument("--plants", type=int, default=2)
    ap.add_argument("--starts", type=int, default=128); ap.add_argument("--steps", type=int, default=100); ap.add_argument("--half-width", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=1); ap.add_argument("--no-model", action="store_true"); ap.add_argument("--time", action="store_true")
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    d = traj.data.copy(); d[10] = a.half_width; d[11] = -a.half_width      # the tube the exits are counted against
    traj = pkg.TrajectoryTube(*d)
    gains = [float(g) for g in a.gains.split(",")]
    G, S, P, M = len(gains), a.sensors, a.plants, a.starts
    B = G * S * P * M
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    state, control, t0, toff = (np.tile(x, (G * S * P,) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1))      # the same M starts in every cell of the grid
    cell = np.repeat(np.arange(G * S * P), M)
    gi, si, pi = (cell // (S * P)).astype(np.int32), ((cell // P) % S).astype(np.int32), (cell % P).astype(np.int32)
    factors = [0.0 if S == 1 else 3.0 * k / (S - 1) for k in range(S)]      # sensor 0 is exact, the last has three times SIGMA
    plants = [pkg.X1(mu=0.92 - 0.4 * k / max(P - 1, 1)) for k in range(P)]
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    mpc.set_plants(plants, pi)
    mpc.set_option("tracking_summary", 1)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    mpc.set_sensors([{"sigma": f * SIGMA} for f in factors], si, seed=a.seed)          # (default streams: instance b draws from stream b)
    mpc.set_estimators([pkg.estimator(gain=g, predict=0 if a.no_model else 1) for g in gains], gi)
    t = time.perf_counter()
    out = mpc.simulate_(a.steps, record=True, measured=True, estimated=True); mpc.synchronize()
    wall = time.perf_counter() - t
    x, y, xh = out[3], out[-2], out[-1]
    sm, n, fx = mpc.tracking_summary()
    print(f"one batch: {G} gains x {S} sensors x {P} plants x {M} starts = {B} instances, {a.steps} steps: {wall * 1e3:.1f} ms (first launches and the records included)")
    rms = lambda v: float(np.sqrt(np.mean(v ** 2)))
    for g in range(G):
        for s in range(S):
            for p in range(P):
                sel = (gi == g) & (si == s) & (pi == p)
                print(f"  gain {gains[g]:g}, sigma x {factors[s]:.1f}, plant mu {plants[p]['mu']:.2f}: max |e| = {sm[sel, 0].max():.3f} m, "
                      f"RMS e = {np.sqrt(sm[sel, 1].sum() / n[sel].sum()):.3f} m, left the +-{a.half_width} m tube: {int(np.sum(fx[sel] >= 0))} of {M}; "
                      f"position error of the measurement {rms(y[:, sel, :2] - x[:, sel, :2]):.3f} m, of the estimate {rms(xh[:, sel, :2] - x[:, sel, :2]):.3f} m")
    mpc.close()
    if a.time:
        timing(pkg, traj, a.batch, a.steps)


if __name__ == "__main__":
    main()
