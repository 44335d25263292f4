#!/usr/bin/env python3
"""Sensor-noise sweep in ONE batch: S sensors x P plants x T tunings x M starts on `skidpadoval` through one closed-loop rollout.  The controller of instance b reads
measured = true + bias + sigma z under sensor set s[b] (pg_set_sensor_sets + pg_set_sensor_index + pg_set_sensor_seed), its plant is vehicle p[b] (pg_set_plant_sets), its
tuning control-parameter set t[b] (pg_set_control_param_sets); the figures come back through the device's tracking summary (option "tracking_summary"), which describes
the TRUE state.  Every instance draws from its own stream; --seed picks the realisation.
--time: ms per rollout step of pg_simulate_dev, pg_simulate_safety_dev and pg_simulate_node_dev at --batch (default 4096), fp64, with and without a sensor library
(tracking summary off), alternated in one process.
usage: tools/gpu_sensor_sweep.py [--sensors 4] [--plants 2] [--tunings 2] [--starts 128] [--steps 100] [--half-width 0.5] [--seed 1] [--time] [--batch 4096]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SIGMA = np.array([0.05, 0.05, 0.005, 0.1, 0.05, 0.01])          # (E, N, psi, Ux, Uy, r): a GPS / INS estimate of moderate quality


def sensors(S):
    """sensor 0 is exact; the others scale SIGMA from 1 to 4 and, every other one, add a 0.1 m bias across the path's East axis"""
    out = [({"sigma": np.zeros(6)}, "exact")]
    for k in range(1, S):
        f = 1.0 + 3.0 * (k - 1) / max(S - 2, 1)
        bias = [0.1, 0, 0, 0, 0, 0] if k % 2 == 0 else [0.0] * 6
        out.append(({"sigma": f * SIGMA, "bias": bias}, f"sigma x {f:.1f}" + (", bias 0.1 m on E" if k % 2 == 0 else "")))
    return out


def timed(run, mpc, inputs, steps):
    mpc.set_inputs(*inputs)
    run(3); mpc.synchronize()                               # (first launches; the instances are warm from here on)
    t = time.perf_counter()
    run(steps); mpc.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def timing(pkg, traj, B, steps, seed):
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=7)
    inputs = (state, control, t0, pkg.synthetic.other_cars(state), toff)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    lib = [s for s, _ in sensors(4)]
    idx = (np.arange(B) % 4).astype(np.int32)
    runs = {"pg_simulate_dev": lambda n: mpc.simulate_(n), "pg_simulate_safety_dev": lambda n: mpc.simulate_safety_(n, use_HJI_policy=False),
            "pg_simulate_node_dev": lambda n: mpc.simulate_node_(n)}
    for name, run in runs.items():
        ms = {"none": [], "library": []}
        for _ in range(3):                                   # alternated: both see the same clocks and the same neighbours
            mpc.clear_sensors()
            ms["none"].append(timed(run, mpc, inputs, steps))
            mpc.set_sensors(lib, idx, seed=seed)
            ms["library"].append(timed(run, mpc, inputs, steps))
        print(f"{name} at B = {B}, ms per step (warm, {steps} steps, median of 3): no library {np.median(ms['none']):.4f}, four-set sensor library {np.median(ms['library']):.4f} "
              f"(all: {', '.join(f'{x:.4f}' for x in ms['none'])} | {', '.join(f'{x:.4f}' for x in ms['library'])})")
    mpc.set_option("tracking_summary", 1)
    tr = timed(runs["pg_simulate_dev"], mpc, inputs, steps)
    print(f"pg_simulate_dev with the library and the tracking summary on (k_measure + projection of the true state + k_track): {tr:.4f} ms per step; "
          f"sensor steps so far {int(mpc.get_option('stat_sensor_steps'))}")
    mpc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sensors", type=int, default=4); ap.add_argument("--plants", type=int, default=2); ap.add_argument("--tunings", type=int, default=2)
    ap.add_argument("--starts", type=int, default=128); ap.add_argument("--steps", type=int, default=100); ap.add_argument("--half-width", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=1); ap.add_argument("--time", action="store_true"); ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    d = traj.data.copy(); d[10] = a.half_width; d[11] = -a.half_width      # the tube the exits are counted against
    traj = pkg.TrajectoryTube(*d)
    S, P, T, M = a.sensors, a.plants, a.tunings, a.starts
    B = S * P * T * M
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    state, control, t0, toff = (np.tile(x, (S * P * T,) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1))      # the same M starts in every cell of the grid
    cell = np.repeat(np.arange(S * P * T), M)
    si, pi, ti = (cell // (P * T)).astype(np.int32), ((cell // T) % P).astype(np.int32), (cell % T).astype(np.int32)
    sens = sensors(S)
    plants = [pkg.X1(mu=0.92 - 0.4 * k / max(P - 1, 1)) for k in range(P)]
    tunings = [dict(pkg.CoupledControlParams(), Q_e=1.0 * 4.0 ** k) for k in range(T)]
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
    mpc.set_control_params(tunings, ti)
    mpc.set_plants(plants, pi)
    mpc.set_option("tracking_summary", 1)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    mpc.set_sensors([s for s, _ in sens], si, seed=a.seed)                  # (default streams: instance b draws from stream b)
    t = time.perf_counter()
    mpc.simulate_(a.steps); mpc.synchronize()
    wall = time.perf_counter() - t
    sm, n, fx = mpc.tracking_summary()
    print(f"one batch: {S} sensors x {P} plants x {T} tunings x {M} starts = {B} instances, {a.steps} steps: {wall * 1e3:.1f} ms (first launches included)")
    for s, (_, label) in enumerate(sens):
        for p in range(P):
            for q in range(T):
                sel = (si == s) & (pi == p) & (ti == q)
                print(f"  sensor {s} ({label}), plant mu {plants[p]['mu']:.2f}, Q_e {tunings[q]['Q_e']:g}: max |e| = {sm[sel, 0].max():.3f} m, "
                      f"RMS e = {np.sqrt(sm[sel, 1].sum() / n[sel].sum()):.3f} m, left the +-{a.half_width} m tube: {int(np.sum(fx[sel] >= 0))} of {M}")
    mpc.close()
    if a.time:
        timing(pkg, traj, a.batch, a.steps, a.seed)


if __name__ == "__main__":
    main()
