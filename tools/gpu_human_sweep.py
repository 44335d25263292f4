#!/usr/bin/env python3
"""Human sweep in ONE batch: H driver models x M starts on `skidpadoval` against a synthetic HJI grid through one safety rollout.  The other car of instance b is driven by
set h[b] of a human library (pg_set_human_sets + pg_set_human_index): hold, the worst case, the worst case from a later step on, a driver who re-decides every 0.3 s, the
worst case at 60 % authority, and a seeded random driver; the figures come back through the safety summary (V_min, first breach, policy steps).
--time: ms per rollout step of pg_simulate_safety_dev and pg_simulate_node_dev at --batch (default 4096), fp64, worst-case human: without a library, with the identity
set of mode 1, with four sets (hold; the worst case held, scaled and limited; the worst case from step 40 on; a random driver) and with the random driver on every lane, alternated in one process (timing(..., other=handle) takes a handle of another build of
the package -- the parent commit's, say -- into the same alternation, without a library).
usage: tools/gpu_human_sweep.py [--starts 128] [--steps 100] [--seed 1] [--time] [--batch 4096]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def timed(run, mpc, inputs, steps):
    mpc.set_inputs(*inputs)
    run(3); mpc.synchronize()                               # (first launches; the instances are warm from here on)
    t = time.perf_counter()
    run(steps); mpc.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def timing(pkg, traj, grid, B, steps, other=None):
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=7)
    inputs = (state, control, t0, pkg.synthetic.other_cars(state), toff)
    H = pkg.human
    four = [H(), H(mode=1, hold_steps=3, step_on=2, step_off=11, gain=0.5, omega_max=0.15, a_min=-2.0, a_max=1.5), H(mode=1, step_on=40),
            H(mode=3, hold_steps=2, sigma=[0.2, 1.5], tau=0.05, omega_max=0.3, a_min=-2.0, a_max=2.0)]
    idx = (np.arange(B) % 4).astype(np.int32)
    handles = {"this": pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)}
    against = other is not None
    if against:
        handles["other"] = other
    for m in handles.values():
        m.set_hji_cache(*grid)
    mpc = handles["this"]
    kinds = {"pg_simulate_safety_dev": lambda m: (lambda n: m.simulate_safety_(n, human="worst")),
             "pg_simulate_node_dev": lambda m: (lambda n: m.simulate_node_(n, use_HJI_policy=True, human="worst"))}
    for name, bind in kinds.items():
        run = bind(mpc)
        ms = {"none": [], "identity": [], "four": [], "random": []}
        if against:
            ms["other build, none"] = []
        for _ in range(5):                                   # alternated: all see the same clocks and the same neighbours
            if against:
                ms["other build, none"].append(timed(bind(handles["other"]), handles["other"], inputs, steps))
            mpc.clear_humans()
            ms["none"].append(timed(run, mpc, inputs, steps))
            mpc.set_humans(H(mode=1))
            ms["identity"].append(timed(run, mpc, inputs, steps))
            mpc.set_humans(four, idx, seed=1)
            ms["four"].append(timed(run, mpc, inputs, steps))
            mpc.set_humans(four[3], seed=1)                  # (every lane draws: Philox, Box-Muller and the AR step)
            ms["random"].append(timed(run, mpc, inputs, steps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(f"{name} at B = {B}, ms per step (warm, {steps} steps, median of 5): " + ", ".join(f"{k} {v:.4f} ({(v - med['none']) * 1e3:+.1f} us)" for k, v in med.items())
              + f"; spread of `none` {(max(ms['none']) - min(ms['none'])) * 1e3:.1f} us"
              + (f", of the other build {(max(ms['other build, none']) - min(ms['other build, none'])) * 1e3:.1f} us" if against else "")
              + f" (all: {' | '.join(', '.join(f'{x:.4f}' for x in v) for v in ms.values())})")
    print(f"human steps so far {int(mpc.get_option('stat_human_steps'))}")
    for m in handles.values():
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=128); ap.add_argument("--steps", type=int, default=100); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--time", action="store_true"); ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    grid = pkg.synthetic.hji_grid()
    H = pkg.human
    after = min(40, a.steps // 2)
    drivers = [("hold", H()), ("worst case", H(mode=1)), (f"worst case from step {after} on", H(mode=1, step_on=after)), ("worst case, re-decided every 0.3 s", H(mode=1, hold_steps=30)),
               ("worst case at 60 % authority", H(mode=1, gain=0.6)), ("random, sigma (0.2 rad/s, 1.5 m/s^2), tau 0.5 s", H(mode=3, sigma=[0.2, 1.5], tau=0.5, a_min=-6.0, a_max=3.0))]
    M = a.starts; B = len(drivers) * M
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    other1 = pkg.synthetic.other_cars(s1)
    state, control, t0, toff, other = (np.tile(x, (len(drivers),) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1, other1))      # the same M starts under every driver
    hi = np.repeat(np.arange(len(drivers)), M).astype(np.int32)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False, hji_eps=1.0)
    mpc.set_hji_cache(*grid)
    mpc.set_inputs(state, control, t0, other, toff)
    mpc.set_humans([d for _, d in drivers], hi, seed=a.seed, streams=np.tile(np.arange(M, dtype=np.uint64), len(drivers)))
    t = time.perf_counter()
    mpc.simulate_safety_(a.steps, use_HJI_policy=True); mpc.synchronize()
    wall = time.perf_counter() - t
    vmin, fb, ps = mpc.safety_summary()
    print(f"one batch: {len(drivers)} drivers x {M} starts = {B} instances, {a.steps} steps, MPC + HJI policy: {wall * 1e3:.1f} ms (first launches included)")
    for k, (name, _) in enumerate(drivers):
        sel = hi == k
        print(f"  {name}: V > 0 kept on {int(np.sum(fb[sel] < 0))} of {M}, median V_min {np.median(vmin[sel]):.3f}, worst {vmin[sel].min():.3f}, policy steps per instance {ps[sel].mean():.1f}")
    mpc.close()
    if a.time:
        timing(pkg, traj, grid, a.batch, a.steps)


if __name__ == "__main__":
    main()
