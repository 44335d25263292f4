#!/usr/bin/env python3
"""Model-mismatch sweep in ONE batch: K plants (friction and mass variants of X1) x M starts on `skidpadoval` through one closed-loop rollout -- the controller keeps X1,
the PLANT of instance b is plant set idx[b] (pg_set_plant_sets + pg_set_plant_index) -- with the per-variant tracking figures of the device's tracking summary
(option "tracking_summary", pg_get_tracking_state): max |e|, RMS e, instances that left the tube.
--time: ms per step of pg_simulate_dev for the same batch under no library, the K-set library and ONE SET PER INSTANCE (Monte Carlo), tracking summary off.
usage: tools/gpu_plant_sweep.py [--variants 8] [--starts 512] [--steps 100] [--half-width 0.5] [--time]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def variants(pkg, K):
    """variant 0 = X1 (no mismatch); the others walk friction down from 0.92 to 0.45 and the corner masses up to + 30 % (Izz with them)"""
    base = pkg.X1()
    out = [(base, "X1")]
    for k in range(1, K):
        f = k / max(K - 1, 1)
        mu, ms = 0.92 - 0.47 * f, 1.0 + 0.3 * ((k * 5) % K) / K
        out.append((pkg.X1(mu=mu, mfl=ms * base["mfl"], mfr=ms * base["mfr"], mrl=ms * base["mrl"], mrr=ms * base["mrr"], Izz=ms * base["Izz"]), f"mu {mu:.2f}, mass x {ms:.2f}"))
    return out


def timed(mpc, state, control, t0, toff, steps):
    mpc.set_inputs(state, control, t0, time_offset=toff)
    mpc.simulate_(3); mpc.synchronize()                     # (first launches; the instances are warm from here on)
    t = time.perf_counter()
    mpc.simulate_(steps); mpc.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=8); ap.add_argument("--starts", type=int, default=512); ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--half-width", type=float, default=0.5); ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    d = traj.data.copy(); d[10] = a.half_width; d[11] = -a.half_width      # the tube the exits are counted against
    traj = pkg.TrajectoryTube(*d)
    K, M = a.variants, a.starts
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    state, control, t0, toff = (np.tile(x, (K,) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1))      # the same M starts under every plant
    idx = np.repeat(np.arange(K, dtype=np.int32), M)
    var = variants(pkg, K)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, K * M, phase_timing=False)
    mpc.set_plants([v for v, _ in var], idx)
    mpc.set_option("tracking_summary", 1)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    t = time.perf_counter()
    mpc.simulate_(a.steps); mpc.synchronize()
    wall = time.perf_counter() - t
    sm, n, fx = mpc.tracking_summary()
    print(f"one batch: {K} plants x {M} starts, {a.steps} steps: {wall * 1e3:.1f} ms (first launches included)")
    for k, (_, label) in enumerate(var):
        sel = idx == k
        print(f"  plant {k} ({label}): max |e| = {sm[sel, 0].max():.3f} m, RMS e = {np.sqrt(sm[sel, 1].sum() / n[sel].sum()):.3f} m, max |Uy/Ux| = {sm[sel, 2].max():.3f}, "
              f"left the +-{a.half_width} m tube: {int(np.sum(fx[sel] >= 0))} of {M} (started outside: {int(np.sum(fx[sel] == 0))})")
    if a.time:
        mpc.set_option("tracking_summary", 0)
        B = K * M
        with_lib = timed(mpc, state, control, t0, toff, a.steps)
        rng = np.random.default_rng(1)
        base = pkg.X1()
        mpc.set_plants([pkg.X1(mu=float(rng.uniform(0.45, 0.92)), mfl=base["mfl"] * float(rng.uniform(0.9, 1.3))) for _ in range(B)], np.arange(B, dtype=np.int32))
        per_instance = timed(mpc, state, control, t0, toff, a.steps)
        mpc.clear_plants()
        none = timed(mpc, state, control, t0, toff, a.steps)
        mpc.set_option("tracking_summary", 1)
        tracked = timed(mpc, state, control, t0, toff, a.steps)
        print(f"pg_simulate_dev at B = {B}, ms per step (warm, {a.steps} steps): no library {none:.4f}, {K}-set library {with_lib:.4f}, one set per instance {per_instance:.4f}; "
              f"no library with the tracking summary on {tracked:.4f}")
    mpc.close()


if __name__ == "__main__":
    main()
