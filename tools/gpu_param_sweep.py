#!/usr/bin/env python3
"""Tuning sweep in ONE batch: K control-parameter sets x M starts through one closed-loop rollout (pg_set_control_param_sets + pg_set_control_param_index), with the
per-set tracking figures; --separate also runs the K sets through K handles of M instances and prints both wall times.
usage: tools/gpu_param_sweep.py [--sets 8] [--starts 512] [--steps 100] [--node] [--separate]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def sweep_sets(pkg, K, seed=0):
    """set 0 = the defaults; the others scale the tracking weights, the speed-feedback gains and the steering-rate limit"""
    rng = np.random.default_rng(seed)
    d = dict(pkg.CoupledControlParams())
    sets = [dict(d)]
    for _ in range(K - 1):
        s = dict(d)
        for f in ("Q_e", "Q_dpsi", "Q_ds", "R_ddelta", "R_dFx", "W_r", "k_V", "k_s"):
            s[f] = d[f] * float(2.0 ** rng.uniform(-2, 2))
        s["deltadot_max"] = d["deltadot_max"] * float(rng.uniform(0.6, 1.0))
        sets.append(s)
    return sets


def rollout(mpc, state, control, t0, toff, steps, node):
    mpc.set_inputs(state, control, t0, time_offset=toff)
    t = time.perf_counter()
    out = mpc.simulate_node_(steps) if node else mpc.simulate_(steps)
    mpc.synchronize()
    return out[0], time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8); ap.add_argument("--starts", type=int, default=512); ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--node", action="store_true"); ap.add_argument("--separate", action="store_true")
    a = ap.parse_args()
    pkg = entry._load_pkg()
    traj = pkg.load_path_fixture("skidpadoval")
    K, M = a.sets, a.starts
    s1, c1, t1, o1 = pkg.synthetic.config2_inputs(traj, M, seed=7)
    state, control, t0, toff = (np.tile(x, (K,) + (1,) * (x.ndim - 1)) for x in (s1, c1, t1, o1))      # the same M starts under every set
    idx = np.repeat(np.arange(K, dtype=np.int32), M)
    sets = sweep_sets(pkg, K)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, K * M, phase_timing=False)
    mpc.set_control_params(sets, idx)
    rollout(mpc, state, control, t0, toff, 2, a.node); mpc.reset()                                    # (first launches: code objects, allocations)
    final, wall = rollout(mpc, state, control, t0, toff, a.steps, a.node)
    qs, _, _ = mpc.nodes()                                  # node 0 of the last step = the measured state in path coordinates: q = (ds, Ux, Uy, r, dpsi, e)
    print(f"one batch: {K} sets x {M} starts, {a.steps} steps: {wall * 1e3:.1f} ms")
    for k in range(K):
        sel = idx == k
        print(f"  set {k}: max |e| = {np.max(np.abs(qs[sel, 0, 5])):.3f} m, final ds: mean {np.mean(qs[sel, 0, 0]):+.3f} m, worst {np.max(np.abs(qs[sel, 0, 0])):.3f} m, mean Ux = {np.mean(final[sel, 3]):.2f} m/s")
    mpc.close()
    if a.separate:
        total = 0.0
        for k in range(K):
            one = pkg.BatchedTrajectoryTrackingMPC(traj, M, control_params=sets[k], phase_timing=False)
            rollout(one, s1, c1, t1, o1, 2, a.node); one.reset()
            _, w = rollout(one, s1, c1, t1, o1, a.steps, a.node); total += w
            one.close()
        print(f"{K} handles of {M}: {total * 1e3:.1f} ms in all ({total / wall:.2f} x the one batch)")


if __name__ == "__main__":
    main()
