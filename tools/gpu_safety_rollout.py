#!/usr/bin/env python3
"""Cost of the safety rollout: ms per step of pg_simulate_safety_dev against pg_simulate_dev on the same inputs, the two alternated in one process (two handles, warm-up
first, then ROUNDS rounds of STEPS steps each, timed with a stream synchronisation on both sides of every round).  One JSON line per configuration.

  config 2: B = 4096, fp64, no grid, other car held at speed 0 (the safety step is then the plain loop plus the fused kernel's records-free bookkeeping)
  config 3: B = 4096, fp32, synthetic.hji_grid_large (13 x 13 x 9^5), synthetic.other_cars, worst-case human, HJI policy on

usage (GPU box): python tools/gpu_safety_rollout.py [2|3 ...] [--rounds R] [--steps S] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import _load_pkg  # noqa: E402

DT = 0.01


def handles(pkg, cfg, traj, B):
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=12345)
    precision = "f64" if cfg == 2 else "f32"
    grid = pkg.synthetic.hji_grid_large() if cfg == 3 else None
    other = pkg.synthetic.other_cars(state, seed=777) if cfg == 3 else None
    out = []
    for _ in range(2):
        m = pkg.BatchedTrajectoryTrackingMPC(traj, B, precision=precision, phase_timing=False)
        if grid is not None:
            m.set_hji_cache(*grid)
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        out.append(m)
    return out


def run(pkg, cfg, rounds, steps, warmup):
    traj = pkg.load_path_fixture("skidpadoval")
    B = 4096
    plain, safe = handles(pkg, cfg, traj, B)
    mode = 0 if cfg == 2 else 1
    go = {"plain": lambda n: plain.lib.pg_simulate_dev(plain.h, n, C.c_double(DT), None, None),
          "safety": lambda n: safe.lib.pg_simulate_safety_dev(safe.h, n, C.c_double(DT), 1, mode, None, None, None, None, None, None, None)}
    hs = {"plain": plain, "safety": safe}
    for k in ("plain", "safety"):
        assert go[k](warmup) == 0, hs[k].lib.pg_last_error(hs[k].h)
        hs[k].synchronize()
    ms = {"plain": [], "safety": []}
    for r in range(rounds):
        for k in (("plain", "safety") if r % 2 == 0 else ("safety", "plain")):
            hs[k].synchronize()
            t = time.perf_counter()
            assert go[k](steps) == 0, hs[k].lib.pg_last_error(hs[k].h)
            hs[k].synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t) / steps)
    vmin, fb, ps = safe.safety_summary()
    st_p = plain.solve_info()[0]; st_s = safe.solve_info()[0]
    res = {"config": cfg, "B": B, "precision": plain.precision, "rounds": rounds, "steps_per_round": steps, "warmup": warmup,
           "plain_ms_per_step_median": float(np.median(ms["plain"])), "safety_ms_per_step_median": float(np.median(ms["safety"])),
           "plain_ms_per_step_mean": float(np.mean(ms["plain"])), "safety_ms_per_step_mean": float(np.mean(ms["safety"])),
           "overhead_pct_median": float(100.0 * (np.median(ms["safety"]) / np.median(ms["plain"]) - 1.0)),
           "overhead_pct_paired": float(100.0 * np.median(np.array(ms["safety"]) / np.array(ms["plain"]) - 1.0)),
           "solved_plain": int(pkg.is_solved(st_p).sum()), "solved_safety": int(pkg.is_solved(st_s).sum()),
           "policy_steps_total": int(ps.sum()), "instances_breached": int((fb >= 0).sum()), "V_min_finite": int(np.isfinite(vmin).sum())}
    plain.close(); safe.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", type=int, default=[2, 3])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert a.rounds * a.steps >= 100, "at least 100 timed steps per side"
    pkg = _load_pkg()
    for cfg in a.configs:
        print(json.dumps(run(pkg, cfg, a.rounds, a.steps, a.warmup)), flush=True)
