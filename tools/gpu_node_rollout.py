#!/usr/bin/env python3
"""Cost of the node loop: ms per step of pg_simulate_node_dev against pg_simulate_safety_dev on the same config 2 inputs (B = 4096, fp64, no grid, other car held),
the two alternated in one process (two handles, warm-up first, then BLOCKS blocks of STEPS steps each, timed with a stream synchronisation on both sides of every block;
the median of the blocks).  Two cases, one JSON line each:

  open:    every gate open (the node loop is then the safety loop plus k_node_gate and k_node_finish)
  paused:  pre_flag = 0 on a fixed 10 % of the instances at every step (the gate copies their warm state out and the finish kernel copies it back)

usage (GPU box): python tools/gpu_node_rollout.py [--blocks R] [--steps S] [--warmup W]"""
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


def run(pkg, case, blocks, steps, warmup):
    import torch
    traj = pkg.load_path_fixture("skidpadoval")
    B = 4096
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=12345)
    hs = {}
    for k in ("safety", "node"):
        m = pkg.BatchedTrajectoryTrackingMPC(traj, B, phase_timing=False)
        m.set_inputs(state, control, t0, time_offset=toff)
        hs[k] = m
    pf = None
    if case == "paused":
        flag = np.ones(B, np.uint8); flag[np.random.default_rng(1).permutation(B)[: B // 10]] = 0
        n = max(steps, warmup)
        pf = torch.as_tensor(np.tile(flag, (n, 1))).to("cuda:0").contiguous()
    pfp = C.c_void_p(pf.data_ptr()) if pf is not None else None
    go = {"safety": lambda n: hs["safety"].lib.pg_simulate_safety_dev(hs["safety"].h, n, C.c_double(DT), 0, 0, None, None, None, None, None, None, None),
          "node": lambda n: hs["node"].lib.pg_simulate_node_dev(hs["node"].h, n, C.c_double(DT), 0, 0, None, pfp, None, None, None, None)}
    for k in ("safety", "node"):
        assert go[k](warmup) == 0, hs[k].lib.pg_last_error(hs[k].h)
        hs[k].synchronize()
    ms = {"safety": [], "node": []}
    for r in range(blocks):
        for k in (("safety", "node") if r % 2 == 0 else ("node", "safety")):
            hs[k].synchronize()
            t = time.perf_counter()
            assert go[k](steps) == 0, hs[k].lib.pg_last_error(hs[k].h)
            hs[k].synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t) / steps)
    _, hb, cn = hs["node"].node_summary()
    st_s = hs["safety"].solve_info()[0]; st_n = hs["node"].solve_info()[0]
    res = {"case": case, "B": B, "precision": "f64", "blocks": blocks, "steps_per_block": steps, "warmup": warmup,
           "safety_ms_per_step_median": float(np.median(ms["safety"])), "node_ms_per_step_median": float(np.median(ms["node"])),
           "overhead_pct_median": float(100.0 * (np.median(ms["node"]) / np.median(ms["safety"]) - 1.0)),
           "overhead_pct_paired": float(100.0 * np.median(np.array(ms["node"]) / np.array(ms["safety"]) - 1.0)),
           "solved_safety": int(pkg.is_solved(st_s).sum()), "solved_node": int(pkg.is_solved(st_n).sum()),
           "pre_flag_off_steps": int(cn[:, 0].sum()), "low_speed_steps": int(cn[:, 2].sum()), "fallbacks": int(cn[:, 3].sum())}
    for m in hs.values():
        m.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    pkg = _load_pkg()
    for case in ("open", "paused"):
        print(json.dumps(run(pkg, case, a.blocks, a.steps, a.warmup)), flush=True)
