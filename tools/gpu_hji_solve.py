#!/usr/bin/env python3
"""Computes an HJI avoid-set grid on the GPU (pg_hji_solve) for a chosen grid and vehicle and writes it as an hji_io file.

The grid has synthetic.hji_grid's box and jitter (default shape 13 x 13 x 9^5, about 10 M nodes; dimension 3 spans [-pi, pi] and wraps with --periodic), the target is
hji_io.collision_target(--half-length, --half-width), the vehicle is vehicles.X1(**overrides) from --mu, --Caf, --Car, --Fx-max, --mass-scale (all four corner masses
and Izz).  Prints the sweeps taken, ms per sweep (host clock around the synchronous call, one warm-up solve of two sweeps first), nodes per second and the fraction of
the memory floor: 8 B per node and pass (V read once, written once), two passes a sweep, over the 8 TB/s peak.  Per-pass kernel times come from running this script
under `rocprofv3 --kernel-trace --stats` (kernels k_hji_sweep_eval, k_hji_sweep_update, k_hji_finish).
usage: tools/gpu_hji_solve.py [--dims 13,13,9,9,9,9,9] [--horizon 3.0] [--cfl 0.8] [--fixed-dt 0] [--max-sweeps 100000] [--periodic] [--precision f64]
                              [--mu 0.92 ...] [--out grid.pghji] [--install]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="13,13,9,9,9,9,9")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--horizon", type=float, default=3.0)
    ap.add_argument("--cfl", type=float, default=0.8)
    ap.add_argument("--fixed-dt", type=float, default=0.0)
    ap.add_argument("--max-sweeps", type=int, default=100000)
    ap.add_argument("--periodic", action="store_true")
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--half-length", type=float, default=2.5)
    ap.add_argument("--half-width", type=float, default=1.0)
    ap.add_argument("--mu", type=float); ap.add_argument("--Caf", type=float); ap.add_argument("--Car", type=float); ap.add_argument("--Fx-max", type=float)
    ap.add_argument("--mass-scale", type=float)
    ap.add_argument("--out")
    ap.add_argument("--install", action="store_true", help="also build the handle's lookup table from the device buffers")
    a = ap.parse_args()
    pkg = entry._load_pkg()
    dims = tuple(int(x) for x in a.dims.split(","))
    rng = np.random.default_rng(a.seed)                                     # synthetic.hji_grid's knots, without its value arrays
    lo = np.array([-20.0, -8.0, -np.pi, 0.5, -2.0, 0.0, -1.0]); hi = np.array([20.0, 8.0, np.pi, 14.0, 2.0, 12.0, 1.0])
    knots = []
    for d in range(7):
        u = np.linspace(0, 1, dims[d])
        u[1:-1] += rng.uniform(-0.25, 0.25, dims[d] - 2) / (dims[d] - 1)
        knots.append((lo[d] + (hi[d] - lo[d]) * u).astype(np.float32))
    over = {k: v for k, v in (("mu", a.mu), ("Caf", a.Caf), ("Car", a.Car), ("Fx_max", a.Fx_max)) if v is not None}
    if a.mass_scale is not None:
        base = pkg.vehicles.X1()
        over.update({k: a.mass_scale * base[k] for k in ("mfl", "mfr", "mrl", "mrr", "Izz")})
    veh = pkg.vehicles.X1(**over)
    l0 = pkg.hji_io.collision_target(knots, a.half_length, a.half_width)
    n = l0.size
    traj = pkg.load_path_fixture("skidpadoval")
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, 64, precision=a.precision)
    opts = dict(cfl=a.cfl, fixed_dt=a.fixed_dt, periodic_psi=a.periodic)
    mpc.solve_hji_cache(knots, l0, a.horizon, vehicle=veh, install=False, max_sweeps=2, **opts)      # warm-up: code objects, allocations
    t = time.perf_counter()
    V, g, st = mpc.solve_hji_cache(knots, l0, a.horizon, vehicle=veh, install=a.install, max_sweeps=a.max_sweeps, **opts)
    wall = time.perf_counter() - t
    t = time.perf_counter()
    mpc.solve_hji_cache(knots, l0, 0.0, vehicle=veh, install=a.install, **opts)                      # the same call without a sweep: upload, finish, download (, install)
    fixed = time.perf_counter() - t
    sw = max(st["sweeps"], 1)
    per = (wall - fixed) / sw
    print(f"grid {'x'.join(map(str, dims))} = {n} nodes, {a.precision}, vehicle overrides {over or 'none'}, periodic {a.periodic}")
    print(f"sweeps {st['sweeps']}  reached_horizon {st['reached_horizon']}  tau {st['tau']:.6f} s  last dt {st['last_dt']:.6f} s  V in [{st['v_min']:.4f}, {st['v_max']:.4f}]")
    print(f"alpha {np.array2string(st['alpha'], precision=4)}")
    print(f"call {wall * 1e3:.1f} ms, of which {fixed * 1e3:.1f} ms without a sweep (upload, gradient, download{', install' if a.install else ''})")
    print(f"per sweep {per * 1e3:.4f} ms = {n / per / 1e9:.3f} G nodes/s; memory floor 2 passes x 8 B x {n} nodes / 8 TB/s = {16 * n / HBM_PEAK * 1e3:.4f} ms: fraction {16 * n / HBM_PEAK / per:.4f}")
    print(f"unsafe nodes (V <= 0): {int(np.sum(V <= 0))} of {n} ({int(np.sum(l0 <= 0))} in the target)")
    if a.out:
        pkg.save_hji_grid(a.out, knots, V, g)
        print(f"wrote {a.out}")
    mpc.close()


if __name__ == "__main__":
    main()
