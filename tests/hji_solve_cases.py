"""The grids, targets and twin runs that tests/test_hji_solve_host.py and tests/test_gpu_hji_solve.py share.

Grids: the smallest shapes at which the indexing of pg_hji_solve can go wrong -- every extent different from its neighbours', dimensions of 2 (both faces one-sided),
no extent a multiple of a wavefront or a block (5,040 and 8,100 nodes: 19.7 and 31.6 blocks of 256), knots jittered as synthetic.hji_grid jitters them over the same
box, whose speed dimension starts at the knot V = 0 (optimal_disturbance is (0, 0) there).  Periodic grids end dimension 3 at float32(+-pi).
Target: hji_io.collision_target(2.5 m x 1.0 m) + 0.05 Ux - 0.02 V: with these coefficients no node of any sweep comes within 1e-6 (relative) of the threshold
lam_norm = 1e-3 of optimal_disturbance (tests/test_hji_solve_host.py counts them), so a comparison with the device never rides on that branch."""
import functools

import numpy as np

import hji_solve_numpy as hs
from conftest import load_pkg

GRIDS = {"A": (7, 5, 4, 3, 2, 3, 2), "B": (5, 6, 5, 3, 3, 2, 3)}
CASES = [("A", False), ("B", True)]          # (grid, periodic psi)
FIXED_DT = 0.02                              # s: below the CFL step of both grids (about 0.05 s), so the fixed-step runs are stable
SWEEPS = 6
HALF_LENGTH, HALF_WIDTH = 2.5, 1.0
LO = np.array([-20.0, -8.0, -np.pi, 0.5, -2.0, 0.0, -1.0]); HI = np.array([20.0, 8.0, np.pi, 14.0, 2.0, 12.0, 1.0])


@functools.lru_cache(maxsize=None)
def grid(name, periodic, seed=5):
    """(knots: tuple of 7 float32 arrays, l0 [prod dims] float32 column-major)"""
    dims = GRIDS[name]
    rng = np.random.default_rng(seed)
    knots = []
    for d in range(7):
        u = np.linspace(0, 1, dims[d])
        u[1:-1] += rng.uniform(-0.25, 0.25, dims[d] - 2) / (dims[d] - 1)
        knots.append((LO[d] + (HI[d] - LO[d]) * u).astype(np.float32))
    return tuple(knots), target(tuple(knots))


def target(knots, cos_psi=0.0):
    pkg = load_pkg()
    dims = [len(k) for k in knots]
    G = np.meshgrid(*[np.asarray(k, dtype=np.float64) for k in knots], indexing="ij")
    extra = (0.05 * G[3] - 0.02 * G[5] + cos_psi * np.cos(G[2])).reshape(-1, order="F")
    return (pkg.hji_io.collision_target(knots, HALF_LENGTH, HALF_WIDTH).astype(np.float64) + extra).astype(np.float32)


def vehicle(key):
    pkg = load_pkg()
    return {"nominal": pkg.vehicles.X1, "mu06": lambda: pkg.vehicles.X1(mu=0.6)}[key]()


@functools.lru_cache(maxsize=None)
def twin(name, periodic, sweeps=SWEEPS, veh="nominal"):
    """the twin's (V, gradV, stats) after `sweeps` fixed steps; computed once, shared, never written to.  stats["near_threshold"]: nodes within 1e-6 (relative) of the
    lam_norm threshold, over all sweeps"""
    knots, l0 = grid(name, periodic)
    near = [0]

    def count(k, x, pbar, V):
        ln = hs.lam_norm(x, pbar)
        near[0] += int(np.sum(np.abs(ln - 1e-3) <= 1e-6 * 1e-3))
    V, g, st = hs.solve(vehicle(veh), knots, l0, 1e9, fixed_dt=FIXED_DT, max_sweeps=sweeps, periodic_psi=periodic, on_sweep=count)
    st["near_threshold"] = near[0]
    for a in (V, g):
        a.setflags(write=False)
    return V, g, st
