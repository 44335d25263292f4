"""A 7-D HJI grid whose whole gradient is live, and the cases tests/test_hji_live_host.py and tests/test_gpu_hji_live.py share.

synthetic.hji_grid has gradV[4] = gradV[6] = 0 at every node, gradV[3] and gradV[5] constant, nothing that depends on x[4] or x[6], and (in the shapes the suite uses)
equal extents in dimensions 3, 4 and 6: optimal_control then steers +delta_max and picks Fx_max for every instance, the steering terms of the safety row are multiplied by
zero, and a lookup that mixes up dimensions 4 and 6 (weights, indices, strides, record bits, output channels) returns the same numbers.  live_grid keeps that grid's box,
knot jitter and base value function (so synthetic.hji_queries and other_cars still land inside it) and adds

    0.05 Uy dN + 0.6 r sin(dpsi + 0.4) + 0.01 Ux Uy + 0.003 V_them dE r + 0.05 sin(PHASE . x)

to V; gradV is the analytic gradient.  The first four terms give channels 5 and 7 (dV/dUy, dV/dr) both signs over the instances of the policy test; the last one makes
every channel depend on every coordinate (without it dV/dUx = 0.05 + 0.01 Uy ignores six of the seven).  Extents 7 x 6 x 5 x 4 x 3 x 5 x 2: dimensions 3, 4 and 6 pairwise
different, dimension 6 with two knots (both of its faces are one-sided cells)."""
import functools

import numpy as np

from conftest import load_pkg

DIMS = (7, 6, 5, 4, 3, 5, 2)
SEED = 11
PHASE = np.array([0.1, 0.2, 0.5, 0.15, 0.4, 0.04, 0.9])
AMP = 0.05


def value_and_gradient(x):
    """(base V of synthetic.hji_grid, V, gradV [..., 7]) at x = the seven coordinate arrays (dE, dN, dpsi, Ux, Uy, V_them, r), in float64"""
    dE, dN, dpsi, Ux, Uy, Vt, r = x
    rho = np.sqrt(dE ** 2 / 4 + dN ** 2 + 1.0)
    base = rho - 3.0 + 0.05 * Ux - 0.02 * Vt + 0.1 * np.cos(dpsi)
    ph = sum(PHASE[d] * x[d] for d in range(7))
    V = base + 0.05 * Uy * dN + 0.6 * r * np.sin(dpsi + 0.4) + 0.01 * Ux * Uy + 0.003 * Vt * dE * r + AMP * np.sin(ph)
    g = np.stack([dE / (4 * rho) + 0.003 * Vt * r,
                  dN / rho + 0.05 * Uy,
                  -0.1 * np.sin(dpsi) + 0.6 * r * np.cos(dpsi + 0.4),
                  0.05 + 0.01 * Uy,
                  0.05 * dN + 0.01 * Ux,
                  -0.02 + 0.003 * dE * r,
                  0.6 * np.sin(dpsi + 0.4) + 0.003 * Vt * dE], axis=-1) + (AMP * np.cos(ph))[..., None] * PHASE
    return base, V, g


@functools.lru_cache(maxsize=None)
def live_grid(dims=DIMS, seed=SEED):
    """(knots: tuple of 7 float32 arrays, V [prod dims] float32 column-major, gradV [prod dims, 7] float32): the format of synthetic.hji_grid.  Computed once, shared,
    never written to."""
    dims = tuple(int(n) for n in dims)
    assert len({dims[3], dims[4], dims[6]}) == 3 and dims[6] == 2, dims
    knots, V0, _ = load_pkg().synthetic.hji_grid(dims=dims, seed=seed)      # the knots (box and jitter) and the base value function
    base, V, g = value_and_gradient(np.meshgrid(*[np.asarray(k, dtype=np.float64) for k in knots], indexing="ij"))
    assert np.array_equal(base.astype(np.float32).reshape(-1, order="F"), V0)
    Vf = V.astype(np.float32).reshape(-1, order="F")                         # Julia arrays are column-major (dim 1 fastest)
    gf = np.stack([g[..., k].astype(np.float32).reshape(-1, order="F") for k in range(7)], axis=1)
    ch = [Vf] + [gf[:, k] for k in range(7)]                                 # the eight channels of a node record
    assert np.mean(ch[5] != 0) > 0.5 and np.mean(ch[7] != 0) > 0.5
    assert not any(np.array_equal(ch[i], ch[j]) for i in range(8) for j in range(i))
    knots = tuple(knots)
    for a in knots + (Vf, gf):
        a.setflags(write=False)
    return knots, Vf, gf


def channel_dependence(dims=DIMS, seed=SEED):
    """[8, 7] bool: channel c of the node record varies along grid dimension d somewhere on the grid"""
    knots, V, g = live_grid(dims, seed)
    out = np.zeros((8, 7), dtype=bool)
    for c in range(8):
        a = (V if c == 0 else g[:, c - 1]).reshape(dims, order="F")
        for d in range(7):
            out[c, d] = bool(np.any(np.diff(a, axis=d) != 0))
    return out


def bounds(knots):
    return np.array([k[0] for k in knots], dtype=np.float64), np.array([k[-1] for k in knots], dtype=np.float64)


# ---- lookup queries ----------------------------------------------------------------------------------------------
def lookup_queries(knots):
    """(x [348, 7], families, node indices [16, 7]): 300 points drawn as test_lookup_matches_oracle draws them (some out of bounds), of which the first two are replaced by the two corners of
    the box; 16 points at node coordinates (weights exactly 0 or 1; the first four on the high face of dimension 4, of dimension 6, of both, and the low corner of both); 16
    points that differ from a base point in x[4] only and 16 that differ in x[6] only.  families: name -> slice of x."""
    lo, hi = bounds(knots)
    rng = np.random.default_rng(0)
    x = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (300, 7))
    x[0] = lo; x[1] = hi
    dims = [len(k) for k in knots]
    idx = np.stack([rng.integers(0, n, 16) for n in dims], axis=1)
    idx[0, 4] = dims[4] - 1; idx[1, 6] = dims[6] - 1
    idx[2, 4] = dims[4] - 1; idx[2, 6] = dims[6] - 1
    idx[3, 4] = 0; idx[3, 6] = 0
    nodes = np.array([[float(knots[d][idx[i, d]]) for d in range(7)] for i in range(16)])
    base = lo + (hi - lo) * rng.uniform(0.1, 0.9, 7)
    parts = [x, nodes]
    for d in (4, 6):
        f = np.tile(base, (16, 1))
        f[:, d] = lo[d] + (hi[d] - lo[d]) * np.linspace(0.02, 0.98, 16)      # crosses every cell of the dimension
        parts.append(f)
    x = np.concatenate(parts)
    fam = {"random": slice(0, 300), "nodes": slice(300, 316), "along4": slice(316, 332), "along6": slice(332, 348)}
    return x, fam, idx


# ---- the instances of the safety-row and policy tests --------------------------------------------------------------
def constraint_inputs(pkg, traj):
    """the inputs of test_constraint_rows_and_solve_with_hji: B = 48"""
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, 48, seed=21)
    return state, control, t0, toff, pkg.synthetic.other_cars(state, seed=5)


def policy_inputs(pkg, traj):
    """the inputs of test_hji_fallback_policy: B = 96, every fifth instance in path-tracking mode"""
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, 96, seed=33)
    toff[::5] = np.nan
    return state, control, t0, toff, pkg.synthetic.other_cars(state, seed=9)


def steer_terms(orc, x7, g, control, h=1e-6):
    """(g[3] d(dUx)/d(delta), g[4] d(dUy)/d(delta) + g[6] d(dr)/d(delta)): the two parts of the steering coefficient M0 of the safety row, by central differences of the
    oracle's world dynamics at uR = (delta, Fxf + Fxr) (HJI_computation.jl:77,166)"""
    q = np.array([x7[0], x7[1], x7[2], x7[3], x7[4], x7[6]])
    Fx = control[1] + control[2]
    d = (orc.world_dynamics(q, [control[0] + h, Fx]) - orc.world_dynamics(q, [control[0] - h, Fx])) / (2 * h)
    return g[3] * d[3], g[4] * d[4] + g[6] * d[5]


TIE_BC = 1e-12          # |Bc| below this x (|g[4]|/m + a |g[6]|/Izz): the steer sign rides on rounding
TIE_SCORE = 1e-10       # best two candidates closer than this (relative): the winner rides on rounding
TIE_CAP = 2             # of 96 instances


def is_tie(veh, g, Bc, scores):
    """optimal_control at gradient g is within rounding of another answer: the steer sign (TIE_BC) or the winner of the line search (TIE_SCORE)"""
    top = np.sort(scores)[-2:]
    scale = abs(g[4]) / veh["m"] + veh["a"] * abs(g[6]) / veh["Izz"]
    return bool(abs(Bc) < TIE_BC * scale or (top[1] - top[0]) < TIE_SCORE * max(abs(top[1]), abs(top[0])))


def policy_reference(orc, state, other):
    """The oracle's optimal_control for every instance, with what decides it.  Returns a dict of arrays over instances: V, inb (inside the grid), g [B, 7], u2 [B, 2], Bc,
    scores [B, 50], win (index of the winning candidate: the first maximiser), tie (steer sign or winner within rounding: TIE_BC, TIE_SCORE; False outside the grid),
    and fx_grid [50], the candidates."""
    B = state.shape[0]
    veh = orc.vehicle()
    out = dict(V=np.zeros(B), inb=np.zeros(B, bool), g=np.zeros((B, 7)), u2=np.zeros((B, 2)), Bc=np.zeros(B), scores=np.zeros((B, 50)), win=np.zeros(B, dtype=int),
               tie=np.zeros(B, bool))
    out["fx_grid"] = fx_grid = np.array([n / 49 * veh["Fx_max"] + (1 - n / 49) * veh["Fx_min"] for n in range(50)])
    for i in range(B):
        V, u2, Bc, sc = orc.hji_optimal_control_detail(state[i], other[i])
        _, g, inb = orc.hji_lookup(orc.hji_relative_state(state[i], other[i]))
        out["V"][i] = V; out["inb"][i] = inb; out["g"][i] = g; out["u2"][i] = u2; out["Bc"][i] = Bc; out["scores"][i] = sc
        if inb:
            out["win"][i] = int(np.argmax(sc))                               # np.argmax keeps the first maximiser, as the strict '>' of the line search does
            assert fx_grid[out["win"][i]] == u2[1], (i, out["win"][i], u2)
            out["tie"][i] = is_tie(veh, g, Bc, sc)
    return out
