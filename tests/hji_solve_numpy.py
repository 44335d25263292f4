"""numpy twin of pg_hji_solve (include/pigeon_mpc.h): the backward reachable tube of the 7-D relative system, float64 with V rounded to float32 after every sweep.
Written from the scheme as the header states it and from src/HJI_computation.jl -- relative_dynamics :74-88, optimal_disturbance :90-131 (tests/safety_numpy.py),
optimal_control :133-158 (new here, the 50-point line search vectorised over the nodes) -- with the bicycle model of tests/plant_numpy.py; independent of the device code.

Scheme (x_i the node, arrays column-major = dimension 1 fastest when flattened):
    p-_d = (V_i - V_{i-e_d}) / (x_d[i_d] - x_d[i_d-1]), p+_d forward; low face p- := p+, high face p+ := p-; periodic psi: node 0's low neighbour is node n-2 at
    spacing x[n-1] - x[n-2], node n-1's high neighbour is node 1 at spacing x[1] - x[0], and the last node's state carries the first knot's angle
    pbar = (p+ + p-) / 2;  uR* = optimal_control(x, pbar), uH* = optimal_disturbance(x, pbar) ((0, 0) where the other car's speed is <= 0);  f = relative_dynamics
    alpha_d = max_i |f_d|;  Hhat = pbar . f + sum_d alpha_d (p+_d - p-_d) / 2;  V <- float32(V + dt min(0, Hhat))
    dt = min(cfl / sum_d (alpha_d / min spacing_d), horizon - tau)  or  min(fixed_dt, horizon - tau)"""
import numpy as np

import plant_numpy as pn
import safety_numpy as sn


def optimal_control(X, x7, g):
    """optimal_control(X, x, gradV, :max; N = 50): (delta_opt [n], Fx_opt [n]); the first strict maximum of the 50 candidates wins (:152)."""
    x7 = np.atleast_2d(np.asarray(x7, dtype=np.float64)); g = np.atleast_2d(np.asarray(g, dtype=np.float64))
    Ux, Uy, r = x7[:, 3], x7[:, 4], x7[:, 6]
    A = g[:, 3] / X["m"]
    B = g[:, 4] / X["m"] + X["a"] * g[:, 6] / X["Izz"]
    Cc = g[:, 4] / X["m"] - X["b"] * g[:, 6] / X["Izz"]
    d = np.where(B >= 0, X["delta_max"], -X["delta_max"])
    sd, cd = np.sin(d), np.cos(d)
    af = np.arctan2(Uy + X["a"] * r, Ux) - d                    # lateral_tire_forces(BM, fake_qR, uR): vehicle_dynamics.jl:78-87
    ar = np.arctan2(Uy - X["b"] * r, Ux)
    V_opt = np.full(x7.shape[0], -np.inf); Fx_opt = np.zeros(x7.shape[0])
    for n in range(50):
        frac = n / 49
        Fx = frac * X["Fx_max"] + (1 - frac) * X["Fx_min"]
        Fxf, Fxr = (Fx * X["fwd_frac"], Fx * X["rwd_frac"]) if Fx > 0 else (Fx * X["fwb_frac"], Fx * X["rwb_frac"])     # longitudinal_tire_forces :279-283
        Fxf = np.full_like(Ux, Fxf); Fxr = np.full_like(Ux, Fxr)
        Fyf = Fxf * 0.0                                         # :64-76
        Fxt = Fxf * cd - Fyf * sd + Fxr
        for _ in range(3):
            Fzf = (X["m"] * X["G"] * X["b"] - X["h"] * Fxt) / X["L"]
            Fyf = pn._fiala_vec(af, X["Caf"], X["mu"], Fxf, Fzf)
            Fxt = Fxf * cd - Fyf * sd + Fxr
        Fzr = (X["m"] * X["G"] * X["a"] + X["h"] * Fxt) / X["L"]
        Fyr = pn._fiala_vec(ar, X["Car"], X["mu"], Fxr, Fzr)
        Vn = A * Fx + B * Fyf + Cc * Fyr
        better = Vn > V_opt
        Fx_opt = np.where(better, Fx, Fx_opt); V_opt = np.where(better, Vn, V_opt)
    return d, Fx_opt


def relative_dynamics(X, x7, uR, uH):
    """f [n, 7] of HJI_computation.jl:74-88: the bicycle (through its actuator limits, vehicle_dynamics.jl:310-314) at (dE, dN, dpsi, Ux, Uy, r) under uR = (delta, Fx),
    the other car under uH = (omega, a)."""
    x7 = np.atleast_2d(np.asarray(x7, dtype=np.float64))
    q = np.stack([x7[:, 0], x7[:, 1], x7[:, 2], x7[:, 3], x7[:, 4], x7[:, 6]], axis=1)
    bd = pn.world_vehicle_model_vec(X, q, np.atleast_2d(np.asarray(uR, dtype=np.float64)))
    uH = np.atleast_2d(np.asarray(uH, dtype=np.float64))
    dE, dN, dpsi, Ux, Uy, V, r = (x7[:, k] for k in range(7))
    return np.stack([V * np.cos(dpsi) - Ux + dN * r, V * np.sin(dpsi) - Uy - dE * r, uH[:, 0] - r, bd[:, 3], bd[:, 4], uH[:, 1], bd[:, 5]], axis=1)


def lam_norm(x7, g):
    """hypot(lam_Ax, lam_w / V) of optimal_disturbance (:101-104), NaN where V <= 0 (those rows never reach the threshold test)."""
    V = x7[:, 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(V > 0, np.hypot(g[:, 5], g[:, 2] / V), np.nan)


def hamiltonian_terms(X, x7, g):
    """(H = g . f, f, uR, uH) at states x7 and gradients g"""
    d, Fx = optimal_control(X, x7, g)
    uR = np.stack([d, Fx], axis=1)
    uH = sn.optimal_disturbance(X, x7, g)
    f = relative_dynamics(X, x7, uR, uH)
    return np.sum(g * f, axis=1), f, uR, uH


def one_sided(V, knots, periodic_psi):
    """(p-, p+): two lists of seven arrays of V's shape"""
    pm, pp = [], []
    for d in range(7):
        k = np.asarray(knots[d], dtype=np.float64); h = np.diff(k); n = len(k)
        W = np.moveaxis(V, d, 0)
        sh = (-1,) + (1,) * 6
        dv = (W[1:] - W[:-1]) / h.reshape(sh)                   # dv[i] = (V[i+1] - V[i]) / (x[i+1] - x[i])
        a = np.empty_like(W); b = np.empty_like(W)
        a[1:] = dv; b[:-1] = dv
        if d == 2 and periodic_psi:
            a[0] = (W[0] - W[n - 2]) / h[n - 2]; b[n - 1] = (W[1] - W[n - 1]) / h[0]
        else:
            a[0] = b[0]; b[n - 1] = a[n - 1]
        pm.append(np.moveaxis(a, 0, d)); pp.append(np.moveaxis(b, 0, d))
    return pm, pp


def node_states(knots, periodic_psi):
    """x [prod dims, 7] float64 in node order (dimension 1 fastest)"""
    ks = [np.asarray(k, dtype=np.float64).copy() for k in knots]
    if periodic_psi:
        ks[2][-1] = ks[2][0]
    G = np.meshgrid(*ks, indexing="ij")
    return np.stack([a.reshape(-1, order="F") for a in G], axis=1)


def _flat(arrs):
    return np.stack([a.reshape(-1, order="F") for a in arrs], axis=1)


def gradient(V_flat, knots, periodic_psi=False):
    """pbar of V [prod dims] (any float type), [prod dims, 7] float64"""
    dims = [len(k) for k in knots]
    V = np.asarray(V_flat, dtype=np.float64).reshape(dims, order="F")
    pm, pp = one_sided(V, knots, periodic_psi)
    return (_flat(pp) + _flat(pm)) / 2


def solve(X, knots, l0, horizon, cfl=0.8, fixed_dt=0.0, max_sweeps=100000, periodic_psi=False, on_sweep=None):
    """(V [prod dims] float32, gradV [prod dims, 7] float32, stats dict: sweeps, reached_horizon, tau, last_dt, alpha [7]).  on_sweep(k, x, pbar, V) is called at
    every sweep before its update."""
    dims = [len(k) for k in knots]
    V = np.asarray(l0, dtype=np.float32).reshape(dims, order="F")
    x = node_states(knots, periodic_psi)
    minsp = np.array([np.min(np.diff(np.asarray(k, dtype=np.float64))) for k in knots])
    tau, sweeps, last_dt, alpha = 0.0, 0, 0.0, np.zeros(7)
    reached = not horizon > 0.0
    while not reached and sweeps < max_sweeps:
        V64 = V.astype(np.float64)
        pm, pp = one_sided(V64, knots, periodic_psi)
        pm, pp = _flat(pm), _flat(pp)
        pbar = (pp + pm) / 2
        if on_sweep is not None:
            on_sweep(sweeps, x, pbar, V)
        H, f, _, _ = hamiltonian_terms(X, x, pbar)
        alpha = np.max(np.abs(f), axis=0)
        diss = np.zeros(x.shape[0])
        for d in range(7):
            diss = diss + alpha[d] * (pp[:, d] - pm[:, d]) * 0.5
        Hhat = H + diss
        with np.errstate(divide="ignore"):
            dt = fixed_dt if fixed_dt > 0.0 else cfl / np.sum(alpha / minsp)
        rem = horizon - tau
        last = not dt < rem
        if last:
            dt = rem
        Vn = V64.reshape(-1, order="F") + dt * np.minimum(0.0, Hhat)
        V = Vn.astype(np.float32).reshape(dims, order="F")
        sweeps += 1; last_dt = dt; tau = horizon if last else tau + dt; reached = last
    Vf = V.reshape(-1, order="F")
    g = gradient(Vf, knots, periodic_psi).astype(np.float32)
    return Vf.copy(), g, {"sweeps": sweeps, "reached_horizon": int(reached), "tau": tau, "last_dt": last_dt, "alpha": alpha}
