"""The yardstick of the plant-set tests: the ego plant of a rollout step and the tracking summary, in numpy, per instance.

plant_step: `propagate(dynamics, state, StepControl(dt, BicycleControl2(control)))` of simulate (model_predictive_control.jl:94) -- classical RK4, `nsub` sub-steps, the
control (delta, Fx = Fxf + Fxr) held, right-hand side oracle/spec_numpy.world_vehicle_model(P, q, u2) (VehicleModel{BicycleModel}, vehicle_dynamics.jl:310-314 over
:111-135, through the actuator limits :293-298) with P the vehicle dictionary OF THAT INSTANCE.  Written from the reference's equations, not from the device code.
spec_numpy's model is scalar Python (0.4 ms a call: a 70-instance, 12-step replay would take 15 s), so the GPU tests use plant_step_vec: the same statements in the same
order on arrays over the instances, every `if` of the scalar model a np.where.  tests/test_plant_sets_host.py pins both to the C++ oracle's plant_step at P = X1 and
to each other under other vehicles.

tracking_summary: what pg_get_tracking_state documents, from per-step arrays of (s, e) -- the step's path_coordinates (trajectories.jl:71-94) -- the body-frame
velocities and the tube's edges at s (interp_by_s, trajectories.jl:32-35)."""
import numpy as np

from oracle import spec_numpy as sp

VEH_FIELDS = ["G", "m", "Izz", "L", "a", "b", "h", "mu", "Caf", "Car", "Cd0", "Cd1", "Cd2", "fwd_frac", "rwd_frac", "fwb_frac", "rwb_frac", "Fx_max", "Fx_min", "Px_max",
              "delta_max", "kappa_max"]


def _rk4_one(P, q, u2, dt, nsub):
    f = lambda x: np.array(sp.world_vehicle_model(P, [float(v) for v in x], u2), dtype=np.float64)
    x = np.array(q, dtype=np.float64); h = dt / nsub
    for _ in range(nsub):
        k1 = f(x); k2 = f(x + k1 * (h * 0.5)); k3 = f(x + k2 * (h * 0.5)); k4 = f(x + k3 * h)
        x = x + (k1 + 2.0 * k2 + 2.0 * k3 + k4) * (h / 6.0)
    return x


def plant_step(P, q, u3, dt, nsub=10):
    """q [B][6] (E, N, psi, Ux, Uy, r), u3 [B][3] (delta, Fxf, Fxr) -> the states one step of length dt later, [B][6].  P: one vehicle dict for every instance, or a
    sequence of B dicts (instance b integrates P[b])."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 6); u3 = np.asarray(u3, dtype=np.float64).reshape(-1, 3)
    per = (lambda b: P) if isinstance(P, dict) else (lambda b: P[b])
    return np.stack([_rk4_one(per(b), q[b], (float(u3[b, 0]), float(u3[b, 1] + u3[b, 2])), dt, nsub) for b in range(q.shape[0])])


def _fiala_vec(alpha, Ca, mu, Fx, Fz):
    """fiala / _fiala of vehicle_dynamics.jl:35-62 on arrays"""
    F_max = mu * Fz
    with np.errstate(invalid="ignore", divide="ignore"):
        Fy_max = np.sqrt(F_max * F_max - Fx * Fx)
        tana = np.tan(alpha)
        slide = 3 * Fy_max / Ca
        ratio = np.abs(tana / slide)
        inside = -Ca * tana * (1 - ratio + ratio * ratio / 3)
        sliding = -Fy_max * np.sign(tana)
    return np.where(np.abs(Fx) >= F_max, F_max * 0.0, np.where(ratio <= 1, inside, sliding))


def world_vehicle_model_vec(P, q, u2):
    """spec_numpy.world_vehicle_model on arrays: P a dict of arrays [B] (or scalars), q [B][6], u2 [B][2] -> [B][6]"""
    Ux, Uy, r = q[:, 3], q[:, 4], q[:, 5]
    d = np.where(u2[:, 0] < -P["delta_max"], -P["delta_max"], u2[:, 0]); d = np.where(d > P["delta_max"], P["delta_max"], d)      # apply_control_limits :293-298
    f = np.where(P["Fx_max"] < u2[:, 1], P["Fx_max"], u2[:, 1]); f = np.where(P["Px_max"] / Ux < f, P["Px_max"] / Ux, f); f = np.where(P["Fx_min"] > f, P["Fx_min"], f)
    Fxf = np.where(f > 0, f * P["fwd_frac"], f * P["fwb_frac"]); Fxr = np.where(f > 0, f * P["rwd_frac"], f * P["rwb_frac"])          # longitudinal_tire_forces :279-283
    s, c = np.sin(q[:, 2]), np.cos(q[:, 2])
    sd, cd = np.sin(d), np.cos(d)                                                                                                     # _body: :111-135
    af = np.arctan2(Uy + P["a"] * r, Ux) - d
    ar = np.arctan2(Uy - P["b"] * r, Ux)
    Fyf = Fxf * 0.0                                                                                                                   # lateral_tire_forces :64-76
    Fx = Fxf * cd - Fyf * sd + Fxr
    for _ in range(3):
        Fzf = (P["m"] * P["G"] * P["b"] - P["h"] * Fx) / P["L"]
        Fyf = _fiala_vec(af, P["Caf"], P["mu"], Fxf, Fzf)
        Fx = Fxf * cd - Fyf * sd + Fxr
    Fzr = (P["m"] * P["G"] * P["a"] + P["h"] * Fx) / P["L"]
    Fyr = _fiala_vec(ar, P["Car"], P["mu"], Fxr, Fzr)
    Fx_drag = -P["Cd0"] - Ux * (P["Cd1"] + P["Cd2"] * Ux)
    Fxf_t = Fxf * cd - Fyf * sd
    Fyf_t = Fyf * cd + Fxf * sd
    return np.stack([-Ux * s - Uy * c, Ux * c - Uy * s, r, (Fxf_t + Fxr + Fx_drag) / P["m"] + r * Uy, (Fyf_t + Fyr) / P["m"] - r * Ux,
                     (P["a"] * Fyf_t - P["b"] * Fyr) / P["Izz"]], axis=1)


def stack_vehicles(P, B):
    """one dict or a sequence of B dicts -> a dict of arrays [B]"""
    Ps = [P] * B if isinstance(P, dict) else list(P)
    assert len(Ps) == B
    return {k: np.array([float(p[k]) for p in Ps]) for k in VEH_FIELDS}


def plant_step_vec(P, q, u3, dt, nsub=10):
    """plant_step, vectorised over the instances (P: one dict, a sequence of B dicts, or stack_vehicles' dict of arrays)"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 6); u3 = np.asarray(u3, dtype=np.float64).reshape(-1, 3)
    Pv = P if isinstance(P, dict) and np.ndim(P["m"]) == 1 else stack_vehicles(P, q.shape[0])
    u2 = np.stack([u3[:, 0], u3[:, 1] + u3[:, 2]], axis=1)
    f = lambda x: world_vehicle_model_vec(Pv, x, u2)
    x = q.copy(); h = dt / nsub
    for _ in range(nsub):
        k1 = f(x); k2 = f(x + k1 * (h * 0.5)); k3 = f(x + k2 * (h * 0.5)); k4 = f(x + k3 * h)
        x = x + (k1 + 2.0 * k2 + 2.0 * k3 + k4) * (h / 6.0)
    return x


def tube_edges(traj12, s):
    """(edge_L, edge_R) of the tube at arclengths s (any shape) -- spec_numpy.Trajectory.interp_by_s, element by element."""
    T = sp.Trajectory(traj12)
    s = np.asarray(s, dtype=np.float64)
    eL = np.empty(s.shape); eR = np.empty(s.shape)
    for i in np.ndindex(s.shape):
        c = T.interp_by_s(float(s[i])); eL[i] = c["edge_L"]; eR[i] = c["edge_R"]
    return eL, eR


def tracking_summary(s, e, Ux, Uy, r, edge_L, edge_R, step0=0):
    """All arguments [steps][B]: step k of the history is the clock's step step0 + k.  Returns (summary [B][6] = max |e|, sum e^2, max |Uy / Ux|, max |r|, min Ux, s of
    the last step; steps [B]; first_exit [B]: the first step with e outside [edge_R, edge_L], -1 if none; margin [B] = min over the steps of the distance of e from the
    nearer edge -- where it is tiny, which side a rounding error puts e on is not decided)."""
    s, e, Ux, Uy, r, edge_L, edge_R = (np.asarray(a, dtype=np.float64) for a in (s, e, Ux, Uy, r, edge_L, edge_R))
    K, B = e.shape
    summary = np.stack([np.max(np.abs(e), axis=0), np.sum(e * e, axis=0), np.max(np.abs(Uy / Ux), axis=0), np.max(np.abs(r), axis=0), np.min(Ux, axis=0), s[-1]], axis=1)
    out = (e > edge_L) | (e < edge_R)
    first_exit = np.where(out.any(axis=0), step0 + np.argmax(out, axis=0), -1).astype(np.int32)
    margin = np.min(np.minimum(np.abs(e - edge_L), np.abs(e - edge_R)), axis=0)
    return summary, np.full(B, K, dtype=np.int32), first_exit, margin


def four_plants(X1):
    """The plant sets of the GPU tests (X1: pigeon.jl_amd.vehicles.X1): the controller's own vehicle, low friction, a heavier car, softer tires with less drive force."""
    base = X1()
    return [base, X1(mu=0.5), X1(mfl=1.2 * base["mfl"], mfr=1.2 * base["mfr"], mrl=1.2 * base["mrl"], mrr=1.2 * base["mrr"], Izz=1.2 * base["Izz"]),
            X1(Caf=0.7 * base["Caf"], Car=0.7 * base["Car"], Fx_max=3000.0)]
