"""X1 parameter dictionary — mirrors /root/reference/src/vehicles.jl:1-59 (same keys, same formulas)."""
import math
import numbers


X1_BASE_FIELDS = ("G", "mfl", "mfr", "mrl", "mrr", "Ixx", "Iyy", "Izz", "L", "d", "hf", "hr", "h1", "mu", "Caf", "Car", "Fx_max", "Px_max", "Cd0", "Cd1", "Cd2",
                  "fwd_frac", "fwb_frac", "delta_max")


def X1(**overrides):
    """X1() is the reference's dictionary.  X1(mu=0.5, mfl=580.0, ...) overrides BASE fields (X1_BASE_FIELDS) and recomputes the derived ones -- m, a, b, h, rwd_frac,
    rwb_frac, Fx_min, kappa_max -- by the same formulas (vehicles.jl:10-56): a plant variant for set_plants."""
    for k in overrides:
        if k not in X1_BASE_FIELDS:
            raise KeyError(f"{k} is not a base field of X1 (derived fields are recomputed: {X1_BASE_FIELDS})")
    o = lambda name, default: float(overrides.get(name, default))
    X = {}
    X["G"] = o("G", 9.80665)
    X["mfl"], X["mfr"], X["mrl"], X["mrr"] = o("mfl", 484.0), o("mfr", 455.0), o("mrl", 521.0), o("mrr", 504.0)
    X["m"] = X["mfl"] + X["mfr"] + X["mrl"] + X["mrr"]
    X["Ixx"], X["Iyy"], X["Izz"] = o("Ixx", 175.0), o("Iyy", 1000.0), o("Izz", 2900.0)
    X["L"] = o("L", 2.87)
    X["d"] = o("d", 1.63)
    X["a"] = (X["mrl"] + X["mrr"]) / X["m"] * X["L"]
    X["b"] = (X["mfl"] + X["mfr"]) / X["m"] * X["L"]
    X["hf"], X["hr"], X["h1"] = o("hf", 0.1), o("hr", 0.1), o("h1", 0.37)
    X["h"] = X["hf"] * X["b"] / X["L"] + X["hr"] * X["a"] / X["L"] + X["h1"]
    X["mu"] = o("mu", 0.92)
    X["Caf"], X["Car"] = o("Caf", 150e3), o("Car", 220e3)
    X["Fx_max"], X["Px_max"] = o("Fx_max", 5600.0), o("Px_max", 75e3)
    X["Cd0"], X["Cd1"], X["Cd2"] = o("Cd0", 241.0), o("Cd1", 25.1), o("Cd2", 0.0)
    X["fwd_frac"] = o("fwd_frac", 0.0)
    X["rwd_frac"] = 1 - X["fwd_frac"]
    X["fwb_frac"] = o("fwb_frac", 0.6)
    X["rwb_frac"] = 1 - X["fwb_frac"]
    X["Fx_min"] = max(-X["m"] * X["G"] * X["a"] * X["mu"] / (X["L"] * X["rwb_frac"] + X["mu"] * X["h"]),
                      -X["m"] * X["G"] * X["b"] * X["mu"] / (X["L"] * X["fwb_frac"] - X["mu"] * X["h"]))
    X["delta_max"] = o("delta_max", 18 * math.pi / 180)
    X["kappa_max"] = math.tan(X["delta_max"]) / X["L"]
    return X


def CoupledControlParams(**kw):
    """Keyword constructor of /root/reference/src/coupled_lat_long.jl:23-40."""
    p = dict(V_min=1.0, V_max=15.0, k_V=10 / 4 / 100, k_s=10 / 4 / 10000, deltadot_max=0.344, Q_ds=1.0, Q_dpsi=1.0, Q_e=1.0,
             W_beta=50 / (10 * math.pi / 180), W_r=50.0, W_HJI=500.0, N_HJI=3, R_delta=0.0, R_ddelta=0.1, R_Fx=0.0, R_dFx=0.5)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def DecoupledControlParams(**kw):
    """Keyword constructor of /root/reference/src/decoupled_lat_long.jl:18-30."""
    d10 = 10 * math.pi / 180
    p = dict(V_min=1.0, V_max=15.0, k_V=10 / 4 / 100, k_s=10 / 4 / 10000, deltadot_max=0.344, Q_dpsi=1 / d10 ** 2, Q_e=1.0, W_beta=50 / d10, W_r=50.0,
             R_delta=0.0, R_ddelta=0.01 / d10 ** 2)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


ACTUATOR_FIELDS = ("delay_steps", "tau_delta", "tau_fx", "rate_delta", "rate_fx", "feedback")


def actuator(**overrides):
    """One actuator set for set_actuators (pg_actuator_set).  actuator() is the identity -- no delay, no lag, no slew limit, the controller sees the command it sent --, which
    reproduces the handle without a library bit for bit; actuator(delay_steps=3, tau_delta=0.1, feedback=1) overrides fields.  Build-defined: the reference has no actuator."""
    a = dict(delay_steps=0, tau_delta=0.0, tau_fx=0.0, rate_delta=math.inf, rate_fx=math.inf, feedback=0)
    for k, v in overrides.items():
        if k not in a:
            raise KeyError(f"{k} is not a field of an actuator set: {ACTUATOR_FIELDS}")
        a[k] = v
    return a


DISTURBANCE_FIELDS = ("step_on", "step_off", "Fx", "Fy", "Mz", "sigma_Fx", "sigma_Fy", "x_cp", "tau_gust", "mu_scale")


def disturbance(**overrides):
    """One disturbance set for set_disturbances (pg_disturbance).  disturbance() is the identity -- always active, no force, no moment, no gust, mu unscaled --, which
    reproduces the handle without a library bit for bit; disturbance(Fy=2000.0, sigma_Fy=800.0, tau_gust=0.3, step_on=3, step_off=9) overrides fields (step_off < 0: the
    window never closes).  Build-defined: the reference has no disturbance."""
    d = dict(step_on=0, step_off=-1, Fx=0.0, Fy=0.0, Mz=0.0, sigma_Fx=0.0, sigma_Fy=0.0, x_cp=0.0, tau_gust=0.0, mu_scale=1.0)
    for k, v in overrides.items():
        if k not in d:
            raise KeyError(f"{k} is not a field of a disturbance set: {DISTURBANCE_FIELDS}")
        d[k] = v
    return d


ESTIMATOR_FIELDS = ("predict", "reserved", "gain")
ESTIMATOR_CHANNELS = ("E", "N", "psi", "Ux", "Uy", "r")


def estimator(**overrides):
    """One estimator set for set_estimators (pg_estimator).  estimator() is the identity -- every gain 1: the controller reads the sensor's output itself --, which reproduces
    the handle without a library bit for bit; estimator(gain=0.2) is the fixed-gain observer with that gain on every channel and the controller's model as the prior
    (predict=1), estimator(gain=[1, 1, 0.2, 0.2, 0, 0.2]) sets the channels (E, N, psi, Ux, Uy, r) one by one, predict=0 makes every channel an exponential low-pass of the
    measurement.  Build-defined: the reference has no estimator."""
    e = dict(predict=1, reserved=0, gain=[1.0] * 6)
    for k, v in overrides.items():
        if k not in e:
            raise KeyError(f"{k} is not a field of an estimator set: {ESTIMATOR_FIELDS}")
        e[k] = v
    g = e["gain"]
    if isinstance(g, dict):
        for c in g:
            if c not in ESTIMATOR_CHANNELS:
                raise KeyError(f"{c} is not a channel of an estimator set: {ESTIMATOR_CHANNELS}")
        e["gain"] = [float(g.get(c, 1.0)) for c in ESTIMATOR_CHANNELS]
    elif isinstance(g, numbers.Real):                      # (numpy scalars included)
        e["gain"] = [float(g)] * 6
    else:
        e["gain"] = [float(x) for x in g]
        if len(e["gain"]) != 6:
            raise ValueError(f"gain has {len(e['gain'])} entries, not one per channel of {ESTIMATOR_CHANNELS}")
    return e


HUMAN_FIELDS = ("mode", "hold_steps", "step_on", "step_off", "gain", "omega_max", "a_min", "a_max", "sigma", "tau")
HUMAN_MODES = {"hold": 0, "worst": 1, "script": 2, "random": 3}


def human(**overrides):
    """One human set for set_humans (pg_human): the driver of the other car in the safety and node rollouts.  human() is the identity of mode 0 -- always active, a decision
    at every step, gain 1, no limits --, and human(mode=m) for m in (0, 1, 2) or ("hold", "worst", "script") reproduces a rollout called with that human mode on a handle
    without a library bit for bit; human(mode="worst", hold_steps=30, gain=0.6, step_on=40) overrides fields; mode 3 / "random" is the seeded driver (sigma, tau).
    gain and sigma take one number for both of (omega, a) or a pair.  Build-defined: the reference only receives the other car from ROS."""
    h = dict(mode=0, hold_steps=1, step_on=0, step_off=-1, gain=[1.0, 1.0], omega_max=math.inf, a_min=-math.inf, a_max=math.inf, sigma=[0.0, 0.0], tau=0.0)
    for k, v in overrides.items():
        if k not in h:
            raise KeyError(f"{k} is not a field of a human set: {HUMAN_FIELDS}")
        h[k] = v
    if isinstance(h["mode"], str):
        if h["mode"] not in HUMAN_MODES:
            raise KeyError(f"{h['mode']} is not a human mode: {tuple(HUMAN_MODES)}")
        h["mode"] = HUMAN_MODES[h["mode"]]
    for name in ("gain", "sigma"):
        v = h[name]
        if isinstance(v, numbers.Real):                    # (numpy scalars included)
            h[name] = [float(v)] * 2
        else:
            h[name] = [float(x) for x in v]
            if len(h[name]) != 2:
                raise ValueError(f"{name} has {len(h[name])} entries, not one per channel of (omega, a)")
    return h


ROUTE_EVENTS = 4
ROUTE_EVENT_FIELDS = ("step", "target", "target_mode", "anchor", "cold", "reserved", "t_join")
ROUTE_ANCHORS = {"keep": 0, "path": 1, "stamp": 2, "project": 3}


def route_event(step, target, anchor="stamp", relative=False, cold=True, t_join=0.0):
    """One event of a route set (pg_route_event): at clock step `step`, ahead of that step's controller, the instance goes to trajectory `target` of the installed library
    (relative=True: `target` trajectories on from the one it is on, modulo the library, negative allowed).  anchor: "keep" (the time offset stays), "path" (NaN: path
    tracking, the /des_path callback), "stamp" (the new trajectory's t = t_join is now; t_join = 0: the /des_traj callback), "project" (the state the controller sees is
    projected on the target and joins it t_join seconds further on; build-defined).  cold=True sets solved = false as the reference's callback does."""
    if isinstance(anchor, str):
        if anchor not in ROUTE_ANCHORS:
            raise KeyError(f"{anchor} is not an anchor: {tuple(ROUTE_ANCHORS)}")
        anchor = ROUTE_ANCHORS[anchor]
    for name, v in (("step", step), ("target", target), ("anchor", anchor)):
        if int(v) != v:
            raise ValueError(f"{name} = {v} is not a whole number")
    return dict(step=int(step), target=int(target), target_mode=int(bool(relative)), anchor=int(anchor), cold=int(bool(cold)), reserved=0, t_join=float(t_join))


def route(*events):
    """One route set for set_routes (pg_route): up to four route_event(...) in the order of their steps; route() is the identity (no event: pg_default_route)."""
    if len(events) > ROUTE_EVENTS:
        raise ValueError(f"a route set holds at most {ROUTE_EVENTS} events, not {len(events)}")
    return [dict(e) for e in events] + [route_event(-1, 0) for _ in range(ROUTE_EVENTS - len(events))]


SPEED_PLAN_FIELDS = ("mu_scale", "V_max", "V_floor", "V_start", "V_end", "ax_max", "ax_min", "ay_max")


def speed_plan(**overrides):
    """One plan set for plan_speeds (pg_speed_plan).  speed_plan() is the library's default (pg_default_speed_plan) -- all of the friction, V_max 30, V_floor 1 = the
    controller's V_min, free end speeds, no extra caps --; speed_plan(mu_scale=0.5, V_max=10.0, V_end=0.0) overrides fields (V_start / V_end: NaN = free, read on an open
    path only; ax_min <= 0 <= ax_max and ay_max > 0, +-Inf = none).  Build-defined: the reference receives its speed profile from a planner outside its tree."""
    p = dict(mu_scale=1.0, V_max=30.0, V_floor=1.0, V_start=math.nan, V_end=math.nan, ax_max=math.inf, ax_min=-math.inf, ay_max=math.inf)
    for k, v in overrides.items():
        if k not in p:
            raise KeyError(f"{k} is not a field of a speed plan: {SPEED_PLAN_FIELDS}")
        p[k] = float(v)
    return p


OFFSET_FIELDS = ("d0", "d1", "s_a", "s_b", "s_c", "s_d", "x_min", "edge_mode", "reserved")


def offset(**overrides):
    """One offset set for offset_paths (pg_offset_set).  offset() is the library's default (pg_default_offset_set), the identity: d0 = d1 = 0, no window (s_a = s_c =
    +Inf), x_min 0.1, edge_mode 0.  d0 / d1: the offset in metres, left positive, outside the windows / on the plateau; the rise d0 -> d1 runs over [s_a, s_b] and the fall
    d1 -> d0 over [s_c, s_d], metres of the source's arc length from its first knot; x_min: the smallest 1 - kappa d a pair may reach; edge_mode 0: the same road (the
    edges move by -d), 1: the tube travels with the path.  lane, lane_change and pass_by build the usual three.  Build-defined: the reference has no path maker."""
    p = dict(d0=0.0, d1=0.0, s_a=math.inf, s_b=math.inf, s_c=math.inf, s_d=math.inf, x_min=0.1, edge_mode=0, reserved=0)
    for k, v in overrides.items():
        if k not in p:
            raise KeyError(f"{k} is not a field of an offset set: {OFFSET_FIELDS}")
        p[k] = int(v) if k in ("edge_mode", "reserved") else float(v)
    return p


def lane(d, **overrides):
    """The same road d metres to the left (d < 0: to the right): offset(d0=d, d1=d)."""
    return offset(d0=d, d1=d, **overrides)


def lane_change(d0, d1, s_a, s_b, **overrides):
    """Leave the lane d0 at s_a and be on the lane d1 at s_b (metres of the source's arc length from its first knot): a single rise, no fall."""
    return offset(d0=d0, d1=d1, s_a=s_a, s_b=s_b, **overrides)


def pass_by(d, s_a, s_b, s_c, s_d, **overrides):
    """Go round something: leave the source at s_a, be d metres to the left at s_b, start back at s_c and be on the source again at s_d."""
    return offset(d0=0.0, d1=d, s_a=s_a, s_b=s_b, s_c=s_c, s_d=s_d, **overrides)


PASS_POLICIES = {"centre": 0, "wider": 1, "left": 2, "right": 3}


def obstacle(E, N, radius):
    """One disc in the world frame for clip_tubes (pg_obstacle)."""
    return dict(E=float(E), N=float(N), radius=float(radius), reserved=0.0)


def obstacle_set(obstacles=(), margin=0.0, taper=math.inf, min_width=0.0, policy="centre"):
    """One obstacle set for clip_tubes (pg_obstacle_set): a list of obstacle(...) dicts, the margin added to every radius (half the car's width plus clearance), the taper
    (metres of edge per metre of arc length by which a clip may relax; +Inf: the hard clip only), the width below which a knot counts as blocked, and the side policy:
    "centre" (an obstacle left of the centre line is passed on the right), "wider" (pass where more room is left), "left" / "right" (always pass on that side), or 0 .. 3.
    obstacle_set() is the library's default (pg_default_obstacle_set), the identity.  Build-defined: the reference has no obstacles."""
    p = PASS_POLICIES[policy] if isinstance(policy, str) else int(policy)
    return dict(obstacles=[dict(o) for o in obstacles], margin=float(margin), taper=float(taper), min_width=float(min_width), policy=p)


def _path_rows(path):
    """(s, E, N, psi, edge_L, edge_R) of a TrajectoryTube or of a channel array [10][L]"""
    if hasattr(path, "edge_L"):
        return path.s, path.E, path.N, path.psi, path.edge_L, path.edge_R
    return path[1], path[4], path[5], path[6], path[8], path[9]


def obstacle_at(channels, u, e, radius):
    """A disc beside a path, on the host: at the arc length u from the path's first knot and e metres to the left of it (the frame of make_starts: the left normal is
    (-cos psi, -sin psi)); E, N and psi are taken linear between the two knots around u.  channels: a TrajectoryTube or the channel array [10][L] of one path."""
    s, E, N, psi, _, _ = _path_rows(channels)
    n = len(s)
    x = float(s[0]) + float(u)
    i = 0
    while i < n - 2 and float(s[i + 1]) <= x:
        i += 1
    w = (x - float(s[i])) / (float(s[i + 1]) - float(s[i]))
    lin = lambda c: float(c[i]) + w * (float(c[i + 1]) - float(c[i]))
    p = lin(psi)
    return obstacle(lin(E) - float(e) * math.cos(p), lin(N) - float(e) * math.sin(p), radius)


def pass_by_around(report_row, edges_at, ramp, x_min=0.1):
    """The pass-by that goes round one obstacle of clip_tubes: report_row is the obstacle's record of the reports (the fields of pg_obstacle_report), edges_at the SOURCE
    path the tube was clipped from (a TrajectoryTube or its channel array [10][L]: its edges are read at k_at, its arc length at k_first and k_last).  The plateau lies in
    the middle of what the disc leaves on the side it is passed on: side = +1 (the left edge was clipped) gives d1 = 0.5 ((a_at - h_at) + edge_R), side = -1 gives
    d1 = 0.5 ((a_at + h_at) + edge_L); the rise ends at u(k_first), the fall starts at u(k_last), each over `ramp` metres.  side = 0 (no knot sees the obstacle) returns
    the identity set.  Raises ValueError where the free side is narrower than 0.  Returns a pass_by(...) set for offset_paths."""
    r = report_row
    side = int(r["side"])
    if side == 0:
        return offset(x_min=x_min)
    s, _, _, _, eL, eR = _path_rows(edges_at)
    k = int(r["k_at"])
    a, h = float(r["a_at"]), float(r["h_at"])
    if side > 0:
        lo, hi = float(eR[k]), a - h
    else:
        lo, hi = a + h, float(eL[k])
    if hi - lo < 0.0:
        raise ValueError(f"pass_by_around: the obstacle leaves {hi - lo:.3f} m on the side it is passed on (knot {k})")
    u1 = float(s[int(r["k_first"])]) - float(s[0])
    u2 = float(s[int(r["k_last"])]) - float(s[0])
    return pass_by(0.5 * (hi + lo), u1 - float(ramp), u1, u2, u2 + float(ramp), x_min=x_min)


REFINE_M_MAX = 4096      # the most parts one source interval may be cut into (pg_refine_paths)


def refine(ds=math.inf, windows=()):
    """One refine set for refine_paths (pg_refine_set).  refine() is the library's default (pg_default_refine_set), the identity.  ds: the largest knot spacing wanted
    everywhere (m; +Inf: none).  windows: up to four (s_lo, s_hi, ds_w) -- the largest spacing ds_w wanted between s_lo and s_hi, metres of the source's arc length from
    its first knot.  A source interval a window reaches into is cut WHOLE into equal parts no longer than ds_w; windows may overlap (the smallest spacing holds), one
    beyond the path's end has no effect.  Build-defined: the reference has no path maker."""
    w = [(float(a), float(b), float(c)) for a, b, c in windows]
    if len(w) > 4:
        raise ValueError(f"refine: {len(w)} windows (at most 4)")
    return dict(ds=float(ds), windows=w)


def refine_parts(rset, diff, u_lo, u_hi):
    """m_i of pg_refine_paths, restated: the parts the source interval [u_lo, u_hi] (arc length from the first knot) of length diff is cut into under the set;
    REFINE_M_MAX + 1 stands for every count above REFINE_M_MAX (the library refuses it).  Python floats are doubles and every operation is one rounding, as in the library."""
    w = rset["ds"]
    for s_lo, s_hi, ds_w in rset["windows"]:
        if s_lo < math.inf and s_lo < u_hi and s_hi > u_lo:
            w = min(w, ds_w)
    if not w < math.inf or diff <= w:
        return 1
    q = diff / w
    if not q <= float(REFINE_M_MAX):
        return REFINE_M_MAX + 1
    return int(math.ceil(q))


def refine_for(offset_set, knots=10):
    """The refine set that gives the rise and the fall window of an offset set (lane_change, pass_by, pass_by_around) at least `knots` knot intervals each: a window
    (s_a, s_b, (s_b - s_a) / knots) per ramp.  An offset set without windows gives the identity."""
    if not (knots == int(knots) and knots >= 1):
        raise ValueError("refine_for: knots is an integer >= 1")
    w = []
    for a, b in ((offset_set["s_a"], offset_set["s_b"]), (offset_set["s_c"], offset_set["s_d"])):
        if math.isfinite(a):
            w.append((a, b, (b - a) / float(knots)))
    return refine(windows=w)


def refine_around(seen, source, ds_w, reach, radius=None):
    """The refine set that puts knots ds_w apart around one disc, from `reach` metres before the first to `reach` after the last place it can be seen.  seen: the disc's
    record of clip_tubes' reports (the fields of pg_obstacle_report), or an obstacle(...) dict; source: the path (a TrajectoryTube or its channel array [10][L]).
    A record with side != 0: from u(k_first) - reach to u(k_last) + reach.  A record with side = 0 (no knot saw the disc): the closest knot's arc length -+ (R + reach),
    R = `radius` (the disc's radius plus the set's margin; the record does not carry it) -- choose reach to cover the knot spacing there.  An obstacle: its projection
    onto the source's chords on the host, -+ (radius + reach)."""
    s, E, N, _, _, _ = _path_rows(source)
    s0, ds_w, reach = float(s[0]), float(ds_w), float(reach)
    if isinstance(seen, dict) and "E" in seen:
        R = float(seen["radius"]) if radius is None else float(radius)
        best = (math.inf, 0.0)
        for i in range(len(s) - 1):
            aE, aN = float(E[i]), float(N[i])
            dE, dN = float(E[i + 1]) - aE, float(N[i + 1]) - aN
            lam = min(1.0, max(0.0, ((seen["E"] - aE) * dE + (seen["N"] - aN) * dN) / (dE * dE + dN * dN)))
            q = (seen["E"] - (aE + lam * dE)) ** 2 + (seen["N"] - (aN + lam * dN)) ** 2
            if q < best[0]:
                best = (q, float(s[i]) + lam * (float(s[i + 1]) - float(s[i])) - s0)
        lo, hi = best[1] - (R + reach), best[1] + (R + reach)
    elif int(seen["side"]) != 0:
        lo, hi = float(s[int(seen["k_first"])]) - s0 - reach, float(s[int(seen["k_last"])]) - s0 + reach
    else:
        if radius is None:
            raise ValueError("refine_around: a record with side = 0 needs radius= (the disc's radius plus the set's margin)")
        lo, hi = float(seen["u_at"]) - (float(radius) + reach), float(seen["u_at"]) + (float(radius) + reach)
    if not hi > lo:
        raise ValueError("refine_around: the window is empty (reach >= 0, and > 0 where a single knot sees the disc)")
    return refine(windows=[(lo, hi, ds_w)])


START_RANGES = ("s", "e", "dpsi", "v", "uy", "dr", "delta", "fx", "dt0", "other_dx", "other_dy", "other_dpsi", "other_v")
START_MODES = ("s_mode", "e_mode", "steady", "time_mode", "other_mode")


def start(**overrides):
    """One start set for make_starts (pg_start_set).  start() is the library's default (pg_default_start_set): every range [0, 0] except the speed factor v = [1, 1],
    every mode 0 -- on the profile, at the first knot.  A range is given as one value or a pair: start(s=(5.0, 120.0), e=(-0.5, 0.5), v=1.05) or by its ends
    (s_lo=5.0, s_hi=120.0); the modes by name (s_mode=1: s as a fraction of the tube's length; e_mode=1: e as a fraction of the local tube, -1 = edge_R, +1 = edge_L;
    steady=1: the body state and control of steady_state_estimates; time_mode=1: path mode, time_offset = NaN; other_mode=1: the other car from the other_* ranges, ego
    frame).  Build-defined: the reference receives its state from the car."""
    p = {f"{n}_{end}": (1.0 if n == "v" else 0.0) for n in START_RANGES for end in ("lo", "hi")}
    p.update({m: 0 for m in START_MODES})
    for k, v in overrides.items():
        if k in START_RANGES:
            lo, hi = (v, v) if isinstance(v, numbers.Real) else v
            p[k + "_lo"], p[k + "_hi"] = float(lo), float(hi)
        elif k in START_MODES:
            p[k] = int(v)
        elif k in p:
            p[k] = float(v)
        else:
            raise KeyError(f"{k} is not a field of a start set: the ranges {START_RANGES} (or <range>_lo / <range>_hi) and the modes {START_MODES}")
    return p


def start_config2(s_range=None, traj_mode=True):
    """The start set whose ranges are those of synthetic.config2_inputs: e +-0.5 m, heading +-0.1 rad, V(s) x [0.9, 1.1], Uy +-0.2, r +-0.05, delta +-0.05, Fx +-500 N,
    t0 +-0.2 s.  The same distribution, different numbers: the draws come from Philox per (seed, stream), not from a PCG64 stream over the batch, and V and t are the
    controller's own lookup instead of a linear interpolation.  s_range = (lo, hi) in metres from the first knot; None takes the whole tube (s_mode 1, [0, 1]) --
    config2_inputs' default window [5, s_end - 60] m needs the tube's length, which after an install only the device holds."""
    s = dict(s=(0.0, 1.0), s_mode=1) if s_range is None else dict(s=tuple(s_range))
    return start(e=(-0.5, 0.5), dpsi=(-0.1, 0.1), v=(0.9, 1.1), uy=(-0.2, 0.2), dr=(-0.05, 0.05), delta=(-0.05, 0.05), fx=(-500.0, 500.0), dt0=(-0.2, 0.2),
                 time_mode=0 if traj_mode else 1, **s)


PATH_SEGMENT_FIELDS = ("length", "kappa0", "kappa1", "edge_L0", "edge_L1", "edge_R0", "edge_R1", "reserved")


def path_segment(**overrides):
    """One segment for make_paths (pg_path_segment).  path_segment() is the library's default (pg_default_path_segment): a 1 m line with the edges at +4 / -4 m
    (trajectories.jl:43-44); path_segment(length=15.0, kappa1=1 / 14.5) is a clothoid from a straight into a left turn of radius 14.5 m.  The curvature and the edges are
    linear in the arc length between the two ends.  edge_L=3.0 / edge_R=-2.0 set both ends of an edge at once.  Build-defined: the reference generates straight lines only."""
    g = dict(length=1.0, kappa0=0.0, kappa1=0.0, edge_L0=4.0, edge_L1=4.0, edge_R0=-4.0, edge_R1=-4.0, reserved=0.0)
    for k, v in overrides.items():
        if k in ("edge_L", "edge_R"):
            g[k + "0"] = g[k + "1"] = float(v)
        elif k in g:
            g[k] = float(v)
        else:
            raise KeyError(f"{k} is not a field of a path segment: {PATH_SEGMENT_FIELDS} (edge_L / edge_R set both ends)")
    return g


WAYPOINT_FIELDS = ("E", "N", "edge_L", "edge_R")


def waypoint(**overrides):
    """One waypoint for fit_paths (pg_waypoint).  waypoint() is the library's default (pg_default_waypoint): the origin with the edges at +4 / -4 m (trajectories.jl:43-44);
    waypoint(E=12.0, N=-3.5, edge_L=3.0) is a surveyed point with its own left edge.  The edges are linear in the chord parameter between two waypoints."""
    w = dict(E=0.0, N=0.0, edge_L=4.0, edge_R=-4.0)
    for k, v in overrides.items():
        if k not in w:
            raise KeyError(f"{k} is not a field of a waypoint: {WAYPOINT_FIELDS}")
        w[k] = float(v)
    return w


def smooth(**overrides):
    """One smoothing set for smooth_waypoints (pg_smooth_set).  smooth() is the library's default (pg_default_smooth_set), the identity.  lam: lambda in m^3, the weight
    of the integral of g''^2 over the chord parameter against the sum of the squared displacements (0: the waypoints come back bit for bit; 0.1 moves the recorded oval's
    points by a quarter of a millimetre and takes the rounding out of its curvature).  pin_ends: the two end waypoints of an open path do not move.  keep_walls: the tube
    edges of a moved waypoint are shifted by the normal part of its displacement, so the walls stay where they were surveyed.  windows: up to four smooth_window(...)
    entries; the last listed one that holds a waypoint's cumulative chord length sets its inverse weight."""
    s = dict(lam=0.0, pin_ends=False, keep_walls=False, windows=[])
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(f"{k} is not a field of a smoothing set: {sorted(s)}")
        s[k] = v
    s["lam"] = float(s["lam"]); s["pin_ends"] = bool(s["pin_ends"]); s["keep_walls"] = bool(s["keep_walls"])
    s["windows"] = [(float(a), float(b), float(c)) for a, b, c in s["windows"]]
    if len(s["windows"]) > 4:
        raise ValueError(f"smooth: {len(s['windows'])} windows (at most 4)")
    return s


def tune(target=1e-3, lambda_lo=1e-6, lambda_hi=1e3, rounds=3, **smooth_kw):
    """One tune set for tune_smoothing (pg_tune_set).  tune() is the library's default (pg_default_tune_set).  target: the rms displacement in metres not to exceed --
    how good the surveyed positions are, say 1e-3 for positions rounded to a millimetre.  lambda_lo < lambda_hi: the first bracket of the weight in m^3.  rounds: 1 .. 8,
    each divides the bracket's ratio by its 16th root.  smooth_kw: pin_ends, keep_walls and windows as smooth() takes them; the weight itself is what the call chooses."""
    if "lam" in smooth_kw:
        raise KeyError("lam is what tune_smoothing chooses: give target, lambda_lo and lambda_hi")
    return dict(base=smooth(**smooth_kw), target=float(target), lambda_lo=float(lambda_lo), lambda_hi=float(lambda_hi), rounds=int(rounds))


def smooth_window(u_lo, u_hi, factor=0.0):
    """One window of a smoothing set: the waypoints whose cumulative chord length (metres from the path's first waypoint) lies in [u_lo, u_hi] get the inverse weight
    `factor` -- 0 pins them ("do not touch the chicane"), above 1 smooths them more than the rest."""
    return (float(u_lo), float(u_hi), float(factor))


def line(h_mean=1.0, **overrides):
    """One line set for optimize_line (pg_line_set).  mu and rho are given as multiples of 1 / h_mean^3, h_mean the path's mean chord in metres: line(h_mean=3.74) is
    mu = 1e-6 / h^3, rho = 0.1 / h^3, the scale at which the bend Hessian's entries are of order one (EXPERIMENTS 43: on the committed ovals taken every 16th point 1000
    iterations leave r_prim at 5e-7 m with rho = 0.1 / h^3, 2e-4 m with 0.03 and 1e-5 m with 0.3; ten times more or less still converges, more slowly).  line() with h_mean = 1 is the library's
    default (pg_default_line_set).  margin: metres kept between the line and each edge.  alpha_max: the largest move along the normal.  iters: 1 .. 4096.  tol: stops
    where both ADMM residuals are at most this (0: all iterations).  pin_ends: the ends of an open path do not move.  keep_walls: the edges are shifted by -alpha, so the
    walls stay where they were surveyed and a second call re-linearises about the first result.  windows: up to four line_window(...) entries; the last listed one that
    holds a waypoint's cumulative chord length sets its margin, or pins it."""
    s = dict(mu=1e-6, rho=0.1, margin=0.5, alpha_max=2.0, tol=0.0, iters=1000, pin_ends=False, keep_walls=False, windows=[])
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(f"{k} is not a field of a line set: {sorted(s)} (and h_mean)")
        s[k] = v
    h3 = float(h_mean) ** 3
    if not (math.isfinite(h3) and h3 > 0.0):
        raise ValueError("line: h_mean is finite and > 0")
    s["mu"] = float(s["mu"]) / h3; s["rho"] = float(s["rho"]) / h3
    for k in ("margin", "alpha_max", "tol"):
        s[k] = float(s[k])
    s["iters"] = int(s["iters"]); s["pin_ends"] = bool(s["pin_ends"]); s["keep_walls"] = bool(s["keep_walls"])
    s["windows"] = [(float(a), float(b), float(c), int(bool(d))) for a, b, c, d in s["windows"]]
    if len(s["windows"]) > 4:
        raise ValueError(f"line: {len(s['windows'])} windows (at most 4)")
    return s


def line_window(u_lo, u_hi, margin=0.5, pin=False):
    """One window of a line set: the waypoints whose cumulative chord length (metres from the path's first waypoint) lies in [u_lo, u_hi] keep `margin` metres to each
    edge instead of the set's own -- or, with pin=True, do not move at all ("the line through the gate is the surveyed one")."""
    return (float(u_lo), float(u_hi), float(margin), int(bool(pin)))


def waypoints_from_tube(tube, every=1, closed=False):
    """The knots 0, every, 2 every, .. of a TrajectoryTube -- or of a committed path as its file holds it (the keys posE_m, posN_m, edgeL_m, edgeR_m) -- as a waypoint list
    for fit_paths: "the same track thinned to every n-th point".  closed=True: the file repeats knot 0 as its last knot, which is dropped (fit_paths closes the path itself);
    closed=False: the last knot is kept whatever `every` is, so the path ends where the tube ends."""
    if not (every == int(every) and every >= 1):
        raise ValueError("waypoints_from_tube: every is an integer >= 1")
    if isinstance(tube, dict) or hasattr(tube, "files"):
        E, N, eL, eR = (tube[k] for k in ("posE_m", "posN_m", "edgeL_m", "edgeR_m"))
    else:
        E, N, eL, eR = tube.E, tube.N, tube.edge_L, tube.edge_R
    n = len(E) - 1 if closed else len(E)
    idx = list(range(0, n, int(every)))
    if not closed and idx[-1] != n - 1:
        idx.append(n - 1)
    return [waypoint(E=E[i], N=N[i], edge_L=eL[i], edge_R=eR[i]) for i in idx]


def line_segments(length, **edges):
    """A straight of `length` m: one segment.  **edges: the edge fields of path_segment, applied to every segment (as in the other builders)."""
    return [path_segment(length=length, **edges)]


def circle_segments(radius, turns=1, **edges):
    """`turns` laps of a circle: one arc of curvature 1 / radius (radius < 0: a right turn) and length 2 pi |radius| turns."""
    if radius == 0 or not turns > 0:
        raise ValueError("circle_segments: radius != 0 and turns > 0")
    k = 1.0 / float(radius)
    return [path_segment(length=2.0 * math.pi * abs(float(radius)) * turns, kappa0=k, kappa1=k, **edges)]


def oval_segments(straight, radius, clothoid, **edges):
    """An oval from the start of a straight, once around (left turns; radius < 0: right turns): two halves of line, clothoid in, arc, clothoid out.  The clothoids take
    clothoid / |radius| of each half turn, the arc the angle pi - clothoid / |radius| that is left -- it has to be positive.  clothoid = 0 drops the clothoids.  The path
    closes by symmetry; make_paths reports what the arithmetic leaves (closure_pos, closure_psi)."""
    straight, radius, clothoid = float(straight), float(radius), float(clothoid)
    if not (straight > 0 and radius != 0 and clothoid >= 0):
        raise ValueError("oval_segments: straight > 0, radius != 0, clothoid >= 0")
    r = abs(radius)
    angle = math.pi - clothoid / r
    if not angle > 0:
        raise ValueError(f"oval_segments: clothoids of {clothoid} m take the whole half turn at radius {r} m (the arc's angle pi - clothoid / radius = {angle} must be positive)")
    k = 1.0 / radius
    arc = angle * r
    for _ in range(4):                                       # 1 / radius is rounded: take the neighbour of angle * radius at which |k| * length rounds to the angle, if one does
        got = abs(k) * arc
        if got == angle:
            break
        arc = math.nextafter(arc, math.inf if got < angle else 0.0)
    else:
        arc = angle * r
    half = [path_segment(length=straight, **edges)]
    if clothoid > 0:
        half.append(path_segment(length=clothoid, kappa0=0.0, kappa1=k, **edges))
    half.append(path_segment(length=arc, kappa0=k, kappa1=k, **edges))
    if clothoid > 0:
        half.append(path_segment(length=clothoid, kappa0=k, kappa1=0.0, **edges))
    return [dict(g) for g in half + half]


LANE_CHANGE_TOL = 1e-11      # m: what lane_change_segments leaves between the offset asked for and the one its segments integrate to


def _lateral_shift(segs, pieces=16):
    """the shift to the left of a path that starts with psi = 0, over its segments: the integral of sin psi by the 4-point Gauss-Legendre rule of pg_make_paths
    (include/pigeon_mpc.h) on `pieces` pieces per segment"""
    X = (-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526)
    W = (0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538)
    psib, shift = 0.0, 0.0
    for g in segs:
        h = g["length"] / pieces
        for p in range(pieces):
            for x, w in zip(X, W):
                u = (p + 0.5 + 0.5 * x) * h
                shift += 0.5 * h * w * math.sin(psib + u * (g["kappa0"] + 0.5 * (g["kappa1"] - g["kappa0"]) * u / g["length"]))
        psib += 0.5 * (g["kappa0"] + g["kappa1"]) * g["length"]
    return shift


def lane_change_segments(offset, length, **edges):
    """A lane change of `offset` m (> 0: to the left, the side of edge_L) over `length` m of arc: four clothoids of length / 4 with the curvature 0 -> k -> 0 -> -k -> 0,
    so the heading ends where it started.  The peak curvature k is solved by bisection on the path's own integral (_lateral_shift: the quadrature of pg_make_paths) until
    the shift is within LANE_CHANGE_TOL = 1e-11 m of the offset; the heading peaks at k length / 4, and an offset that would need more than a quarter turn is refused."""
    offset, length = float(offset), float(length)
    if not (length > 0 and math.isfinite(offset)):
        raise ValueError("lane_change_segments: length > 0 and a finite offset")
    q = length / 4.0

    def segs(k):
        return [path_segment(length=q, kappa0=a, kappa1=b, **edges) for a, b in ((0.0, k), (k, 0.0), (0.0, -k), (-k, 0.0))]

    if offset == 0:
        return segs(0.0)
    sign, want = math.copysign(1.0, offset), abs(offset)
    lo, hi = 0.0, 2.0 * math.pi / length                     # (the heading peaks at a quarter turn at hi: the shift grows with k up to there)
    if _lateral_shift(segs(hi)) < want:
        raise ValueError(f"lane_change_segments: {want} m cannot be reached in {length} m without turning past a quarter turn")
    for _ in range(200):
        k = 0.5 * (lo + hi)
        d = _lateral_shift(segs(k)) - want
        if abs(d) <= 0.1 * LANE_CHANGE_TOL or k in (lo, hi):
            break
        lo, hi = (k, hi) if d < 0 else (lo, k)
    return segs(sign * k)
