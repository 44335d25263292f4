"""Host-side mirror of the reference's MPC call convention for a BATCH of independent instances.

Reference seam (relative to /root/reference/src): the five generic functions of model_predictive_control.jl:70-78
applied to a mutable TrajectoryTrackingMPC (:32-68), called in this order by ros_integration.jl:96-99,124 and by
simulate (:80-100).  Julia's `f!(mpc)` spelling becomes `f_(mpc)` here; argument meaning and order are unchanged.
Everything numerical happens in libpigeon_hip.so (HIP, gfx950); this module only marshals arrays.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .trajectories import TrajectoryTube
from .vehicles import X1, CoupledControlParams, DecoupledControlParams, actuator as _identity_actuator, disturbance as _identity_disturbance, estimator as _identity_estimator, human as _identity_human, route as _route, speed_plan as _default_speed_plan, path_segment as _default_path_segment, waypoint as _default_waypoint, start as _default_start, offset as _default_offset, obstacle_set as _default_obstacle_set, refine as _default_refine, smooth as _default_smooth, tune as _default_tune, line as _default_line, refine_parts as _refine_parts, REFINE_M_MAX

c_dp = C.POINTER(C.c_double)
c_i32p = C.POINTER(C.c_int32)

SOLVED, MAX_ITER, NUMERICAL, INFEASIBLE_X0, SOLVED_UNVERIFIED = 1, 2, 3, 4, 5
SPEED_PLAN_STATS_DTYPE = np.dtype([(n, np.float64 if c is C.c_double else np.int32) for n, c in _lib.pg_speed_plan_stats._fields_])      # 48 bytes, the layout of pg_speed_plan_stats
PATH_STATS_DTYPE = np.dtype([(n, np.float64) for n, _ in _lib.pg_path_stats._fields_])      # 48 bytes, the layout of pg_path_stats
OFFSET_STATS_DTYPE = np.dtype([(n, np.float64 if c is C.c_double else np.int32) for n, c in _lib.pg_offset_stats._fields_])      # 64 bytes, the layout of pg_offset_stats
SMOOTH_STATS_DTYPE = np.dtype([(n, np.float64) for n, _ in _lib.pg_smooth_stats._fields_])      # 72 bytes, the layout of pg_smooth_stats
TUNE_STATS_DTYPE = np.dtype([(n, np.float64) for n, _ in _lib.pg_tune_stats._fields_])      # 72 bytes, the layout of pg_tune_stats
LINE_STATS_DTYPE = np.dtype([(n, np.float64) for n, _ in _lib.pg_line_stats._fields_])      # 96 bytes, the layout of pg_line_stats
REFINE_STATS_DTYPE = np.dtype([(n, np.float64 if c is C.c_double else np.int32) for n, c in _lib.pg_refine_stats._fields_])      # 64 bytes, the layout of pg_refine_stats
CLIP_STATS_DTYPE = np.dtype([("width_min", np.float64), ("u_width_min", np.float64), ("reserved_d", np.float64, (2,))] + [(n, np.int32) for n in ("n_clip_L", "n_clip_R", "n_blocked", "n_centre_out", "n_seen", "n_ignored")] + [("reserved", np.int32, (2,))])      # 64 bytes, the layout of pg_clip_stats
OBSTACLE_REPORT_DTYPE = np.dtype([(n, np.float64 if c is C.c_double else np.int32) for n, c in _lib.pg_obstacle_report._fields_])      # 64 bytes, the layout of pg_obstacle_report
FIT_STATS_DTYPE = np.dtype([(n, np.float64) for n, _ in _lib.pg_fit_stats._fields_])      # 80 bytes, the layout of pg_fit_stats


def is_solved(status):
    """True where the solver returned an answer that met its tolerances: PG_SOLVED (with the polish on: a VERIFIED KKT point) or PG_SOLVED_UNVERIFIED (the
    interior-point iterate no active-set round could verify; include/pigeon_mpc.h)."""
    status = np.asarray(status)
    return (status == SOLVED) | (status == SOLVED_UNVERIFIED)


def _p(a, ctype=c_dp):
    return None if a is None else a.ctypes.data_as(ctype)


def _f64(x, shape=None):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


class BatchedTrajectoryTrackingMPC:
    """B copies of CoupledTrajectoryTrackingMPC(vehicle, trajectory; ...) (coupled_lat_long.jl:42-60) on one MI355X."""

    def __init__(self, trajectory, batch_capacity, vehicle=None, control_params=None, N_short=10, N_long=20, dt_short=0.01, dt_long=0.2,
                 use_correction_step=True, rk4_substeps=10, device=0, ipm_max_iter=40, ipm_tol=None, ipm_mu0=100.0, hji_eps=0.05, formulation="coupled",
                 precision="f64", walls=False, wall_weight=1000.0, polish=None, polish_rho=None, polish_tol=None, polish_ipm_tol=None, warm_polish=None, cold_guess=None,
                 options=None, phase_timing=True, allow_f32_long_lateral=False):
        """options: {name: value} of build-defined options applied right after pg_create (pg_set_option, include/pigeon_mpc.h); precision "f64-diag" loads the
        diagnostic build of the fp64 library (tests / tools only).  phase_timing: this mirror is the test / bench harness and switches the library's per-phase HIP events ON
        by default (phase_ms(); the library's own default is off -- 2-4 % of a step: bench.py times its loops with phase_timing=False)."""
        self.precision = precision
        self.real = np.float32 if precision == "f32" else np.float64      # element type of DEVICE arrays handed to the *_dev entry points
        self.lib = _lib.load_library(precision)
        cfg = _lib.pg_config()
        assert formulation in ("coupled", "decoupled")
        self.formulation = formulation
        (self.lib.pg_default_config if formulation == "coupled" else self.lib.pg_default_config_decoupled)(C.byref(cfg))
        # solver tolerances default to the library's own (they depend on its arithmetic type: pg_default_config*)
        ipm_tol = cfg.ipm_tol if ipm_tol is None else ipm_tol
        if polish is not None:                    # None: the library's default (on for both formulations)
            cfg.polish = int(bool(polish))
        if polish_rho is not None:
            cfg.polish_rho = float(polish_rho)
        if polish_tol is not None:
            cfg.polish_tol = float(polish_tol)
        if polish_ipm_tol is not None:
            cfg.polish_ipm_tol = float(polish_ipm_tol)
        if warm_polish is not None:
            cfg.warm_polish = int(bool(warm_polish))
        if cold_guess is not None:
            cfg.cold_guess = int(cold_guess)
        self.vehicle = X1() if vehicle is None else dict(vehicle)
        default_cp = CoupledControlParams() if formulation == "coupled" else DecoupledControlParams()
        self.control_params = default_cp if control_params is None else dict(control_params)
        for name, _ in _lib.pg_vehicle._fields_:
            setattr(cfg.vehicle, name, float(self.vehicle[name]))
        for name, _ in _lib.pg_control_params._fields_:
            if name == "_pad" or name not in self.control_params:      # the lateral formulation has no Q_ds / R_Fx / R_dFx / W_HJI / N_HJI
                continue
            setattr(cfg.control, name, int(self.control_params[name]) if name == "N_HJI" else float(self.control_params[name]))
        cfg.N_short, cfg.N_long, cfg.dt_short, cfg.dt_long = N_short, N_long, dt_short, dt_long
        cfg.use_correction_step, cfg.rk4_substeps, cfg.batch_capacity, cfg.device = int(use_correction_step), rk4_substeps, batch_capacity, device
        cfg.ipm_max_iter, cfg.ipm_tol, cfg.ipm_mu0, cfg.hji_eps = ipm_max_iter, ipm_tol, ipm_mu0, hji_eps
        cfg.walls = int(bool(walls))          # build-defined extension: soft rows edge_R - sw <= e <= edge_L + sw (decoupled formulation)
        cfg.wall_weight = float(wall_weight)
        cfg.allow_f32_long_lateral = int(bool(allow_f32_long_lateral))      # (the fp32 library refuses the decoupled formulation beyond 32 intervals without it: pigeon_mpc.h)
        self.wall_weight = float(wall_weight)
        self.walls = bool(walls)
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = self.lib.pg_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise _lib.PigeonError(f"pg_create failed with status {rc}: {self.lib.pg_last_error(None).decode()}")
        self.N_short, self.N_long = N_short, N_long
        self.N = N_short + N_long
        self.NN = self.N + 1
        self.capacity = batch_capacity
        self.B = 0
        un = np.zeros(2)
        self._chk(self.lib.pg_get_u_normalization(self.h, _p(un)), "pg_get_u_normalization")
        self.u_normalization = un
        self.qp_len = self.lib.pg_qp_len(self.h)
        self.trajectory = None
        try:
            self.set_option("phase_timing", 1 if phase_timing else 0)
        except _lib.PigeonError:          # (an older build selected through PIGEON_HIP_LIB for an A/B run: its events are always on)
            pass
        for name, value in (options or {}).items():
            self.set_option(name, value)
        if trajectory is not None:
            self.set_trajectory(trajectory)

    def _chk(self, rc, what):
        _lib.check(self.lib, self.h, rc, what)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.pg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- mpc.trajectory = ... (ros_integration.jl:53) ----
    def set_trajectory(self, traj):
        """One TrajectoryTube for the whole batch, or a list of tubes (a library; select per instance with set_trajectory_index)."""
        if isinstance(traj, (list, tuple)):
            return self.set_trajectories(traj)
        self.trajectory = traj
        self.trajectories = [traj]
        cols = [np.ascontiguousarray(traj.data[i]) for i in range(12)]
        self._chk(self.lib.pg_set_trajectory(self.h, len(traj), *[_p(c) for c in cols]), "pg_set_trajectory")

    # ---- one controller per (x0, reference trajectory) pair: the batch carries a library of tubes and a per-instance selection ----
    _CH_ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]                       # t, s, V, A, E, N, psi, kappa, edge_L, edge_R of the 12-channel tube

    def set_trajectories(self, trajs, index=None):
        trajs = list(trajs)
        Lmax = max(len(t) for t in trajs)
        L = np.array([len(t) for t in trajs], dtype=np.int32)
        pack = np.zeros((len(trajs), 10, Lmax))
        for k, t in enumerate(trajs):
            pack[k, :, :len(t)] = t.data[self._CH_ROWS]
            pack[k, :, len(t):] = t.data[self._CH_ROWS][:, -1:]     # padding is never read (L[k] bounds every search)
        self._chk(self.lib.pg_set_trajectories(self.h, len(trajs), Lmax, _p(L, C.POINTER(C.c_int32)), _p(pack)), "pg_set_trajectories")
        self.trajectories = trajs
        self.trajectory = trajs[0]
        if index is not None:
            self.set_trajectory_index(index)

    def set_trajectory_index(self, index):
        self.trajectory_index = self._set_index("trajectory", index)

    # ---- making the speed profile (pg_plan_speeds): every (path, plan set) tube of a path library x a library of plan sets, computed on the device ----
    @classmethod
    def pack_speed_plans(cls, sets):
        """dicts (vehicles.speed_plan(**overrides); missing fields: the defaults) or pg_speed_plan structures -> a ctypes array of pg_speed_plan.  Raises ValueError for
        a set outside the ranges of include/pigeon_mpc.h (the library refuses the same sets with PG_ERR_INVALID)."""
        def fill(rec, p):
            full = _default_speed_plan(**p)
            for name, _ in _lib.pg_speed_plan._fields_:
                setattr(rec, name, float(full[name]))
        arr = cls._pack(_lib.pg_speed_plan, [sets] if isinstance(sets, (dict, _lib.pg_speed_plan)) else sets, fill)
        if len(arr) < 1:
            raise ValueError("plan_speeds: at least one plan set")
        for k, r in enumerate(arr):
            ok = (math.isfinite(r.mu_scale) and r.mu_scale > 0 and math.isfinite(r.V_max) and r.V_max > 0 and 0 < r.V_floor <= r.V_max
                  and all(math.isnan(v) or (math.isfinite(v) and v >= 0) for v in (r.V_start, r.V_end)) and r.ax_min <= 0 <= r.ax_max and r.ay_max > 0)
            if not ok:
                raise ValueError(f"plan_speeds: set {k} is outside the ranges of pg_speed_plan (mu_scale, V_max > 0 and finite; 0 < V_floor <= V_max; V_start / V_end NaN or "
                                 "finite and >= 0; ax_min <= 0 <= ax_max; ay_max > 0)")
        return arr

    @classmethod
    def pack_paths(cls, paths, closed=None):
        """TrajectoryTubes (a list, or one) or the channel array [n_path][10][Lmax] with every knot valid -> (L int32 [n_path], channels float64 [n_path][10][Lmax],
        closed int32 [n_path]).  closed: None (all open), one flag for every path, or one per path.  Raises ValueError for what the library refuses on the path side:
        fewer than 2 knots (3 on a closed path), s that does not increase strictly, a non-finite geometry value."""
        if isinstance(paths, np.ndarray):
            ch = _f64(paths)
            if ch.ndim != 3 or ch.shape[1] != 10:
                raise ValueError("plan_speeds: the channel array is [n_path][10][Lmax]")
            L = np.full(ch.shape[0], ch.shape[2], dtype=np.int32)
        else:
            paths = [paths] if isinstance(paths, TrajectoryTube) else list(paths)
            if not paths:
                raise ValueError("plan_speeds: at least one path")
            L = np.array([len(t) for t in paths], dtype=np.int32)
            ch = np.zeros((len(paths), 10, int(L.max())))
            for k, t in enumerate(paths):
                ch[k, :, :len(t)] = t.data[cls._CH_ROWS]
        cl = np.zeros(len(L), dtype=np.int32)
        if closed is not None:
            c = np.atleast_1d(np.asarray(closed)).astype(bool)
            if c.shape not in ((1,), (len(L),)):
                raise ValueError(f"plan_speeds: closed has {c.size} entries for {len(L)} paths")
            cl[:] = c
        for k in range(len(L)):
            n = int(L[k])
            if n < 2 or (cl[k] and n < 3):
                raise ValueError(f"plan_speeds: path {k} has {n} knots (an open path needs 2, a closed one 3)")
            geo = ch[k][[1, 4, 5, 6, 7, 8, 9], :n]
            if not np.isfinite(geo).all():
                raise ValueError(f"plan_speeds: path {k} has a non-finite geometry value")
            if not (np.diff(ch[k, 1, :n]) > 0).all():
                raise ValueError(f"plan_speeds: s of path {k} does not increase strictly")
        return L, ch, cl

    @classmethod
    def tubes_from_channels(cls, channels, L, n_sets=1):
        """channels [n_path * n_sets][10][Lmax] as pg_plan_speeds returns them, L [n_path] -> the TrajectoryTubes in the order k = path * n_sets + set (theta, phi zero,
        as TrajectoryTube.from_path)."""
        out = []
        for k in range(channels.shape[0]):
            n = int(L[k // n_sets]); c = channels[k, :, :n]
            out.append(TrajectoryTube(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], np.zeros(n), np.zeros(n), c[8], c[9]))
        return out

    def _made_tubes(self, channels, L, n_sets, install):
        """the tubes a maker returns; with install they are the handle's library from here on, as the library already holds them"""
        tubes = self.tubes_from_channels(channels, L, n_sets)
        if install:
            self.trajectories = tubes
            self.trajectory = tubes[0]
        return tubes

    def plan_speeds(self, paths, sets, vehicles=None, closed=None, install=False):
        """Friction-limited speed profiles on the device (pg_plan_speeds; the scheme is stated in include/pigeon_mpc.h): paths = TrajectoryTubes or the channel array
        (their t, V, A are ignored), sets = vehicles.speed_plan(**overrides) dicts, vehicles = None (the handle's) or one vehicle per set, closed = None / one flag /
        one per path.  Returns (tubes, stats): the n_path * n_sets TrajectoryTubes in the order k = path * n_sets + set, and a structured array with the fields of
        pg_speed_plan_stats.  install=True makes them the handle's trajectory library (as set_trajectories(tubes) would, without the host round trip; select with
        set_trajectory_index)."""
        L, ch, cl = self.pack_paths(paths, closed)
        arr = self.pack_speed_plans(sets)
        veh = None
        if vehicles is not None:
            veh = self.pack_vehicles([vehicles] if isinstance(vehicles, (dict, _lib.pg_vehicle)) else vehicles)
            if len(veh) != len(arr):
                raise ValueError(f"plan_speeds: {len(veh)} vehicles for {len(arr)} sets")
        n_traj = len(L) * len(arr)
        out = np.zeros((n_traj, 10, ch.shape[2]))
        st = (_lib.pg_speed_plan_stats * n_traj)()
        self._chk(self.lib.pg_plan_speeds(self.h, len(L), ch.shape[2], _p(L, c_i32p), _p(cl, c_i32p), _p(ch), len(arr), arr, veh, int(bool(install)), _p(out), st),
                  "pg_plan_speeds")
        return self._made_tubes(out, L, len(arr), install), np.frombuffer(st, dtype=SPEED_PLAN_STATS_DTYPE).copy()

    # ---- making the path (pg_make_paths): a library of paths from line, arc and clothoid segments, computed on the device ----
    @classmethod
    def pack_path_specs(cls, paths, n_knots, V_ref=6.0, pose=(0.0, 0.0, 0.0), closed=False):
        """paths: a list of segment lists (vehicles.path_segment(**overrides) dicts, as the builders of vehicles.py return them; or pg_path_segment structures); n_knots,
        V_ref, closed: one value for every path or one per path; pose: one (E0, N0, psi0) or one per path -> (specs, segments): ctypes arrays of pg_path_spec [n_path] and
        pg_path_segment [all segments, path after path].  Raises ValueError for what the library refuses with PG_ERR_INVALID (include/pigeon_mpc.h)."""
        paths = [list(p) for p in paths]
        if not paths:
            raise ValueError("make_paths: at least one path")
        n = len(paths)

        def per_path(x, what, width=None):
            a = np.asarray(x, dtype=np.float64)
            if a.shape == (() if width is None else (width,)):
                a = np.broadcast_to(a, (n,) + a.shape)
            if a.shape != ((n,) if width is None else (n, width)):
                raise ValueError(f"make_paths: {what} is one value for every path or one per path ({n} paths)")
            return a

        knots, V, cl, poses = per_path(n_knots, "n_knots"), per_path(V_ref, "V_ref"), per_path(closed, "closed"), per_path(pose, "pose", 3)

        def fill(rec, g):
            full = _default_path_segment(**g)
            for name, _ in _lib.pg_path_segment._fields_:
                setattr(rec, name, float(full[name]))
        for k, p in enumerate(paths):
            if not p:
                raise ValueError(f"make_paths: path {k} has no segment")
        segs = cls._pack(_lib.pg_path_segment, [g for p in paths for g in p], fill)
        for j, g in enumerate(segs):
            if not (math.isfinite(g.length) and g.length > 0):
                raise ValueError(f"make_paths: segment {j} needs a finite length > 0")
            if not all(math.isfinite(v) for v in (g.kappa0, g.kappa1, g.edge_L0, g.edge_L1, g.edge_R0, g.edge_R1)):
                raise ValueError(f"make_paths: segment {j} has a non-finite curvature or edge")
            if not (g.edge_L0 > g.edge_R0 and g.edge_L1 > g.edge_R1):
                raise ValueError(f"make_paths: segment {j} needs edge_L > edge_R at both ends")
            if g.reserved != 0:
                raise ValueError(f"make_paths: reserved of segment {j} must be 0")
        specs = (_lib.pg_path_spec * n)()
        at = 0
        for k, p in enumerate(paths):
            if not np.isfinite(poses[k]).all():
                raise ValueError(f"make_paths: the pose of path {k} is not finite")
            if not (math.isfinite(V[k]) and V[k] > 0):
                raise ValueError(f"make_paths: path {k} needs a finite V_ref > 0")
            if not (knots[k] == int(knots[k]) and 2 <= knots[k] <= 2**31 - 1):
                raise ValueError(f"make_paths: path {k} needs an integer n_knots >= 2")
            if cl[k] and knots[k] < 3:
                raise ValueError(f"make_paths: path {k} is closed and has {int(knots[k])} knots (a closed path needs 3)")
            s = specs[k]
            s.E0, s.N0, s.psi0, s.V_ref = (float(x) for x in (*poses[k], V[k]))
            s.seg0, s.n_seg, s.n_knots, s.closed = at, len(p), int(knots[k]), int(bool(cl[k]))
            at += len(p)
        return specs, segs

    def make_paths(self, paths, ds=None, n_knots=None, V_ref=6.0, pose=(0.0, 0.0, 0.0), closed=False, install=False):
        """A path library on the device (pg_make_paths; the scheme is stated in include/pigeon_mpc.h): paths = a list of segment lists (vehicles.line_segments,
        circle_segments, oval_segments, lane_change_segments, or path_segment dicts of your own).  Give the knots as n_knots (one value or one per path) or as a spacing
        ds (n_knots = max(2, ceil(total / ds) + 1) per path).  V_ref fills the constant-speed profile (V = V_ref, A = 0, t = s / V_ref), pose = (E0, N0, psi0) of knot 0,
        closed = the caller's statement for plan_speeds (each one value or one per path).  Returns (tubes, stats): the TrajectoryTubes and a structured array with the
        fields of pg_path_stats (length, turn, closure_pos, closure_psi, kappa_abs_max, ds).  install=True makes them the handle's trajectory library (as
        set_trajectories(tubes) would, without the host round trip; select with set_trajectory_index)."""
        paths = [list(p) for p in paths]
        if (ds is None) == (n_knots is None):
            raise ValueError("make_paths: give ds or n_knots (one of them)")
        if n_knots is None:
            if not (np.all(np.isfinite(ds)) and np.all(np.asarray(ds) > 0)):
                raise ValueError("make_paths: ds must be finite and > 0")
            dss = np.broadcast_to(np.asarray(ds, dtype=np.float64), (len(paths),))
            totals = [sum(float(g["length"] if isinstance(g, dict) else g.length) for g in p) for p in paths]
            if not np.all(np.isfinite(totals)):
                raise ValueError("make_paths: a segment's length is not finite")
            n_knots = [max(2, math.ceil(t / d) + 1) for t, d in zip(totals, dss)]
        specs, segs = self.pack_path_specs(paths, n_knots, V_ref=V_ref, pose=pose, closed=closed)
        n = len(specs)
        Lmax = max(s.n_knots for s in specs)
        out = np.zeros((n, 10, Lmax))
        L = np.zeros(n, dtype=np.int32)
        st = (_lib.pg_path_stats * n)()
        self._chk(self.lib.pg_make_paths(self.h, n, specs, len(segs), segs, Lmax, int(bool(install)), _p(L, c_i32p), None, _p(out), st), "pg_make_paths")
        return self._made_tubes(out, L, 1, install), np.frombuffer(st, dtype=PATH_STATS_DTYPE).copy()

    # ---- fitting the path (pg_fit_paths): a library of paths through waypoints, cubic splines resampled in arc length on the device ----
    @classmethod
    def pack_fit_specs(cls, paths, Lmax=None, precision="f64"):
        """paths: a list of dict(waypoints=[vehicles.waypoint(**overrides) dicts or pg_waypoint structures], n_knots=.., V_ref=6.0, closed=False) -> (specs, waypoints,
        Lmax): ctypes arrays of pg_fit_spec [n_path] and pg_waypoint [all waypoints, path after path], and Lmax (None: the largest n_knots).  Raises ValueError for what the
        library refuses with PG_ERR_INVALID (include/pigeon_mpc.h); precision names the library's element type for the "dense" refusal."""
        paths = list(paths)
        if not paths:
            raise ValueError("fit_paths: at least one path")

        def fill(rec, w):
            full = _default_waypoint(**w)
            for name, _ in _lib.pg_waypoint._fields_:
                setattr(rec, name, float(full[name]))
        lists = []
        for k, p in enumerate(paths):
            unknown = set(p) - {"waypoints", "n_knots", "V_ref", "closed"}
            if unknown or "waypoints" not in p or "n_knots" not in p:
                raise ValueError(f"fit_paths: path {k} is dict(waypoints=, n_knots=, V_ref=6.0, closed=False); got {sorted(p)}")
            lists.append(list(p["waypoints"]))
        wps = cls._pack(_lib.pg_waypoint, [w for l in lists for w in l], fill)
        specs = (_lib.pg_fit_spec * len(paths))()
        eps = 2.0 ** -23 if precision == "f32" else 2.0 ** -52
        at = 0
        for k, (p, l) in enumerate(zip(paths, lists)):
            n_knots, V, cl, n = p["n_knots"], float(p.get("V_ref", 6.0)), bool(p.get("closed", False)), len(l)
            if not (n_knots == int(n_knots) and 2 <= n_knots <= 2**31 - 1):
                raise ValueError(f"fit_paths: path {k} needs an integer n_knots >= 2")
            if n < (3 if cl else 2) or (cl and n_knots < 3):
                raise ValueError(f"fit_paths: path {k} has {n} waypoints and {int(n_knots)} knots (an open path needs 2 waypoints, a closed one 3 waypoints and 3 knots)")
            if not (math.isfinite(V) and V > 0):
                raise ValueError(f"fit_paths: path {k} needs a finite V_ref > 0")
            C_sum = 0.0
            for i in range(n):
                w = wps[at + i]
                if not all(math.isfinite(v) for v in (w.E, w.N, w.edge_L, w.edge_R)):
                    raise ValueError(f"fit_paths: waypoint {i} of path {k} has a non-finite field")
                if not w.edge_L > w.edge_R:
                    raise ValueError(f"fit_paths: waypoint {i} of path {k} needs edge_L > edge_R")
            for j in range(n if cl else n - 1):
                a, b = wps[at + j], wps[at + (j + 1) % n]
                dE = b.E - a.E; dN = b.N - a.N
                h = math.sqrt(dE * dE + dN * dN)
                if not (math.isfinite(h) and h > 0):
                    raise ValueError(f"fit_paths: waypoints {j} and {(j + 1) % n} of path {k} lie at the same point (a chord must be finite and > 0)")
                C_sum += h
            per = float(int(n_knots) - 1)
            if not (per <= 1.0 / (4.0 * eps) and C_sum / per >= 2.0 ** -100 and C_sum <= 2.0 ** 100):
                raise ValueError(f"fit_paths: the knots of path {k} are so dense that s cannot be shown to increase strictly in the library's element type")
            s = specs[k]
            s.V_ref, s.wp0, s.n_wp, s.n_knots, s.closed = V, at, n, int(n_knots), int(cl)
            at += n
        most = max(s.n_knots for s in specs)
        if Lmax is None:
            Lmax = most
        if not (Lmax == int(Lmax) and max(2, most) <= Lmax <= 2**31 - 1):
            raise ValueError(f"fit_paths: Lmax is an integer >= the largest n_knots ({most})")
        if len(paths) * 10.0 * Lmax * 8.0 >= 2.0 ** 62:
            raise ValueError("fit_paths: n_path * 10 * Lmax elements are more than the allocation arithmetic holds")
        return specs, wps, int(Lmax)

    def fit_paths(self, paths, Lmax=None, install=False):
        """A path library through waypoints on the device (pg_fit_paths; the scheme is stated in include/pigeon_mpc.h): paths = a list of dict(waypoints=[vehicles.waypoint
        dicts, e.g. vehicles.waypoints_from_tube(tube, every=4, closed=True)], n_knots=.., V_ref=6.0, closed=False).  An interpolating cubic spline over the chord length,
        natural (open) or periodic (closed: do not repeat the first point), resampled at n_knots knots equally spaced in arc length; V = V_ref, A = 0, t = s / V_ref.
        Returns (tubes, closed, stats): the TrajectoryTubes, the int32 flags plan_speeds takes as closed=, and a structured array with the fields of pg_fit_stats (length,
        turn, closure_pos, closure_psi, kappa_abs_max, ds, chord_min, chord_max, s_err_max).  install=True makes the tubes the handle's trajectory library (as
        set_trajectories(tubes) would, without the host round trip; select with set_trajectory_index)."""
        specs, wps, Lmax = self.pack_fit_specs(paths, Lmax, "f32" if self.precision == "f32" else "f64")
        n = len(specs)
        out = np.zeros((n, 10, Lmax))
        L = np.zeros(n, dtype=np.int32); cl = np.zeros(n, dtype=np.int32)
        st = (_lib.pg_fit_stats * n)()
        self._chk(self.lib.pg_fit_paths(self.h, n, specs, len(wps), wps, Lmax, int(bool(install)), _p(L, c_i32p), _p(cl, c_i32p), _p(out), st), "pg_fit_paths")
        return self._made_tubes(out, L, 1, install), cl, np.frombuffer(st, dtype=FIT_STATS_DTYPE).copy()

    # ---- offsetting the path (pg_offset_paths): every (path, offset set) pair of a path library x a library of offset sets, computed on the device ----
    @classmethod
    def pack_offsets(cls, sets):
        """dicts (vehicles.offset / lane / lane_change / pass_by; missing fields: the defaults) or pg_offset_set structures -> a ctypes array of pg_offset_set.  Raises
        ValueError for a set outside the ranges of include/pigeon_mpc.h (the library refuses the same sets with PG_ERR_INVALID)."""
        def fill(rec, p):
            full = _default_offset(**p)
            for name, ctype in _lib.pg_offset_set._fields_:
                setattr(rec, name, int(full[name]) if ctype is C.c_int32 else float(full[name]))
        arr = cls._pack(_lib.pg_offset_set, [sets] if isinstance(sets, (dict, _lib.pg_offset_set)) else sets, fill)
        if len(arr) < 1:
            raise ValueError("offset_paths: at least one offset set")
        for k, r in enumerate(arr):
            rise, fall = math.isfinite(r.s_a), math.isfinite(r.s_c)
            if not (math.isfinite(r.d0) and math.isfinite(r.d1)):
                raise ValueError(f"offset_paths: d0 or d1 of set {k} is not finite")
            if not ((rise or r.s_a == math.inf) and (fall or r.s_c == math.inf)):
                raise ValueError(f"offset_paths: s_a and s_c of set {k} are finite or +Inf")
            if (rise and not (math.isfinite(r.s_b) and r.s_b > r.s_a)) or (fall and not (math.isfinite(r.s_d) and r.s_d > r.s_c)) or math.isnan(r.s_b) or math.isnan(r.s_d):
                raise ValueError(f"offset_paths: a window of set {k} needs a finite end beyond its start (s_b > s_a, s_d > s_c)")
            if fall and not rise:
                raise ValueError(f"offset_paths: set {k} has a fall without a rise")
            if rise and fall and r.s_c < r.s_b:
                raise ValueError(f"offset_paths: set {k} needs s_c >= s_b (the fall starts after the rise has ended)")
            if not 0.0 < r.x_min <= 1.0:
                raise ValueError(f"offset_paths: set {k} needs x_min in (0, 1]")
            if r.edge_mode not in (0, 1):
                raise ValueError(f"offset_paths: edge_mode of set {k} is 0 or 1")
            if r.reserved != 0:
                raise ValueError(f"offset_paths: reserved of set {k} must be 0")
        return arr

    def offset_paths(self, paths, sets, closed=None, install=False):
        """Lanes, lane changes and pass-bys of a path library on the device (pg_offset_paths; the scheme is stated in include/pigeon_mpc.h): paths = TrajectoryTubes or the
        channel array, sets = vehicles.lane(3.5) / lane_change(0, 3.5, 40, 70) / pass_by(3.0, 120, 135, 145, 160) / offset(**overrides) dicts, closed = None / one flag /
        one per path.  Output knot i belongs to source knot i; V is copied and t, A follow the new arc length -- hand the result to plan_speeds (closed=np.repeat(closed,
        len(sets))) for a friction-limited profile on the new curvature.  Returns (tubes, stats): the n_path * n_sets TrajectoryTubes in the order k = path * n_sets + set,
        and a structured array with the fields of pg_offset_stats.  install=True makes them the handle's trajectory library (as set_trajectories(tubes) would, without the
        host round trip; select with set_trajectory_index, switch with route events)."""
        L, ch, cl = self.pack_paths(paths, closed)
        arr = self.pack_offsets(sets)
        n_traj = len(L) * len(arr)
        out = np.zeros((n_traj, 10, ch.shape[2]))
        st = (_lib.pg_offset_stats * n_traj)()
        self._chk(self.lib.pg_offset_paths(self.h, len(L), ch.shape[2], _p(L, c_i32p), _p(cl, c_i32p), _p(ch), len(arr), arr, int(bool(install)), None, None, _p(out), st),
                  "pg_offset_paths")
        return self._made_tubes(out, L, len(arr), install), np.frombuffer(st, dtype=OFFSET_STATS_DTYPE).copy()

    # ---- clipping the tube (pg_clip_tubes): every (path, obstacle set) pair of a path library x a library of obstacle sets, computed on the device ----
    @classmethod
    def pack_obstacle_sets(cls, sets):
        """vehicles.obstacle_set(...) dicts (one, or a list) -> (a ctypes array of pg_obstacle_set, a ctypes array of pg_obstacle): the obstacles of the sets one after the
        other in one array, `first` / `count` of each set pointing into it.  Raises ValueError for a set outside the ranges of include/pigeon_mpc.h (the library refuses the
        same sets with PG_ERR_INVALID)."""
        sets = [sets] if isinstance(sets, dict) else list(sets)
        if len(sets) < 1:
            raise ValueError("clip_tubes: at least one obstacle set")
        n_obs = sum(len(s["obstacles"]) for s in sets)
        arr = (_lib.pg_obstacle_set * len(sets))()
        obs = (_lib.pg_obstacle * max(n_obs, 1))()
        at = 0
        for k, s in enumerate(sets):
            extra = set(s) - {"obstacles", "margin", "taper", "min_width", "policy"}
            if extra:
                raise ValueError(f"clip_tubes: set {k} has fields an obstacle set does not have: {sorted(extra)}")
            full = _default_obstacle_set(**s)
            margin, taper, min_width, policy = full["margin"], full["taper"], full["min_width"], full["policy"]
            if len(full["obstacles"]) > 64:
                raise ValueError(f"clip_tubes: set {k} has {len(full['obstacles'])} obstacles (at most 64)")
            if not (math.isfinite(margin) and margin >= 0.0):
                raise ValueError(f"clip_tubes: margin of set {k} is not finite and >= 0")
            if not taper > 0.0:
                raise ValueError(f"clip_tubes: taper of set {k} is not > 0 (+Inf: no taper)")
            if not (math.isfinite(min_width) and min_width >= 0.0):
                raise ValueError(f"clip_tubes: min_width of set {k} is not finite and >= 0")
            if policy not in (0, 1, 2, 3):
                raise ValueError(f"clip_tubes: policy of set {k} is outside 0 .. 3")
            arr[k].first, arr[k].count, arr[k].margin, arr[k].taper, arr[k].min_width, arr[k].policy = at, len(full["obstacles"]), margin, taper, min_width, policy
            for o in full["obstacles"]:
                E, N, radius, reserved = float(o["E"]), float(o["N"]), float(o["radius"]), float(o.get("reserved", 0.0))
                if not (math.isfinite(E) and math.isfinite(N) and math.isfinite(radius)):
                    raise ValueError(f"clip_tubes: E, N or radius of an obstacle of set {k} is not finite")
                if radius < 0.0 or not radius + margin > 0.0:
                    raise ValueError(f"clip_tubes: an obstacle of set {k} needs radius >= 0 and radius + margin > 0")
                if reserved != 0.0:
                    raise ValueError(f"clip_tubes: reserved of an obstacle of set {k} must be 0")
                obs[at].E, obs[at].N, obs[at].radius = E, N, radius
                at += 1
        return arr, obs, n_obs

    def clip_tubes(self, paths, sets, closed=None, install=False):
        """The tubes of a path library narrowed around obstacle sets, on the device (pg_clip_tubes; the scheme is stated in include/pigeon_mpc.h): paths = TrajectoryTubes or
        the channel array, sets = vehicles.obstacle_set([vehicles.obstacle(E, N, radius) or vehicles.obstacle_at(path, u, e, radius), ...], margin=, taper=, min_width=,
        policy=) dicts, closed = None / one flag / one per path.  Only edge_L and edge_R change; whatever reads them (walls, first_exit, make_starts' e_frac, offset_paths'
        n_outside) then sees the obstacles.  Returns (tubes, stats, reports): the n_path * n_sets TrajectoryTubes in the order k = path * n_sets + set, a structured array
        with the fields of pg_clip_stats, and a structured array [n_path * n_sets][max_count] with the fields of pg_obstacle_report (slot j: obstacle j of the pair's set;
        vehicles.pass_by_around turns a record into the pass-by that goes round it).  install=True makes the tubes the handle's trajectory library (as set_trajectories(tubes)
        would, without the host round trip)."""
        L, ch, cl = self.pack_paths(paths, closed)
        arr, obs, n_obs = self.pack_obstacle_sets(sets)
        n_traj = len(L) * len(arr)
        max_count = max(s.count for s in arr)
        out = np.zeros((n_traj, 10, ch.shape[2]))
        st = (_lib.pg_clip_stats * n_traj)()
        rp = (_lib.pg_obstacle_report * max(n_traj * max_count, 1))()
        self._chk(self.lib.pg_clip_tubes(self.h, len(L), ch.shape[2], _p(L, c_i32p), _p(cl, c_i32p), _p(ch), len(arr), arr, n_obs, obs, int(bool(install)), None, None, _p(out),
                                         st, rp), "pg_clip_tubes")
        reports = np.frombuffer(rp, dtype=OBSTACLE_REPORT_DTYPE)[:n_traj * max_count].reshape(n_traj, max_count).copy()
        return self._made_tubes(out, L, len(arr), install), np.frombuffer(st, dtype=CLIP_STATS_DTYPE).copy(), reports

    # ---- refining the path (pg_refine_paths): every (path, refine set) pair of a path library x a library of refine sets, computed on the device ----
    @classmethod
    def pack_refines(cls, sets):
        """vehicles.refine(...) dicts (refine / refine_for / refine_around; one, or a list) or pg_refine_set structures -> a ctypes array of pg_refine_set.  Raises
        ValueError for a set outside the ranges of include/pigeon_mpc.h (the library refuses the same sets with PG_ERR_INVALID)."""
        def fill(rec, p):
            extra = set(p) - {"ds", "windows"}
            if extra:
                raise ValueError(f"refine_paths: a set has fields a refine set does not have: {sorted(extra)}")
            full = _default_refine(**p)
            rec.ds = full["ds"]
            for j in range(4):
                rec.s_lo[j], rec.s_hi[j], rec.ds_w[j] = full["windows"][j] if j < len(full["windows"]) else (math.inf, math.inf, math.inf)
        arr = cls._pack(_lib.pg_refine_set, [sets] if isinstance(sets, (dict, _lib.pg_refine_set)) else sets, fill)
        if len(arr) < 1:
            raise ValueError("refine_paths: at least one refine set")
        for k, r in enumerate(arr):
            if not (r.ds == math.inf or (math.isfinite(r.ds) and r.ds > 0.0)):
                raise ValueError(f"refine_paths: ds of set {k} is +Inf or finite and > 0")
            for j in range(4):
                used = math.isfinite(r.s_lo[j])
                if not (used or r.s_lo[j] == math.inf):
                    raise ValueError(f"refine_paths: s_lo of window {j} of set {k} is finite or +Inf")
                if used and not (math.isfinite(r.s_hi[j]) and r.s_hi[j] > r.s_lo[j] and math.isfinite(r.ds_w[j]) and r.ds_w[j] > 0.0):
                    raise ValueError(f"refine_paths: window {j} of set {k} needs a finite s_hi > s_lo and a finite ds_w > 0")
                if not used and (math.isnan(r.s_hi[j]) or math.isnan(r.ds_w[j])):
                    raise ValueError(f"refine_paths: s_hi or ds_w of the unused window {j} of set {k} is NaN")
            if any(v != 0.0 for v in r.reserved):
                raise ValueError(f"refine_paths: reserved of set {k} must be 0")
        return arr

    @staticmethod
    def refined_lengths(L, ch, arr):
        """L_out [n_path * n_sets] of pg_refine_paths, on the host: 1 + the sum of vehicles.refine_parts over the intervals of every (path, set) pair.  Raises ValueError
        where the library refuses an interval of more than 4096 parts."""
        out = np.zeros(len(L) * len(arr), dtype=np.int32)
        for p in range(len(L)):
            s = [float(v) for v in ch[p, 1, :int(L[p])]]
            u = [v - s[0] for v in s]
            for j, r in enumerate(arr):
                rset = dict(ds=r.ds, windows=[(r.s_lo[q], r.s_hi[q], r.ds_w[q]) for q in range(4)])
                plain = rset["ds"] == math.inf and all(w[0] == math.inf for w in rset["windows"])
                count = 1
                for i in range(len(s) - 1):
                    m = 1 if plain else _refine_parts(rset, s[i + 1] - s[i], u[i], u[i + 1])
                    if m > REFINE_M_MAX:
                        raise ValueError(f"refine_paths: path {p}, set {j}, interval {i} would be cut into more than {REFINE_M_MAX} parts")
                    count += m
                if count > 2**31 - 1:
                    raise ValueError(f"refine_paths: path {p}, set {j} has {count} knots")
                out[p * len(arr) + j] = count
        return out

    def refine_paths(self, paths, sets, closed=None, Lmax_out=None, install=False):
        """Knots inserted into a path library where a manoeuvre or an obstacle needs them, on the device (pg_refine_paths; the scheme is stated in include/pigeon_mpc.h):
        paths = TrajectoryTubes or the channel array, sets = vehicles.refine(ds, windows) / refine_for(offset_set) / refine_around(report_row, source, ds_w, reach) dicts,
        closed = None / one flag / one per path.  Every source knot stays a knot with its own values and the arc length is the source's, so offset sets, obstacle reports
        and route events written against the source hold on the result.  Lmax_out: the knot capacity of the output (None: the largest L_out, computed on the host).
        Returns (tubes, stats): the n_path * n_sets TrajectoryTubes in the order k = path * n_sets + set, each with its own knot count, and a structured array with the
        fields of pg_refine_stats.  install=True makes them the handle's trajectory library (as set_trajectories(tubes) would, without the host round trip)."""
        L, ch, cl = self.pack_paths(paths, closed)
        arr = self.pack_refines(sets)
        n_traj = len(L) * len(arr)
        if Lmax_out is None:
            Lmax_out = int(self.refined_lengths(L, ch, arr).max())
        if not (Lmax_out == int(Lmax_out) and 2 <= Lmax_out <= 2**31 - 1):
            raise ValueError("refine_paths: Lmax_out is an integer >= 2")
        Lmax_out = int(Lmax_out)
        out = np.zeros((n_traj, 10, Lmax_out))
        Lo = np.zeros(n_traj, dtype=np.int32)
        st = (_lib.pg_refine_stats * n_traj)()
        self._chk(self.lib.pg_refine_paths(self.h, len(L), ch.shape[2], _p(L, c_i32p), _p(cl, c_i32p), _p(ch), len(arr), arr, Lmax_out, int(bool(install)), _p(Lo, c_i32p), None,
                                           _p(out), st), "pg_refine_paths")
        return self._made_tubes(out, Lo, 1, install), np.frombuffer(st, dtype=REFINE_STATS_DTYPE).copy()

    # ---- smoothing surveyed waypoints (pg_smooth_waypoints): every (path, smoothing set) pair of a waypoint library x a library of smoothing sets, on the device ----
    @classmethod
    def pack_smooths(cls, sets):
        """vehicles.smooth(...) dicts (one, or a list) or pg_smooth_set structures -> a ctypes array of pg_smooth_set.  Raises ValueError for a set outside the ranges of
        include/pigeon_mpc.h (the library refuses the same sets with PG_ERR_INVALID)."""
        def fill(rec, p):
            full = _default_smooth(**p)
            rec.lam, rec.pin_ends, rec.keep_walls, rec.n_win = full["lam"], int(full["pin_ends"]), int(full["keep_walls"]), len(full["windows"])
            for j in range(4):
                rec.u_lo[j], rec.u_hi[j], rec.factor[j] = full["windows"][j] if j < rec.n_win else (0.0, 0.0, 1.0)
        arr = cls._pack(_lib.pg_smooth_set, [sets] if isinstance(sets, (dict, _lib.pg_smooth_set)) else sets, fill)
        if len(arr) < 1:
            raise ValueError("smooth_waypoints: at least one smoothing set")
        for k, r in enumerate(arr):
            if not (math.isfinite(r.lam) and r.lam >= 0.0):
                raise ValueError(f"smooth_waypoints: lam of set {k} is finite and >= 0")
            if not 0 <= r.n_win <= 4:
                raise ValueError(f"smooth_waypoints: n_win of set {k} lies in [0, 4]")
            for j in range(r.n_win):
                if not r.u_lo[j] <= r.u_hi[j]:
                    raise ValueError(f"smooth_waypoints: window {j} of set {k} needs u_lo <= u_hi")
                if not (math.isfinite(r.factor[j]) and r.factor[j] >= 0.0):
                    raise ValueError(f"smooth_waypoints: factor of window {j} of set {k} is finite and >= 0")
            if r.reserved != 0:
                raise ValueError(f"smooth_waypoints: reserved of set {k} must be 0")
        return arr

    @staticmethod
    def smoothed_fit_paths(paths, smoothed, k):
        """The fit_paths list for "every path under set k": paths as smooth_waypoints took them (each needs n_knots), smoothed = its first return value."""
        return [dict(p, waypoints=smoothed[k][i]) for i, p in enumerate(paths)]

    def smooth_waypoints(self, paths, sets):
        """Surveyed waypoints smoothed on the device (pg_smooth_waypoints; the scheme is stated in include/pigeon_mpc.h): a cubic smoothing spline of E and N over the
        chord length for every (path, set) pair.  paths = a list of dict(waypoints=[vehicles.waypoint dicts], closed=False) -- the dicts fit_paths takes; n_knots and V_ref
        are not looked at --, sets = vehicles.smooth(lam=.., pin_ends=.., keep_walls=.., windows=[vehicles.smooth_window(..)]) dicts.  Returns (smoothed, stats):
        smoothed[k][i] is the waypoint list of path i under set k (smoothed_fit_paths(paths, smoothed, k) is the list fit_paths takes for set k), stats a structured
        array [n_path][n_sets] with the fields of pg_smooth_stats (dev_max, dev_rms, i_dev_max, bend, n_outside, width_min, pivot_min, chord_min)."""
        paths = [dict(p) for p in paths]
        for k, p in enumerate(paths):
            if len(p.get("waypoints", ())) < (5 if p.get("closed", False) else 2):
                raise ValueError(f"smooth_waypoints: path {k} needs 2 waypoints (a closed path 5)")
            p.setdefault("n_knots", 3)
        specs, wps, _ = self.pack_fit_specs(paths)
        arr = self.pack_smooths(sets)
        n, ns, nw = len(specs), len(arr), len(wps)
        out = (_lib.pg_waypoint * (ns * nw))()
        st = (_lib.pg_smooth_stats * (n * ns))()
        self._chk(self.lib.pg_smooth_waypoints(self.h, n, specs, nw, wps, ns, arr, out, st), "pg_smooth_waypoints")
        flat = np.frombuffer(out, dtype=np.float64).reshape(ns, nw, 4)
        smoothed = [[[dict(E=float(w[0]), N=float(w[1]), edge_L=float(w[2]), edge_R=float(w[3])) for w in flat[k, s.wp0:s.wp0 + s.n_wp]] for s in specs] for k in range(ns)]
        return smoothed, np.frombuffer(st, dtype=SMOOTH_STATS_DTYPE).copy().reshape(n, ns)

    # ---- choosing the smoothing weight (pg_tune_smoothing): every (path, tune set) pair smoothed to a target rms, the weight searched on the device ----
    @classmethod
    def pack_tunes(cls, sets):
        """vehicles.tune(...) dicts (one, or a list) or pg_tune_set structures -> a ctypes array of pg_tune_set.  Raises ValueError for a set outside the ranges of
        include/pigeon_mpc.h (the library refuses the same sets with PG_ERR_INVALID)."""
        def fill(rec, p):
            unknown = set(p) - {"base", "target", "lambda_lo", "lambda_hi", "rounds"}
            if unknown:
                raise ValueError(f"tune_smoothing: {sorted(unknown)} are not fields of a tune set")
            full = _default_tune(**{k: v for k, v in p.items() if k != "base"})
            rec.base = cls.pack_smooths([p.get("base", full["base"])])[0]
            rec.target, rec.lambda_lo, rec.lambda_hi, rec.rounds, rec.reserved = full["target"], full["lambda_lo"], full["lambda_hi"], full["rounds"], 0
        arr = cls._pack(_lib.pg_tune_set, [sets] if isinstance(sets, (dict, _lib.pg_tune_set)) else sets, fill)
        if len(arr) < 1:
            raise ValueError("tune_smoothing: at least one tune set")
        for k, r in enumerate(arr):
            cls.pack_smooths([r.base])
            if r.base.lam != 0.0:
                raise ValueError(f"tune_smoothing: base.lam of set {k} must be 0 (the weight is what the call chooses)")
            if not (math.isfinite(r.target) and r.target > 0.0):
                raise ValueError(f"tune_smoothing: target of set {k} is finite and > 0")
            if not (math.isfinite(r.lambda_lo) and math.isfinite(r.lambda_hi) and 0.0 < r.lambda_lo < r.lambda_hi):
                raise ValueError(f"tune_smoothing: the bounds of set {k} are finite with 0 < lambda_lo < lambda_hi")
            if not 1 <= r.rounds <= 8:
                raise ValueError(f"tune_smoothing: rounds of set {k} lies in [1, 8]")
            if r.reserved != 0:
                raise ValueError(f"tune_smoothing: reserved of set {k} must be 0")
        return arr

    def tune_smoothing(self, paths, sets):
        """Surveyed waypoints smoothed to a target rms on the device (pg_tune_smoothing; the scheme is stated in include/pigeon_mpc.h): for every (path, set) pair the
        largest weight of a geometric ladder between lambda_lo and lambda_hi whose dev_rms stays within the set's target, and the path smoothed under it.  paths as
        smooth_waypoints takes them, sets = vehicles.tune(target=.., lambda_lo=.., lambda_hi=.., rounds=.., pin_ends=.., keep_walls=.., windows=[..]) dicts.  Returns
        (smoothed, stats, tune): smoothed and stats as smooth_waypoints returns them, tune a structured array [n_path][n_sets] with the fields of pg_tune_stats (lam,
        lo, hi, rms_lo, rms_hi, verdict, rounds_done, monotone)."""
        paths = [dict(p) for p in paths]
        for k, p in enumerate(paths):
            if len(p.get("waypoints", ())) < (5 if p.get("closed", False) else 2):
                raise ValueError(f"tune_smoothing: path {k} needs 2 waypoints (a closed path 5)")
            p.setdefault("n_knots", 3)
        specs, wps, _ = self.pack_fit_specs(paths)
        arr = self.pack_tunes(sets)
        n, ns, nw = len(specs), len(arr), len(wps)
        out = (_lib.pg_waypoint * (ns * nw))()
        st = (_lib.pg_smooth_stats * (n * ns))()
        tn = (_lib.pg_tune_stats * (n * ns))()
        self._chk(self.lib.pg_tune_smoothing(self.h, n, specs, nw, wps, ns, arr, out, st, tn), "pg_tune_smoothing")
        flat = np.frombuffer(out, dtype=np.float64).reshape(ns, nw, 4)
        smoothed = [[[dict(E=float(w[0]), N=float(w[1]), edge_L=float(w[2]), edge_R=float(w[3])) for w in flat[k, s.wp0:s.wp0 + s.n_wp]] for s in specs] for k in range(ns)]
        return smoothed, np.frombuffer(st, dtype=SMOOTH_STATS_DTYPE).copy().reshape(n, ns), np.frombuffer(tn, dtype=TUNE_STATS_DTYPE).copy().reshape(n, ns)

    # ---- the line inside the tube (pg_optimize_line): every (path, line set) pair of a waypoint library x a library of line sets, on the device ----
    @classmethod
    def pack_lines(cls, sets):
        """vehicles.line(...) dicts (one, or a list) or pg_line_set structures -> a ctypes array of pg_line_set.  Raises ValueError for a set outside the ranges of
        include/pigeon_mpc.h (the library refuses the same sets with PG_ERR_INVALID)."""
        def fill(rec, p):
            full = _default_line(**p)
            rec.mu, rec.rho, rec.margin, rec.alpha_max, rec.tol = full["mu"], full["rho"], full["margin"], full["alpha_max"], full["tol"]
            rec.iters, rec.pin_ends, rec.keep_walls, rec.n_win = full["iters"], int(full["pin_ends"]), int(full["keep_walls"]), len(full["windows"])
            for j in range(4):
                rec.u_lo[j], rec.u_hi[j], rec.win_margin[j], rec.win_pin[j] = full["windows"][j] if j < rec.n_win else (0.0, 0.0, 0.0, 0)
        arr = cls._pack(_lib.pg_line_set, [sets] if isinstance(sets, (dict, _lib.pg_line_set)) else sets, fill)
        if len(arr) < 1:
            raise ValueError("optimize_line: at least one line set")
        for k, r in enumerate(arr):
            for name, strict in (("mu", True), ("rho", True), ("alpha_max", True), ("margin", False), ("tol", False)):
                v = getattr(r, name)
                if not (math.isfinite(v) and (v > 0.0 if strict else v >= 0.0)):
                    raise ValueError(f"optimize_line: {name} of set {k} is finite and {'> 0' if strict else '>= 0'}")
            if not 1 <= r.iters <= 4096:
                raise ValueError(f"optimize_line: iters of set {k} lies in [1, 4096]")
            if not 0 <= r.n_win <= 4:
                raise ValueError(f"optimize_line: n_win of set {k} lies in [0, 4]")
            for j in range(r.n_win):
                if not r.u_lo[j] <= r.u_hi[j]:
                    raise ValueError(f"optimize_line: window {j} of set {k} needs u_lo <= u_hi")
                if not (math.isfinite(r.win_margin[j]) and r.win_margin[j] >= 0.0):
                    raise ValueError(f"optimize_line: the margin of window {j} of set {k} is finite and >= 0")
            if r.reserved[0] != 0 or r.reserved[1] != 0:
                raise ValueError(f"optimize_line: reserved of set {k} must be 0")
        return arr

    def optimize_line(self, paths, sets):
        """The line of least bending energy inside the tube, on the device (pg_optimize_line; the scheme is stated in include/pigeon_mpc.h): every waypoint moved along
        its normal inside its own edge_R .. edge_L, for every (path, set) pair.  paths as smooth_waypoints takes them (waypoints metres apart: thin a dense survey with
        vehicles.waypoints_from_tube(every=) first), sets = vehicles.line(h_mean=.., margin=.., alpha_max=.., iters=.., tol=.., pin_ends=.., keep_walls=..,
        windows=[vehicles.line_window(..)]) dicts.  Returns (lines, stats): lines[k][i] is the waypoint list of path i under set k (smoothed_fit_paths(paths, lines, k) is
        the list fit_paths takes for set k), stats a structured array [n_path][n_sets] with the fields of pg_line_stats (bend_in, bend_out, alpha_abs_max, i_alpha_max,
        n_active, r_prim, r_dual, iters_done, pivot_min, chord_min, width_min)."""
        paths = [dict(p) for p in paths]
        for k, p in enumerate(paths):
            if len(p.get("waypoints", ())) < (5 if p.get("closed", False) else 2):
                raise ValueError(f"optimize_line: path {k} needs 2 waypoints (a closed path 5)")
            p.setdefault("n_knots", 3)
        specs, wps, _ = self.pack_fit_specs(paths)
        arr = self.pack_lines(sets)
        n, ns, nw = len(specs), len(arr), len(wps)
        out = (_lib.pg_waypoint * (ns * nw))()
        st = (_lib.pg_line_stats * (n * ns))()
        self._chk(self.lib.pg_optimize_line(self.h, n, specs, nw, wps, ns, arr, out, st), "pg_optimize_line")
        flat = np.frombuffer(out, dtype=np.float64).reshape(ns, nw, 4)
        lines = [[[dict(E=float(w[0]), N=float(w[1]), edge_L=float(w[2]), edge_R=float(w[3])) for w in flat[k, s.wp0:s.wp0 + s.n_wp]] for s in specs] for k in range(ns)]
        return lines, np.frombuffer(st, dtype=LINE_STATS_DTYPE).copy().reshape(n, ns)

    # ---- making the starts (pg_make_starts): the inputs of a batch placed on the installed trajectory library under a library of start sets, on the device ----
    @classmethod
    def pack_starts(cls, sets):
        """dicts (vehicles.start(**overrides); missing fields: the defaults) or pg_start_set structures -> a ctypes array of pg_start_set.  Raises ValueError for what the
        library refuses with PG_ERR_INVALID (include/pigeon_mpc.h)."""
        def fill(rec, p):
            full = _default_start(**p)
            for name, ctype in _lib.pg_start_set._fields_:
                if name != "reserved":
                    setattr(rec, name, int(full[name]) if ctype is C.c_int32 else float(full[name]))
        arr = cls._pack(_lib.pg_start_set, [sets] if isinstance(sets, (dict, _lib.pg_start_set)) else sets, fill)
        if len(arr) == 0:
            raise ValueError("make_starts: at least one start set")
        for k, p in enumerate(arr):
            for n in _lib.START_RANGES:
                lo, hi = getattr(p, n + "_lo"), getattr(p, n + "_hi")
                if not (math.isfinite(lo) and math.isfinite(hi)):
                    raise ValueError(f"make_starts: set {k}: the range {n} is not finite")
                if lo > hi:
                    raise ValueError(f"make_starts: set {k}: the range {n} needs lo <= hi")
            if not p.v_lo > 0:
                raise ValueError(f"make_starts: set {k}: the speed factor needs v_lo > 0")
            if any(getattr(p, m) not in (0, 1) for m in _lib.START_MODES):
                raise ValueError(f"make_starts: set {k}: a mode is 0 or 1")
            if any(p.reserved):
                raise ValueError(f"make_starts: set {k}: reserved must be 0")
        return arr

    def make_starts(self, sets, index=None, seed=0, streams=None, B=None, install=True):
        """The inputs of a batch placed on the INSTALLED trajectory library on the device (pg_make_starts; the scheme is stated in include/pigeon_mpc.h): sets = one
        vehicles.start(**overrides) dict or a list of them, index = the set of every instance (None: set 0), seed and streams = the 64-bit stream id of every instance
        (None: its position in the batch); a start is a function of (seed, stream id, set, tube) alone.  B = the batch size (None: the length of index or of streams, else
        the current batch).  With several tubes installed an instance is placed on its own (set_trajectory_index first).  install=True makes them the handle's inputs, as
        set_inputs with the returned arrays would, without the host round trip.  Returns a dict of arrays: state [B][6], control [B][3], t0 [B], other [B][4],
        time_offset [B], placed [B][4] = (s, e, dpsi, V(s))."""
        arr = self.pack_starts(sets)
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint64).reshape(-1)
        if B is None:
            B = len(idx) if idx is not None else len(st) if st is not None else self.B
        B = int(B)
        for what, a in (("index", idx), ("streams", st)):
            if a is not None and len(a) != B:
                raise ValueError(f"make_starts: {what} has {len(a)} entries for B = {B}")
        out = dict(state=np.zeros((B, 6)), control=np.zeros((B, 3)), t0=np.zeros(B), other=np.zeros((B, 4)), time_offset=np.zeros(B), placed=np.zeros((B, 4)))
        self._chk(self.lib.pg_make_starts(self.h, B, len(arr), arr, _p(idx, c_i32p), C.c_uint64(int(seed)), _p(st, C.POINTER(C.c_uint64)), int(bool(install)),
                                          *(_p(out[k]) for k in ("state", "control", "t0", "other", "time_offset", "placed"))), "pg_make_starts")
        if install:
            self.B = B
        return out

    # ---- the per-instance libraries share one protocol (pg_set_<name>_sets / pg_set_<name>_index / pg_clear_<name>_sets / pg_get_<name>_sets): the four routines below ----
    @staticmethod
    def _pack(ctype, sets, fill):
        """structures of `ctype` (copied) or whatever fill(record, item) understands -> a ctypes array of `ctype`."""
        sets = list(sets)
        arr = (ctype * len(sets))()
        for k, v in enumerate(sets):
            if isinstance(v, ctype):
                C.memmove(C.byref(arr[k]), C.byref(v), C.sizeof(ctype))
            else:
                fill(arr[k], v)
        return arr

    def _set_index(self, name, index):
        index = np.ascontiguousarray(index, dtype=np.int32)
        self._chk(getattr(self.lib, f"pg_set_{name}_index")(self.h, len(index), _p(index, c_i32p)), f"pg_set_{name}_index")
        return index

    def _set_sets(self, name, ctype, pack, sets, index):
        """one set (dict / structure) for the whole batch, or a list of sets; then the per-instance selection, if given."""
        arr = pack([sets] if isinstance(sets, (dict, ctype)) else sets)
        self._chk(getattr(self.lib, f"pg_set_{name}_sets")(self.h, len(arr), arr), f"pg_set_{name}_sets")
        if index is not None:
            self._set_index(name, index)

    def _get_sets(self, name, ctype, as_dict):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        get = getattr(self.lib, f"pg_get_{name}_sets")
        n = C.c_int32(0)
        self._chk(get(self.h, C.byref(n), None, 0, None, 0), f"pg_get_{name}_sets")           # first call: how many sets
        arr = (ctype * max(n.value, 1))()
        index = np.full(self.B, -1, dtype=np.int32)
        self._chk(get(self.h, C.byref(n), arr, n.value, _p(index, c_i32p), self.B), f"pg_get_{name}_sets")
        return [as_dict(arr[k]) for k in range(n.value)], index

    def _set_seed(self, name, seed, streams):
        st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint64)
        self._chk(getattr(self.lib, f"pg_set_{name}_seed")(self.h, C.c_uint64(int(seed)), max(self.B, 1) if st is None else len(st), _p(st, C.POINTER(C.c_uint64))), f"pg_set_{name}_seed")

    def _clear(self, name):
        self._chk(getattr(self.lib, f"pg_clear_{name}_sets")(self.h), f"pg_clear_{name}_sets")

    def _state(self, name, width):
        """[B][width]: what pg_get_<name>_state reads"""
        out = np.zeros((self.B, width))
        self._chk(getattr(self.lib, f"pg_get_{name}_state")(self.h, _p(out)), f"pg_get_{name}_state")
        return out

    def _hist(self, setter, width, steps, library=None):
        """registers a [steps][B][width] device record with the next rollout call through `setter` and returns it; None when `library` is given and none is installed"""
        if library is not None:
            n = C.c_int32(0)
            self._chk(getattr(self.lib, f"pg_get_{library}_sets")(self.h, C.byref(n), None, 0, None, 0), f"pg_get_{library}_sets")
            if n.value == 0:
                return None
        torch, tdt, dev = self._torch()
        buf = torch.empty(int(steps), self.B, width, dtype=tdt, device=dev)
        self._chk(getattr(self.lib, setter)(self.h, C.c_void_p(buf.data_ptr()), int(steps)), setter)
        return buf

    # ---- one controller per (x0, control_params) pair: a library of parameter sets and a per-instance selection (a tuning sweep in one batch) ----
    def pack_control_params(self, sets):
        """dicts (missing fields: the handle's own control_params) or pg_control_params structures -> a ctypes array of pg_control_params."""
        def fill(rec, cp):
            C.memmove(C.byref(rec), C.byref(self.cfg.control), C.sizeof(_lib.pg_control_params))
            for name, _ in _lib.pg_control_params._fields_:
                if name != "_pad" and name in cp:
                    setattr(rec, name, int(cp[name]) if name == "N_HJI" else float(cp[name]))
        return self._pack(_lib.pg_control_params, sets, fill)

    def set_control_params(self, sets, index=None):
        """One set (dict / structure) for the whole batch, or a list of sets; select per instance with `index` or set_control_param_index."""
        self._set_sets("control_param", _lib.pg_control_params, self.pack_control_params, sets, index)

    def set_control_param_index(self, index):
        self._set_index("control_param", index)

    def clear_control_params(self):
        self._clear("control_param")

    def control_param_sets(self):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("control_param", _lib.pg_control_params, lambda r: {name: getattr(r, name) for name, _ in r._fields_ if name != "_pad"})

    # ---- the PLANT of the rollouts, per instance (model-mismatch studies): a library of vehicles and a per-instance selection.  The controller keeps self.vehicle ----
    def pack_vehicles(self, sets):
        """vehicle dicts (vehicles.X1(**overrides); missing fields: the handle's own vehicle) or pg_vehicle structures -> a ctypes array of pg_vehicle."""
        def fill(rec, v):
            for name, _ in _lib.pg_vehicle._fields_:
                setattr(rec, name, float(v[name] if name in v else self.vehicle[name]))
        return self._pack(_lib.pg_vehicle, sets, fill)

    def set_plants(self, sets, index=None):
        """The vehicle the ego plant of simulate_ / simulate_safety_ / simulate_node_ integrates (pg_set_plant_sets): one set (dict / structure) for the whole batch, or a
        list of sets; select per instance with `index` or set_plant_index.  Resets nothing: the plant is no part of any QP."""
        self._set_sets("plant", _lib.pg_vehicle, self.pack_vehicles, sets, index)

    def set_plant_index(self, index):
        self._set_index("plant", index)

    def clear_plants(self):
        self._clear("plant")

    def plant_sets(self):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("plant", _lib.pg_vehicle, lambda r: {name: getattr(r, name) for name, _ in r._fields_})

    def tracking_summary(self):
        """Per instance since the rollout's clock last restarted (option "tracking_summary" = 1 first; pg_get_tracking_state): (summary [B][6] = max |e|, sum e^2,
        max |Uy / Ux|, max |r|, min Ux, s of the last step; steps [B]; first_exit [B]: first step index with e outside the tube's edges, -1: none)."""
        sm = np.zeros((self.B, 6)); n = np.zeros(self.B, dtype=np.int32); fx = np.zeros(self.B, dtype=np.int32)
        self._chk(self.lib.pg_get_tracking_state(self.h, _p(sm), _p(n, C.POINTER(C.c_int32)), _p(fx, C.POINTER(C.c_int32))), "pg_get_tracking_state")
        return sm, n, fx

    # ---- the SENSOR of the rollouts, per instance (measurement noise): a library of (sigma, bias) sets, a per-instance selection, a seed and stream ids ----
    SENSOR_CHANNELS = ("E", "N", "psi", "Ux", "Uy", "r")

    def pack_sensors(self, sets):
        """sensor dicts {"sigma": [6] or {channel: value}, "bias": ...} (missing: 0), (sigma, bias) pairs or pg_sensor structures -> a ctypes array of pg_sensor."""
        def six(v):
            if v is None:
                return [0.0] * 6
            if isinstance(v, dict):
                return [float(v.get(c, 0.0)) for c in self.SENSOR_CHANNELS]
            return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(6)]

        def fill(rec, v):
            sg, bs = (v.get("sigma"), v.get("bias")) if isinstance(v, dict) else v
            rec.sigma[:] = six(sg); rec.bias[:] = six(bs)
        return self._pack(_lib.pg_sensor, sets, fill)

    def set_sensors(self, sets, index=None, seed=0, streams=None):
        """What the controller of simulate_ / simulate_safety_ / simulate_node_ reads in place of the true state (pg_set_sensor_sets): measured = true + bias + sigma z per
        channel of (E, N, psi, Ux, Uy, r).  One set (dict / structure) for the whole batch, or a list of sets selected per instance with `index`; `seed` and the 64-bit
        `streams` [B] (None: stream[b] = b) fix the draws (pg_set_sensor_seed).  Resets nothing.  Unlike the C calls, where seed and streams persist across installs, EVERY call here
        installs seed and streams too: re-installing a library without them puts the seed back to 0 and the streams back to b (set_sensor_seed afterwards, or pass them again)."""
        self._set_sets("sensor", _lib.pg_sensor, self.pack_sensors, sets, index)
        self.set_sensor_seed(seed, streams)

    def set_sensor_seed(self, seed=0, streams=None):
        self._set_seed("sensor", seed, streams)

    def clear_sensors(self):
        self._clear("sensor")

    def sensors(self):
        """(list of {"sigma": [6], "bias": [6]}, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("sensor", _lib.pg_sensor, lambda r: {"sigma": list(r.sigma), "bias": list(r.bias)})

    def sensor_draws(self, step0, steps, B=None):
        """The standard normals z [steps][B][6] the rollouts draw at clock steps [step0, step0 + steps), computed on the device by the function k_measure calls (pg_sensor_draws)."""
        B = self.B if B is None else int(B)
        z = np.zeros((int(steps), B, 6))
        self._chk(self.lib.pg_sensor_draws(self.h, int(step0), int(steps), B, _p(z)), "pg_sensor_draws")
        return z

    def measured_state(self):
        """[B][6]: what the controller read at the last rollout step under a sensor library (pg_get_measured_state)."""
        return self._state("measured", 6)

    # ---- the ACTUATOR of the rollouts, per instance (command delay, lag, slew): a library of pg_actuator_set and a per-instance selection ----
    @classmethod
    def pack_actuators(cls, sets):
        """actuator dicts (vehicles.actuator(**overrides); missing fields: the identity's) or pg_actuator_set structures -> a ctypes array of pg_actuator_set."""
        def fill(rec, v):
            a = _identity_actuator(**v)
            d = int(a["delay_steps"])
            if d != a["delay_steps"] or not 0 <= d <= _lib.PG_ACT_MAX_DELAY:
                raise ValueError(f"delay_steps = {a['delay_steps']} is outside 0 .. PG_ACT_MAX_DELAY = {_lib.PG_ACT_MAX_DELAY} rollout steps")
            rec.delay_steps = d; rec.feedback = int(a["feedback"])
            for name in ("tau_delta", "tau_fx", "rate_delta", "rate_fx"):
                setattr(rec, name, float(a[name]))
        return cls._pack(_lib.pg_actuator_set, sets, fill)

    def set_actuators(self, sets, idx=None):
        """What the plant of simulate_ / simulate_safety_ integrates in place of the command (pg_set_actuator_sets): per channel of (delta, Fxf, Fxr) the command delayed by
        delay_steps, through a first-order lag tau and a slew limit rate; feedback = 1 shows the controller the actuator's position as current_control.  One set (dict /
        structure) for the whole batch, or a list of sets selected per instance with `idx`.  Resets nothing.  simulate_node_ / node_step_ refuse to run under a library."""
        self._set_sets("actuator", _lib.pg_actuator_set, self.pack_actuators, sets, idx)

    def set_actuator_index(self, idx):
        self._set_index("actuator", idx)

    def clear_actuators(self):
        self._clear("actuator")

    def get_actuators(self):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("actuator", _lib.pg_actuator_set, lambda r: {name: getattr(r, name) for name, _ in r._fields_})

    def actuator_state(self):
        """[B][3]: the applied control a of the last rollout step under a library; the handle's control before the first one since the clock restarted (pg_get_actuator_state)."""
        return self._state("actuator", 3)

    def actuator_response(self, commands, dt):
        """The law alone, on the device through the function the rollouts call (pg_actuator_response): commands [steps][B][3] -> applied [steps][B][3] under the installed
        library and index, from a fresh state.  B is the batch of the inputs last installed."""
        c = _f64(commands).reshape(-1, self.B, 3)
        out = np.zeros_like(c)
        self._chk(self.lib.pg_actuator_response(self.h, c.shape[0], C.c_double(dt), _p(c), _p(out)), "pg_actuator_response")
        return out

    # ---- the DISTURBANCE of the rollouts, per instance (forces, gusts, low-friction windows): a library of pg_disturbance, a per-instance selection, a seed and stream ids ----
    @classmethod
    def pack_disturbances(cls, sets):
        """disturbance dicts (vehicles.disturbance(**overrides); missing fields: the identity's) or pg_disturbance structures -> a ctypes array of pg_disturbance."""
        def fill(rec, v):
            d = _identity_disturbance(**v)
            for name in ("step_on", "step_off"):
                if int(d[name]) != d[name]:
                    raise ValueError(f"{name} = {d[name]} is not a whole number of rollout steps")
                setattr(rec, name, int(d[name]))
            for name in ("Fx", "Fy", "Mz", "sigma_Fx", "sigma_Fy", "x_cp", "tau_gust", "mu_scale"):
                setattr(rec, name, float(d[name]))
        return cls._pack(_lib.pg_disturbance, sets, fill)

    def set_disturbances(self, sets, index=None, seed=0, streams=None):
        """What acts on the ego plant of simulate_ / simulate_safety_ / simulate_node_ from outside (pg_set_disturbance_sets): inside the window [step_on, step_off) a
        body-frame force (Fx, Fy), a yaw moment Mz, a seeded coloured gust (sigma_Fx, sigma_Fy, x_cp, tau_gust) and a factor mu_scale on the plant's friction, held for
        the step.  One set (dict / structure) for the whole batch, or a list of sets selected per instance with `index`; `seed` and the 64-bit `streams` [B] (None:
        stream[b] = b) fix the gust (pg_set_disturbance_seed).  The controller never sees any of it.  Resets nothing.  As set_sensors, EVERY call here installs seed and
        streams too (set_disturbance_seed afterwards, or pass them again)."""
        self._set_sets("disturbance", _lib.pg_disturbance, self.pack_disturbances, sets, index)
        self.set_disturbance_seed(seed, streams)

    def set_disturbance_index(self, index):
        self._set_index("disturbance", index)

    def set_disturbance_seed(self, seed=0, streams=None):
        self._set_seed("disturbance", seed, streams)

    def clear_disturbances(self):
        self._clear("disturbance")

    def disturbances(self):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("disturbance", _lib.pg_disturbance, lambda r: {name: getattr(r, name) for name, _ in r._fields_})

    def disturbance_response(self, step0, steps, dt):
        """The law alone, on the device through the function the rollouts call (pg_disturbance_response): w [steps][B][4] = (wFx, wFy, wMz, wmu) of the clock steps
        [step0, step0 + steps) under the installed library, index, seed and streams, from a fresh gust state at step0.  B is the batch of the inputs last installed."""
        w = np.zeros((int(steps), self.B, 4))
        self._chk(self.lib.pg_disturbance_response(self.h, int(step0), int(steps), C.c_double(dt), _p(w)), "pg_disturbance_response")
        return w

    def disturbance_state(self):
        """[B][4]: w of the last rollout step under a disturbance library (pg_get_disturbance_state)."""
        return self._state("disturbance", 4)

    # ---- the ESTIMATOR of the rollouts, per instance (a fixed-gain observer between the sensor and the controller): a library of pg_estimator and a per-instance selection ----
    @classmethod
    def pack_estimators(cls, sets):
        """estimator dicts (vehicles.estimator(**overrides); missing fields: the identity's) or pg_estimator structures -> a ctypes array of pg_estimator."""
        def fill(rec, v):
            e = _identity_estimator(**v)
            for name in ("predict", "reserved"):
                if int(e[name]) != e[name]:
                    raise ValueError(f"{name} = {e[name]} is not a whole number")
                setattr(rec, name, int(e[name]))
            rec.gain[:] = e["gain"]
        return cls._pack(_lib.pg_estimator, sets, fill)

    def set_estimators(self, sets, index=None):
        """What the controller of simulate_ / simulate_safety_ / simulate_node_ reads in place of the sensor's output (pg_set_estimator_sets): per channel of (E, N, psi, Ux,
        Uy, r) estimate = prior + gain (measurement - prior), the prior one step of the controller's own model from the previous estimate (predict=1) or that estimate
        itself (predict=0).  One set (dict / structure) for the whole batch, or a list of sets selected per instance with `index`.  The plant, the records and the
        summaries keep the truth.  Resets nothing."""
        self._set_sets("estimator", _lib.pg_estimator, self.pack_estimators, sets, index)

    def set_estimator_index(self, index):
        self._set_index("estimator", index)

    def clear_estimators(self):
        self._clear("estimator")

    def get_estimators(self):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("estimator", _lib.pg_estimator, lambda r: {"predict": r.predict, "reserved": r.reserved, "gain": list(r.gain)})

    def estimated_state(self):
        """[B][6]: what the controller read at the last rollout step under an estimator library (pg_get_estimated_state)."""
        return self._state("estimated", 6)

    def estimator_response(self, y, u, dt):
        """The law alone, on the device through the function the rollouts call (pg_estimator_response): measurements y [steps][B][6] and controls u [steps][B][3] (u[k]: what
        the controller is handed at step k; step k's prior is driven by u[k - 1]) -> estimates [steps][B][6] under the installed library and index, from a fresh state.
        B is the batch of the inputs last installed."""
        y = _f64(y).reshape(-1, self.B, 6); u = _f64(u).reshape(-1, self.B, 3)
        if u.shape[0] != y.shape[0]:
            raise ValueError(f"y has {y.shape[0]} steps and u has {u.shape[0]}")
        out = np.zeros_like(y)
        self._chk(self.lib.pg_estimator_response(self.h, y.shape[0], C.c_double(dt), _p(y), _p(u), _p(out)), "pg_estimator_response")
        return out

    # ---- the HUMAN of the safety and node rollouts, per instance (the other car's driver): a library of pg_human, a per-instance selection, a seed and stream ids ----
    @classmethod
    def pack_humans(cls, sets):
        """human dicts (vehicles.human(**overrides); missing fields: the identity's) or pg_human structures -> a ctypes array of pg_human."""
        def fill(rec, v):
            d = _identity_human(**v)
            for name in ("mode", "hold_steps", "step_on", "step_off"):
                if int(d[name]) != d[name]:
                    raise ValueError(f"{name} = {d[name]} is not a whole number")
                setattr(rec, name, int(d[name]))
            rec.gain[:] = d["gain"]; rec.sigma[:] = d["sigma"]
            for name in ("omega_max", "a_min", "a_max", "tau"):
                setattr(rec, name, float(d[name]))
        return cls._pack(_lib.pg_human, sets, fill)

    def set_humans(self, sets, index=None, seed=0, streams=None):
        """Who drives the other car of simulate_safety_ / simulate_node_ (pg_set_human_sets): per instance hold (mode 0), the worst case (1), the caller's script (2) or a
        seeded random driver (3), inside the window [step_on, step_off), decided every hold_steps steps, scaled by gain and limited to omega_max, [a_min, a_max].  One set
        (dict / structure) for the whole batch, or a list of sets selected per instance with `index`; `seed` and the 64-bit `streams` [B] (None: stream[b] = b) fix the
        random driver (pg_set_human_seed).  Under a library the rollouts' `human` argument no longer decides; pass human_u when a set has mode 2.  Resets nothing.  As
        set_disturbances, EVERY call here installs seed and streams too."""
        self._set_sets("human", _lib.pg_human, self.pack_humans, sets, index)
        self.set_human_seed(seed, streams)

    def set_human_index(self, index):
        self._set_index("human", index)

    def set_human_seed(self, seed=0, streams=None):
        self._set_seed("human", seed, streams)

    def clear_humans(self):
        self._clear("human")

    def humans(self):
        """(list of dicts, index array over the current batch; -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("human", _lib.pg_human, lambda r: {name: (list(getattr(r, name)) if name in ("gain", "sigma") else getattr(r, name)) for name, _ in r._fields_})

    def human_response(self, step0, x7, vg8, dt, script=None):
        """The law alone, on the device through the function the rollouts call (pg_human_response): relative states x7 [steps][B][7], lookups vg8 [steps][B][8] (V, then the
        gradient) and script [steps][B][2] (None unless a set has mode 2) -> (omega, a) [steps][B][2] of the clock steps [step0, step0 + steps) under the installed library,
        index, seed and streams, from a fresh state at step0.  B is the batch of the inputs last installed."""
        x7 = _f64(x7).reshape(-1, self.B, 7); vg8 = _f64(vg8).reshape(-1, self.B, 8)
        if vg8.shape[0] != x7.shape[0]:
            raise ValueError(f"x7 has {x7.shape[0]} steps and vg8 has {vg8.shape[0]}")
        sc = None if script is None else _f64(script).reshape(x7.shape[0], self.B, 2)
        out = np.zeros((x7.shape[0], self.B, 2))
        self._chk(self.lib.pg_human_response(self.h, int(step0), x7.shape[0], C.c_double(dt), _p(x7), _p(vg8), _p(sc), _p(out)), "pg_human_response")
        return out

    def human_state(self):
        """[B][2]: (omega, a) of the last rollout step under a human library (pg_get_human_state)."""
        return self._state("human", 2)

    # ---- the ROUTE of the rollouts, per instance (a trajectory change during the run: nominal_trajectory_callback): a library of pg_route and a per-instance selection ----
    @classmethod
    def pack_routes(cls, sets):
        """route sets (vehicles.route(*events): a list of up to four event dicts; a shorter list is filled with unused slots) or pg_route structures -> a ctypes array of pg_route."""
        def fill(rec, events):
            events = list(events)
            if len(events) > _lib.PG_ROUTE_EVENTS:
                raise ValueError(f"a route set holds at most {_lib.PG_ROUTE_EVENTS} events, not {len(events)}")
            for k, e in enumerate(events + _route()[len(events):]):
                for name, _ in _lib.pg_route_event._fields_:
                    setattr(rec.ev[k], name, float(e[name]) if name == "t_join" else int(e[name]))
        return cls._pack(_lib.pg_route, sets, fill)

    def set_routes(self, sets, index=None):
        """Which trajectory of the installed library an instance tracks WHEN during simulate_ / simulate_safety_ / simulate_node_ (pg_set_route_sets): per instance up to four
        events "at clock step k go to trajectory j, anchored so" (vehicles.route, vehicles.route_event).  One set (a list of events / structure) for the whole batch, or a
        list of sets selected per instance with `index`.  The index set_trajectory_index installed is every instance's home: a restarted clock starts there again."""
        if isinstance(sets, _lib.pg_route) or (isinstance(sets, (list, tuple)) and (not sets or isinstance(sets[0], dict))):
            sets = [sets]                                        # (one set: a list of event dicts, possibly empty)
        self._set_sets("route", _lib.pg_route, self.pack_routes, list(sets), index)

    def set_route_index(self, index):
        self._set_index("route", index)

    def clear_routes(self):
        self._clear("route")

    def routes(self):
        """(list of sets, each a list of four event dicts; index array over the current batch, -1 where no index covers an instance) as installed; ([], ...) without a library."""
        return self._get_sets("route", _lib.pg_route, lambda r: [{name: getattr(e, name) for name, _ in e._fields_} for e in r.ev])

    def route_state(self):
        """dict of [B] arrays (pg_get_route_state): traj (the trajectory each instance is on now), fired (events since the clock last restarted), last_step (clock step of
        the last one, -1: none), t_at (where the new trajectory was joined) and e_at (lateral offset of a "project" event's projection, NaN otherwise)."""
        i32 = lambda: np.zeros(self.B, dtype=np.int32)
        tr, fi, ls, ta, ea = i32(), i32(), i32(), np.zeros(self.B), np.zeros(self.B)
        self._chk(self.lib.pg_get_route_state(self.h, _p(tr, c_i32p), _p(fi, c_i32p), _p(ls, c_i32p), _p(ta), _p(ea)), "pg_get_route_state")
        return dict(traj=tr, fired=fi, last_step=ls, t_at=ta, e_at=ea)

    def record_route(self, steps):
        """Registers an int32 device tensor [steps][B] with the NEXT rollout call and returns it: the trajectory each step's controller ran on (pg_set_route_history_dev)."""
        torch, _, dev = self._torch()
        buf = torch.empty(int(steps), self.B, dtype=torch.int32, device=dev)
        self._chk(self.lib.pg_set_route_history_dev(self.h, C.c_void_p(buf.data_ptr()), int(steps)), "pg_set_route_history_dev")
        return buf

    def _torch(self):
        """(torch, the library's own element type: what device arrays handed to the *_dev entry points hold, the handle's device)"""
        import torch
        return torch, torch.float32 if self.precision == "f32" else torch.float64, f"cuda:{self.cfg.device}"

    # ---- mpc.HJI_cache = HJICache(...) (Pigeon.jl:40) ----
    def set_hji_cache(self, grid_knots, V_raw, gradV_raw):
        dims = np.array([len(k) for k in grid_knots], dtype=np.int32)
        kc = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float32) for k in grid_knots]))
        V = np.ascontiguousarray(V_raw, dtype=np.float32).reshape(-1)
        g = np.ascontiguousarray(gradV_raw, dtype=np.float32).reshape(-1)
        assert V.size == int(np.prod(dims.astype(np.int64))) and g.size == 7 * V.size
        self._chk(self.lib.pg_set_hji_grid(self.h, _p(dims, C.POINTER(C.c_int32)), _p(kc, C.POINTER(C.c_float)), _p(V, C.POINTER(C.c_float)),
                                           _p(g, C.POINTER(C.c_float))), "pg_set_hji_grid")

    def clear_hji_cache(self):
        self._chk(self.lib.pg_clear_hji_grid(self.h), "pg_clear_hji_grid")

    def solve_hji_cache(self, grid_knots, l0, horizon, vehicle=None, install=True, **opts):
        """Computes the avoid-set grid on the device (pg_hji_solve): the reachable tube of the target l0 [prod dims] (column-major, e.g. hji_io.collision_target) over
        `horizon` seconds for `vehicle` (a vehicles.X1(**overrides) dict or a pg_vehicle; None: the handle's own).  opts: cfl, fixed_dt, max_sweeps, periodic_psi.
        Returns (V [prod dims] float32, gradV [prod dims, 7] float32, stats dict) -- what set_hji_cache takes; install=True leaves the handle as set_hji_cache would.
        A refused argument or a NaN in V raises PigeonError; its `stats` attribute then holds the stats of the sweeps taken."""
        dims = np.array([len(k) for k in grid_knots], dtype=np.int32)
        kc = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float32) for k in grid_knots]))
        l0 = np.ascontiguousarray(l0, dtype=np.float32).reshape(-1)
        n = int(np.prod(dims.astype(np.int64)))
        assert len(dims) == 7 and l0.size == n
        o = self.lib.pg_default_hji_solve_opts()
        o.horizon = float(horizon)
        periodic = bool(opts.pop("periodic_psi", False))
        o.flags = _lib.PG_HJI_PERIODIC_PSI if periodic else 0
        for k in list(opts):
            if k not in ("cfl", "fixed_dt", "max_sweeps"):
                raise KeyError(f"{k} is not an option of solve_hji_cache: cfl, fixed_dt, max_sweeps, periodic_psi")
            setattr(o, k, int(opts[k]) if k == "max_sweeps" else float(opts[k]))
        veh = None if vehicle is None else self.pack_vehicles([vehicle])
        V = np.zeros(n, dtype=np.float32); g = np.zeros((n, 7), dtype=np.float32)
        st = _lib.pg_hji_solve_stats()
        fp = C.POINTER(C.c_float)
        rc = self.lib.pg_hji_solve(self.h, _p(dims, c_i32p), _p(kc, fp), _p(l0, fp), veh, C.byref(o), int(bool(install)), _p(V, fp), _p(g, fp), C.byref(st))
        stats = {"sweeps": st.sweeps, "reached_horizon": st.reached_horizon, "bad_sweep": st.bad_sweep, "tau": st.tau, "last_dt": st.last_dt,
                 "alpha": np.array(list(st.alpha)), "v_min": st.v_min, "v_max": st.v_max}
        try:
            self._chk(rc, "pg_hji_solve")
        except _lib.PigeonError as e:
            e.stats = stats; e.status = rc
            raise
        return V, g, stats

    # ---- mpc.solved = false (ros_integration.jl:34,41,147) ----
    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._chk(self.lib.pg_reset(self.h, _p(m, C.POINTER(C.c_uint8))), "pg_reset")

    # ---- mpc.current_state / current_control / other_car_state / time_offset + the time argument of compute_time_steps! ----
    def set_inputs(self, current_state, current_control, t, other_car_state=None, time_offset=None):
        s = _f64(current_state).reshape(-1, 6)
        B = s.shape[0]
        c = _f64(current_control, (B, 3)); t0 = _f64(t, (B,))
        o = None if other_car_state is None else _f64(other_car_state, (B, 4))
        to = None if time_offset is None else _f64(time_offset, (B,))
        self._chk(self.lib.pg_set_inputs(self.h, B, _p(s), _p(c), _p(t0), _p(o), _p(to)), "pg_set_inputs")
        self.B = B

    def set_inputs_dev(self, B, state_ptr, control_ptr, t0_ptr, other_ptr=None, toff_ptr=None):
        """Inputs already resident in HBM (raw device addresses, e.g. torch.Tensor.data_ptr())."""
        vp = lambda a: C.c_void_p(a) if a else None
        self._chk(self.lib.pg_set_inputs_dev(self.h, B, vp(state_ptr), vp(control_ptr), vp(t0_ptr), vp(other_ptr), vp(toff_ptr)), "pg_set_inputs_dev")
        self.B = B

    # ---- the five reference calls ----
    def compute_time_steps_(self, t0=None):
        """compute_time_steps!(mpc, t0): model_predictive_control.jl:70.  t0 (array of B) may also come from set_inputs."""
        if t0 is not None:
            raise ValueError("pass t through set_inputs(state, control, t, ...): the batch keeps its inputs in device memory")
        self._chk(self.lib.pg_compute_time_steps(self.h), "pg_compute_time_steps")

    def compute_linearization_nodes_(self):
        self._chk(self.lib.pg_compute_linearization_nodes(self.h), "pg_compute_linearization_nodes")

    def update_QP_(self):
        self._chk(self.lib.pg_update_qp(self.h), "pg_update_qp")

    def solve_(self):
        self._chk(self.lib.pg_solve(self.h), "pg_solve")

    def get_next_control(self):
        """BicycleControl (delta, Fxf, Fxr) per instance: coupled_lat_long.jl:370-374."""
        u = np.zeros((self.B, 3))
        self._chk(self.lib.pg_get_next_control(self.h, _p(u)), "pg_get_next_control")
        return u

    def get_next_control_hji(self, use_HJI_policy=True):
        """ros_integration.jl:114-124: (u [B,3], source [B] (0 MPC / 1 HJI policy / 2 unsafe but policy off), optimal_control (delta, Fx) [B,2])"""
        u = np.zeros((self.B, 3)); src = np.zeros(self.B, dtype=np.int32); u2 = np.zeros((self.B, 2))
        self._chk(self.lib.pg_get_next_control_hji(self.h, int(bool(use_HJI_policy)), _p(u), _p(src, C.POINTER(C.c_int32)), _p(u2)), "pg_get_next_control_hji")
        return u, src, u2

    def step_(self, current_state, current_control, t, other_car_state=None, time_offset=None):
        """The whole callback body of ros_integration.jl:94-99,124 for every instance; returns (u, status, iters)."""
        s = _f64(current_state).reshape(-1, 6); B = s.shape[0]
        c = _f64(current_control, (B, 3)); t0 = _f64(t, (B,))
        o = None if other_car_state is None else _f64(other_car_state, (B, 4))
        to = None if time_offset is None else _f64(time_offset, (B,))
        u = np.zeros((B, 3)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
        self._chk(self.lib.pg_step(self.h, B, _p(s), _p(c), _p(t0), _p(o), _p(to), _p(u), _p(st, C.POINTER(C.c_int32)), _p(it, C.POINTER(C.c_int32))), "pg_step")
        self.B = B
        return u, st, it

    MPC_ = step_      # the convenience names BASELINE.json's north star uses

    def step_dev(self, u_out_ptr=None):
        self._chk(self.lib.pg_step_dev(self.h, C.c_void_p(u_out_ptr) if u_out_ptr else None), "pg_step_dev")

    def get_next_control_dev(self, u_ptr):
        """get_next_control into a device array [B][3] of the library's element type (raw address; None: nothing is written).  Asynchronous on the handle's stream."""
        self._chk(self.lib.pg_get_next_control_dev(self.h, C.c_void_p(u_ptr) if u_ptr else None), "pg_get_next_control_dev")

    def get_next_control_hji_dev(self, use_HJI_policy, u_ptr, source_ptr=None):
        """get_next_control_hji into device arrays: u [B][3] of the library's element type, source [B] int32 (either may be None).  Asynchronous on the handle's stream."""
        vp = lambda a: C.c_void_p(a) if a else None
        self._chk(self.lib.pg_get_next_control_hji_dev(self.h, int(bool(use_HJI_policy)), vp(u_ptr), vp(source_ptr)), "pg_get_next_control_hji_dev")

    def hji_lookup_dev(self, B, x7_ptr, V_ptr=None, gradV_ptr=None):
        """hji_lookup on device arrays of the library's element type: x7 [B][7] in, V [B] and gradV [B][7] out (either may be None).  Returns once the outputs are written."""
        vp = lambda a: C.c_void_p(a) if a else None
        self._chk(self.lib.pg_hji_lookup_dev(self.h, int(B), vp(x7_ptr), vp(V_ptr), vp(gradV_ptr)), "pg_hji_lookup_dev")

    def hji_lookup8_dev(self, B, x7_ptr, out8_ptr):
        """The packed lookup: out8 [B][8] = (V, gradV[0..6]) per row of x7 [B][7], device arrays of the library's element type.  Asynchronous on the handle's stream."""
        vp = lambda a: C.c_void_p(a) if a else None
        self._chk(self.lib.pg_hji_lookup8_dev(self.h, int(B), vp(x7_ptr), vp(out8_ptr)), "pg_hji_lookup8_dev")

    HUMAN_MODES = {"hold": 0, "worst": 1, "script": 2}
    # the records a library adds to those of a rollout with record=True: (key, history setter, library, width)
    LIBRARY_RECORDS = (("applied", "pg_set_applied_history_dev", "actuator", 3), ("command", "pg_set_command_history_dev", "actuator", 3),
                       ("disturbance", "pg_set_disturbance_history_dev", "disturbance", 4), ("human_u", "pg_set_human_history_dev", "human", 2))

    def _rollout(self, steps, record, measured, shapes, int_record, call, human="hold", human_u=None, other=True, estimated=False):
        """The rollouts' shared plumbing.  Device records [steps][B] + shapes[name] in the library's element type and one int32 record `int_record` (record=True), the scripted
        human [steps][B][2], the measured history, under an actuator library the applied / command histories [steps][B][3] (record=True; they join the records as "applied"
        and "command"), under a disturbance library the history of w [steps][B][4] (record=True; "disturbance"), under a human library (rollouts with another car) the
        history of the library's (omega, a) [steps][B][2] (record=True; "human_u"); call(ptr, hu, hist) makes the library call (ptr: tensor or None -> c_void_p); then the state is read back.  Returns
        ((state, control, t[, other]), the records as fp64 / int32 numpy arrays or None, (measured history,) or () followed by (estimated history,) or () -- estimated=True
        registers the [steps][B][6] record of the estimate, as measured=True registers the measured one)."""
        assert human in self.HUMAN_MODES, human
        hu = None; hist = {}
        if human == "script" and human_u is None:
            raise ValueError('human="script" needs human_u [steps][B][2]')
        if human_u is not None and other:                       # (the script of human="script", or of the mode-2 sets of a human library)
            torch, tdt, dev = self._torch()
            hu = torch.as_tensor(np.ascontiguousarray(human_u, dtype=np.float64).reshape(steps, self.B, 2)).to(device=dev, dtype=tdt).contiguous()
        if record:
            torch, tdt, dev = self._torch()
            hist = {k: torch.empty((steps, self.B) + s, dtype=tdt, device=dev) for k, s in shapes.items()}
            if int_record:
                hist[int_record] = torch.empty((steps, self.B), dtype=torch.int32, device=dev)
        mbuf = self._hist("pg_set_measured_history_dev", 6, steps) if measured else None
        ebuf = self._hist("pg_set_estimated_history_dev", 6, steps) if estimated else None
        abuf = {}
        for key, setter, library, width in self.LIBRARY_RECORDS if record else ():
            buf = self._hist(setter, width, steps, library) if other or library != "human" else None
            if buf is not None:
                abuf[key] = buf
        call(lambda t: C.c_void_p(t.data_ptr()) if t is not None else None, hu, hist)
        s = np.zeros((self.B, 6)); c = np.zeros((self.B, 3)); t = np.zeros(self.B); o = np.zeros((self.B, 4))
        self._chk(self.lib.pg_get_state(self.h, _p(s), _p(c), _p(t)), "pg_get_state")
        if other:
            self._chk(self.lib.pg_get_safety_state(self.h, _p(o), None, None, None), "pg_get_safety_state")
        out = {k: v.cpu().numpy().astype(np.float64 if k in shapes else np.int32) for k, v in hist.items()} if record else None
        for k, v in abuf.items():
            out[k] = v.cpu().numpy().astype(np.float64)
        tail = tuple(b.cpu().numpy().astype(np.float64) for b in (mbuf, ebuf) if b is not None)
        return (s, c, t, o) if other else (s, c, t), out, tail

    def simulate_(self, steps, dt=0.01, record=False, measured=False, estimated=False):
        """simulate (model_predictive_control.jl:80-100) on the device from the inputs last installed; returns (state, control, t) after `steps`
        steps and, with record=True, the histories qs [steps][B][6], us [steps][B][3] (the values pushed at :88-89).  measured=True (a sensor library is installed)
        appends the measured history [steps][B][6] to what is returned, estimated=True (an estimator library is installed) the estimated history [steps][B][6] behind it.
        Under an actuator library `us` is the APPLIED control, and record=True appends
        {"command": [steps][B][3], "applied": [steps][B][3]} as the last element; under a disturbance library that last dictionary holds "disturbance": w [steps][B][4]
        (it is appended for either library)."""
        def call(ptr, hu, hist):
            self._chk(self.lib.pg_simulate_dev(self.h, steps, C.c_double(dt), ptr(hist.get("state")), ptr(hist.get("control"))), "pg_simulate_dev")
        st, out, tail = self._rollout(steps, record, measured, {"state": (6,), "control": (3,)}, None, call, other=False, estimated=estimated)
        act = {k: out[k] for k in ("command", "applied", "disturbance") if record and k in out}
        act = (act,) if act else ()
        return st + ((out["state"], out["control"]) if record else (None, None)) + tail + act

    def simulate_safety_(self, steps, dt=0.01, use_HJI_policy=True, human="hold", human_u=None, record=False, measured=False, estimated=False):
        """Safety rollout (pg_simulate_safety_dev): simulate with the control the ROS node sends (ros_integration.jl:114-124) fed back, against an other car that moves.
        human: "hold" (omega, a) = (0, 0), "worst" optimal_disturbance (HJI_computation.jl:90-131), "script" human_u [steps][B][2] = (omega, a).  Returns (state, control, t,
        other) after `steps` steps and, with record=True, a dict of histories: state [steps][B][6], control [steps][B][3], other [steps][B][4], human [steps][B][2], V [steps][B],
        source [steps][B] (0 MPC / 1 HJI policy / 2 V <= eps with the policy off) -- the values at the start of each step, and the human control and V of that step.
        measured=True (a sensor library is installed) appends the measured history [steps][B][6] to what is returned, estimated=True (an estimator library is installed) the
        estimated history [steps][B][6] behind it.  Under an actuator library "control" is the APPLIED
        control and the dict also holds "command" and "applied" [steps][B][3]; under a disturbance library it holds "disturbance": w [steps][B][4].  Under a
        human library (set_humans) the sets decide the other car's driver, human_u is the script of their mode-2 sets, and the dict also holds "human_u" [steps][B][2], what
        k_human handed the plant (equal to "human")."""
        def call(ptr, hu, hist):
            self._chk(self.lib.pg_simulate_safety_dev(self.h, int(steps), C.c_double(dt), int(bool(use_HJI_policy)), self.HUMAN_MODES[human], ptr(hu),
                                                      *(ptr(hist.get(k)) for k in ("state", "control", "other", "human", "V", "source"))), "pg_simulate_safety_dev")
        st, out, tail = self._rollout(steps, record, measured, {"state": (6,), "control": (3,), "other": (4,), "human": (2,), "V": ()}, "source", call, human, human_u, estimated=estimated)
        return st + ((out,) if record else ()) + tail

    def safety_summary(self):
        """Per instance since the rollout's clock last restarted: (V_min [B], first_breach [B] (first step index with V <= 0, -1: none), policy_steps [B])."""
        vmin = np.zeros(self.B); fb = np.zeros(self.B, dtype=np.int32); ps = np.zeros(self.B, dtype=np.int32)
        self._chk(self.lib.pg_get_safety_state(self.h, None, _p(vmin), _p(fb, C.POINTER(C.c_int32)), _p(ps, C.POINTER(C.c_int32))), "pg_get_safety_state")
        return vmin, fb, ps

    # ---- from_autobox_callback (ros_integration.jl:48-151) for every instance: pg_node_step_dev / pg_simulate_node_dev ----
    NODE_EVENTS = {"mpc": 0, "hji_policy": 1, "feather": 2, "nan_fallback": 3, "pre_flag_off": 4, "outside_trajectory": 5, "low_speed": 6}

    def _pre_flag_dev(self, pre_flag, shape):
        if pre_flag is None:
            return None
        torch, _, dev = self._torch()
        return torch.as_tensor(np.ascontiguousarray(pre_flag, dtype=np.uint8).reshape(shape)).to(device=dev).contiguous()

    def node_step_(self, use_HJI_policy=False, pre_flag=None):
        """One node callback per instance on the installed inputs (pg_node_step_dev): the installed control is the to_autobox message.  pre_flag [B] (None: engaged).
        Returns (cmd [B][3], se [B][2], event [B], message [B][3]): the published command (NaN where nothing was published), (s, e) of the step's projection, the
        pg_node_event code, and the message after the callback (the installed control now).  The clock does not advance."""
        torch, tdt, dev = self._torch()
        cmd = torch.full((self.B, 3), float("nan"), dtype=tdt, device=dev); se = torch.empty((self.B, 2), dtype=tdt, device=dev)
        ev = torch.empty(self.B, dtype=torch.int32, device=dev)
        pf = self._pre_flag_dev(pre_flag, (self.B,))
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.pg_node_step_dev(self.h, int(bool(use_HJI_policy)), ptr(pf), ptr(cmd), ptr(se), ptr(ev)), "pg_node_step_dev")
        c = np.zeros((self.B, 3))
        self._chk(self.lib.pg_get_state(self.h, None, _p(c), None), "pg_get_state")
        return cmd.cpu().numpy().astype(np.float64), se.cpu().numpy().astype(np.float64), ev.cpu().numpy(), c

    def simulate_node_(self, steps, dt=0.01, use_HJI_policy=False, human="hold", human_u=None, pre_flag=None, record=False, measured=False, estimated=False):
        """The node's closed loop (pg_simulate_node_dev): per step the gates, the compute calls, the callback's decision (NaN fallback included), the ego plant driven by the
        APPLIED command of the step's start, the other car as simulate_safety_.  pre_flag [steps][B] (None: engaged).  Returns (state, message, t, other, applied) after `steps`
        steps and, with record=True, a dict of histories: state [steps][B][6], applied [steps][B][3], V [steps][B], event [steps][B] (pg_node_event).
        measured=True (a sensor library is installed) appends the measured history [steps][B][6] to what is returned, estimated=True (an estimator library is installed) the
        estimated history [steps][B][6] behind it.  Under a disturbance library the dict also holds
        "disturbance": w [steps][B][4], and under a human library (set_humans: the sets decide the driver, human_u is the script of their mode-2 sets) "human_u" [steps][B][2]."""
        def call(ptr, hu, hist):
            pf = self._pre_flag_dev(pre_flag, (steps, self.B))
            self._chk(self.lib.pg_simulate_node_dev(self.h, int(steps), C.c_double(dt), int(bool(use_HJI_policy)), self.HUMAN_MODES[human], ptr(hu), ptr(pf),
                                                    *(ptr(hist.get(k)) for k in ("state", "applied", "event", "V"))), "pg_simulate_node_dev")
        st, out, tail = self._rollout(steps, record, measured, {"state": (6,), "applied": (3,), "V": ()}, "event", call, human, human_u, estimated=estimated)
        a = np.zeros((self.B, 3))
        self._chk(self.lib.pg_get_node_state(self.h, _p(a), None, None), "pg_get_node_state")
        return st + (a,) + ((out,) if record else ()) + tail

    def node_summary(self):
        """(applied [B][3], heartbeat [B], counts [B][4] = steps with pre_flag off / outside the window / low speed / NaN fallback since the clock last restarted)."""
        a = np.zeros((self.B, 3)); hb = np.zeros(self.B, dtype=np.int32); cn = np.zeros((self.B, 4), dtype=np.int32)
        self._chk(self.lib.pg_get_node_state(self.h, _p(a), _p(hb, C.POINTER(C.c_int32)), _p(cn, C.POINTER(C.c_int32))), "pg_get_node_state")
        return a, hb, cn

    def simulate_clock(self, steps, t_start, dt=0.01):
        """The times the rollout's loop variable takes, per instance: (t_start .+ (0:dt:trajectory.t[end]))[1:steps] as Julia's range arithmetic gives them
        (model_predictive_control.jl:87; pg_simulate_clock) -- [steps][B]."""
        ts = _f64(t_start).reshape(-1).copy(); out = np.zeros((steps, len(ts)))
        self._chk(self.lib.pg_simulate_clock(self.h, C.c_double(dt), int(steps), len(ts), _p(ts), _p(out)), "pg_simulate_clock")
        return out

    def synchronize(self):
        self._chk(self.lib.pg_synchronize(self.h), "pg_synchronize")

    def set_stream(self, hip_stream):
        self._chk(self.lib.pg_set_stream(self.h, C.c_void_p(hip_stream)), "pg_set_stream")

    def set_fusion(self, mode):
        """Fused step (update_QP! inside the solve kernel, include/pigeon_mpc.h pg_set_fusion): False / 0 never (the default), True / 1 always, 2 for all-warm batches."""
        self._chk(self.lib.pg_set_fusion(self.h, int(mode)), "pg_set_fusion")

    def set_pipeline(self, mode):
        """Pipelined nodes + update_QP launch for large batches with cold instances (include/pigeon_mpc.h pg_set_pipeline): True / 1 where it applies (default), False / 0 never."""
        self._chk(self.lib.pg_set_pipeline(self.h, int(mode)), "pg_set_pipeline")

    def set_option(self, name, value):
        """Build-defined option of this handle by name (include/pigeon_mpc.h pg_set_option: solver rules, launch shape, lateral-solver tuning)."""
        self._chk(self.lib.pg_set_option(self.h, name.encode(), C.c_double(float(value))), f"pg_set_option({name})")

    def get_option(self, name):
        """Current value of an option, or a read-only launch statistic ("stat_pipelined_launches", ...)."""
        v = C.c_double(0.0)
        self._chk(self.lib.pg_get_option(self.h, name.encode(), C.byref(v)), f"pg_get_option({name})")
        return v.value

    def pipeline_fallbacks(self):
        """Cumulative number of waiting wavefronts of the pipelined nodes + update_QP launch that gave up (the step was then redone launch per phase)."""
        n = C.c_int64(0)
        self._chk(self.lib.pg_get_pipeline_fallbacks(self.h, C.byref(n)), "pg_get_pipeline_fallbacks")
        return int(n.value)

    def phase_ms(self):
        out = (C.c_float * 3)()
        self._chk(self.lib.pg_get_phase_ms(self.h, out), "pg_get_phase_ms")
        return [out[i] for i in range(3)]

    # ---- read-backs ----
    def time_steps(self):
        ts = np.zeros((self.B, self.NN)); dt = np.zeros((self.B, self.N)); pts = np.zeros((self.B, self.NN))
        self._chk(self.lib.pg_get_time_steps(self.h, _p(ts), _p(dt), _p(pts)), "pg_get_time_steps")
        return ts, dt, pts

    def nodes(self):
        qs = np.zeros((self.B, self.NN, 6)); us = np.zeros((self.B, self.NN, 2)); ps = np.zeros((self.B, self.NN, 4))
        self._chk(self.lib.pg_get_nodes(self.h, _p(qs), _p(us), _p(ps)), "pg_get_nodes")
        return qs, us, ps

    def path_coordinates(self):
        sep = np.zeros((self.B, 3))
        self._chk(self.lib.pg_get_path_coordinates(self.h, _p(sep)), "pg_get_path_coordinates")
        return sep

    def qp_data(self, b0=0, n=None):
        n = self.B - b0 if n is None else n
        out = np.zeros((n, self.qp_len))
        self._chk(self.lib.pg_get_qp(self.h, b0, n, _p(out)), "pg_get_qp")
        return out

    def set_qp_data(self, qp, b0=0):
        """Install QP data (layout of qp_data) for instances [b0, b0 + len(qp)): solve_() then solves exactly these problems (include/pigeon_mpc.h pg_set_qp)."""
        q = _f64(qp).reshape(-1, self.qp_len)
        self._chk(self.lib.pg_set_qp(self.h, b0, q.shape[0], _p(q)), "pg_set_qp")

    def solution(self):
        x = np.zeros((self.B, self.NN, 8)); sg = np.zeros((self.B, self.N, 3))
        self._chk(self.lib.pg_get_solution(self.h, _p(x), _p(sg)), "pg_get_solution")
        return x, sg

    def solve_info(self):
        st = np.zeros(self.B, dtype=np.int32); it = np.zeros(self.B, dtype=np.int32); act = np.zeros((self.B, self.N), dtype=np.uint16); mu = np.zeros(self.B)
        self._chk(self.lib.pg_get_solve_info(self.h, _p(st, C.POINTER(C.c_int32)), _p(it, C.POINTER(C.c_int32)), _p(act, C.POINTER(C.c_uint16)), _p(mu)),
                  "pg_get_solve_info")
        return st, it, act, mu

    def polish_info(self):
        """Per instance: 0 polish not run, k >= 1 verified in round k, -1 not verified (interior-point iterate kept)."""
        p = np.zeros(self.B, dtype=np.int32)
        self._chk(self.lib.pg_get_polish_info(self.h, _p(p, C.POINTER(C.c_int32))), "pg_get_polish_info")
        return p

    def multipliers(self):
        """Multipliers of the inequality rows of the last solve [B, N, 16], indexed like the bits of the active masks (include/pigeon_mpc.h pg_get_multipliers)."""
        lam = np.zeros((self.B, self.N, 16))
        self._chk(self.lib.pg_get_multipliers(self.h, _p(lam)), "pg_get_multipliers")
        return lam

    def hji_constraint(self):
        M = np.zeros((self.B, 2)); b = np.zeros(self.B); V = np.zeros(self.B)
        self._chk(self.lib.pg_get_hji_constraint(self.h, _p(M), _p(b), _p(V)), "pg_get_hji_constraint")
        return M, b, V

    def wall_edges(self):
        """(edge_L, edge_R) at nodes 2..N+1 [B, N, 2] (wall extension)"""
        e = np.zeros((self.B, self.N, 2))
        self._chk(self.lib.pg_get_walls(self.h, _p(e)), "pg_get_walls")
        return e

    def hji_lookup(self, x7):
        """cache[x] for a batch of HJIRelativeState rows: HJI_computation.jl:66-72."""
        x = _f64(x7).reshape(-1, 7); B = x.shape[0]
        V = np.zeros(B); g = np.zeros((B, 7))
        self._chk(self.lib.pg_hji_lookup(self.h, B, _p(x), _p(V), _p(g)), "pg_hji_lookup")
        return V, g

    def hji_value_slice(self, q7, colors=False, contour=True):
        """rviz.jl:23-40,60-69 for a batch of relative states: V [B, n1, n2] at every knot pair of grid dimensions 1, 2 (the other five components from q7),
        optionally the marker colours [B, n1, n2, 3] and the zero-level crossings on the grid edges (cross_x [B, n1-1, n2], cross_y [B, n1, n2-1]; NaN = none)."""
        q = _f64(q7).reshape(-1, 7); B = q.shape[0]
        dims = np.zeros(7, dtype=np.int32)
        self._chk(self.lib.pg_hji_grid_dims(self.h, _p(dims, C.POINTER(C.c_int32))), "pg_hji_grid_dims")
        n1, n2 = int(dims[0]), int(dims[1])
        V = np.zeros((B, n1, n2)); rgb = np.zeros((B, n1, n2, 3)) if colors else None
        cx = np.zeros((B, n1 - 1, n2)) if contour else None; cy = np.zeros((B, n1, n2 - 1)) if contour else None
        self._chk(self.lib.pg_hji_slice(self.h, B, _p(q), _p(V), _p(rgb), _p(cx), _p(cy)), "pg_hji_slice")
        return V, rgb, cx, cy

    # ---- canonical active-set indices (row numbering of the reference's QP) ----
    def canonical_active_set(self, b, act_masks, qp_row, lam=None, tol=1e-6):
        """Signed 1-based row indices of the reference QP that are active for instance b: +i upper bound, -i lower bound.
        act_masks: [N] uint16 from solve_info(); qp_row: this instance's pg_get_qp block (for the fixed first node).
        lam: this instance's multipliers [N, 16] (multipliers()[b]): with them the CANONICAL rule applies -- a row is active when its bit is set AND its multiplier
        exceeds tol, the rule oracle.active_set applies to the oracle's multipliers (rows held with a zero multiplier are degenerate: either side is a KKT point)."""
        N, Ns = self.N, self.N_short
        cp = self.control_params
        r_C1 = 0; r_C2 = r_C1 + 2 * N; r_C3 = r_C2 + Ns; r_C4 = r_C3 + N; r_C5 = r_C4 + N; r_C6 = r_C5 + N + 1; r_C7 = r_C6 + N + 1
        r_C8 = r_C7 + N + 1; r_C9 = r_C8 + 6; r_C10 = r_C9 + 2; r_C11 = r_C10 + 6 * Ns; r_C12 = r_C11 + Ns; r_C13 = r_C12 + 6 * self.N_long
        out = []
        nh = min(int(cp["N_HJI"]), Ns)
        # node 1 (fixed): sigma_HJI_1 = max(0, -(M u_1 + b)); its two rows are decided in closed form
        M = qp_row[-3:-1]; bh = qp_row[-1]; u1 = qp_row[-5:-3]
        if nh >= 1 and cp["W_HJI"] > 0:
            if M @ u1 + bh < 0:
                out.append(-(r_C11 + 0 + 1))
            else:
                out.append(-(r_C2 + 0 + 1))
        for k in range(N):
            m = int(act_masks[k]); node = k + 1
            bit = lambda j: ((m >> j) & 1) and (lam is None or lam[k][j] > tol)
            if bit(0): out.append(-(r_C5 + node + 1))
            if bit(1): out.append(+(r_C6 + node + 1))
            if bit(2): out.append(-(r_C7 + node + 1))
            base = r_C13 + 9 * k
            if bit(3): out.append(+(base + 0 + 1))
            if bit(4): out.append(-(base + 1 + 1))
            if bit(5): out.append(+(base + 2 + 1))
            for i in range(4):
                if bit(6 + i): out.append(+(base + 3 + i + 1))
            if bit(10): out.append(-(r_C1 + 2 * k + 0 + 1))
            if bit(11): out.append(-(r_C1 + 2 * k + 1 + 1))
            if bit(12): out.append(+(base + 7 + 1))
            if bit(13): out.append(-(base + 8 + 1))
            if node < nh:
                if bit(14): out.append(-(r_C11 + node + 1))
                if bit(15): out.append(-(r_C2 + node + 1))
        return sorted(out, key=abs)


def CoupledTrajectoryTrackingMPC(vehicle, trajectory, batch_capacity=1, **kw):
    """Name of the reference constructor (coupled_lat_long.jl:42); returns the batched type."""
    return BatchedTrajectoryTrackingMPC(trajectory, batch_capacity, vehicle=vehicle, **kw)


def DecoupledTrajectoryTrackingMPC(vehicle, trajectory, batch_capacity=1, **kw):
    """Name of the reference constructor (decoupled_lat_long.jl:32); returns the batched type."""
    return BatchedTrajectoryTrackingMPC(trajectory, batch_capacity, vehicle=vehicle, formulation="decoupled", **kw)


def decoupled_canonical_active_set(N, N_short, act_masks, walls=False, lam=None, tol=1e-6):
    """Signed 1-based active rows of the reference's LATERAL QP (decoupled_lat_long.jl:166-211 row order) from the per-stage masks (lam [N, 16]: the canonical rule of
    BatchedTrajectoryTrackingMPC.canonical_active_set -- bit set and multiplier > tol).
    With the wall extension the 3N wall rows are numbered after the reference's rows: (e - sw <= edge_L, e + sw >= edge_R, sw >= 0) per node 2..N+1."""
    Ns, Nl = N_short, N - N_short
    r_1 = 0; r_2 = 2 * N; r_3 = r_2 + N; r_4 = r_3 + 4; r_5 = r_4 + 1; r_6 = r_5 + 4 * Ns; r_7 = r_6 + 4 * Nl
    out = []
    for k in range(N):
        m = int(act_masks[k]); base = r_7 + 8 * k
        bit = lambda j: ((m >> j) & 1) and (lam is None or lam[k][j] > tol)
        if bit(3): out.append(+(base + 0 + 1))
        if bit(4): out.append(-(base + 1 + 1))
        for i in range(4):
            if bit(6 + i): out.append(+(base + 2 + i + 1))
        if bit(10): out.append(-(r_1 + 2 * k + 0 + 1))
        if bit(11): out.append(-(r_1 + 2 * k + 1 + 1))
        if bit(12): out.append(+(base + 6 + 1))
        if bit(13): out.append(-(base + 7 + 1))
        if walls:
            r_8 = r_7 + 8 * N
            if bit(0): out.append(+(r_8 + 3 * k + 0 + 1))
            if bit(1): out.append(-(r_8 + 3 * k + 1 + 1))
            if bit(2): out.append(-(r_8 + 3 * k + 2 + 1))
    return sorted(out, key=abs)


def simulate(mpc: BatchedTrajectoryTrackingMPC, plant_step, q0, u0, steps, dt=0.01, t_start=None, time_offset=None):
    """Closed-loop harness with the semantics of simulate (model_predictive_control.jl:80-100): the state is advanced with the
    OLD control, then the control is replaced (one-step actuation delay).  `plant_step(q[B,6], u[B,3], dt) -> q` is supplied by
    the caller (the nonlinear plant is not part of the GPU hot path)."""
    q = _f64(q0).reshape(-1, 6).copy(); u = _f64(u0, q.shape[:1] + (3,)).copy()
    t = np.zeros(q.shape[0]) if t_start is None else _f64(t_start, (q.shape[0],)).copy()
    hist = []
    clock = mpc.simulate_clock(steps, t, dt)          # `for t in 0:dt:trajectory.t[end]` (:87) is a Julia range, not an accumulation
    for k in range(steps):
        hist.append((q.copy(), u.copy()))
        mpc.set_inputs(q, u, clock[k], time_offset=time_offset)
        mpc.compute_time_steps_(); mpc.compute_linearization_nodes_(); mpc.update_QP_(); mpc.solve_()
        q = plant_step(q, u, dt)
        u = mpc.get_next_control()
    return hist
