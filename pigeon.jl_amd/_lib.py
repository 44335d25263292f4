"""ctypes binding of libpigeon_hip.so (C ABI: include/pigeon_mpc.h).  No CPU fallback: a missing library or GPU raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpigeon_hip.so")             # fp64 (the reference's arithmetic type)
LIB_PATH_F32 = os.path.join(_HERE, "csrc", "libpigeon_hip_f32.so")     # fp32 build of the same sources (BASELINE configs 3/4)
LIB_PATH_DIAG = os.path.join(_HERE, "csrc", "libpigeon_hip_diag.so")   # fp64, -DPG_DIAG: fault injection and traces for tests / tools (precision "f64-diag"); never the product
_libs = {}


class PigeonError(RuntimeError):
    pass


class pg_vehicle(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["G", "m", "Izz", "L", "a", "b", "h", "mu", "Caf", "Car", "Cd0", "Cd1", "Cd2", "fwd_frac", "rwd_frac",
                                          "fwb_frac", "rwb_frac", "Fx_max", "Fx_min", "Px_max", "delta_max", "kappa_max"]]


class pg_control_params(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["V_min", "V_max", "k_V", "k_s", "deltadot_max", "Q_ds", "Q_dpsi", "Q_e", "W_beta", "W_r", "W_HJI",
                                          "R_delta", "R_ddelta", "R_Fx", "R_dFx"]] + [("N_HJI", C.c_int32), ("_pad", C.c_int32)]


class pg_config(C.Structure):
    _fields_ = [("vehicle", pg_vehicle), ("control", pg_control_params), ("N_short", C.c_int32), ("N_long", C.c_int32), ("dt_short", C.c_double),
                ("dt_long", C.c_double), ("use_correction_step", C.c_int32), ("rk4_substeps", C.c_int32), ("hji_eps", C.c_double),
                ("batch_capacity", C.c_int32), ("device", C.c_int32), ("ipm_max_iter", C.c_int32), ("formulation", C.c_int32), ("ipm_tol", C.c_double),
                ("ipm_mu0", C.c_double), ("walls", C.c_int32), ("allow_f32_long_lateral", C.c_int32), ("wall_weight", C.c_double),
                ("polish", C.c_int32), ("_pad3", C.c_int32), ("polish_rho", C.c_double), ("polish_tol", C.c_double), ("polish_ipm_tol", C.c_double),
                ("warm_polish", C.c_int32), ("cold_guess", C.c_int32)]


# every symbol include/pigeon_mpc.h declares (tests check that the built library exports each one)
SYMBOLS = ["pg_precision_bits", "pg_abi_layout", "pg_default_config", "pg_default_config_decoupled", "pg_create", "pg_destroy", "pg_last_error", "pg_get_config", "pg_get_u_normalization", "pg_set_trajectory", "pg_set_trajectories", "pg_set_trajectory_index", "pg_default_speed_plan", "pg_plan_speeds", "pg_default_path_segment", "pg_make_paths", "pg_default_waypoint", "pg_fit_paths", "pg_default_offset_set", "pg_offset_paths", "pg_default_obstacle_set", "pg_clip_tubes", "pg_default_refine_set", "pg_refine_paths", "pg_default_smooth_set", "pg_smooth_waypoints", "pg_default_tune_set", "pg_tune_smoothing", "pg_default_line_set", "pg_optimize_line", "pg_default_start_set", "pg_make_starts",
           "pg_set_control_param_sets", "pg_set_control_param_index", "pg_clear_control_param_sets", "pg_get_control_param_sets",
           "pg_set_plant_sets", "pg_set_plant_index", "pg_clear_plant_sets", "pg_get_plant_sets", "pg_get_tracking_state",
           "pg_set_sensor_sets", "pg_set_sensor_index", "pg_set_sensor_seed", "pg_clear_sensor_sets", "pg_get_sensor_sets", "pg_sensor_draws", "pg_get_measured_state", "pg_set_measured_history_dev",
           "pg_set_actuator_sets", "pg_set_actuator_index", "pg_clear_actuator_sets", "pg_get_actuator_sets", "pg_set_applied_history_dev", "pg_set_command_history_dev", "pg_get_actuator_state", "pg_actuator_response",
           "pg_set_disturbance_sets", "pg_set_disturbance_index", "pg_set_disturbance_seed", "pg_clear_disturbance_sets", "pg_get_disturbance_sets", "pg_disturbance_response", "pg_get_disturbance_state", "pg_set_disturbance_history_dev",
           "pg_set_estimator_sets", "pg_set_estimator_index", "pg_clear_estimator_sets", "pg_get_estimator_sets", "pg_get_estimated_state", "pg_set_estimated_history_dev", "pg_estimator_response",
           "pg_set_human_sets", "pg_set_human_index", "pg_set_human_seed", "pg_clear_human_sets", "pg_get_human_sets", "pg_get_human_state", "pg_set_human_history_dev", "pg_human_response",
           "pg_default_route", "pg_set_route_sets", "pg_set_route_index", "pg_clear_route_sets", "pg_get_route_sets", "pg_get_route_state", "pg_set_route_history_dev",
           "pg_set_hji_grid", "pg_clear_hji_grid", "pg_default_hji_solve_opts", "pg_hji_solve", "pg_reset", "pg_set_inputs", "pg_set_inputs_dev", "pg_compute_time_steps",
           "pg_compute_linearization_nodes", "pg_update_qp", "pg_solve", "pg_get_next_control", "pg_get_next_control_dev", "pg_get_next_control_hji", "pg_get_next_control_hji_dev", "pg_step", "pg_step_dev", "pg_simulate_dev", "pg_simulate_clock", "pg_get_state", "pg_simulate_safety_dev", "pg_get_safety_state", "pg_node_step_dev", "pg_simulate_node_dev", "pg_get_node_state",
           "pg_set_stream", "pg_set_fusion", "pg_set_pipeline", "pg_set_option", "pg_get_option", "pg_get_pipeline_fallbacks", "pg_synchronize", "pg_get_time_steps", "pg_get_nodes", "pg_get_path_coordinates", "pg_qp_len", "pg_get_qp", "pg_set_qp", "pg_get_solution",
           "pg_get_solve_info", "pg_get_polish_info", "pg_get_multipliers", "pg_get_phase_ms", "pg_hji_lookup", "pg_hji_lookup_dev", "pg_hji_lookup8_dev", "pg_hji_grid_dims", "pg_hji_slice", "pg_get_hji_constraint", "pg_get_walls"]


def _set_prototypes(name, ctype, seed=False):
    """the prototypes every per-instance library has (pg_set_<name>_sets / _index, pg_clear_<name>_sets, pg_get_<name>_sets), and pg_set_<name>_seed of a seeded one"""
    p = {f"pg_set_{name}_sets": [C.c_void_p, C.c_int32, C.POINTER(ctype)],
         f"pg_set_{name}_index": [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]}
    if seed:
        p[f"pg_set_{name}_seed"] = [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]
    p[f"pg_clear_{name}_sets"] = [C.c_void_p]
    p[f"pg_get_{name}_sets"] = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ctype), C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    return p


# control-parameter library (include/pigeon_mpc.h: pg_set_control_param_sets and its companions)
CONTROL_PARAM_SET_PROTOTYPES = _set_prototypes("control_param", pg_control_params)


# plant library and tracking summary (include/pigeon_mpc.h: pg_set_plant_sets and its companions, pg_get_tracking_state)
PLANT_SET_PROTOTYPES = {
    **_set_prototypes("plant", pg_vehicle),
    "pg_get_tracking_state": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
}


class pg_sensor(C.Structure):
    """include/pigeon_mpc.h pg_sensor: per channel of (E, N, psi, Ux, Uy, r) a standard deviation and a constant bias."""
    _fields_ = [("sigma", C.c_double * 6), ("bias", C.c_double * 6)]


# sensor library (include/pigeon_mpc.h: pg_set_sensor_sets and its companions)
SENSOR_SET_PROTOTYPES = {
    **_set_prototypes("sensor", pg_sensor, seed=True),
    "pg_sensor_draws": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)],
    "pg_get_measured_state": [C.c_void_p, C.POINTER(C.c_double)],
    "pg_set_measured_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
}


PG_ACT_MAX_DELAY = 16


class pg_actuator_set(C.Structure):
    """include/pigeon_mpc.h pg_actuator_set: transport delay in rollout steps, what the controller sees as current_control (0 the command, 1 the actuator's position),
    first-order time constants (s) and slew limits (rad/s, N/s; +Inf = none) of steering and of each longitudinal force channel."""
    _fields_ = [("delay_steps", C.c_int32), ("feedback", C.c_int32), ("tau_delta", C.c_double), ("tau_fx", C.c_double), ("rate_delta", C.c_double), ("rate_fx", C.c_double)]


# actuator library (include/pigeon_mpc.h: pg_set_actuator_sets and its companions)
ACTUATOR_SET_PROTOTYPES = {
    **_set_prototypes("actuator", pg_actuator_set),
    "pg_set_applied_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
    "pg_set_command_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
    "pg_get_actuator_state": [C.c_void_p, C.POINTER(C.c_double)],
    "pg_actuator_response": [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)],
}


class pg_disturbance(C.Structure):
    """include/pigeon_mpc.h pg_disturbance: the window in clock steps (step_off < 0: open-ended), the constant body-frame force (N) and yaw moment (N m), the gust's standard
    deviations (N), the lever arm of its side force (m), its correlation time (s; 0 = white) and the factor on the plant's mu while active."""
    _fields_ = [("step_on", C.c_int32), ("step_off", C.c_int32), ("Fx", C.c_double), ("Fy", C.c_double), ("Mz", C.c_double), ("sigma_Fx", C.c_double), ("sigma_Fy", C.c_double),
                ("x_cp", C.c_double), ("tau_gust", C.c_double), ("mu_scale", C.c_double)]


# disturbance library (include/pigeon_mpc.h: pg_set_disturbance_sets and its companions)
DISTURBANCE_SET_PROTOTYPES = {
    **_set_prototypes("disturbance", pg_disturbance, seed=True),
    "pg_disturbance_response": [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double)],
    "pg_get_disturbance_state": [C.c_void_p, C.POINTER(C.c_double)],
    "pg_set_disturbance_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
}


class pg_estimator(C.Structure):
    """include/pigeon_mpc.h pg_estimator: whether the prior is one step of the controller's model (1) or the previous estimate (0), a reserved word (0) and the fixed gain per
    channel of (E, N, psi, Ux, Uy, r), each in [0, 1]."""
    _fields_ = [("predict", C.c_int32), ("reserved", C.c_int32), ("gain", C.c_double * 6)]


# estimator library (include/pigeon_mpc.h: pg_set_estimator_sets and its companions)
ESTIMATOR_SET_PROTOTYPES = {
    **_set_prototypes("estimator", pg_estimator),
    "pg_get_estimated_state": [C.c_void_p, C.POINTER(C.c_double)],
    "pg_set_estimated_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
    "pg_estimator_response": [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
}

class pg_human(C.Structure):
    """include/pigeon_mpc.h pg_human: the driver model (0 hold, 1 worst case, 2 the caller's script, 3 seeded random), the steps a decision is kept, the window in clock
    steps (step_off < 0: open-ended), the factor on the decided (omega, a), the limits (Inf: none) and the random driver's standard deviations and correlation time."""
    _fields_ = [("mode", C.c_int32), ("hold_steps", C.c_int32), ("step_on", C.c_int32), ("step_off", C.c_int32), ("gain", C.c_double * 2), ("omega_max", C.c_double),
                ("a_min", C.c_double), ("a_max", C.c_double), ("sigma", C.c_double * 2), ("tau", C.c_double)]


# human library (include/pigeon_mpc.h: pg_set_human_sets and its companions)
HUMAN_SET_PROTOTYPES = {
    **_set_prototypes("human", pg_human, seed=True),
    "pg_get_human_state": [C.c_void_p, C.POINTER(C.c_double)],
    "pg_set_human_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
    "pg_human_response": [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
}


PG_ROUTE_EVENTS = 4
PG_ROUTE_ABSOLUTE, PG_ROUTE_RELATIVE = 0, 1
PG_ROUTE_KEEP, PG_ROUTE_PATH, PG_ROUTE_STAMP, PG_ROUTE_PROJECT = 0, 1, 2, 3


class pg_route_event(C.Structure):
    """include/pigeon_mpc.h pg_route_event: the clock step at which it fires (< 0: unused slot), the target and how to read it (0 absolute, 1 relative to the current index),
    the anchor of the new time offset (0 keep, 1 path, 2 stamp, 3 project), whether the instance starts cold, a reserved 0, the seconds into the new trajectory."""
    _fields_ = [("step", C.c_int32), ("target", C.c_int32), ("target_mode", C.c_int32), ("anchor", C.c_int32), ("cold", C.c_int32), ("reserved", C.c_int32), ("t_join", C.c_double)]


class pg_route(C.Structure):
    """include/pigeon_mpc.h pg_route: PG_ROUTE_EVENTS events, the used slots first and in the order of their steps."""
    _fields_ = [("ev", pg_route_event * PG_ROUTE_EVENTS)]


# route library (include/pigeon_mpc.h: pg_set_route_sets and its companions)
ROUTE_SET_PROTOTYPES = {
    **_set_prototypes("route", pg_route),
    "pg_get_route_state": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "pg_set_route_history_dev": [C.c_void_p, C.c_void_p, C.c_int32],
}


PG_HJI_PERIODIC_PSI = 1


class pg_hji_solve_opts(C.Structure):
    """include/pigeon_mpc.h pg_hji_solve_opts: horizon (s), CFL number, a fixed step (0: the CFL rule), the bound on the sweeps, the flags (PG_HJI_PERIODIC_PSI)."""
    _fields_ = [("horizon", C.c_double), ("cfl", C.c_double), ("fixed_dt", C.c_double), ("max_sweeps", C.c_int32), ("flags", C.c_int32)]


class pg_hji_solve_stats(C.Structure):
    """include/pigeon_mpc.h pg_hji_solve_stats."""
    _fields_ = [("sweeps", C.c_int32), ("reached_horizon", C.c_int32), ("bad_sweep", C.c_int32), ("reserved", C.c_int32), ("tau", C.c_double), ("last_dt", C.c_double),
                ("alpha", C.c_double * 7), ("v_min", C.c_double), ("v_max", C.c_double)]


# grid solver (include/pigeon_mpc.h: pg_hji_solve)
HJI_SOLVE_PROTOTYPES = {
    "pg_hji_solve": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(pg_vehicle), C.POINTER(pg_hji_solve_opts), C.c_int32,
                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(pg_hji_solve_stats)],
}


class pg_speed_plan(C.Structure):
    """include/pigeon_mpc.h pg_speed_plan: the share of the friction to use, the speed cap and floor, the end speeds of an open path (NaN: free), the extra caps on the
    tangential (ax_min <= 0 <= ax_max) and lateral acceleration (Inf: none)."""
    _fields_ = [(n, C.c_double) for n in ["mu_scale", "V_max", "V_floor", "V_start", "V_end", "ax_max", "ax_min", "ay_max"]]


class pg_speed_plan_stats(C.Structure):
    """include/pigeon_mpc.h pg_speed_plan_stats: one per output trajectory."""
    _fields_ = [("t_end", C.c_double), ("v_min", C.c_double), ("v_max", C.c_double), ("usage_max", C.c_double),
                ("n_cap", C.c_int32), ("n_accel", C.c_int32), ("n_brake", C.c_int32), ("reserved", C.c_int32)]


# speed planner (include/pigeon_mpc.h: pg_plan_speeds)
SPEED_PLAN_PROTOTYPES = {
    "pg_plan_speeds": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.POINTER(pg_speed_plan),
                       C.POINTER(pg_vehicle), C.c_int32, C.POINTER(C.c_double), C.POINTER(pg_speed_plan_stats)],
}


class pg_path_segment(C.Structure):
    """include/pigeon_mpc.h pg_path_segment: length, curvature at the start and the end (linear in between), the tube edges at the start and the end, a reserved 0."""
    _fields_ = [(n, C.c_double) for n in ["length", "kappa0", "kappa1", "edge_L0", "edge_L1", "edge_R0", "edge_R1", "reserved"]]


class pg_path_spec(C.Structure):
    """include/pigeon_mpc.h pg_path_spec: the pose of knot 0, the constant speed of the profile, the path's range of segments, its knot count and whether the caller calls it closed."""
    _fields_ = [("E0", C.c_double), ("N0", C.c_double), ("psi0", C.c_double), ("V_ref", C.c_double), ("seg0", C.c_int32), ("n_seg", C.c_int32), ("n_knots", C.c_int32),
                ("closed", C.c_int32)]


class pg_path_stats(C.Structure):
    """include/pigeon_mpc.h pg_path_stats: one per path."""
    _fields_ = [(n, C.c_double) for n in ["length", "turn", "closure_pos", "closure_psi", "kappa_abs_max", "ds"]]


# path maker (include/pigeon_mpc.h: pg_make_paths)
PATH_MAKE_PROTOTYPES = {
    "pg_make_paths": [C.c_void_p, C.c_int32, C.POINTER(pg_path_spec), C.c_int32, C.POINTER(pg_path_segment), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                      C.POINTER(C.c_double), C.POINTER(pg_path_stats)],
}


class pg_waypoint(C.Structure):
    """include/pigeon_mpc.h pg_waypoint: a surveyed point (E, N) and the tube edges at it."""
    _fields_ = [(n, C.c_double) for n in ["E", "N", "edge_L", "edge_R"]]


class pg_fit_spec(C.Structure):
    """include/pigeon_mpc.h pg_fit_spec: the constant speed of the profile, the path's range of waypoints, its knot count and whether it is closed (periodic)."""
    _fields_ = [("V_ref", C.c_double), ("wp0", C.c_int32), ("n_wp", C.c_int32), ("n_knots", C.c_int32), ("closed", C.c_int32)]


class pg_fit_stats(C.Structure):
    """include/pigeon_mpc.h pg_fit_stats: one per path -- the six fields of pg_path_stats, the shortest and the longest chord, what the inversion left, a reserved 0."""
    _fields_ = [(n, C.c_double) for n in ["length", "turn", "closure_pos", "closure_psi", "kappa_abs_max", "ds", "chord_min", "chord_max", "s_err_max", "reserved"]]


# path fitter (include/pigeon_mpc.h: pg_fit_paths)
PATH_FIT_PROTOTYPES = {
    "pg_fit_paths": [C.c_void_p, C.c_int32, C.POINTER(pg_fit_spec), C.c_int32, C.POINTER(pg_waypoint), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                     C.POINTER(C.c_double), C.POINTER(pg_fit_stats)],
}


class pg_offset_set(C.Structure):
    """include/pigeon_mpc.h pg_offset_set: the offset outside the windows and on the plateau (m, left positive), the rise and the fall window in the source's arc length
    (a start of +Inf: no such window), the smallest 1 - kappa d a pair may reach, how the edges follow (0 the same road, 1 the tube travels with the path), a reserved 0."""
    _fields_ = [(n, C.c_double) for n in ["d0", "d1", "s_a", "s_b", "s_c", "s_d", "x_min"]] + [("edge_mode", C.c_int32), ("reserved", C.c_int32)]


class pg_offset_stats(C.Structure):
    """include/pigeon_mpc.h pg_offset_stats: one per output trajectory."""
    _fields_ = [(n, C.c_double) for n in ["length", "ds_min", "ds_max", "kappa_abs_max", "x_min", "d_abs_max", "closure_pos"]] + [("n_outside", C.c_int32), ("reserved", C.c_int32)]


# path offsetter (include/pigeon_mpc.h: pg_offset_paths)
PATH_OFFSET_PROTOTYPES = {
    "pg_offset_paths": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.POINTER(pg_offset_set), C.c_int32,
                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(pg_offset_stats)],
}


class pg_obstacle(C.Structure):
    """include/pigeon_mpc.h pg_obstacle: a disc in the world frame, a reserved 0."""
    _fields_ = [(n, C.c_double) for n in ["E", "N", "radius", "reserved"]]


class pg_obstacle_set(C.Structure):
    """include/pigeon_mpc.h pg_obstacle_set: the range of the call's obstacle array, the margin added to every radius, the taper (m of edge per m of arc length; +Inf: none),
    the width below which a knot counts as blocked, the side policy (0 centre, 1 wider, 2 pass left, 3 pass right), zeros."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("margin", C.c_double), ("taper", C.c_double), ("min_width", C.c_double), ("policy", C.c_int32), ("reserved", C.c_int32),
                ("pad", C.c_double * 3)]


class pg_clip_stats(C.Structure):
    """include/pigeon_mpc.h pg_clip_stats: one per output trajectory."""
    _fields_ = [("width_min", C.c_double), ("u_width_min", C.c_double), ("reserved_d", C.c_double * 2)] + [(n, C.c_int32) for n in ["n_clip_L", "n_clip_R", "n_blocked", "n_centre_out", "n_seen", "n_ignored"]] + [("reserved", C.c_int32 * 2)]


class pg_obstacle_report(C.Structure):
    """include/pigeon_mpc.h pg_obstacle_report: one per (output trajectory, obstacle slot)."""
    _fields_ = [(n, C.c_double) for n in ["u_at", "a_at", "h_at", "dist_at", "free_left", "free_right"]] + [(n, C.c_int32) for n in ["k_at", "k_first", "k_last", "side"]]


# tube clipper (include/pigeon_mpc.h: pg_clip_tubes)
TUBE_CLIP_PROTOTYPES = {
    "pg_clip_tubes": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.POINTER(pg_obstacle_set), C.c_int32,
                      C.POINTER(pg_obstacle), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(pg_clip_stats), C.POINTER(pg_obstacle_report)],
}


class pg_refine_set(C.Structure):
    """include/pigeon_mpc.h pg_refine_set: the largest spacing wanted everywhere (+Inf: none), up to four windows in the source's arc length (s_lo = +Inf: unused) with the
    largest spacing wanted inside each, three reserved zeros."""
    _fields_ = [("ds", C.c_double), ("s_lo", C.c_double * 4), ("s_hi", C.c_double * 4), ("ds_w", C.c_double * 4), ("reserved", C.c_double * 3)]


class pg_refine_stats(C.Structure):
    """include/pigeon_mpc.h pg_refine_stats: one per output trajectory."""
    _fields_ = [(n, C.c_double) for n in ["length", "ds_min", "ds_max", "closure_pos_max", "closure_psi_max", "kappa_abs_max"]] + [("n_added", C.c_int32), ("m_max", C.c_int32), ("reserved", C.c_double)]


# path refiner (include/pigeon_mpc.h: pg_refine_paths)
PATH_REFINE_PROTOTYPES = {
    "pg_refine_paths": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.POINTER(pg_refine_set), C.c_int32, C.c_int32,
                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(pg_refine_stats)],
}


class pg_smooth_set(C.Structure):
    """include/pigeon_mpc.h pg_smooth_set: lambda (m^3), up to four windows in the path's cumulative chord length with the inverse weight inside each, the flags."""
    _fields_ = [("lam", C.c_double), ("u_lo", C.c_double * 4), ("u_hi", C.c_double * 4), ("factor", C.c_double * 4), ("n_win", C.c_int32), ("pin_ends", C.c_int32),
                ("keep_walls", C.c_int32), ("reserved", C.c_int32)]       # (lam: the header's `lambda`, a Python keyword)


class pg_smooth_stats(C.Structure):
    """include/pigeon_mpc.h pg_smooth_stats: one per (path, set) pair."""
    _fields_ = [(n, C.c_double) for n in ["dev_max", "dev_rms", "i_dev_max", "bend", "n_outside", "width_min", "pivot_min", "chord_min", "reserved"]]


# waypoint smoother (include/pigeon_mpc.h: pg_smooth_waypoints)
WP_SMOOTH_PROTOTYPES = {
    "pg_smooth_waypoints": [C.c_void_p, C.c_int32, C.POINTER(pg_fit_spec), C.c_int32, C.POINTER(pg_waypoint), C.c_int32, C.POINTER(pg_smooth_set), C.POINTER(pg_waypoint),
                            C.POINTER(pg_smooth_stats)],
}


class pg_tune_set(C.Structure):
    """include/pigeon_mpc.h pg_tune_set: the smoothing set without a weight, the dev_rms not to exceed, the first bracket of lambda and the rounds."""
    _fields_ = [("base", pg_smooth_set), ("target", C.c_double), ("lambda_lo", C.c_double), ("lambda_hi", C.c_double), ("rounds", C.c_int32), ("reserved", C.c_int32)]


class pg_tune_stats(C.Structure):
    """include/pigeon_mpc.h pg_tune_stats: one per (path, set) pair."""
    _fields_ = [(n, C.c_double) for n in ["lam", "lo", "hi", "rms_lo", "rms_hi", "verdict", "rounds_done", "monotone", "reserved"]]      # (lam: the header's `lambda`)


# smoothing weight search (include/pigeon_mpc.h: pg_tune_smoothing)
WP_TUNE_PROTOTYPES = {
    "pg_tune_smoothing": [C.c_void_p, C.c_int32, C.POINTER(pg_fit_spec), C.c_int32, C.POINTER(pg_waypoint), C.c_int32, C.POINTER(pg_tune_set), C.POINTER(pg_waypoint),
                          C.POINTER(pg_smooth_stats), C.POINTER(pg_tune_stats)],
}


class pg_line_set(C.Structure):
    """include/pigeon_mpc.h pg_line_set: the regularisation and the ADMM penalty (1/m^3), the margin to the edges, the largest move, the stopping tolerance, up to four
    windows in the path's cumulative chord length with their own margin or a pin, the iteration count and the flags."""
    _fields_ = [("mu", C.c_double), ("rho", C.c_double), ("margin", C.c_double), ("alpha_max", C.c_double), ("tol", C.c_double), ("u_lo", C.c_double * 4), ("u_hi", C.c_double * 4),
                ("win_margin", C.c_double * 4), ("win_pin", C.c_int32 * 4), ("iters", C.c_int32), ("n_win", C.c_int32), ("pin_ends", C.c_int32), ("keep_walls", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class pg_line_stats(C.Structure):
    """include/pigeon_mpc.h pg_line_stats: one per (path, set) pair."""
    _fields_ = [(n, C.c_double) for n in ["bend_in", "bend_out", "alpha_abs_max", "i_alpha_max", "n_active", "r_prim", "r_dual", "iters_done", "pivot_min", "chord_min", "width_min",
                                          "reserved"]]


# line optimiser (include/pigeon_mpc.h: pg_optimize_line)
LINE_OPT_PROTOTYPES = {
    "pg_optimize_line": [C.c_void_p, C.c_int32, C.POINTER(pg_fit_spec), C.c_int32, C.POINTER(pg_waypoint), C.c_int32, C.POINTER(pg_line_set), C.POINTER(pg_waypoint),
                         C.POINTER(pg_line_stats)],
}


START_RANGES = ["s", "e", "dpsi", "v", "uy", "dr", "delta", "fx", "dt0", "other_dx", "other_dy", "other_dpsi", "other_v"]      # the 13 channels of the draws, in their order
START_MODES = ["s_mode", "e_mode", "steady", "time_mode", "other_mode"]


class pg_start_set(C.Structure):
    """include/pigeon_mpc.h pg_start_set: 13 uniform ranges (lo, hi) -- arclength, lateral offset, heading offset, factor on V(s), offsets on Uy, r, delta, Fx and t0, the
    other car in the ego frame -- and the modes (s as a fraction, e as a fraction of the tube, steady-state body state, path mode, other car on), three reserved zeros."""
    _fields_ = [(f"{n}_{end}", C.c_double) for n in START_RANGES for end in ("lo", "hi")] + [(n, C.c_int32) for n in START_MODES] + [("reserved", C.c_int32 * 3)]


# start maker (include/pigeon_mpc.h: pg_make_starts)
START_MAKE_PROTOTYPES = {
    "pg_make_starts": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(pg_start_set), C.POINTER(C.c_int32), C.c_uint64, C.POINTER(C.c_uint64), C.c_int32] + [C.POINTER(C.c_double)] * 6,
}


# device-resident entry points (include/pigeon_mpc.h: pg_set_inputs_dev, pg_step_dev, pg_get_next_control*_dev, pg_hji_lookup*_dev): every array is a raw device address
DEVICE_RESIDENT_PROTOTYPES = {
    "pg_set_inputs_dev": [C.c_void_p, C.c_int32] + [C.c_void_p] * 5,
    "pg_step_dev": [C.c_void_p, C.c_void_p],
    "pg_get_next_control_dev": [C.c_void_p, C.c_void_p],
    "pg_get_next_control_hji_dev": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
    "pg_hji_lookup_dev": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "pg_hji_lookup8_dev": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
}


def load_library(precision="f64"):
    """Loads the HIP library of the requested arithmetic type.  PyTorch-ROCm is imported first so that both share ONE HIP runtime in this process."""
    assert precision in ("f64", "f32", "f64-diag")
    if precision in _libs:
        return _libs[precision]
    path = {"f64": LIB_PATH, "f32": LIB_PATH_F32, "f64-diag": LIB_PATH_DIAG}[precision]
    # A/B runs of an experimental build select it here (PIGEON_HIP_LIB / PIGEON_HIP_LIB_F32 = path of the .so) instead of copying it over the shipped library
    # (read by this Python mirror only: the C library itself reads nothing from the environment)
    path = os.environ.get({"f64": "PIGEON_HIP_LIB", "f32": "PIGEON_HIP_LIB_F32", "f64-diag": "PIGEON_HIP_LIB_DIAG"}[precision], path)
    if not os.path.exists(path):
        raise PigeonError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
    try:
        import torch  # noqa: F401  (plumbing: device memory / streams / torch.distributed live in the same HIP runtime)
    except Exception:
        pass
    lib = C.CDLL(path)
    lib.pg_last_error.restype = C.c_char_p
    lib.pg_last_error.argtypes = [C.c_void_p]
    for s in SYMBOLS:
        getattr(lib, s)
    for prototypes in (CONTROL_PARAM_SET_PROTOTYPES, PLANT_SET_PROTOTYPES, SENSOR_SET_PROTOTYPES, ACTUATOR_SET_PROTOTYPES, DISTURBANCE_SET_PROTOTYPES, ESTIMATOR_SET_PROTOTYPES,
                       HUMAN_SET_PROTOTYPES, ROUTE_SET_PROTOTYPES, HJI_SOLVE_PROTOTYPES, SPEED_PLAN_PROTOTYPES, PATH_MAKE_PROTOTYPES, PATH_FIT_PROTOTYPES, PATH_OFFSET_PROTOTYPES, TUBE_CLIP_PROTOTYPES, PATH_REFINE_PROTOTYPES, WP_SMOOTH_PROTOTYPES, LINE_OPT_PROTOTYPES, START_MAKE_PROTOTYPES, DEVICE_RESIDENT_PROTOTYPES):
        for name, argtypes in prototypes.items():
            getattr(lib, name).argtypes = argtypes
            getattr(lib, name).restype = C.c_int
    lib.pg_default_hji_solve_opts.argtypes = []
    lib.pg_default_hji_solve_opts.restype = pg_hji_solve_opts
    lib.pg_default_speed_plan.argtypes = []
    lib.pg_default_speed_plan.restype = pg_speed_plan
    lib.pg_default_path_segment.argtypes = []
    lib.pg_default_path_segment.restype = pg_path_segment
    lib.pg_default_waypoint.argtypes = []
    lib.pg_default_waypoint.restype = pg_waypoint
    lib.pg_default_offset_set.argtypes = []
    lib.pg_default_offset_set.restype = pg_offset_set
    lib.pg_default_obstacle_set.argtypes = []
    lib.pg_default_obstacle_set.restype = pg_obstacle_set
    lib.pg_default_refine_set.argtypes = []
    lib.pg_default_refine_set.restype = pg_refine_set
    lib.pg_default_smooth_set.argtypes = []
    lib.pg_default_smooth_set.restype = pg_smooth_set
    lib.pg_default_tune_set.argtypes = []
    lib.pg_default_tune_set.restype = pg_tune_set
    lib.pg_default_line_set.argtypes = []
    lib.pg_default_line_set.restype = pg_line_set
    lib.pg_default_start_set.argtypes = []
    lib.pg_default_start_set.restype = pg_start_set
    lib.pg_default_route.argtypes = []
    lib.pg_default_route.restype = pg_route
    assert lib.pg_precision_bits() == (32 if precision == "f32" else 64)
    check_layout(lib)
    _libs[precision] = lib
    return lib


LAYOUT_FIELDS = ["control", "N_short", "dt_short", "use_correction_step", "hji_eps", "batch_capacity", "ipm_max_iter", "formulation", "ipm_tol", "ipm_mu0", "walls", "wall_weight",
                 "polish", "polish_rho", "polish_tol", "polish_ipm_tol", "warm_polish", "cold_guess"]


def mirror_layout():
    """The numbers pg_abi_layout reports, computed from the ctypes mirrors above."""
    return [C.sizeof(pg_config), C.sizeof(pg_vehicle), C.sizeof(pg_control_params)] + [getattr(pg_config, f).offset for f in LAYOUT_FIELDS] + \
           [pg_control_params.N_HJI.offset, pg_vehicle.kappa_max.offset]


def check_layout(lib):
    """The ctypes structs are a hand copy of include/pigeon_mpc.h: refuse to run against a library whose struct layout differs."""
    n = lib.pg_abi_layout(None, 0)
    out = (C.c_int32 * n)()
    lib.pg_abi_layout(out, n)
    if list(out) != mirror_layout():
        raise PigeonError(f"struct layout of the ctypes mirror {mirror_layout()} differs from the library's {list(out)}: update pigeon.jl_amd/_lib.py to include/pigeon_mpc.h")


def check(lib, h, rc, what):
    if rc != 0:
        msg = lib.pg_last_error(h)
        raise PigeonError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")
