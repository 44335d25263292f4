/*
 * pigeon_mpc.h — C ABI of the MI355X-native batched MPC hot path (libpigeon_hip.so).
 *
 * The reference (StanfordASL/Pigeon.jl) has NO FFI for this path; its seam is a Julia call convention: five generic
 * functions applied in fixed order to a mutable TrajectoryTrackingMPC
 *   compute_time_steps!(mpc, t)          src/model_predictive_control.jl:70   (-> :17-30)
 *   compute_linearization_nodes!(mpc)    src/model_predictive_control.jl:72   (-> src/coupled_lat_long.jl:62-142)
 *   update_QP!(mpc)                      src/model_predictive_control.jl:74   (-> src/coupled_lat_long.jl:315-368)
 *   solve!(mpc)                          src/model_predictive_control.jl:76   (-> Parametron -> OSQP, third-party)
 *   get_next_control(mpc)                src/model_predictive_control.jl:78   (-> src/coupled_lat_long.jl:370-374)
 * called from src/ros_integration.jl:96-99,124 and src/model_predictive_control.jl:90-95.  Each entry point below names
 * the reference interface it replaces.  A batch of B independent MPC instances shares one handle (one vehicle for the
 * controller -- the PLANT of the rollouts may differ per instance, pg_set_plant_sets --, one HJI grid; one reference trajectory or a library of them with a per-instance selection, pg_set_trajectories; one set
 * of control parameters or a library of sets with a per-instance selection, pg_set_control_param_sets); per-instance
 * persistent state (solved flag, previous time grid, previous primal solution) lives in device memory inside the handle.
 *
 * Conventions: every function returns 0 on success or a negative pg_status; no exceptions cross the ABI; all
 * arrays are instance-major ("array of structs": state[b*6 + k]) in double precision; pointers are HOST pointers
 * unless the parameter name ends in _dev.  One handle per host thread and device.
 *
 * Two builds export this same ABI: libpigeon_hip.so computes the path in fp64 (the reference's type), libpigeon_hip_f32.so in fp32
 * (BASELINE configs 3/4).  Host arrays are double in both; DEVICE arrays of path data (pg_real_dev) have the library's own element
 * type, which pg_precision_bits() reports (64 or 32).  Absolute times (t0, time_offset, the time grid) are double in both builds.
 */
#ifndef PIGEON_MPC_H
#define PIGEON_MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pg_handle pg_handle;
typedef void pg_real_dev;       /* device array of double (libpigeon_hip.so) or float (libpigeon_hip_f32.so) */
/* 64 for libpigeon_hip.so, 32 for libpigeon_hip_f32.so */
int pg_precision_bits(void);

enum pg_status {
    PG_OK = 0,
    PG_ERR_NO_DEVICE = -1,      /* HIP runtime found no usable gfx950 device: the product path NEVER falls back to a CPU */
    PG_ERR_INVALID = -2,        /* bad argument (null pointer, B > capacity, L < 2, ...) */
    PG_ERR_HIP = -3,            /* a HIP call failed; pg_last_error() has the text */
    PG_ERR_STATE = -4           /* call order violated (e.g. no trajectory installed) */
};

/* per-instance solver status words written by pg_solve (the reference never inspects OSQP's status,
 * src/ros_integration.jl:127 "TODO"; the NaN fallback of :134-147 is reproduced by the caller from these) */
enum pg_solve_status {
    PG_SOLVED = 1,
    PG_MAX_ITER = 2,            /* iteration cap reached before the tolerances were met */
    PG_NUMERICAL = 3,           /* NaN/Inf met in the data or the iterates (e.g. the H4 hazard: other-car speed 0) */
    PG_INFEASIBLE_X0 = 4,       /* a hard bound on the fixed first node is violated (Ux_1 outside [V_min,V_max], Fx_1 < Fx_min) */
    PG_SOLVED_UNVERIFIED = 5    /* (polish on) the interior point met its tolerances but NO active-set round verified a KKT point (pg_get_polish_info = -1): the control is
                                 * the interior-point iterate at its rounding floor -- within 1e-6 of the optimum on every tracking batch tested, up to 2e-3 off in the wide
                                 * random regime of tests/test_gpu_fuzz.py.  A caller that treats it like PG_SOLVED gets round-2 behaviour; with polish = 0 the interior
                                 * point's own convergence is all there is and the status stays PG_SOLVED */
};
/* "the solver returned an answer that met its tolerances" (verified or not): what a caller that used to test status == PG_SOLVED most likely means, e.g. the `solved`
 * decision of the ROS loop (src/ros_integration.jl:127-147).  With the polish on, ~1 % of the N = 50 lateral benchmark instances end PG_SOLVED_UNVERIFIED.
 * (The warm start of the next step accepts both in k_solve_lat; k_solve, the coupled solver, starts an unverified instance cold: its multipliers at hand-over
 * belong to a working set that did not verify.) */
#define PG_IS_SOLVED(st) ((st) == PG_SOLVED || (st) == PG_SOLVED_UNVERIFIED)

/* vehicle dictionary: src/vehicles.jl:1-59; field sets of src/vehicle_dynamics.jl:7-29,272-292 */
typedef struct pg_vehicle {
    double G, m, Izz, L, a, b, h, mu, Caf, Car, Cd0, Cd1, Cd2;
    double fwd_frac, rwd_frac, fwb_frac, rwb_frac;
    double Fx_max, Fx_min, Px_max, delta_max, kappa_max;
} pg_vehicle;

/* CoupledControlParams: src/coupled_lat_long.jl:1-40 */
typedef struct pg_control_params {
    double V_min, V_max, k_V, k_s, deltadot_max;
    double Q_ds, Q_dpsi, Q_e, W_beta, W_r, W_HJI;
    double R_delta, R_ddelta, R_Fx, R_dFx;
    int32_t N_HJI;
    int32_t _pad;
} pg_control_params;

/* keyword arguments of CoupledTrajectoryTrackingMPC (src/coupled_lat_long.jl:42-43) + build-defined knobs */
typedef struct pg_config {
    pg_vehicle vehicle;
    pg_control_params control;
    int32_t N_short, N_long;        /* default 10, 20 */
    double dt_short, dt_long;       /* default 0.01, 0.2 */
    int32_t use_correction_step;    /* default 1 */
    int32_t rk4_substeps;           /* sub-steps of the RK4 `propagate` inside linearize (third-party default 10) */
    double hji_eps;                 /* HJI_eps, src/model_predictive_control.jl:67 (0.05) */
    int32_t batch_capacity;         /* maximum B */
    int32_t device;                 /* HIP device ordinal */
    int32_t ipm_max_iter;           /* interior-point iteration cap (default 40) */
    int32_t formulation;            /* PG_COUPLED (src/coupled_lat_long.jl) or PG_DECOUPLED (src/decoupled_lat_long.jl) */
    double ipm_tol;                 /* complementarity / infeasibility tolerance of the interior point (default 1e-12 in the fp64 library, 1e-5 in the fp32 one) */
    double ipm_mu0;                 /* initial barrier parameter (default 100) */
    int32_t walls;                  /* BUILD-DEFINED EXTENSION (BASELINE config 5 "both_walls"; the reference snapshot carries edge_L/edge_R through
                                     * TrajectoryTube, src/trajectories.jl:19-20,33, but no constraint reads them, README.md:54): 1 adds to the DECOUPLED
                                     * formulation, at nodes t = 2..N+1, the rows  e_t <= edge_L(s_t) + sw_t,  e_t >= edge_R(s_t) - sw_t,  sw_t >= 0  and the
                                     * cost  wall_weight * dt_t * sw_t  (soft, like the stability-envelope rows of :193-211); 0 (default) = the reference's QP */
    int32_t allow_f32_long_lateral; /* (occupies what was explicit padding up to round 5: the layout is unchanged, pg_default_config* zero it)  The fp32 library REFUSES the decoupled
                                     * formulation with more than 32 intervals at pg_create unless this is 1: single precision on the open-loop unstable 8 s lateral horizon solves
                                     * 99.7 % of the N = 50 benchmark batch with the applied steering up to 6e-3 rad off the exact optimum -- fp64 is the precision
                                     * for that configuration, and a caller has to ask for the other one explicitly.  Ignored by the fp64 library */
    double wall_weight;             /* linear penalty on the wall slack per second (default 1000) */
    int32_t polish;                 /* 1 (default, both formulations): after the interior point has converged, an active-set polish (OSQP's `polish`, off in the reference's settings,
                                     * src/coupled_lat_long.jl:201-203) solves the equality-constrained problem on the detected active set with the same Riccati passes
                                     * and verifies primal/dual feasibility; removes the sqrt(mu) error of nearly degenerate rows.  0 = interior-point iterate as is */
    int32_t _pad3;
    double polish_rho;              /* penalty on the active rows inside the polish solves (default 1e7 in the fp64 library, 1e3 in the fp32 one; k_solve_lat, the lateral formulation's kernel for
                                     * horizons beyond 20 intervals, multiplies it by 1e3 in fp64: see pg_solve_lat.hip) */
    double polish_tol;              /* feasibility tolerance of the polish verification (default 1e-9 / 1e-4) */
    double polish_ipm_tol;          /* with polish = 1 the interior point first stops at this (looser) tolerance and hands over to the polish (default 3e-6 / 1e-4);
                                     * if the polish cannot verify an active set from there (or the sets cycle), the interior point resumes down to ipm_tol and the polish
                                     * gets a second and last chance; if that fails too the interior-point iterate is the answer, exactly as with polish = 0.
                                     * Values <= ipm_tol disable the early hand-over */
    int32_t warm_polish;            /* 1 (default): an instance whose previous step ended in a solved QP (solved flag set, status PG_SOLVED -- the lateral kernel also accepts PG_SOLVED_UNVERIFIED) first tries the polish from that
                                     * step's active set and multipliers on the new QP data -- the counterpart of the reference's OSQP warm start
                                     * (src/coupled_lat_long.jl:218).  A verified round is the exact optimum of the new QP (iters = 0 then); otherwise the interior point runs
                                     * as for a cold instance.  Ignored when polish = 0 */
    int32_t cold_guess;             /* rounds (default 8; 0 = off) a COLD instance may spend on the polish started from the EMPTY active set before the interior point is
                                     * called: round 1 is the unconstrained LQ optimum, violated rows join the set, rows with negative multipliers leave it.  A verified round
                                     * is the exact optimum (iters = 0 then), as for the warm start; most instances of a tracking problem have a handful of active rows and
                                     * verify within 1-4 rounds (a rate-limited steering ramp: up to ~10), each the price of one interior-point iteration.  Instances whose rounds do not verify (or cycle) run the
                                     * interior point exactly as with cold_guess = 0.  Ignored when polish = 0 */
} pg_config;

enum pg_formulation { PG_COUPLED = 0, PG_DECOUPLED = 1 };

/* Layout check for hand-written mirrors of this header (ctypes, Julia): fills out[0..] with sizeof(pg_config), sizeof(pg_vehicle), sizeof(pg_control_params)
 * and the byte offsets inside pg_config of: control, N_short, dt_short, use_correction_step, hji_eps, batch_capacity, ipm_max_iter, formulation, ipm_tol, ipm_mu0,
 * walls, wall_weight, polish, polish_rho, polish_tol, polish_ipm_tol, warm_polish, cold_guess; then offsetof(pg_control_params, N_HJI) and offsetof(pg_vehicle, kappa_max).
 * Returns the number of entries (23); out may be NULL, at most n entries are written. */
int pg_abi_layout(int32_t* out, int32_t n);

/* X1() and the default keyword values of the reference constructors (coupled formulation) */
int pg_default_config(pg_config* cfg);
/* DecoupledTrajectoryTrackingMPC(vehicle, trajectory; ...) defaults: src/decoupled_lat_long.jl:18-33.  The lateral formulation uses the
 * fields V_min, V_max, k_V, k_s, deltadot_max, Q_dpsi, Q_e, W_beta, W_r, R_delta, R_ddelta of pg_control_params; delta is NOT normalised
 * (pg_get_u_normalization returns (1,1)); pg_get_next_control returns delta from the QP and Fx from the seeded node 2 (:275-278).
 * The warm branch of the NODES does not exist in this formulation (:52-104 always re-seeds); the solver warm-starts (WarmStart = true, :139: pg_config.warm_polish).
 * The HJI row is not part of it. */
int pg_default_config_decoupled(pg_config* cfg);

/* CoupledTrajectoryTrackingMPC(vehicle, trajectory; ...)  src/coupled_lat_long.jl:42-60 (trajectory installed separately) */
int pg_create(const pg_config* cfg, pg_handle** out);
int pg_destroy(pg_handle* h);
const char* pg_last_error(const pg_handle* h);
int pg_get_config(const pg_handle* h, pg_config* out);
/* u_normalization, src/coupled_lat_long.jl:199 */
int pg_get_u_normalization(const pg_handle* h, double out[2]);

/* mpc.trajectory = TrajectoryTube(t,s,V,A,E,N,psi,kappa,theta,phi,edge_L,edge_R)  src/trajectories.jl:8-44; src/ros_integration.jl:53 */
int pg_set_trajectory(pg_handle* h, int32_t L, const double* t, const double* s, const double* V, const double* A, const double* E,
                      const double* N, const double* psi, const double* kappa, const double* theta, const double* phi,
                      const double* edge_L, const double* edge_R);
/* Batched form of the same assignment when instances track DIFFERENT references (one controller per (x0, reference trajectory) pair,
 * src/model_predictive_control.jl:36 `trajectory::TrajectoryTube{T}` is a per-controller field): install a library of n_traj tubes once,
 * then select one per instance.  channels is [n_traj][10][Lmax] doubles, channel order t, s, V, A, E, N, psi, kappa, edge_L, edge_R
 * (src/trajectories.jl:8-21); L[k] <= Lmax is the node count of trajectory k (the tail of a shorter one is ignored).
 * pg_set_trajectory(...) == a library of one; installing a library drops any previous index. */
int pg_set_trajectories(pg_handle* h, int32_t n_traj, int32_t Lmax, const int32_t* L, const double* channels);
/* index[b] in [0, n_traj): the trajectory instance b tracks.  Persistent across steps until the library or the index is replaced.
 * With n_traj > 1 the phase calls return PG_ERR_STATE until an index covering the current batch is installed. */
int pg_set_trajectory_index(pg_handle* h, int32_t B, const int32_t* index);

/* Making the speed profile: friction-limited V, A and t of every (path, plan set) pair of a path library and a library of plan sets, computed on the device in the
 * layout pg_set_trajectories takes.  The reference takes UxDes / AxDes as its path message gives them (src/ros_integration.jl:13-16) from a planner outside its tree, so
 * the scheme is build-defined (tests/speed_plan_numpy.py is its numpy twin).  It works on W = V^2, all arithmetic in the library's element type, every operation rounded
 * on its own; only t is accumulated in double and rounded on store.  No grade force, as the plant applies none (src/vehicle_dynamics.jl:122).
 *   Limits    a_lim = mu_scale vehicle.mu vehicle.G, ay = min(a_lim, ay_max);  cap_i = max(V_floor^2, min(V_max^2, ay / |kappa_i|)), V_max^2 where kappa_i = 0;
 *             along(W, kappa) = sqrt(max(a_lim^2 - (W kappa)^2, 0));  Fd(V) = Cd0 + V (Cd1 + Cd2 V), V = sqrt(W);
 *             acc(W, kappa) = min((min(m along, Fx_max, Px_max / V) - Fd) / m, ax_max);  dec(W, kappa) = max(min((min(m along, -Fx_min) + Fd) / m, -ax_min), 0).
 *   Open      W_i = cap_i, the first / last knot lowered to max(V_start, V_floor)^2 / max(V_end, V_floor)^2 when given (never above the cap).
 *             Backward, i = L-2 .. 0: W_i = min(W_i, W_{i+1} + 2 ds_i dec(W_{i+1}, kappa_{i+1})), ds_i = s_{i+1} - s_i.
 *             Forward, i = 0 .. L-2: W_{i+1} = min(W_{i+1}, max(W_i + 2 ds_i acc(W_i, kappa_i), V_floor^2)).
 *   Closed    knot L-1 is knot 0 again.  Both passes start at i0, the first knot of largest |kappa| among knots 0 .. L-2 (the smallest cap: W = cap stays there), and
 *             go once around modulo L-1 in L-2 steps -- knot i0 itself is not revisited --, the wrap interval being s_{L-1} - s_{L-2}.  W_{L-1} = W_0 at the end.
 *             V_start / V_end are ignored.
 *   Result    V = sqrt(W);  A_i = (W_{i+1} - W_i) / (2 ds_i), A_{L-1} = 0 (open) or A_0 (closed);  t_0 = 0, t_{i+1} = t_i + 2 ds_i / (V_i + V_{i+1}) (math.jl:2).
 *             The limiter of a knot is the last pass that lowered it, else the cap (knot L-1 of a closed path: that of knot 0).
 * The scheme is explicit -- dec and acc are evaluated at the knot the pass comes from --, so the result may use slightly more than a_lim between two knots of different
 * curvature: usage_max reports it -- measured at V_max 20: 1.05-1.08 on the committed ovals and vail (knots 0.10-0.24 m apart), 1.19 on variable_speed (28 knots about
 * 2 m apart) at mu_scale 0.5, 0 on the straight lines (EXPERIMENTS 27) --; no implicit solve hides it. */
typedef struct pg_speed_plan {
    double mu_scale;        /* a_lim = mu_scale * vehicle.mu * vehicle.G; > 0, finite */
    double V_max;           /* > 0, finite */
    double V_floor;         /* > 0, <= V_max: no knot is planned slower (keeps t finite); default 1.0 = control V_min */
    double V_start, V_end;  /* open path: speed at the first / last knot (finite, >= 0); NaN: free.  Ignored on a closed path */
    double ax_max, ax_min;  /* extra caps on the tangential acceleration, ax_min <= 0 <= ax_max; +Inf / -Inf: none */
    double ay_max;          /* extra cap on V^2 |kappa|, > 0; +Inf: none */
} pg_speed_plan;            /* 64 bytes */
typedef struct pg_speed_plan_stats {   /* one per output trajectory */
    double t_end, v_min, v_max;
    double usage_max;       /* max over knots of sqrt(A^2 + (V^2 kappa)^2) / a_lim of the RESULT */
    int32_t n_cap, n_accel, n_brake, reserved;   /* knots whose speed is set by the cap, the forward pass, the backward pass; they sum to L */
} pg_speed_plan_stats;      /* 48 bytes */
/* { 1, 30, 1, NaN, NaN, +Inf, -Inf, +Inf } */
pg_speed_plan pg_default_speed_plan(void);
/* channels_in [n_path][10][Lmax] in the layout and channel order of pg_set_trajectories; its t, V and A channels are ignored, so a library in use can be re-planned as it
 * stands.  closed[k] != 0: knot L[k]-1 of path k is the same point as knot 0 (the caller's statement; NULL: every path is open).  vehicles NULL: pg_config.vehicle for
 * every set; else [n_sets], one vehicle per set.  Output trajectory k = path * n_sets + set: channels_out [n_path * n_sets][10][Lmax] and stats [n_path * n_sets]
 * (either may be NULL).  The seven geometry channels of the valid knots are copied bit for bit (as the library's element type holds them); every channel is 0 at and
 * past L[k].  install != 0 replaces the handle's trajectory library from the device buffers, with no host round trip: the handle is then exactly as after
 * pg_set_trajectories(h, n_path * n_sets, Lmax, L repeated, channels_out) -- the fp64 end times, the dropped index.  Synchronous.  A handle that never calls this
 * launches what it launched before.
 * PG_ERR_INVALID (the handle and its installed library are left unchanged): a null L, channels_in or sets; n_path or n_sets < 1; Lmax < 2; L[k] outside [2, Lmax]; a
 * closed path of fewer than 3 knots; s that does not increase strictly over the valid knots (in the library's element type); a non-finite geometry value in a valid
 * knot; a set outside the ranges above; a vehicle pg_set_plant_sets would refuse; more than 65535 x 16 sets. */
int pg_plan_speeds(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in, int32_t n_sets,
                   const pg_speed_plan* sets, const pg_vehicle* vehicles, int32_t install, double* channels_out, pg_speed_plan_stats* stats);

/* Making the path: a library of paths from line, arc and clothoid segments -- the curvature is linear in the arc length inside a segment --, computed on the device in the
 * layout pg_set_trajectories takes.  The reference generates straight lines only (src/trajectories.jl:46-58) and reads every other path from a file, so the scheme is
 * build-defined (tests/path_make_numpy.py is its numpy twin).  ALL arithmetic is double in both libraries, every operation rounded on its own (no contraction), and the
 * result is rounded to the library's element type on store: the fp32 library's output is exactly the fp64 library's rounded to float, and the stats are the same doubles.
 *   Bounds    (host) b_0 = 0, b_{j+1} = b_j + length_j;  psib_0 = psi0, psib_{j+1} = psib_j + (0.5 (kappa0_j + kappa1_j)) length_j;  total = b_{n_seg}.
 *   Knots     ds = total / (n_knots - 1);  s_i = i ds for i < n_knots - 1, s_last = total.  Knot i lies in the segment of the largest j with b_j <= s_i (b_j <= s_i < b_{j+1});
 *             the last knot lies at the end of the last segment.  With u = s_i - b_j (the last knot: u = length of the last segment, what total - b_j is before the
 *             roundings of the sums -- the heading of a path that ends on an arc then closes to the last bit):  kappa_i = kappa0 + ((kappa1 - kappa0) u) / length;
 *             psi_i = psi(j, u) = psib_j + u (kappa0 + ((0.5 (kappa1 - kappa0)) u) / length);  the edges as kappa;  t_i = s_i / V_ref, V_i = V_ref, A_i = 0.
 *             s, psi, kappa, the edges, t, V and A therefore reproduce the twin bit for bit.
 *   Position  dE/ds = -sin psi, dN/ds = cos psi (the committed paths' convention).  The interval [s_i, s_{i+1}] starts as the piece (j, u) of knot i; while b_{j+1} <
 *             s_{i+1} and a segment follows, the piece [u, length_j] of segment j is closed and the next starts at (j + 1, 0); the last piece is [u, s_{i+1} - b_j].
 *             A piece [ua, ub] of segment j: half = 0.5 (ub - ua), mid = 0.5 (ua + ub), nodes u_k = mid + half x_k over the four Gauss-Legendre points in ascending
 *             order (x = -+0.8611363115940526 with weight 0.3478548451374538, -+0.3399810435848563 with 0.6521451548625461);  dE = -(half sum_k w_k sin psi(j, u_k)),
 *             dN = half sum_k w_k cos psi(j, u_k), the sums from 0 in the order of the nodes.  The pieces of an interval are added in order from 0.
 *   Prefix    With c = ceil((n_knots - 1) / 256), block b holds the intervals b c .. b c + c - 1.  r_i (i >= 1) is the sum, in order from 0, of the increments of the
 *             intervals of block (i - 1) / c up to and including interval i - 1; T_b is the sum over all of block b (0 for an empty block).  The 256 totals are combined
 *             in groups of 64: inside a group by doubling -- for d = 1, 2, 4, 8, 16, 32 in turn, every T_b with b mod 64 >= d becomes T_b + T_{b-d}, all b of a step
 *             from the values before it --, which leaves the inclusive sums I_b;  G_0 = 0, G_{g+1} = G_g + I_{64 g + 63};  P_b = G_{b / 64} + (I_{b-1} if b mod 64 > 0,
 *             else 0).  E_0 = E0 and E_i = E0 + (P_{(i-1)/c} + r_i); N alike.  The order depends on the path's own n_knots alone: not on n_path, on the path's place
 *             in the library or on Lmax.  Against a serial sum the difference stays within 4 (n_knots + 64) 2^-53 total.
 * The accuracy is that of the 4-point rule per piece: against the Fresnel integrals 4.5e-14 m on a 20 m clothoid to 0.2 1/m at ds 1 m and 1.2e-11 m at ds 2 m (tests/test_path_make_host.py).
 * No repair of a path that does not close: closure_pos / closure_psi report the gap. */
typedef struct pg_path_segment {
    double length;          /* > 0, finite */
    double kappa0, kappa1;  /* curvature at the segment's start and end, linear in between: line (0, 0), arc (k, k), clothoid (k0 != k1); finite, either sign */
    double edge_L0, edge_L1;   /* tube edges at start / end, linear in between; finite, edge_L > edge_R at both ends */
    double edge_R0, edge_R1;
    double reserved;        /* 0 */
} pg_path_segment;          /* 64 bytes */
typedef struct pg_path_spec {
    double E0, N0, psi0;    /* pose of knot 0; finite */
    double V_ref;           /* > 0, finite: fills V = V_ref, A = 0, t = s / V_ref (the committed paths are constant-speed profiles of this kind) */
    int32_t seg0, n_seg;    /* this path's segments: segments[seg0 .. seg0 + n_seg), n_seg >= 1, inside [0, n_seg_total) */
    int32_t n_knots;        /* 2 <= n_knots <= Lmax; a closed path needs >= 3 */
    int32_t closed;         /* the caller's statement, passed through to closed_out (what pg_plan_speeds takes as closed[]) */
} pg_path_spec;             /* 48 bytes */
typedef struct pg_path_stats {   /* one per path; computed in double in both libraries */
    double length;          /* sum of the segment lengths = s of the last knot */
    double turn;            /* psi(last knot) - psi0 */
    double closure_pos;     /* hypot(E, N of the last knot - E, N of knot 0) */
    double closure_psi;     /* turn reduced to (-pi, pi] (the IEEE remainder by 6.283185307179586, -pi mapped to +pi) */
    double kappa_abs_max;   /* over the knots */
    double ds;              /* length / (n_knots - 1) */
} pg_path_stats;            /* 48 bytes */
/* { 1, 0, 0, 4, 4, -4, -4, 0 }: a 1 m line with the edge defaults of src/trajectories.jl:43-44 */
pg_path_segment pg_default_path_segment(void);
/* Output [n_path][10][Lmax] in the layout and channel order of pg_set_trajectories (t, s, V, A, E, N, psi, kappa, edge_L, edge_R), 0 at and past n_knots, as
 * pg_plan_speeds writes its tails.  L_out [n_path] (= n_knots), closed_out [n_path] (= closed), channels_out and stats [n_path] may each be NULL.  Segment ranges of
 * different paths may overlap (one oval at several poses).  install != 0 hands the device buffer to the handle, with no host round trip: the handle is then exactly as
 * after pg_set_trajectories(h, n_path, Lmax, L_out, channels_out) -- the fp64 end times (total / V_ref as the library's element type holds it), the dropped index, the
 * PG_ERR_STATE of the phase calls until an index is set when n_path > 1.  Synchronous.  A handle that never calls this launches what it launched before.
 * PG_ERR_INVALID, everything validated before the first allocation (the handle and its installed library are left unchanged): a null specs or segments; n_path < 1;
 * n_seg_total < 1; Lmax < 2; n_knots outside [2, Lmax]; a closed path of fewer than 3 knots; n_seg < 1 or a segment range outside [0, n_seg_total); a length that is not
 * finite and > 0; a non-finite kappa, edge or pose; edge_L <= edge_R at either end of a segment; V_ref not finite or <= 0; reserved != 0 (segments no path refers to are
 * not looked at); knots so dense that s does not increase strictly in the library's element type; n_path * 10 * Lmax elements beyond the allocation arithmetic. */
int pg_make_paths(pg_handle* h, int32_t n_path, const pg_path_spec* specs, int32_t n_seg_total, const pg_path_segment* segments, int32_t Lmax,
                  int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_path_stats* stats);

/* Fitting the path: a library of paths through waypoints -- surveyed or recorded (E, N) points with their tube edges --, computed on the device in the layout
 * pg_set_trajectories takes: an interpolating cubic spline of E and of N over the chord-length parameter, natural on an open path and periodic on a closed one, resampled
 * at n_knots knots equally spaced in arc length.  The reference reads its paths from files (src/ros_integration.jl:13-16), so the scheme is build-defined
 * (tests/path_fit_numpy.py is its numpy twin).  ALL arithmetic is double in both libraries, every operation rounded on its own (no contraction), and the result is rounded
 * to the library's element type on store: the fp32 library's output is exactly the fp64 library's rounded to float, and the stats are the same doubles.  Below, a
 * parenthesis is one rounded operation and a sum or product without one is taken from the left.
 *   Spans     An open path has the spans j = 0 .. n_wp - 2, a closed one n_wp spans, the last from waypoint n_wp - 1 back to waypoint 0 (the caller does not repeat the
 *             first point).  Span j runs from waypoint j to waypoint jn = (j + 1) mod n_wp:  h_j = sqrt((dE dE) + (dN dN)) with dE = E_jn - E_j, dN = N_jn - N_j (no hypot);
 *             the slopes d_j = dE / h_j and dN / h_j.
 *   Spline    Per coordinate y, in the second-derivative form:  h_{i-1} M_{i-1} + b_i M_i + h_i M_{i+1} = g_i with b_i = 2 (h_{i-1} + h_i), g_i = 6 (d_i - d_{i-1}).
 *             Open: M_0 = M_{n_wp-1} = 0 and the rows lo = 1 .. hi = n_wp - 2 (none for two waypoints: a straight line).  Closed: the rows lo = 0 .. hi = n_wp - 1 with the
 *             indices modulo n_wp, a cyclic system solved by Sherman-Morrison with gamma = -b_0, that is the correction vector u = (-b_0, 0, .., 0, hl) with hl =
 *             h_{n_wp-1}, b_0 = 2 (hl + h_0), against v = (1, 0, .., 0, -hl / b_0): the tridiagonal part keeps its rows but for bb_0 = 2 b_0 and bb_hi = b_hi + ((hl hl) / b_0), and has a third right-hand
 *             side g = u.  With three waypoints every off-diagonal place of the 3 x 3 matrix is taken -- band and corners still do not share a place --, and the same
 *             steps apply.  The Thomas recurrences, without pivoting (strictly diagonally dominant), per right-hand side; the pivots depend on h alone:
 *             beta_lo = bb_lo;  for i = lo + 1 .. hi: w = h_{i-1} / beta_{i-1}, beta_i = bb_i - (w h_{i-1}), g_i = g_i - (w g_{i-1});
 *             x_hi = g_hi / beta_hi;  for i = hi - 1 .. lo: x_i = (g_i - (h_i x_{i+1})) / beta_i.
 *             Open: M = x.  Closed, with z the solution for u:  den = (1 + z_0) - ((hl z_hi) / b_0);  fact = (x_0 - ((hl x_hi) / b_0)) / den;  M_i = x_i - (fact z_i).
 *   Cubic     In span j, u in [0, h_j]:  c1 = d_j - ((h_j ((2 M_j) + M_jn)) / 6), c3 = (M_jn - M_j) / (6 h_j);
 *             y(u) = y_j + (u (c1 + (u ((0.5 M_j) + (u c3))))),  y'(u) = c1 + (u (M_j + (u (3 c3)))),  y''(u) = M_j + (u (6 c3)).
 *   Lengths   v(u) = sqrt((E' E') + (N' N')).  A piece [ua, ub]: half = 0.5 (ub - ua), mid = 0.5 (ua + ub), the four Gauss-Legendre nodes u_k = mid + (half x_k) and
 *             weights of pg_make_paths in ascending order, piece = half sum_k (w_k v(u_k)), the sum from 0 in the order of the nodes.  l_j(u) = piece [0, 0.5 u] + piece
 *             [0.5 u, u];  l_j = l_j(h_j).  S_0 = 0 and S_{j+1} = P_{j / c} + r_{j+1} in the blocked prefix order of pg_make_paths (Prefix) over the l_j, with c =
 *             ceil(n_span / 256): the order depends on the path's own span count alone.  total = S_{n_span}.
 *   Knots     ds = total / (n_knots - 1);  s_i = i ds for i < n_knots - 1, s_last = total.  Knot i lies in the span of the largest j with S_j <= s_i; target = s_i - S_j;
 *             u_0 = clamp((target h_j) / l_j), then exactly three Newton steps u <- clamp(u - ((l_j(u) - target) / v(u))), clamp(u) = 0 unless u >= 0, h_j where u > h_j.
 *             The count is fixed, so the bits depend on no convergence test; s_err_max reports what is left.  The last knot lies in the last span at u = h_j, and its E
 *             and N are those of the waypoint the span ends on (waypoint 0 of a closed path), not y(h_j).
 *   Channels  E = E(u), N = N(u);  v2 = (E' E') + (N' N'), kappa = ((E' N'') - (E'' N')) / (v2 sqrt(v2)): with dE/ds = -sin psi, dN/ds = cos psi (the committed paths'
 *             convention) a left turn is positive, a counter-clockwise circle gives +1 / R;  psi_raw = atan2(-E', N');  an edge = edge_j + (((edge_jn - edge_j) u) / h_j);
 *             t = s / V_ref, V = V_ref, A = 0.
 *   Unwrap    k_0 = 0;  k_i = k_{i-1} - 1 where psi_raw_i - psi_raw_{i-1} > 3.141592653589793, k_{i-1} + 1 where it is < -3.141592653589793, else k_{i-1};
 *             psi_i = psi_raw_i + (k_i 6.283185307179586).  The prefix is over integers: its order cannot show.
 * Everything but atan2 reproduces the twin bit for bit; psi, turn and closure_psi are within 8 * 2^-52 * max(pi, |psi|) of it.  Interpolation, not smoothing: noisy waypoints
 * (a rounded survey) go through pg_smooth_waypoints below first, whose output is what this call takes. */
typedef struct pg_waypoint {
    double E, N;            /* finite; two neighbouring waypoints of a path must not coincide */
    double edge_L, edge_R;  /* the tube edges at the waypoint, linear in u across a span; finite, edge_L > edge_R */
} pg_waypoint;              /* 32 bytes */
typedef struct pg_fit_spec {
    double V_ref;           /* > 0, finite: fills V = V_ref, A = 0, t = s / V_ref */
    int32_t wp0, n_wp;      /* this path's waypoints: waypoints[wp0 .. wp0 + n_wp), inside [0, n_wp_total); n_wp >= 2, a closed path >= 3 */
    int32_t n_knots;        /* 2 <= n_knots <= Lmax; a closed path needs >= 3 */
    int32_t closed;         /* != 0: periodic, the last span returns to waypoint 0 and the last knot is knot 0 again; passed through to closed_out */
} pg_fit_spec;              /* 24 bytes */
typedef struct pg_fit_stats {    /* one per path; computed in double in both libraries */
    double length;          /* total = s of the last knot */
    double turn;            /* psi(last knot) - psi(knot 0) */
    double closure_pos;     /* sqrt(dE dE + dN dN) between the last knot and knot 0: 0 on a closed path by construction, the gap of an open one */
    double closure_psi;     /* turn reduced to (-pi, pi] (the IEEE remainder by 6.283185307179586, -pi mapped to +pi) */
    double kappa_abs_max;   /* over the knots */
    double ds;              /* length / (n_knots - 1) */
    double chord_min, chord_max;   /* over the spans */
    double s_err_max;       /* largest |l_j(u) - target| left by the inversion, over the knots */
    double reserved;        /* 0 */
} pg_fit_stats;             /* 80 bytes */
/* { 0, 0, 4, -4 }: the edge defaults of src/trajectories.jl:43-44 */
pg_waypoint pg_default_waypoint(void);
/* Output [n_path][10][Lmax] in the channel order and with the tail rule of pg_make_paths.  L_out [n_path] (= n_knots), closed_out [n_path] (= closed, what pg_plan_speeds
 * takes as closed[]), channels_out and stats [n_path] may each be NULL.  Waypoint ranges of different paths may overlap (one survey fitted at several knot counts).
 * install != 0 hands the device buffer to the handle, with no host round trip: the handle is then exactly as after pg_set_trajectories(h, n_path, Lmax, L_out,
 * channels_out).  Synchronous.  A handle that never calls this launches what it launched before.
 * PG_ERR_INVALID, everything validated before the first allocation (the handle and its installed library are left unchanged): a null specs or waypoints; n_path < 1;
 * n_wp_total < 1; Lmax < 2; n_knots outside [2, Lmax]; an open path with n_wp < 2; a closed path with n_wp < 3 or n_knots < 3; a waypoint range outside [0, n_wp_total);
 * a non-finite waypoint field; edge_L <= edge_R; a span whose chord is not finite and > 0 (two neighbouring waypoints at the same point, last-to-first on a closed path
 * included); V_ref not finite or <= 0 (waypoints no path refers to are not looked at); knots so dense that s cannot be shown to increase strictly in the library's
 * element type -- decided before the spline exists, from the sum C of the chords: refused unless n_knots - 1 <= 1 / (4 eps) (2^21 in the fp32 library; every int32 in the
 * fp64 library) and 2^-100 <= C / (n_knots - 1), C <= 2^100 --; n_path * 10 * Lmax elements or the scratch of all spans beyond the allocation arithmetic. */
int pg_fit_paths(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints, int32_t Lmax,
                 int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_fit_stats* stats);

/* Offsetting the path: every (path, offset set) pair of a path library and a library of offset sets as a trajectory, computed on the device in the layout
 * pg_set_trajectories takes -- the same road d metres to the left (a lane), a lane change between two arc lengths, a pass-by that goes round something and comes back.
 * The reference reads its paths from files (src/ros_integration.jl:13-16) or makes straight lines (src/trajectories.jl:46-58), so the scheme is build-defined
 * (tests/path_offset_numpy.py is its numpy twin).  It is knot-wise: output knot i belongs to source knot i, nothing is resampled.  channels_in is read as the doubles
 * given, ALL arithmetic is double in both libraries, every operation rounded on its own (no contraction), and the result is rounded to the library's element type once,
 * on store: the fp32 library's output is exactly the fp64 library's rounded to float, and the stats are the same doubles.  Below, a parenthesis is one rounded operation
 * and a sum or product without one is taken from the left.
 *   Window    win(u; a, b) = (f, f', f'') of sigma(tau) = tau^3 (10 - 15 tau + 6 tau^2) and its derivatives in u (C2: the curvature stays continuous across a window's
 *             ends):  a = +Inf: (0, 0, 0).  Else w = b - a, tau = (u - a) / w;  unless tau > 0: (0, 0, 0);  where tau >= 1: (1, 0, 0);  else with z = tau (1 - tau):
 *             f = ((tau tau) tau) (10 + (tau ((6 tau) - 15))),  f' = (30 (z z)) / w,  f'' = ((60 z) (1 - (2 tau))) / (w w).
 *   Offset    With u = s - s_first of the SOURCE, rise = win(u; s_a, s_b), fall = win(u; s_c, s_d) and dd = d1 - d0:
 *             d = d0 + (dd (rise - fall)),  d' = dd (rise' - fall'),  d'' = dd (rise'' - fall'').
 *   Arclength Interval i = [s_i, s_{i+1}]: diff = s_{i+1} - s_i, half = 0.5 diff, mid = 0.5 (s_i + s_{i+1}); the four Gauss-Legendre nodes u_k = mid + (half x_k) and
 *             weights of pg_make_paths in ascending order.  At a node kappa = kappa_i + (((kappa_{i+1} - kappa_i) (u_k - s_i)) / diff) -- linear inside the interval, the
 *             controller's own lookup --, d and d' are those of Offset at u_k - s_first, x = 1 - (kappa d), g = sqrt((x x) + (d' d'));
 *             extra_i = half sum_k (w_k (g - 1)), the sum from 0 in the order of the nodes.  The g - 1 form is deliberate: the four weights sum to 1.9999999999999996, and
 *             with it the identity set returns s' = s bit for bit.  X_0 = 0 and X_{i+1} = P_{i / c} + r_{i+1} in the blocked prefix order of pg_make_paths (Prefix) over
 *             the extra_i, with c = ceil((L - 1) / 256): the order depends on the path's own knot count alone.  s'_i = s_i + X_i.
 *   Frame     That of pg_make_starts: psi is measured from North, the left normal is (-cos psi, -sin psi), a left turn has kappa > 0.  At knot i, with d, d', d'' at
 *             u = s_i - s_first:  x = 1 - (kappa_i d), y = d', g2 = (x x) + (y y), g = sqrt(g2);  E' = E_i - (d cos psi_i), N' = N_i - (d sin psi_i);
 *             psi' = psi_i + atan2(y, x);  kappa' = (kappa_i + (((x d'') + (y ((ks d) + (kappa_i d')))) / g2)) / g.
 *             ks is the source's d kappa / ds at the knot: (kappa_{i+1} - kappa_{i-1}) / (s_{i+1} - s_{i-1}) inside; at the ends of an open path the same with the
 *             missing neighbour replaced by the knot itself (one-sided); at knot 0 and knot L-1 of a closed path (the same point)
 *             (kappa_1 - kappa_{L-2}) / ((s_1 - s_0) + (s_{L-1} - s_{L-2})).
 *   Speed     The Result rule of pg_plan_speeds on the new s:  V' = V;  ds'_i = s'_{i+1} - s'_i;  A'_i = ((V_{i+1} V_{i+1}) - (V_i V_i)) / (2 ds'_i), A'_{L-1} = 0 on an
 *             open path and A'_0 on a closed one;  dt_i = (2 ds'_i) / (V_i + V_{i+1});  t'_0 = t_0 and t'_{i+1} = t_0 + (P_{i / c} + r_{i+1}), the same blocked prefix over
 *             the dt_i.  A friction-limited profile for the new curvature -- the inner lane of a bend needs a slower one -- is pg_plan_speeds' job: hand it channels_out
 *             and closed_out.
 *   Edges     edge_mode 0, the same road: edge' = edge - d for both edges;  edge_mode 1, the tube travels with the path: the edges are copied.
 *   Stats     length = s'_{L-1} - s'_0;  ds_min, ds_max over the ds'_i;  kappa_abs_max over |kappa'|;  x_min over the x of the knots;  d_abs_max over |d| of the knots;
 *             closure_pos = sqrt((dE dE) + (dN dN)) between the last and the first output knot;  n_outside counts the knots where edge_R' < 0 < edge_L' does not hold
 *             (reported, not refused).
 * t, s, V, A, kappa, both edges and every stat but closure_pos reproduce the twin bit for bit (they carry no libm call but sqrt); psi is within 8 * 2^-52 * max(pi, |psi|)
 * of it (atan2), E and N within 8 * 2^-52 * (|d| + |E or N|) (sin, cos and the last rounding). */
typedef struct pg_offset_set {
    double d0, d1;            /* lateral offset in metres, left positive: d0 outside the windows, d1 on the plateau; finite */
    double s_a, s_b;          /* rise d0 -> d1 over [s_a, s_b], metres of the SOURCE arclength from its first knot; s_a = +Inf: no rise (d = d0 throughout) */
    double s_c, s_d;          /* fall d1 -> d0 over [s_c, s_d]; s_c = +Inf: no fall (a single lane change) */
    double x_min;             /* refuse a pair where 1 - kappa_i d_i < x_min at a valid knot (the offset reaches the centre of curvature); in (0, 1], default 0.1 */
    int32_t edge_mode;        /* 0: the same road (edge' = edge - d); 1: the tube travels with the path (edges copied) */
    int32_t reserved;         /* 0 */
} pg_offset_set;              /* 64 bytes */
typedef struct pg_offset_stats {   /* one per output trajectory; computed in double in both libraries */
    double length, ds_min, ds_max, kappa_abs_max, x_min, d_abs_max, closure_pos;
    int32_t n_outside, reserved;
} pg_offset_stats;            /* 64 bytes */
/* { 0, 0, +Inf, +Inf, +Inf, +Inf, 0.1, 0, 0 }: the identity */
pg_offset_set pg_default_offset_set(void);
/* channels_in [n_path][10][Lmax], L and closed are what pg_plan_speeds takes (closed NULL: every path is open); here V and t_0 of the valid knots are read as well.
 * Output trajectory k = path * n_sets + set, as in pg_plan_speeds: channels_out [n_path * n_sets][10][Lmax], stats [n_path * n_sets], L_out [n_path * n_sets] (=
 * L[path]) and closed_out [n_path * n_sets] (= closed[path]; 0 where closed is NULL); each may be NULL.  Every channel is 0 at and past L.  install != 0 hands the device buffer to the
 * handle, with no host round trip: the handle is then exactly as after pg_set_trajectories(h, n_path * n_sets, Lmax, L_out, channels_out).  Synchronous.  A handle that
 * never calls this launches what it launched before.
 * PG_ERR_INVALID, everything the host can decide validated before the first allocation (the handle and its installed library are left unchanged): a null L, channels_in or
 * sets; n_path or n_sets < 1; Lmax < 2; L[k] outside [2, Lmax]; a closed path of fewer than 3 knots; s that does not increase strictly over the valid knots (in the
 * library's element type); a non-finite geometry value, a V that is not finite and > 0 or a non-finite t_0 in a valid knot; a non-finite d0 or d1; s_a or s_c that is
 * neither finite nor +Inf; a window with a start whose end is not finite and beyond it (s_b <= s_a, s_d <= s_c, NaN); s_c < s_b when both windows exist; a fall without a
 * rise; x_min outside (0, 1]; edge_mode outside {0, 1}; reserved != 0; a (path, set) pair with 1 - kappa_i d_i < x_min at a valid knot (the message names path, set
 * and knot); a closed path whose first or last knot lies inside a window, or whose two ends lie on different plateaus (such an offset curve does not close);
 * n_path * n_sets * 10 * Lmax elements beyond the allocation arithmetic.  After the launch and before any install: a pair whose s' does not increase strictly in the
 * library's element type.  Windows that lie beyond a path's end are not an error: that path keeps d0. */
int pg_offset_paths(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,
                    int32_t n_sets, const pg_offset_set* sets, int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_offset_stats* stats);

/* Clipping the tube: every (path, obstacle set) pair of a path library and a library of obstacle sets as a trajectory, computed on the device in the layout
 * pg_set_trajectories takes -- the same path, its two edge channels narrowed around the discs of the set: the thing a pass-by of pg_offset_paths goes round.  Whatever
 * reads the edges (the wall rows of the decoupled formulation, first_exit of the tracking summary, e_frac of pg_make_starts, n_outside of pg_offset_paths) then sees the
 * obstacle.  The reference has no obstacles (src/trajectories.jl:8-44 only stores edge_L, edge_R), so the scheme is build-defined (tests/tube_clip_numpy.py is its numpy
 * twin).  It is knot-wise.  channels_in is read as the doubles given, ALL arithmetic is double in both libraries, every operation rounded on its own (no contraction), and a
 * value is rounded to the library's element type once, on store: the fp32 library's output is exactly the fp64 library's rounded to float, and the stats and reports are
 * the same doubles.  Below, a parenthesis is one rounded operation; min, max and | | are exact.
 *   Frame     That of pg_make_starts / pg_offset_paths: psi is measured from North, the tangent in (E, N) is (-sin psi, cos psi), the left normal is (-cos psi, -sin psi),
 *             and edge_R < 0 < edge_L on an unobstructed road.  Knot i is a valid knot of the path; knot L-1 of a closed path is knot 0 again: it takes part in no
 *             search and in no count, and its two output edges are those of knot 0.  Obstacle j is an obstacle of the set, R = (radius + margin).
 *   Sight     wE = E_j - E_i, wN = N_j - N_i;  a = (wE (-cos psi_i)) + (wN (-sin psi_i)) (to the left),  b = (wE (-sin psi_i)) + (wN cos psi_i) (ahead),
 *             q = (wE wE) + (wN wN).  Knot i SEES j when |b| < R and, with h = sqrt((R R) - (b b)), (a - h) < edge_L_i and (a + h) > edge_R_i: the chord the disc cuts
 *             out of the knot's normal line reaches into the SOURCE tube.
 *   Closest   k_at = the knot of smallest q, the lowest index on ties.  The report's values are those of this knot: dist_at = sqrt(q), a_at = a, u_at = s - s_first,
 *             h_at = h (0 where |b| >= R there), free_right = (a_at - h_at) - edge_R, free_left = edge_L - (a_at + h_at).
 *   Side      One decision per (pair, obstacle), taken at k_at, so a tube never splits.  PG_PASS_CENTRE: the obstacle is on the left when a_at > 0.  PG_PASS_WIDER: pass
 *             on the side of the larger free_*, on equality the CENTRE rule.  PG_PASS_LEFT: the obstacle counts as on the right.  PG_PASS_RIGHT: as on the left.
 *             side = +1: the left edge is clipped (we pass on the right); -1: the right edge; 0: no knot sees it (it is ignored; k_first = k_last = -1).
 *   Hard clip cL_i and cR_i start from edge_L_i and edge_R_i.  At every knot that sees j: cL_i = min(cL_i, (a - h)) when side = +1, cR_i = max(cR_i, (a + h)) when
 *             side = -1.  k_first / k_last are the lowest and the highest seeing knot.
 *   Taper     dist(i, k) = |s_i - s_k| on an open path, min(|s_i - s_k|, ((s_{L-1} - s_0) - |s_i - s_k|)) on a closed one.  With m = taper finite:
 *             edge_L'_i = min(cL_i, min over the knots k with cL_k < edge_L_k of (cL_k + (m dist(i, k)))),
 *             edge_R'_i = max(cR_i, max over the knots k with cR_k > edge_R_k of (cR_k - (m dist(i, k)))).  With m = +Inf: edge' = c.
 *             Every term is an expression of its own and min / max are exact, so the result does not depend on the order in which the k are visited.
 *   Stats     Over the knots that take part, on the doubles before the store: width_min = min of (edge_L' - edge_R'), u_width_min = s - s_first there (the lowest knot
 *             on ties);  n_clip_L / n_clip_R count the knots where edge_L' / edge_R' differs from the source;  n_blocked those where (edge_L' - edge_R') < min_width;
 *             n_centre_out those where edge_R' < 0 < edge_L' fails;  n_seen / n_ignored the obstacles of the set with side != 0 / == 0.  Blocked and centre-out knots
 *             are reported, never refused.
 *   Output    The other eight channels are copied (as the element type holds them), L_out and closed_out as in pg_offset_paths.
 * What the knots see: a disc that lies between two knots farther apart than its chord is seen by neither and comes back side = 0 -- on a line with knots 10 m apart a disc
 * of R = 1.5 m at 215 m is such a one.  A tube wider than the distance to the opposite side of a loop is outside the scheme.  Choose the knots to the obstacle.
 * The copied channels, every integer and every edge of a knot no obstacle touches reproduce the twin bit for bit; a touched edge and the report's doubles are within
 * 8 * 2^-52 * (|wE| + |wN| + R) * (1 + |b| / h) of it (sin, cos, a two-term product sum, and the condition of sqrt((R R) - (b b))). */
enum pg_pass_policy { PG_PASS_CENTRE = 0, PG_PASS_WIDER = 1, PG_PASS_LEFT = 2, PG_PASS_RIGHT = 3 };
typedef struct pg_obstacle {
    double E, N, radius;      /* a disc in the world frame; finite, radius >= 0 */
    double reserved;          /* 0 */
} pg_obstacle;                /* 32 bytes */
typedef struct pg_obstacle_set {
    int32_t first, count;     /* obstacles[first .. first+count) of the call's array; count in [0, 64]; sets may share and overlap ranges */
    double margin;            /* added to every radius: half the car's width plus clearance; finite, >= 0 */
    double taper;             /* metres of edge per metre of arclength by which a clip may relax; > 0, or +Inf: no taper, the hard clip only */
    double min_width;         /* a knot whose clipped width is below this counts as blocked; finite, >= 0 */
    int32_t policy, reserved; /* PG_PASS_CENTRE 0, PG_PASS_WIDER 1, PG_PASS_LEFT 2, PG_PASS_RIGHT 3; 0 */
    double pad[3];            /* 0 */
} pg_obstacle_set;            /* 64 bytes */
typedef struct pg_clip_stats {     /* one per output trajectory; computed in double in both libraries */
    double width_min, u_width_min;
    double reserved_d[2];
    int32_t n_clip_L, n_clip_R, n_blocked, n_centre_out, n_seen, n_ignored, reserved[2];
} pg_clip_stats;              /* 64 bytes */
typedef struct pg_obstacle_report {   /* one per (output trajectory, obstacle slot) */
    double u_at, a_at, h_at, dist_at, free_left, free_right;
    int32_t k_at, k_first, k_last, side;
} pg_obstacle_report;         /* 64 bytes */
/* { 0, 0, 0.0, +Inf, 0.0, 0, 0, {0, 0, 0} }: the identity */
pg_obstacle_set pg_default_obstacle_set(void);
/* channels_in [n_path][10][Lmax], L and closed are what pg_offset_paths takes (closed NULL: every path is open); V, A and t are copied, not read.  obstacles [n_obs] is
 * shared by the sets.  Output trajectory k = path * n_sets + set: channels_out [n_path * n_sets][10][Lmax], stats [n_path * n_sets], L_out, closed_out as in
 * pg_offset_paths, report [n_path * n_sets][max_count] with max_count the largest count of the call (slot j of a pair: obstacle first + j of its set; the unused slots are
 * all zero with k_at = k_first = k_last = -1); each may be NULL.  Every channel is 0 at and past L.  install != 0 hands the device buffer to the handle, with no host round
 * trip: the handle is then exactly as after pg_set_trajectories(h, n_path * n_sets, Lmax, L_out, channels_out).  Synchronous.  A handle that never calls this launches
 * what it launched before.
 * PG_ERR_INVALID, all of it validated before the first allocation (the handle and its installed library are left unchanged): a null L, channels_in or sets; n_path or
 * n_sets < 1; Lmax < 2; L[k] outside [2, Lmax]; a closed path of fewer than 3 knots; s that does not increase strictly over the valid knots (in the library's element
 * type); a non-finite geometry value (s, E, N, psi, kappa, either edge) in a valid knot; n_obs < 0, or obstacles NULL while some count > 0; first < 0, count outside
 * [0, 64] or first + count > n_obs; a non-finite E, N or radius, a radius < 0 or a reserved != 0 of an obstacle some set uses; radius + margin not > 0; margin or
 * min_width not finite and >= 0; taper not > 0 (NaN included); policy outside 0 .. 3; reserved or pad != 0; n_path * n_sets * 10 * Lmax elements beyond the allocation
 * arithmetic. */
int pg_clip_tubes(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,
                  int32_t n_sets, const pg_obstacle_set* sets, int32_t n_obs, const pg_obstacle* obstacles, int32_t install,
                  int32_t* L_out, int32_t* closed_out, double* channels_out, pg_clip_stats* stats, pg_obstacle_report* report);

/* Refining the path: every (path, refine set) pair of a path library and a library of refine sets as a trajectory, computed on the device in the layout
 * pg_set_trajectories takes -- the same path with more knots where a manoeuvre or an obstacle needs them.  pg_offset_paths and pg_clip_tubes are knot-wise ("What the
 * knots see" above): this is the maker that chooses the knots for a library that already exists, whatever made it.  Every source knot stays a knot, with its own values,
 * and the arc length is the source's: offset sets, obstacle reports and route events written against the source stay valid on the result.  The reference has no path
 * maker (src/ros_integration.jl:13-16 reads files), so the scheme is build-defined (tests/path_refine_numpy.py is its numpy twin).  channels_in is read as the doubles
 * given, ALL arithmetic is double in both libraries, every operation rounded on its own (no contraction), and a value is rounded to the library's element type once, on
 * store: the fp32 library's output is exactly the fp64 library's rounded to float, and the stats are the same doubles.  Below, a parenthesis is one rounded operation;
 * min, max, ceil and | | are exact.
 *   Parts     u_i = s_i - s_first.  Source interval i = [s_i, s_{i+1}], diff = s_{i+1} - s_i.  Its wanted spacing w_i = the minimum of ds and of the ds_w of every used
 *             window (s_lo < +Inf) that reaches into the interval's interior: s_lo < u_{i+1} and s_hi > u_i.  m_i = 1 when w_i is +Inf or diff <= w_i; else with
 *             q = diff / w_i:  m_i = ceil(q), refused unless q <= 4096.  The interval is cut into m_i equal parts.
 *   Offsets   o_0 = 0, o_{i+1} = o_i + m_i, L_out = o_{L-1} + 1.  The prefix is over integers: its order cannot show (on the device it is the blocked scan of
 *             pg_make_paths (Prefix) with c = ceil((L - 1) / 256)).  Output knot o_i + k is sub-knot k of interval i, 0 <= k < m_i; output knot L_out - 1 is the last
 *             source knot.  Sub-knot 0 of an interval and the last knot are SOURCE knots: all ten channels are copied.
 *   Sub-knot  0 < k < m_i:  tau = (diff k) / m_i,  s = s_i + tau.  With lin(x) = x_i + (((x_{i+1} - x_i) tau) / diff):  kappa = lin(kappa), edge_L = lin(edge_L),
 *             edge_R = lin(edge_R) -- linear inside the interval, the controller's own lookup.
 *   Heading   b = (0.5 (kappa_{i+1} - kappa_i)) / diff,  a = ((psi_{i+1} - psi_i) / diff) - (b diff),  psi(v) = psi_i + (v (a + (v b))),  psi = psi(tau): the clothoid the two
 *             curvatures define, tilted so that it ends on the source's psi_{i+1}.  On a pg_make_paths library a is kappa_i up to rounding; closure_psi_max reports
 *             |a - kappa_i| diff.
 *   Position  dE/ds = -sin psi, dN/ds = cos psi.  A piece [va, vb]: half = 0.5 (vb - va), mid = 0.5 (va + vb), the four Gauss-Legendre nodes v_q = mid + (half x_q) and
 *             weights of pg_make_paths in ascending order;  pE = -(half sum_q (w_q sin psi(v_q))),  pN = half sum_q (w_q cos psi(v_q)), the sums from 0 in the order of
 *             the nodes.  I(v) = piece [0, (0.5 v)] + piece [(0.5 v), v], as l_j(u) of pg_fit_paths.  The closure of the interval:  cE = (E_{i+1} - E_i) - IE(diff),
 *             cN alike -- how far the source's own E and N are from its psi and kappa.  E = E_i + (IE(tau) + ((tau / diff) cE)),  N alike: the refined curve passes
 *             through every source knot.
 *   Speed     W = (V_i V_i) + ((((V_{i+1} V_{i+1}) - (V_i V_i)) tau) / diff),  V = sqrt(W),  A = A_i (constant over an interval under the Result rule of pg_plan_speeds);
 *             t = t_i + (((t_{i+1} - t_i) ((2 tau) / (V_i + V))) / ((2 diff) / (V_i + V_{i+1}))): the Result rule on the sub-interval, scaled so that it ends on the
 *             source's t_{i+1}.
 *   Stats     length = s_{L-1} - s_0;  ds_min, ds_max over the differences of neighbouring output s (as doubles);  n_added = L_out - L;  m_max = the largest m_i;
 *             closure_pos_max = the largest sqrt((cE cE) + (cN cN));  closure_psi_max = the largest (|a - kappa_i| diff);  kappa_abs_max over the output knots.
 * L_out, t, s, V, A, psi, kappa, both edges and every stat but closure_pos_max reproduce the twin bit for bit (they carry no libm call but sqrt); E, N and
 * closure_pos_max are within 8 * 2^-52 * (|E or N| + ds_max of the source) of it (sin, cos).  Left out: coarsening (no source knot is ever dropped), equal spacing over
 * the whole path (the parts are equal inside a source interval only), and reading the source from the installed library (it is handed in, as to the other makers). */
typedef struct pg_refine_set {
    double ds;                /* the largest spacing wanted everywhere, metres: +Inf (none), or finite and > 0 */
    double s_lo[4], s_hi[4];  /* up to 4 windows in metres of the SOURCE arclength from its first knot; s_lo = +Inf: the slot is unused.  Else s_lo finite, s_hi finite and > s_lo */
    double ds_w[4];           /* the largest spacing wanted inside window j; finite and > 0 in a used slot.  Windows may overlap: the smallest spacing holds */
    double reserved[3];       /* 0 */
} pg_refine_set;              /* 128 bytes */
typedef struct pg_refine_stats {   /* one per output trajectory; computed in double in both libraries */
    double length, ds_min, ds_max, closure_pos_max, closure_psi_max, kappa_abs_max;
    int32_t n_added, m_max;
    double reserved;          /* 0 */
} pg_refine_stats;            /* 64 bytes */
/* { +Inf, {+Inf x 4}, {+Inf x 4}, {+Inf x 4}, {0, 0, 0} }: the identity */
pg_refine_set pg_default_refine_set(void);
/* channels_in [n_path][10][Lmax], L and closed are what pg_offset_paths takes (closed NULL: every path is open); V and t of the valid knots are read as well.  Output
 * trajectory k = path * n_sets + set: channels_out [n_path * n_sets][10][Lmax_out], stats [n_path * n_sets], L_out [n_path * n_sets] (the pair's own knot count) and
 * closed_out [n_path * n_sets] (= closed[path]; 0 where closed is NULL); each may be NULL.  Every channel is 0 at and past L_out.  install != 0 hands the device buffer to
 * the handle, with no host round trip: the handle is then exactly as after pg_set_trajectories(h, n_path * n_sets, Lmax_out, L_out, channels_out).  Synchronous.  A handle
 * that never calls this launches what it launched before.
 * PG_ERR_INVALID, everything the host can decide validated before the first allocation (the handle and its installed library are left unchanged): a null L, channels_in or
 * sets; n_path or n_sets < 1; Lmax or Lmax_out < 2; L[k] outside [2, Lmax]; a closed path of fewer than 3 knots; s that does not increase strictly over the valid knots
 * (in the library's element type); a non-finite geometry value, a V that is not finite and > 0 or a non-finite t in a valid knot; ds that is neither +Inf nor finite and
 * > 0; s_lo that is neither finite nor +Inf; a used window whose s_hi is not finite and > s_lo or whose ds_w is not finite and > 0; a NaN in an unused slot; reserved
 * != 0; a (path, set) pair with an interval of more than 4096 parts (the message names path, set and interval); a pair whose L_out exceeds Lmax_out (the message names
 * path, set, the count and Lmax_out); n_path * n_sets * 10 * max(Lmax, Lmax_out) elements beyond the allocation arithmetic.  After the launch and before any install: a
 * pair whose s does not increase strictly in the library's element type (the fp32 library under a very fine ds_w).  A window beyond a path's end has no effect. */
int pg_refine_paths(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,
                    int32_t n_sets, const pg_refine_set* sets, int32_t Lmax_out, int32_t install,
                    int32_t* L_out, int32_t* closed_out, double* channels_out, pg_refine_stats* stats);

/* Smoothing surveyed waypoints: every (path, smoothing set) pair of a library of waypoint lists and a library of smoothing sets as smoothed waypoints, computed on the
 * device -- a cubic smoothing spline (Reinsch) of E and of N over the chord-length parameter, natural on an open path and periodic on a closed one.  pg_fit_paths
 * interpolates, so the rounding of a recorded survey is differentiated twice into kappa; this is the call that comes before it: waypoints in, waypoints out, and a library
 * of sets with per-pair stats to choose lambda from.  The reference reads its paths from files (src/ros_integration.jl:13-16), so the scheme is build-defined
 * (tests/wp_smooth_numpy.py is its twin).  Waypoints are doubles in both libraries and ALL arithmetic is double, every operation rounded on its own (no contraction): both
 * libraries return the same bits.  The scheme has only + - * / sqrt, so the twin reproduces every output bit for bit.  Below, a parenthesis is one rounded operation, a sum
 * or product without one is taken from the left, and min, max, | | and the comparisons are exact.  n = n_wp; im = i - 1, ip = i + 1, modulo n.
 *   Chords    The spans and h_j = sqrt((dE dE) + (dN dN)) of the INPUT waypoints exactly as pg_fit_paths states them (Spans), with p_j = 1 / h_j and the slopes dE / h_j,
 *             dN / h_j.  An open path has no span n - 1: h_{n-1} = p_{n-1} = 0 and its slopes are 0 (only places the rows below do not reach read them).
 *   U         U_0 = 0 and U_{j+1} = P_{j / c} + r_{j+1}, the blocked prefix order of pg_make_paths (Prefix) over h_0 .. h_{n-2}, c = ceil((n - 1) / 256): the
 *             cumulative chord length of waypoint i, in which the windows are given.
 *   winv      winv_i = 1; then for k = 0 .. n_win - 1 in turn: where u_lo[k] <= U_i <= u_hi[k], winv_i = factor[k] (the last listed window that holds U_i wins).
 *             pin_ends on an open path: winv_0 = winv_{n-1} = 0.  winv = 0 pins a waypoint, a factor above 1 smooths it more.
 *   System    (R + lambda Q^T Winv Q) gamma = Q^T y per coordinate y in {E, N}, with Q the second-difference operator (column i holds p_im, q_i = (-p_im) - p_i and p_i
 *             in the rows im, i, ip), R_ii = (h_im + h_i) / 3, R_{i,ip} = h_i / 6.  The band of row i in closed form:
 *               a0 = ((winv_im (p_im p_im)) + (winv_i (q_i q_i))) + (winv_ip (p_i p_i));   a1 = p_i ((winv_i q_i) + (winv_ip q_ip));   a2 = winv_ip (p_i p_ip);
 *               D_i = ((h_im + h_i) / 3) + (lambda a0);   E1_i = (h_i / 6) + (lambda a1)  [the place (i, ip)];   E2_i = lambda a2  [the place (i, ip + 1)];
 *             the right-hand side f_i = slope_i - slope_im.  The matrix is symmetric positive definite and pentadiagonal.
 *   Band      The rows r = 0 .. m - 1 of a band (D, E1, E2) by the LDL^T recurrence without pivoting; an entry before row 0 is 0, a pivot before row 0 is 1:
 *               e1 = E1_{r-1}, e2 = E2_{r-2};  l2_r = e2 / d_{r-2};  c1 = e1 - (e2 l1_{r-1});  l1_r = c1 / d_{r-1};  d_r = (D_r - (e2 l2_r)) - (c1 l1_r);
 *               z_r = (f_r - (l1_r z_{r-1})) - (l2_r z_{r-2});   then for r = m - 1 .. 0:  x_r = ((z_r / d_r) - (l1_{r+1} x_{r+1})) - (l2_{r+2} x_{r+2}), a term past the
 *             last row left out as 0.  One factorisation serves every right-hand side.
 *   Open      The rows are the waypoints 1 .. n - 2 (m = n - 2), gamma_0 = gamma_{n-1} = 0 (natural ends).  Two waypoints have no row.
 *   Closed    All n rows, indices modulo n: a cyclic pentadiagonal system, solved exactly by bordering.  The band B is the rows and columns 0 .. n - 3 (m = n - 2), the
 *             border the unknowns a = n - 2 and b = n - 1.  Column a of C has E2_{n-2}, E2_{n-4}, E1_{n-3} in the rows 0, n - 4, n - 3; column b has E1_{n-1}, E2_{n-1},
 *             E2_{n-3} in the rows 0, 1, n - 3 (n >= 5 keeps them apart).  Za, Zb solve B Z = C, x0 solves B x0 = f.  A product C^T x is its three terms in the order of
 *             the rows listed, from the left.  S00 = D_a - (Ca^T Za), S01 = E1_a - (Ca^T Zb), S11 = D_b - (Cb^T Zb), det = (S00 S11) - (S01 S01);
 *             ra = f_a - (Ca^T x0), rb = f_b - (Cb^T x0);  gamma_a = ((S11 ra) - (S01 rb)) / det,  gamma_b = ((S00 rb) - (S01 ra)) / det;
 *             gamma_i = (x0_i - (Za_i gamma_a)) - (Zb_i gamma_b) for i <= n - 3.
 *   Result    g_i = y_i - (lambda (winv_i (((p_im gamma_im) + (q_i gamma_i)) + (p_i gamma_ip)))): lambda = 0 and a pinned waypoint return y_i itself (y - (0 x); a
 *             coordinate that is -0 may come back as +0).  gamma are the second derivatives of the result at the waypoints.
 *   Walls     The tangent at waypoint i is the first derivative of the spline through g with the second derivatives gamma, over the input's chords:
 *             t = ((g_ip - g_i) / h_i) - ((h_i ((2 gamma_i) + gamma_ip)) / 6); at the last waypoint of an open path, from the span that ends on it:
 *             t = ((g_i - g_im) / h_im) + ((h_im ((2 gamma_i) + gamma_im)) / 6).  v = sqrt((tE tE) + (tN tN)); the left normal of the library's convention (dE/ds =
 *             -sin psi, dN/ds = cos psi, e positive to the left) is nE = (-tN) / v, nN = tE / v.  With dE = gE_i - E_i, dN = gN_i - N_i:  c = (dE nE) + (dN nN), the
 *             normal part of the displacement.  keep_walls: edge_L = edge_L - c, edge_R = edge_R - c (the tube stays where it was surveyed); else both are copied.
 *   Stats     dev_i = sqrt((dE dE) + (dN dN));  dev_max and the smallest i that reaches it;  dev_rms = sqrt(Sum((dE dE) + (dN dN)) / n);
 *             bend = Sum((0 + bE_i) + bN_i) with b_i = gamma_i ((((h_im / 6) gamma_im) + (((h_im + h_i) / 3) gamma_i)) + ((h_i / 6) gamma_ip)): gamma^T R gamma, the
 *             integral of g''^2;  n_outside counts c > edge_L or c < edge_R against the input's edges;  width_min over (edge_L - edge_R) of the output;  pivot_min over
 *             the d_r and, on a closed path, S00 and det / S00;  chord_min over the chords of the OUTPUT waypoints, computed as h_j above.
 *   Sum       Block b = 0 .. 255 holds the waypoints [b c, min((b + 1) c, n)), c = ceil(n / 256), summed from 0 in order; the 256 block totals are summed by the
 *             tree of neighbouring pairs (T_0 + T_1, T_2 + T_3, ..; then those pairwise; ..).  The order depends on the path's own n alone.
 * A pair's bits depend on its own path and set alone: not on the batch, its order or n_wp_total.  Choosing lambda is pg_tune_smoothing below.  Left out:
 * weights per waypoint inside pg_waypoint, smoothing the edges themselves, decimating (waypoints_from_tube(every=) stays the way), a device-pointer hand-over into
 * pg_fit_paths, least-squares splines with fewer knots than waypoints. */
typedef struct pg_smooth_set {
    double lambda;            /* m^3, finite and >= 0: weighs the integral of g''^2 over the chord parameter against the sum of the squared displacements */
    double u_lo[4], u_hi[4];  /* the first n_win windows, in metres of the path's cumulative chord length U; u_lo <= u_hi, neither NaN */
    double factor[4];         /* winv inside window k: finite and >= 0; 0 pins, above 1 smooths more */
    int32_t n_win;            /* 0 .. 4 */
    int32_t pin_ends;         /* != 0: the two end waypoints of an OPEN path do not move; not looked at on a closed path */
    int32_t keep_walls;       /* != 0: edge_L and edge_R of a moved waypoint are shifted by the normal part of its displacement */
    int32_t reserved;         /* 0 */
} pg_smooth_set;              /* 120 bytes */
typedef struct pg_smooth_stats {   /* one per (path, set) pair; computed in double in both libraries */
    double dev_max, dev_rms;  /* the displacement sqrt(dE dE + dN dN) over the path's waypoints, metres */
    double i_dev_max;         /* the waypoint (counted from the path's first) of dev_max */
    double bend;              /* gamma^T R gamma summed over E and N */
    double n_outside;         /* smoothed points whose normal displacement left the surveyed tube */
    double width_min;         /* the smallest edge_L - edge_R of the output */
    double pivot_min;         /* the smallest pivot of the factorisation; +Inf for two waypoints */
    double chord_min;         /* the smallest chord of the output waypoints */
    double reserved;          /* 0 */
} pg_smooth_stats;            /* 72 bytes */
/* { 0, {0 x 4}, {0 x 4}, {1 x 4}, 0, 0, 0, 0 }: the identity */
pg_smooth_set pg_default_smooth_set(void);
/* specs is the array pg_fit_paths takes; only wp0, n_wp and closed are read.  waypoints_out [n_sets][n_wp_total]: block k is the whole input array under set k, so
 * set k is fitted by adding k * n_wp_total to every wp0, and all sets in one pg_fit_paths call; a waypoint no path refers to is copied as given.  stats [n_path *
 * n_sets], pair = path * n_sets + set, the order of pg_offset_paths.  Each may be NULL.  Unlike pg_fit_paths, the waypoint ranges of two paths must not overlap (two
 * writers of one output waypoint).  Nothing is installed: waypoints are not a library.  Synchronous.  A handle that never calls this launches what it launched before.
 * PG_ERR_INVALID, everything the host can decide validated before the first allocation (the handle and its installed library are left unchanged): a null specs,
 * waypoints or sets; n_path, n_sets or n_wp_total < 1; an open path with n_wp < 2; a closed path with n_wp < 5 (band and border must not share a place); a waypoint range
 * outside [0, n_wp_total); ranges of two paths that overlap (the message names both); a non-finite waypoint field; edge_L <= edge_R; a chord that is not finite and > 0;
 * lambda or a factor of a listed window that is not finite and >= 0; n_win outside [0, 4]; a listed window with a NaN bound or u_lo > u_hi; reserved != 0; n_path *
 * n_sets beyond 31 bits or the scratch of all pairs beyond the allocation arithmetic.  After the launch and before anything is copied out, naming path, set and
 * waypoint: a pivot that is not > 0; a non-finite output; edge_L <= edge_R after keep_walls; two neighbouring output waypoints at the same point. */
int pg_smooth_waypoints(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,
                        int32_t n_sets, const pg_smooth_set* sets, pg_waypoint* waypoints_out, pg_smooth_stats* stats);

/* Choosing the smoothing weight: every (path, tune set) pair of a library of waypoint lists and a library of tune sets smoothed as pg_smooth_waypoints smooths it, under
 * the largest weight of a geometric ladder between lambda_lo and lambda_hi whose dev_rms does not exceed the set's target -- "move the points by that much rms and no
 * more" -- searched and solved on the device in one launch (tests/wp_tune_numpy.py is its twin).  The scheme has only + - * / sqrt and exact comparisons, in double in
 * both libraries, every operation rounded on its own: both libraries return the twin's bits.  A parenthesis is one rounded operation.
 *   F         F(lambda) = dev_rms (Stats of pg_smooth_waypoints) of this path under `base` with that lambda: that scheme unchanged, Sum order included.
 *   Ladder    For a bracket (lo, hi): c_0 = lo, c_16 = hi, then four levels of midpoints, each from its two neighbours on the level above:  c_8 = sqrt((c_0 c_16));
 *             c_4 = sqrt((c_0 c_8)), c_12 = sqrt((c_8 c_16));  c_2, c_6, c_10, c_14 from c_0, c_4, c_8, c_12, c_16;  the odd ones from the even ones.
 *   Round 0   The ladder of (lambda_lo, lambda_hi); F at all 17 candidates.  F(c_0) > target: verdict -1, lambda = c_0, the bracket (c_0, c_0), rms_lo = rms_hi =
 *             F(c_0), done.  Else F(c_16) <= target: verdict +1, lambda = c_16, the bracket (c_16, c_16), rms_lo = rms_hi = F(c_16), done (a path of two waypoints has
 *             F = 0 everywhere and always ends here).  Else verdict 0 and the narrowing.
 *   Narrowing j* = the smallest j in 1 .. 16 with F(c_j) > target; the new bracket is (c_{j*-1}, c_{j*}), rms_lo = F(c_{j*-1}), rms_hi = F(c_{j*}).  The rule is total
 *             (F(c_0) <= target < F(c_16) holds from round 0 on); it is bisection only where F is monotone.
 *   Rounds    Round t = 1 .. rounds - 1: the ladder of the last bracket.  Stop: where two neighbouring candidates of that ladder are equal, the round evaluates nothing
 *             and the search ends with the bracket it has.  Otherwise F at its 17 candidates (the two ends give what they gave before: evaluation is deterministic) and
 *             the narrowing.  rounds_done counts the rounds that evaluated candidates, round 0 included.
 *   monotone  1 if in every round that evaluated, F(c_j) <= F(c_{j+1}) for j = 0 .. 15; else 0.
 *   Result    lambda = lo of the last bracket, so dev_rms <= target whenever verdict is 0 or +1.  waypoints_out and stats of the pair are those of pg_smooth_waypoints
 *             under `base` with that lambda, bit for bit; rms_lo equals stats.dev_rms.
 * A pair's bits depend on its own path and set alone.  Left out: criteria other than dev_rms (dev_max, a curvature bound, cross-validation), a target per window, a
 * device-pointer hand-over into pg_fit_paths. */
typedef struct pg_tune_set {
    pg_smooth_set base;            /* windows, pin_ends, keep_walls as pg_smooth_waypoints reads them; base.lambda must be 0 */
    double target;                 /* metres, finite and > 0: the dev_rms (Stats of pg_smooth_waypoints) not to exceed */
    double lambda_lo, lambda_hi;   /* m^3, finite, 0 < lambda_lo < lambda_hi: the first bracket */
    int32_t rounds;                /* 1 .. 8: each divides the bracket's ratio by its 16th root */
    int32_t reserved;              /* 0 */
} pg_tune_set;                     /* 152 bytes */
typedef struct pg_tune_stats {     /* one per (path, set) pair, doubles */
    double lambda;                 /* the chosen weight */
    double lo, hi;                 /* the last bracket */
    double rms_lo, rms_hi;         /* dev_rms at its ends */
    double verdict;                /* 0 bracketed; -1 dev_rms(lambda_lo) > target already; +1 dev_rms(lambda_hi) <= target still */
    double rounds_done;            /* rounds that evaluated candidates */
    double monotone;               /* 1 if in every round dev_rms was non-decreasing along the ladder, else 0 */
    double reserved;               /* 0 */
} pg_tune_stats;                   /* 72 bytes */
/* base = pg_default_smooth_set(), target 1e-3, lambda_lo 1e-6, lambda_hi 1e3, rounds 3, 0 */
pg_tune_set pg_default_tune_set(void);
/* specs, waypoints, waypoints_out [n_sets][n_wp_total], stats and the pair order path * n_sets + set mean what they mean in pg_smooth_waypoints: block k is the whole
 * input array under set k, so one pg_fit_paths call still fits all sets.  tune [n_path * n_sets].  Each of the three outputs may be NULL.  Synchronous; nothing is
 * installed.  A handle that never calls this launches what it launched before.
 * PG_ERR_INVALID before the first allocation (the handle and its installed library are left unchanged): everything pg_smooth_waypoints refuses about specs, waypoints
 * and `base`; base.lambda != 0; a target that is not finite and > 0; bounds that are not finite with 0 < lambda_lo < lambda_hi; rounds outside [1, 8]; reserved != 0;
 * the scratch of all pairs beyond the allocation arithmetic.  After the launch and before anything is copied out: a pivot that is not > 0, or an F that is not finite,
 * at a candidate of any evaluated round (the message names path, set and round); then pg_smooth_waypoints' four refusals for the final solve. */
int pg_tune_smoothing(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,
                      int32_t n_sets, const pg_tune_set* sets, pg_waypoint* waypoints_out, pg_smooth_stats* stats, pg_tune_stats* tune);

/* The line inside the tube: every (path, line set) pair of a library of waypoint lists and a library of line sets as waypoints moved along their normals, each inside its
 * own edge_R .. edge_L, to the least discrete bending energy -- the line of least curvature the walls allow, which pg_plan_speeds turns into speed --, computed on the
 * device.  Waypoints in, waypoints out, as pg_smooth_waypoints: the output goes straight into pg_fit_paths.  The reference reads its paths from files
 * (src/ros_integration.jl:13-16), so the scheme is build-defined (tests/line_opt_numpy.py is its twin).  Waypoints are doubles in both libraries and ALL arithmetic is
 * double, every operation rounded on its own (no contraction); the scheme has only + - * / sqrt and exact comparisons, so both libraries return the twin's bits in every
 * output and stat.  A parenthesis is one rounded operation, a sum or product without one is taken from the left.  n = n_wp; im = i - 1, ip = i + 1, modulo n.
 *   Chords    h_j, p_j = 1 / h_j and the slopes of the INPUT waypoints exactly as pg_smooth_waypoints states them (Chords; place n - 1 of an open path holds 0),
 *             q_i = (-p_im) - p_i, and U as there (U).
 *   Normal    The tangent at waypoint i is the chord from waypoint im to waypoint ip: tE = E_ip - E_im, tN = N_ip - N_im; at the two ends of an open path it is
 *             one-sided (waypoint 0: from 0 to 1; waypoint n - 1: from n - 2 to n - 1).  v = sqrt((tE tE) + (tN tN)), nE = (-tN) / v, nN = tE / v: the library's left
 *             normal (dE/ds = -sin psi, dN/ds = cos psi, e positive to the left: the convention of Walls in pg_smooth_waypoints).  The unknown alpha_i moves waypoint i
 *             by alpha_i metres along n_i.
 *   Bend rows Every waypoint j with two neighbours has a row (all of a closed path; 1 .. n - 2 of an open one): f_j = slope_j - slope_jm per coordinate, the weight
 *             w_j = 2 / (h_jm + h_j); a waypoint without a row (the two ends of an open path) has w_j = 0.  The energy is
 *               J(alpha) = Sum_j w_j |f_j + (p_jm alpha_jm n_jm) + (q_j alpha_j n_j) + (p_j alpha_jp n_jp)|^2,
 *             the second divided difference of the moved points over the INPUT's chords (the usual linearisation: chords and normals stay the input's).
 *   Hessian   H = A^T W A + mu I, pentadiagonal in alpha and cyclic on a closed path.  With a0_i, a1_i, a2_i the closed forms of pg_smooth_waypoints (System) with w in
 *             the place of winv, each taken as 0 + (1 a) (that band with lambda = 1 and 0 in the place of its R terms), and the dot products c0_i = (nE_i nE_i) + (nN_i nN_i), c1_i = (nE_i nE_ip) + (nN_i nN_ip), c2_i = (nE_i nE_ip2) + (nN_i nN_ip2)
 *             (ip2 = i + 2 modulo n):  D_i = (c0_i a0_i) + mu;  E1_i = c1_i a1_i  [the place (i, ip)];  E2_i = c2_i a2_i  [the place (i, ip + 1)].  On an open path
 *             p_{n-1} = 0 and w_0 = w_{n-1} = 0 make the places that would wrap 0.
 *             g = A^T W f:  with k_y,j = w_j f_y,j per coordinate y,  s_y = ((p_im k_y,im) + (q_i k_y,i)) + (p_i k_y,ip);  g_i = (nE_i s_E) + (nN_i s_N).
 *   Box       margin_i = margin; then for k = 0 .. n_win - 1 in turn: where u_lo[k] <= U_i <= u_hi[k], margin_i = win_margin[k] and pinned_i = (win_pin[k] != 0) (the
 *             last listed window that holds U_i decides both).  lo_i = max(edge_R_i + margin_i, -alpha_max), hi_i = min(edge_L_i - margin_i, alpha_max); a pinned
 *             waypoint has lo_i = hi_i = 0; pin_ends pins the two ends of an OPEN path.  clip(x)_i = c where c = x if x > lo_i else lo_i, then hi_i where c > hi_i.
 *   Solve     ADMM with the scaled dual and ONE factorisation of K = H + rho I, whose band is (D_i + rho, E1_i, E2_i).  The band recurrence, the way back and the
 *             bordering are those of pg_smooth_waypoints (Band, Closed) word for word: on an open path over all n rows (m = n); on a closed one the band is the rows
 *             0 .. n - 3 with the border a = n - 2, b = n - 1, and Za, Zb, S00, S01, S11 and det are computed once.
 *             Start: z_i = clip(0)_i, u_i = 0.  Iteration k = 1, 2, ..:
 *               b_i = (rho (z_i - u_i)) - g_i;   x = K^-1 b;   z'_i = clip(x_i + u_i);   u_i = u_i + (x_i - z'_i);
 *               r_prim = max_i |x_i - z'_i|;   r_dual = rho (max_i |z'_i - z_i|);   z = z'.
 *             Both residuals are maxima (from 0, by >), so their order cannot show.  The solve stops after `iters` iterations, or after the first iteration with
 *             r_prim <= tol and r_dual <= tol (tol = 0 runs them all unless both residuals are exactly 0); iters_done = k.
 *   Result    alpha = z, inside the box by construction whatever the iteration count.  E_out = E + (alpha nE), N_out = N + (alpha nN); a waypoint with alpha = 0
 *             returns its input bits (copied, not computed).  keep_walls: edge_L = edge_L - alpha, edge_R = edge_R - alpha (the walls stay where they were surveyed,
 *             so a second call re-linearises about the first result); else both are copied.
 *   Stats     term_i(alpha) = w_i ((rE rE) + (rN rN)) with r_y = ((f_y,i + (p_im (alpha_im n_y,im))) + (q_i (alpha_i n_y,i))) + (p_i (alpha_ip n_y,ip));
 *             bend_in = Sum_i w_i ((fE_i fE_i) + (fN_i fN_i)) = J(0), bend_out = Sum_i term_i(alpha) = J(alpha), by the Sum rule of pg_smooth_waypoints;
 *             alpha_abs_max and the smallest i that reaches it;  n_active counts alpha_i == lo_i or alpha_i == hi_i (a pinned waypoint counts);  r_prim, r_dual of
 *             the last iteration;  pivot_min over the d_r and, on a closed path, S00 and det / S00;  chord_min over the chords of the OUTPUT waypoints, computed as
 *             h_j above;  width_min over (edge_L - edge_R) of the output.
 * A pair's bits depend on its own path and set alone.  The scheme is for waypoints METRES apart: the bend Hessian's condition grows like n^4, and on a dense survey (the
 * recorded ovals: 999 waypoints 0.24 m apart) this ADMM does not converge in 1000 iterations at any rho -- thin it with waypoints_from_tube(every=) first.  r_prim,
 * r_dual and iters_done tell the caller.  Left out: re-linearising inside the call (call it again on its output), minimum-time objectives, a curvature bound, weights
 * per waypoint, a device-pointer hand-over into pg_fit_paths, an adaptive rho. */
typedef struct pg_line_set {
    double mu;                /* 1/m^3, finite and > 0: the regularisation mu I of the Hessian */
    double rho;               /* 1/m^3, finite and > 0: the ADMM penalty */
    double margin;            /* metres, finite and >= 0: kept between the line and each edge */
    double alpha_max;         /* metres, finite and > 0: the largest move along the normal */
    double tol;               /* metres, finite and >= 0: stops where r_prim <= tol and r_dual <= tol */
    double u_lo[4], u_hi[4];  /* the first n_win windows, in metres of the path's cumulative chord length U; u_lo <= u_hi, neither NaN */
    double win_margin[4];     /* the margin inside window k: finite and >= 0 */
    int32_t win_pin[4];       /* != 0: window k pins its waypoints (lo = hi = 0) */
    int32_t iters;            /* 1 .. 4096 */
    int32_t n_win;            /* 0 .. 4 */
    int32_t pin_ends;         /* != 0: the two end waypoints of an OPEN path do not move; not looked at on a closed path */
    int32_t keep_walls;       /* != 0: edge_L and edge_R of a moved waypoint are shifted by -alpha */
    int32_t reserved[2];      /* 0 */
} pg_line_set;                /* 176 bytes */
typedef struct pg_line_stats {     /* one per (path, set) pair; doubles, computed in double in both libraries */
    double bend_in, bend_out; /* J(0) and J(alpha), 1/m */
    double alpha_abs_max;     /* metres */
    double i_alpha_max;       /* the waypoint (counted from the path's first) of alpha_abs_max */
    double n_active;          /* waypoints whose alpha is at a bound */
    double r_prim, r_dual;    /* of the last iteration */
    double iters_done;
    double pivot_min;         /* the smallest pivot of the factorisation of H + rho I */
    double chord_min;         /* the smallest chord of the output waypoints */
    double width_min;         /* the smallest edge_L - edge_R of the output */
    double reserved;          /* 0 */
} pg_line_stats;              /* 96 bytes */
/* { mu 1e-6, rho 0.1, margin 0.5, alpha_max 2, tol 0, windows {0 x 4}, {0 x 4}, {0 x 4}, {0 x 4}, iters 1000, 0, 0, 0, {0, 0} }: mu and rho want scaling by
 * 1 / h_mean^3 of the path (vehicles.line does it in the Python mirror) */
pg_line_set pg_default_line_set(void);
/* specs, waypoints, waypoints_out [n_sets][n_wp_total] and the pair order path * n_sets + set mean what they mean in pg_smooth_waypoints; stats [n_path * n_sets].
 * waypoints_out and stats may each be NULL.  Nothing is installed: waypoints are not a library.  Synchronous.  A handle that never calls this launches what it launched
 * before.
 * PG_ERR_INVALID before the first allocation (the handle and its installed library are left unchanged): everything pg_smooth_waypoints refuses about specs and waypoints
 * (a closed path of fewer than 5 waypoints and overlapping ranges included); mu, rho or alpha_max that is not finite and > 0; margin, tol or a listed window's margin
 * that is not finite and >= 0; iters outside [1, 4096]; n_win outside [0, 4]; a listed window with a NaN bound or u_lo > u_hi; reserved != 0; a waypoint with lo > hi
 * (the message names path, set and waypoint); the scratch of all pairs beyond the allocation arithmetic.  After the launch and before anything is copied out, naming
 * path, set and waypoint: a pivot that is not > 0; a non-finite output; two neighbouring output waypoints at the same point. */
int pg_optimize_line(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,
                     int32_t n_sets, const pg_line_set* sets, pg_waypoint* waypoints_out, pg_line_stats* stats);

/* Making the starts (pg_make_starts): the inputs of a batch -- state, control, t0, other car, time offset, what pg_set_inputs takes -- placed on the INSTALLED trajectory
 * library under a library of start sets, on the device, one lane per instance (pg_start_make.hip: k_make_starts).  The reference receives its state from the car
 * (src/ros_integration.jl:48-99), so the feature is build-defined (tests/start_make_numpy.py is its numpy twin).  After pg_make_paths / pg_fit_paths / pg_plan_speeds
 * with install != 0 the host holds no tube to interpolate; this call needs none.  "Starts" joins the sweep axes sensors x plants x tunings x tracks: a library of
 * start sets, a per-instance set index, a seed and 64-bit stream ids; every draw is a pure function of (seed, stream id, channel), never of the batch.
 *   Draws     26 uniform ranges (lo, hi) in the order of the structure = 13 channels c: s, e, dpsi, v, uy, dr, delta, fx, dt0, other_dx, other_dy, other_dpsi, other_v.
 *             Channel c takes word c % 4 of Philox4x32-10 block 4 + c / 4: key (seed_lo, seed_hi), counter (0, 4 + c / 4, stream_lo, stream_hi) -- blocks 0-3 belong to
 *             the sensor, the disturbance and the human.  u = (x + 0.5) 2^-32 in double; value = lo + (u (hi - lo)), so lo == hi gives lo exactly.
 *   s         s_first + value (s_mode 0) or s_first + (value (s_last - s_first)) (s_mode 1), clamped to [s_first, s_last] of the instance's own tube (trajectory
 *             index[b] of the installed library).  No wrap on a closed path.
 *   Lookup    the controller's own, in DOUBLE in both libraries on the channels as the library holds them (the fp32 library: every channel rounded to float):
 *             i from the count of knots < s, A = (V_i+1 - V_i) / (t_i+1 - t_i), ds = s - s_i, dt = ds / V_i where |A| < 1e-3, else (sqrt((2 A ds) + (V_i V_i)) - V_i) / A;
 *             V = V_i + (A dt), t(s) = t_i + dt (src/trajectories.jl:55-68 as written: in double the cancellation of the root costs at most 2^-52 V_i / |A| s, and this
 *             form equals the numpy statement of the reference bit for bit; the controller's own traj[s] rationalises the root, one rounding apart);  j from the count of
 *             knots <= s, w = (s - s_j) / (s_j+1 - s_j), c = c_j + (w (c_j+1 - c_j)) for psi, kappa, E, N, edge_L, edge_R (:32-35).  Every operation rounded once.
 *   Place     e = value (e_mode 0) or (0.5 (edge_L + edge_R)) + (value (0.5 (edge_L - edge_R))) (e_mode 1).  psi is measured from North, the left normal is
 *             (-cos psi, -sin psi):  E = E_p - (e cos psi_p), N = N_p - (e sin psi_p), psi = psi_p + dpsi.
 *   Body      steady 0: Ux = v V, Uy = 0, r = kappa Ux, delta = Fx = 0.  steady 1: steady_state_estimates(pg_config.vehicle, v V, A, kappa) with the reference's defaults
 *             (src/vehicle_dynamics.jl:319: 4 iterations, r = (v V) kappa, the other estimates 0), in the library's element type -- the function that seeds the cold nodes;
 *             Ux, Uy, r, delta and Fx = Fxf + Fxr are taken from it.  Then Uy += uy, r += dr, delta += delta, Fx += fx, and (Fxf, Fxr) = longitudinal_tire_forces(Fx)
 *             (:279-283).  No control limits are applied.
 *   Other     other_mode 1: in the frame of the MADE ego heading, forward (-sin psi, cos psi), left (-cos psi, -sin psi): E_o = (E + (dx (-sin psi))) + (dy (-cos psi)),
 *             N_o = (N + (dx cos psi)) + (dy (-sin psi)), psi_o = psi + dpsi_o, V_o = value.  other_mode 0: zeros.
 *   Store     state, control and other car rounded ONCE to the library's element type; t0 = t(s) + dt0, time_offset (0, or NaN with time_mode 1) and placed in double.  The
 *             host outputs are the stored values widened to double.
 * Everything but sincos (and, with steady 1, steady_state) reproduces the twin bit for bit. */
typedef struct pg_start_set {
    double s_lo, s_hi;           /* arclength: metres from the tube's first knot (s_mode 0) or fraction of its length (s_mode 1) */
    double e_lo, e_hi;           /* lateral offset, left positive: metres (e_mode 0) or fraction of the local tube (e_mode 1: e = mid + f half, mid/half from edge_L, edge_R at s) */
    double dpsi_lo, dpsi_hi;     /* heading minus path heading */
    double v_lo, v_hi;           /* factor on the tube's V(s); > 0 */
    double uy_lo, uy_hi, dr_lo, dr_hi;           /* added to Uy and r */
    double delta_lo, delta_hi, fx_lo, fx_hi;     /* added to delta and total Fx */
    double dt0_lo, dt0_hi;       /* t0 = t(s) + this */
    double other_dx_lo, other_dx_hi, other_dy_lo, other_dy_hi, other_dpsi_lo, other_dpsi_hi, other_v_lo, other_v_hi;  /* ego frame: forward, left */
    int32_t s_mode, e_mode;
    int32_t steady;              /* 0: Ux = v V(s), Uy = 0, r = kappa Ux, delta = Fx = 0;  1: steady_state_estimates(vehicle, v V(s), A(s), kappa(s)) */
    int32_t time_mode;           /* 0: time_offset = 0 (trajectory mode); 1: NaN (path mode) */
    int32_t other_mode;          /* 0: other car zeros; 1: placed relative to the ego from the other_* ranges */
    int32_t reserved[3];         /* must be 0 */
} pg_start_set;                  /* 240 bytes */
/* every range [0,0] except v = [1,1]; every mode 0: "on the profile, at the first knot" */
pg_start_set pg_default_start_set(void);
/* sets [n_sets]; set_index [B] (NULL: set 0 for every instance); stream [B] (NULL: stream[b] = b).  state_out [B][6], control_out [B][3], t0_out [B], other_out [B][4],
 * time_offset_out [B], placed_out [B][4] = (s, e, dpsi, V(s) of the tube); each may be NULL.
 * install != 0: the handle is exactly as after pg_set_inputs(h, B, state_out, control_out, t0_out, other_out, time_offset_out) -- the same buffers, the restarted rollout
 * clock, the restart of every library state --, with no host round trip.  install == 0 leaves the handle's inputs untouched.  Synchronous.  A handle that never calls this
 * launches what it launched before.
 * PG_ERR_INVALID, everything validated before the first allocation (the handle's inputs and clock are left untouched): a null sets; n_sets < 1 (the set libraries have no
 * upper bound, nor has this); B outside [1, batch_capacity]; an index outside [0, n_sets); a non-finite range field; lo > hi; v_lo <= 0; a mode outside {0, 1};
 * reserved != 0.  pg_set_inputs accepts an other car and time_offset = 0 under both formulations, so neither other_mode nor time_mode is refused under the decoupled one.
 * PG_ERR_STATE: no trajectory library installed; a library of several tubes without a trajectory index that covers B (an instance reads its own tube through it). */
int pg_make_starts(pg_handle* h, int32_t B, int32_t n_sets, const pg_start_set* sets, const int32_t* set_index, uint64_t seed, const uint64_t* stream, int32_t install,
                   double* state_out, double* control_out, double* t0_out, double* other_out, double* time_offset_out, double* placed_out);

/* control_params of one controller per instance (src/coupled_lat_long.jl:42-60, src/decoupled_lat_long.jl:32-50): a library of control-parameter sets and a per-instance
 * selection, the counterpart of pg_set_trajectories / pg_set_trajectory_index for the controller's tuning -- a tuning sweep or robustness study (the same starts and paths
 * under many weightings, speed bounds and steering-rate limits) runs as ONE batch.  With no library the handle behaves as pg_config.control says.  A library of ONE set
 * applies to every instance without an index (a handle is retuned this way without being recreated).  With n_sets > 1 the phase calls, pg_step*, pg_simulate*_dev and
 * pg_node_step_dev return PG_ERR_STATE until an index covering the current batch is installed.  Library and index persist until replaced; installing a library drops the
 * previous index.  An instance whose effective set changes (compared field by field) -- through a new library, a new index entry or pg_clear_control_param_sets -- is reset
 * as pg_reset does it (its warm start belonged to another QP); the others keep their solver state.  A rejected call (PG_ERR_INVALID) leaves the handle unchanged; a call
 * that fails with PG_ERR_HIP may have installed its library or index with the resets still owed -- pg_reset(h, NULL) settles that.  pg_get_config keeps
 * returning the creation-time config.  PG_ERR_INVALID: n_sets < 1; a set with a non-finite field, V_min >= V_max, deltadot_max <= 0, a negative weight (Q_*, W_*, R_*),
 * R_ddelta <= 0 or (coupled handle) R_dFx <= 0 -- the two rate weights make the optimum unique; pg_create does not validate pg_config.control and that stays so --; a set
 * whose N_HJI differs from the handle's (N_HJI decides which rows exist: structure, not tuning); an index entry outside [0, n_sets); B outside [1, batch_capacity].  Every
 * other field may differ between sets, W_HJI included; a decoupled handle uses the subset of fields listed at pg_default_config_decoupled.
 * Cost with n_sets > 1: a kernel keeps the address of its instance's record and loads each parameter where it uses it (scalar loads where a wavefront serves one instance,
 * per-lane loads elsewhere); the pipelined nodes + update_QP launch (pg_set_pipeline) is followed by one more small launch that rewrites the 2 B N steering-rate bounds of
 * the QP data per instance.  With no library or a library of one nothing is loaded: the set is a launch argument, as pg_config.control is.  The lateral solver keeps its
 * arrangement (four instances per wavefront) under a library. */
int pg_set_control_param_sets(pg_handle* h, int32_t n_sets, const pg_control_params* sets);
int pg_set_control_param_index(pg_handle* h, int32_t B, const int32_t* index);   /* index[b] in [0, n_sets) */
int pg_clear_control_param_sets(pg_handle* h);                                    /* back to pg_config.control */
/* the installed library: *n_sets = its size (0: none); out[0 .. min(n_sets, max_sets)) the sets as installed; index[0 .. B) the installed selection, -1 for instances the
 * index does not cover.  n_sets, out and index may each be NULL. */
int pg_get_control_param_sets(pg_handle* h, int32_t* n_sets, pg_control_params* out, int32_t max_sets, int32_t* index, int32_t B);

/* Plant sets: the vehicle the PLANT of a rollout integrates, per instance -- model-mismatch studies (the tuning under mu = 0.6 instead of 0.92; a grid of plants x tunings x
 * starts) as ONE batch.  A library of pg_vehicle sets and a per-instance selection, shaped like pg_set_control_param_sets.
 * What it replaces: mpc.dynamics in exactly ONE place, the ego `propagate` of a rollout step (src/model_predictive_control.jl:94; RK4, rk4_substeps sub-steps, world-frame
 * bicycle model through the actuator limits), in pg_simulate_dev, pg_simulate_safety_dev and pg_simulate_node_dev.  The controller's side keeps pg_config.vehicle: nodes,
 * linearisation, QP, u_normalization, the HJI relative dynamics and policy, optimal_disturbance.  pg_step*, the five phase calls and pg_node_step_dev never read the plant
 * library: they run with a library installed and no index.
 * Lifetime: a library of ONE set applies to every instance without an index.  With n_sets > 1 the three rollouts return PG_ERR_STATE until an index covering the batch is
 * installed.  Library and index persist until replaced; installing a library drops the previous index.  n_sets may be as large as batch_capacity (one plant per instance:
 * Monte Carlo).  With no library the plant is pg_config.vehicle, and the rollouts launch exactly the kernels they launched before this call existed.
 * No side effects: the plant is NO PART OF ANY QP, so -- unlike pg_set_control_param_sets -- installing, changing or clearing it resets nothing: solver state and warm
 * starts, the rollout clock, the safety, node and tracking summaries are untouched, and the captured pg_step graph is not affected.
 * PG_ERR_INVALID (the handle is left unchanged): n_sets < 1; a non-finite field; any of G, m, Izz, L, a, b, mu, Caf, Car, Fx_max, Px_max, delta_max <= 0; Fx_min >= 0; an
 * index entry outside [0, n_sets); B outside [1, batch_capacity].
 * Cost: under a library the kernel that moves the plant is another one (k_advance_lib, k_advance_safety_lib, k_node_finish_lib: lane = instance, the lane's record
 * copied into registers once per step); the launch sequence of a step does not depend on the data. */
int pg_set_plant_sets(pg_handle* h, int32_t n_sets, const pg_vehicle* sets);
int pg_set_plant_index(pg_handle* h, int32_t B, const int32_t* index);   /* index[b] in [0, n_sets) */
int pg_clear_plant_sets(pg_handle* h);                                    /* back to pg_config.vehicle */
/* the installed library: *n_sets = its size (0: none); out[0 .. min(n_sets, max_sets)) the sets as installed; index[0 .. B) the installed selection, -1 for instances the
 * index does not cover.  n_sets, out and index may each be NULL. */
int pg_get_plant_sets(pg_handle* h, int32_t* n_sets, pg_vehicle* out, int32_t max_sets, int32_t* index, int32_t B);

/* Sensor sets: the state the CONTROLLER of a rollout step reads, per instance -- tuning x plant x sensor-noise studies as ONE batch.  A library of pg_sensor sets and a
 * per-instance selection, shaped like pg_set_plant_sets.  On the car `from_autobox` carries an ESTIMATE of (E, N, psi, Ux, Uy, r) (src/ros_integration.jl:48-66); every gate,
 * projection, linearisation and HJI lookup of the callback runs on it.  With a library installed each step of pg_simulate_dev, pg_simulate_safety_dev and
 * pg_simulate_node_dev splits the state in two:
 *   TRUE state      what the plant integrates (also under a plant library), what state_hist records, pg_get_state returns and the tracking summary describes;
 *   MEASURED state  = true + bias[c] + sigma[c] z[c] per channel, in the library's element type: what everything the controller does in that step reads -- the node gate
 *                   (the Ux < 1 pause; a NaN), the projection and the time grid in path mode, nodes, linearisation, QP and solve, the HJI relative state, lookup and
 *                   policy selection (and with them the worst-case human, who is computed from that lookup), the (s, e) a node step publishes.
 *                   A channel with sigma == 0 and bias == 0 is COPIED: bit-equal, -0.0 and NaN payloads included.
 * The other car, the commands and the clock are not perturbed.  pg_step*, the five phase calls and pg_node_step_dev never read the sensor library: a caller who owns the
 * state can perturb it themselves.
 * The draws depend on nothing but (seed, stream[b], step, channel): z is standard normal from the counter-based generator Philox4x32-10 (the Random123 definition:
 * multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85, ten rounds) with key = (seed_lo, seed_hi) and counter = (step, j, stream_lo, stream_hi).
 * step is the rollout clock's step index (the one first_breach and first_exit use: it continues across calls and restarts with the clock); stream[b] is a 64-bit id per
 * instance, b by default.  Block j = 0 yields words x0..x3: (z_E, z_N) from (x0, x1), (z_psi, z_Ux) from (x2, x3); block j = 1 yields (z_Uy, z_r) from its (x0, x1) (its
 * x2, x3 are reserved).  A pair (xa, xb) becomes two normals by Box-Muller: u1 = ((xa >> 8) + 0.5) 2^-24, u2 = ((xb >> 8) + 0.5) 2^-24, rho = sqrt(-2 ln u1),
 * (rho cos 2 pi u2, rho sin 2 pi u2), the transcendentals in the library's arithmetic type.  TRUNCATION: u1 >= 2^-25, so |z| <= sqrt(-2 ln 2^-25) = 5.887.
 * (u1, u2 are exact in double.  In float n + 0.5 is exact below n = 2^23 only: the fp32 library forms ln u1 of the upper half as log1p of the complement
 * -(2^24 - n - 0.5) 2^-24, which is exact, and rounds u2 with the angle.)  Consequences: the same instance sees the same noise whatever the batch size or its position
 * in the batch; a rollout split into two calls continues the sequence; restarting the clock (pg_set_inputs*) replays it; a fresh realisation is a new seed.
 * Lifetime: a library of ONE set applies to every instance without an index.  With n_sets > 1 the three rollouts return PG_ERR_STATE until an index covering the batch is
 * installed.  Installing a library drops the previous index; seed and streams persist (also across pg_clear_sensor_sets).  With no library the controller reads the true
 * state, nothing is allocated and the rollouts queue exactly the launches they queued before this call existed.
 * No side effects: installing, changing or clearing library, index, seed or streams resets nothing -- solver state and warm starts, the rollout clock, the safety, node and
 * tracking summaries are untouched, and the captured pg_step graph is not affected.
 * PG_ERR_INVALID (the handle is left unchanged): n_sets < 1; a non-finite field; sigma[c] < 0; an index entry outside [0, n_sets); B outside [1, batch_capacity].
 * Cost: one lane-per-instance launch per rollout step (k_measure) ahead of the step's gate and compute kernels, which are handed the measured buffer in place of the state
 * (no copy, no kernel changed); with the tracking summary on, one more projection launch, of the true state (the step's own projection is the measured one). */
typedef struct pg_sensor { double sigma[6]; double bias[6]; } pg_sensor;      /* (E, N, psi, Ux, Uy, r) */
int pg_set_sensor_sets(pg_handle* h, int32_t n_sets, const pg_sensor* sets);
int pg_set_sensor_index(pg_handle* h, int32_t B, const int32_t* index);          /* index[b] in [0, n_sets) */
/* seed (default 0) and stream ids: stream [B], or NULL for stream[b] = b; instances the array does not cover keep stream[b] = b.  Needs no library */
int pg_set_sensor_seed(pg_handle* h, uint64_t seed, int32_t B, const uint64_t* stream);
int pg_clear_sensor_sets(pg_handle* h);                                          /* back to measured = true */
/* the installed library, as pg_get_plant_sets */
int pg_get_sensor_sets(pg_handle* h, int32_t* n_sets, pg_sensor* out, int32_t max_sets, int32_t* index, int32_t B);
/* the z the rollouts draw for clock steps [step0, step0 + steps), z [steps][B][6] on the host, computed ON THE DEVICE by the function k_measure calls (k_sensor_draws) --
 * what pg_simulate_clock is to the clock.  Reads seed and streams only: needs no library and no inputs.  step0 >= 0, steps >= 1, B in [1, batch_capacity] */
int pg_sensor_draws(pg_handle* h, int32_t step0, int32_t steps, int32_t B, double* z);
/* measured [B][6] of the last rollout step that ran under a library; PG_ERR_STATE before one (installing inputs or clearing the library forgets it) */
int pg_get_measured_state(pg_handle* h, double* measured);
/* the NEXT rollout call writes the measured state of its step k < steps to buf[k][B][6] (library element type); one-shot -- that call consumes the registration whether it succeeds or returns an error --; NULL cancels.  PG_ERR_STATE without a library */
int pg_set_measured_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps);

/* Actuator sets: what the PLANT of a rollout step integrates in place of the command, per instance -- tuning x plant x sensor x actuator studies as ONE batch.  A library of
 * pg_actuator_set and a per-instance selection, shaped like pg_set_plant_sets.  BUILD-DEFINED: the reference has no actuator.  Its `simulate` applies the command of the
 * previous step exactly (src/model_predictive_control.jl:94-95); on the car `from_autobox_callback` (src/ros_integration.jl:51-52) sets `current_control` to the command
 * last SENT (:52), the line that would take the steering and forces last MEASURED is commented out above it (:51), so the node linearises and rate-limits about an input
 * the car has not reached yet.  With a library installed pg_simulate_dev and pg_simulate_safety_dev keep, per instance and channel j of (delta, Fxf, Fxr), at clock
 * step k with command c_k (what `control` holds at the start of the step):
 *   g   = c_{k - delay_steps}                            (entries before the clock's first step = c at the clock start)
 *   y   = tau == 0 ? g : a_{k-1} + alpha (g - a_{k-1}),  alpha = -expm1(-dt / tau), in the library's element type
 *   a_k = rate == +Inf ? y : a_{k-1} + clamp(y - a_{k-1}, -rate dt, +rate dt),      a_{-1} = c at the clock start
 * (tau, rate) = (tau_delta, rate_delta) for delta and (tau_fx, rate_fx) for each of Fxf, Fxr.  The plant of step k integrates a_k, held for the step (the StepControl of :94
 * with a_k in place of c_k).  tau == 0 and rate == +Inf are COPIES without arithmetic: the identity set {0, 0, 0, 0, +Inf, +Inf} reproduces the handle without a library bit
 * for bit, -0.0 and NaN payloads included.
 * feedback: 0 = the controller's current_control (node 0 of the horizon, u_curr of the QP, the steering-rate rows) is the command last sent (:52, the deployed node);
 *           1 = it is the actuator's position a_k (:51, the commented-out line).
 * The control RECORD of a rollout under a library (control_hist_dev of pg_simulate_dev, the `push!(us, ...)` of :89; control_hist_dev of pg_simulate_safety_dev) is the APPLIED
 * control a_k: the recorded step replays through the plant.  The commands are available through pg_set_command_history_dev; pg_get_state's control stays the command.
 * State: a [B][3], the last PG_ACT_MAX_DELAY commands and their position restart WITH THE ROLLOUT CLOCK (pg_set_inputs*, another dt, another path end); a rollout call that
 * continues the clock continues them.  Installing sets or an index between rollouts resets nothing: an instance whose delay grew reads older commands that are already there.
 * Lifetime, index rule and errors as pg_set_plant_sets.  PG_ERR_INVALID (the handle is left unchanged): delay_steps outside [0, PG_ACT_MAX_DELAY]; tau_delta / tau_fx
 * negative or not finite; rate_delta / rate_fx not > 0 (NaN included; +Inf is valid); feedback other than 0 / 1 -- the message names the field and the set.
 * OUT OF SCOPE: the node callback keeps "message" and "applied" apart and leaves `applied` unwritten for a gated-out instance, so the next command cannot be handed back by a
 * plain copy: pg_simulate_node_dev and pg_node_step_dev return PG_ERR_STATE while an actuator library is installed.  pg_step* and the phase calls ignore the library.
 * Cost: one lane-per-instance launch (k_actuate) ahead of the step's compute kernels and one device-to-device copy of B x 3 elements behind the plant kernel, which is
 * handed a buffer holding a_k as its `control` and leaves the next command there (no kernel changed).  Without a library: nothing allocated, the launches of before. */
#define PG_ACT_MAX_DELAY 16
typedef struct pg_actuator_set { int32_t delay_steps; int32_t feedback; double tau_delta; double tau_fx; double rate_delta; double rate_fx; } pg_actuator_set;
int pg_set_actuator_sets(pg_handle* h, int32_t n_sets, const pg_actuator_set* sets);
int pg_set_actuator_index(pg_handle* h, int32_t B, const int32_t* index);        /* index[b] in [0, n_sets) */
int pg_clear_actuator_sets(pg_handle* h);                                        /* back to applied = command */
/* the installed library, as pg_get_plant_sets */
int pg_get_actuator_sets(pg_handle* h, int32_t* n_sets, pg_actuator_set* out, int32_t max_sets, int32_t* index, int32_t B);
/* the NEXT rollout call writes a_k (applied) / c_k (command) of its step k < steps to buf[k][B][3] (library element type); one-shot -- that call consumes the registration
 * whether it succeeds or returns an error --; NULL cancels.  PG_ERR_STATE without a library */
int pg_set_applied_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps);
int pg_set_command_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps);
/* applied [B][3] = a of the last rollout step under a library; before the first such step since the clock restarted: the handle's control */
int pg_get_actuator_state(pg_handle* h, double* applied);
/* the law alone, ON THE DEVICE through the function k_actuate calls (k_actuator_response): commands [steps][B][3] on the host -> applied [steps][B][3], with the installed
 * library and index over the current batch B (pg_set_inputs*), from a fresh state (a_{-1} = commands[0]).  Touches neither the rollout clock nor the handle's actuator
 * state (scratch of its own).  steps >= 1, dt > 0; PG_ERR_STATE without inputs, without a library or with an index that does not cover the batch */
int pg_actuator_response(pg_handle* h, int32_t steps, double dt, const double* commands, double* applied);

/* Disturbance sets: what acts on the car FROM OUTSIDE in a rollout step, per instance -- a side wind, a headwind or grade force, a seeded gust, a low-friction window in the
 * middle of a corner -- tuning x plant x sensor x actuator x disturbance studies as ONE batch.  A library of pg_disturbance, a per-instance selection, a seed and 64-bit
 * stream ids, shaped like pg_set_sensor_sets.  BUILD-DEFINED: the reference has no counterpart.  Its `simulate` integrates the nominal model
 * (src/model_predictive_control.jl:94) and the tube's theta, phi are carried and read by nothing.
 * With a library installed the EGO plant of a step of pg_simulate_dev, pg_simulate_safety_dev and pg_simulate_node_dev integrates the body model plus
 * w_k = (wFx, wFy, wMz, wmu), held for the step.  Per instance at clock step k (the step index of first_breach, first_exit and the sensor draws):
 *   (z_x, z_y) = Box-Muller of words (x0, x1) of Philox4x32-10 block j = 2: counter (k, 2, stream_lo, stream_hi), key = the DISTURBANCE library's own seed; u and the
 *                Box-Muller construction as for the sensor draws (blocks 0 and 1 belong to them; words x2, x3 of block 2 are reserved).  stream[b] defaults to b.
 *   n_k        = z_k                                                                    when there is no state of step k - 1, or tau_gust == 0
 *              = rho n_{k-1} + sqrt(-expm1(-2 dt / tau_gust)) z_k,  rho = exp(-dt / tau_gust)      otherwise, per component, in the library's element type, every product
 *                and sum rounded once.  Both forms are stationary with unit variance.  The state advances at EVERY step under a library, inside the window or not.
 *                "No state of step k - 1": the clock's first step (pg_set_inputs*, another dt, another path end restart it, as they restart the actuator state) and the
 *                first step after a library was installed on a handle that had none (pg_clear_disturbance_sets drops the state).  Installing sets, an index, a seed or
 *                streams over an installed library resets nothing.
 *   active     = step_on <= k and (step_off < 0 or k < step_off)
 *   w_k        = (0, 0, 0, 1)                                                           when not active
 *              = (Fx + sigma_Fx n_x,  Fy + g_y,  Mz + x_cp g_y,  mu_scale),  g_y = sigma_Fy n_y     when active.  A sigma of exactly 0 contributes nothing: no multiply
 *                and no add (the component is the constant itself).
 * The plant of step k integrates, in EVERY RK4 sub-step, dUx += wFx / m, dUy += wFy / m, dr += wMz / Izz on top of the body model, whose tire model uses mu * wmu.
 * m, Izz and mu are those of the plant's own vehicle: the instance's plant set under a plant library, else pg_config.vehicle.
 * ZERO RULE: a component of w that is exactly 0 is not added and wmu == 1 is not multiplied, so the identity set {0, -1, 0, 0, 0, 0, 0, 0, 0, 1} and any set outside its
 * window reproduce the handle without a library bit for bit.
 * The CONTROLLER never sees w: nodes, linearisation, QP, HJI dynamics and policy keep pg_config.vehicle and no force.  The other car is not disturbed.  pg_step*, the phase
 * calls and pg_node_step_dev ignore the library.
 * Lifetime, index rule and errors as pg_set_plant_sets.  PG_ERR_INVALID (the handle is left unchanged; the message names the field and the set): a non-finite field;
 * sigma_Fx / sigma_Fy < 0; tau_gust < 0; mu_scale <= 0; step_on < 0.
 * Cost: one lane-per-instance launch (k_disturb) at the top of the step, and the step's plant kernel is the library kernel's instantiation with a disturbance.  Without a library: nothing
 * allocated, the launches of before. */
typedef struct pg_disturbance {
    int32_t step_on, step_off;     /* active at clock steps k with step_on <= k and (step_off < 0 or k < step_off) */
    double  Fx, Fy, Mz;            /* body-frame force at the CG (N), yaw moment (N m), constant while active */
    double  sigma_Fx, sigma_Fy;    /* stationary standard deviation of the gust force (N) */
    double  x_cp;                  /* the gust's Fy acts x_cp metres ahead of the CG: gust moment = x_cp * gust Fy */
    double  tau_gust;              /* correlation time of the gust (s); 0 = white */
    double  mu_scale;              /* the plant's mu is multiplied by this while active */
} pg_disturbance;                  /* 72 bytes */
int pg_set_disturbance_sets(pg_handle* h, int32_t n_sets, const pg_disturbance* sets);
int pg_set_disturbance_index(pg_handle* h, int32_t B, const int32_t* index);     /* index[b] in [0, n_sets) */
/* key of the draws and stream[b] for b < B (NULL: stream[b] = b; instances beyond B: b), as pg_set_sensor_seed.  Both persist across pg_clear_disturbance_sets and a later install */
int pg_set_disturbance_seed(pg_handle* h, uint64_t seed, int32_t B, const uint64_t* stream);
int pg_clear_disturbance_sets(pg_handle* h);                                     /* back to the undisturbed plant */
/* the installed library, as pg_get_plant_sets */
int pg_get_disturbance_sets(pg_handle* h, int32_t* n_sets, pg_disturbance* out, int32_t max_sets, int32_t* index, int32_t B);
/* the law alone, ON THE DEVICE through the function k_disturb calls (k_disturbance_response): w_out [steps][B][4] on the host = w of the clock steps [step0, step0 + steps)
 * with the installed library, index, seed and streams over the current batch B (pg_set_inputs*), from a FRESH gust state at step0.  Touches neither the rollout clock nor
 * the handle's gust state.  step0 >= 0, steps >= 1, dt > 0; PG_ERR_STATE without inputs, without a library or with an index that does not cover the batch */
int pg_disturbance_response(pg_handle* h, int32_t step0, int32_t steps, double dt, double* w_out);
/* w [B][4] of the last rollout step under a library; PG_ERR_STATE before the first one since the inputs were installed */
int pg_get_disturbance_state(pg_handle* h, double* w);
/* the NEXT rollout call writes w of its step k < steps to buf[k][B][4] (library element type); one-shot -- that call consumes the registration whether it succeeds or
 * returns an error --; NULL cancels.  PG_ERR_STATE without a library */
int pg_set_disturbance_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps);

/* Estimator sets: the block between the sensor and the controller of a rollout step, per instance -- a fixed-gain observer that blends the measurement with a model
 * prediction -- tuning x plant x sensor x actuator x disturbance x estimator studies as ONE batch.  A library of pg_estimator and a per-instance selection, shaped like
 * pg_set_actuator_sets.  BUILD-DEFINED: the reference has no estimator; its node receives an estimate from the car (src/ros_integration.jl:48-52).
 * With a library installed the gate and the compute calls of a step of pg_simulate_dev, pg_simulate_safety_dev and pg_simulate_node_dev read the ESTIMATE xh_k in place of
 * the state.  Per instance at clock step k (the step index of first_breach, first_exit and the sensor draws):
 *   y_k      = the sensor's output of the step: the measured state under a sensor library, else the true state
 *   u_{k-1}  = the control the controller was handed at step k - 1 (the command; under an actuator library with feedback == 1 the actuator's position)
 *   p_k      = advance(xh_{k-1}, u_{k-1}, dt)      predict == 1: one step of the CONTROLLER's model, pg_config.vehicle (never the plant library's) -- RK4 with rk4_substeps
 *                                                  sub-steps over the rollout's dt, (delta, Fx = Fxf + Fxr) held, exactly as the plant of a handle without libraries integrates
 *            = xh_{k-1}                            predict == 0: every channel an exponential low-pass of the measurement
 *   xh_k[c]  = p_k[c] + gain[c] (y_k[c] - p_k[c])  per channel c of (E, N, psi, Ux, Uy, r), in the library's element type, the product and the two sums rounded once each.
 *                                                  A plain difference on psi as well: the plant's psi is the unwrapped integral of r.  gain[c] == 1 COPIES y_k[c] and
 *                                                  gain[c] == 0 COPIES p_k[c]: no arithmetic.
 *   xh_k     = y_k                                 when no estimate of step k - 1 exists: the first rollout step after pg_set_inputs*, after the clock restarted (another
 *                                                  dt, another path end) or after pg_clear_estimator_sets.  Installing sets or an index resets nothing.
 *   xh_k     = y_k                                 for an instance whose prior p_k has a non-finite component: that instance's estimator starts again
 * IDENTITY: a set whose six gains are all 1 runs no prediction and copies y_k, so {predict, 0, {1, 1, 1, 1, 1, 1}} reproduces the handle without a library bit for bit.
 * What follows the estimate: the node gates (low speed reads xh's Ux), the projection and the (s, e) a node step publishes, the linearisation nodes, the QP's q_curr, the
 * HJI relative state, the policy selection and the worst-case human.  What keeps the truth: the plant, the records (state_hist), pg_get_state and the tracking summary
 * (with the summary on, the true state is projected once more per step, as under a sensor library).  pg_step*, the phase calls and pg_node_step_dev ignore the library.
 * The node rollout runs under it; a gated-out instance's estimator advances like every other.
 * Lifetime, index rule and errors as pg_set_plant_sets.  PG_ERR_INVALID (the handle is left unchanged; the message names the set and the field): a gain outside [0, 1] or
 * not finite; predict not 0 or 1; reserved != 0.
 * Cost: one lane-per-instance launch (k_estimate) per step, behind k_measure; its observer lanes run one RK4 step.  Without a library: nothing allocated, the launches of
 * before; the read-only option "stat_estimator_steps" (rollout steps that ran under a library) stays 0. */
typedef struct pg_estimator {
    int32_t predict;               /* 1: the prior is one step of the controller's model; 0: the prior is the previous estimate */
    int32_t reserved;              /* must be 0 */
    double  gain[6];               /* per channel of (E, N, psi, Ux, Uy, r), each in [0, 1]: 1 = the measurement itself, 0 = the prior alone */
} pg_estimator;                    /* 56 bytes */
int pg_set_estimator_sets(pg_handle* h, int32_t n_sets, const pg_estimator* sets);
int pg_set_estimator_index(pg_handle* h, int32_t B, const int32_t* index);       /* index[b] in [0, n_sets) */
int pg_clear_estimator_sets(pg_handle* h);                                       /* back to the sensor's output; the estimate is dropped */
/* the installed library, as pg_get_plant_sets */
int pg_get_estimator_sets(pg_handle* h, int32_t* n_sets, pg_estimator* out, int32_t max_sets, int32_t* index, int32_t B);
/* estimated [B][6] = xh of the last rollout step under a library; PG_ERR_STATE before the first one since the inputs were installed */
int pg_get_estimated_state(pg_handle* h, double* estimated);
/* the NEXT rollout call writes xh of its step k < steps to buf[k][B][6] (library element type); one-shot -- that call consumes the registration whether it succeeds or
 * returns an error --; NULL cancels.  PG_ERR_STATE without a library */
int pg_set_estimated_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps);
/* the law alone, ON THE DEVICE through the function k_estimate calls (k_estimator_response): y [steps][B][6] and u [steps][B][3] on the host (u[k]: the control the
 * controller is handed at step k; step k's prior is driven by u[k - 1], so u[steps - 1] is read by nothing) -> xhat [steps][B][6], with the installed library and index
 * over the current batch B (pg_set_inputs*), from a fresh state (xhat[0] = y[0]).  Touches neither the rollout clock nor the handle's estimate (scratch of its own).
 * steps >= 1, dt > 0; PG_ERR_STATE without inputs, without a library or with an index that does not cover the batch */
int pg_estimator_response(pg_handle* h, int32_t steps, double dt, const double* y, const double* u, double* xhat);

/* Human sets: the DRIVER OF THE OTHER CAR in pg_simulate_safety_dev and pg_simulate_node_dev, per instance -- which kind of driver the deployed law keeps V > 0 against, as
 * ONE batch with the other seven axes.  A library of pg_human and a per-instance selection, shaped like pg_set_disturbance_sets (a seed and 64-bit stream ids of its own).
 * BUILD-DEFINED: the reference only receives the other car from ROS.
 * With a library installed the two rollouts queue one lane-per-instance launch (k_human) per step, behind the step's compute calls and tracking summary -- mode 1 reads the
 * step's relative state and HJI lookup -- and ahead of the launch that moves the plants, which is handed the result as a script (its human_mode = 2: it records and
 * integrates what it is handed).  Per instance at clock step k (the step index of first_breach, first_exit and the sensor draws):
 *   not active (k < step_on, or step_off >= 0 and k >= step_off):   u_k = (0, 0)
 *   active, deciding -- (k - step_on) % hold_steps == 0, or no u of step k - 1 exists (the clock restarted, the first step after a library was installed on a handle that
 *   had none, the first step after pg_clear_human_sets):
 *       raw   = (0, 0)                                   mode 0
 *             = what human_mode = 1 applies               mode 1: optimal_disturbance at the step's relative state; (0, 0) without a grid, on a decoupled handle and where
 *                                                         the other car's speed is <= 0
 *             = human_u_dev[k][b]                         mode 2
 *             = (sigma[0] n_w, sigma[1] n_a)              mode 3: n is the unit-variance AR(1) of the gust (pg_disturbance: n_k = z_k on a missing state or tau == 0, else
 *                                                         rho n_{k-1} + sqrt(-expm1(-2 dt / tau)) z_k, rho = exp(-dt / tau)), z = Box-Muller of words (x0, x1) of Philox
 *                                                         block 3, counter (k, 3, stream_lo, stream_hi), key = THIS library's seed (blocks 0 to 2 are the sensor's and the
 *                                                         gust's).  n advances at every step for an instance whose set has mode 3, active or not.  sigma == 0: exactly 0
 *       u[c]  = gain[c] raw[c]  (gain[c] == 1 COPIES), then |omega| <= omega_max and a_min <= a <= a_max by compare-and-select: a value inside the limits keeps its bits
 *   active, not deciding:                                           u_k = u_{k-1}, copied
 * IDENTITY: {m, 1, 0, -1, {1, 1}, +Inf, -Inf, +Inf, {0, 0}, 0} reproduces a rollout called with human_mode = m on a handle without a library bit for bit, m in {0, 1, 2}.
 * Under a library the rollouts' human_mode argument is still validated but the sets decide; human_u_dev is required exactly when an installed set has mode 2
 * (PG_ERR_INVALID otherwise).  pg_simulate_dev, pg_step*, the phase calls and pg_node_step_dev ignore the library.  The driver's state (u_{k-1}, n) restarts with the
 * rollout clock and continues across calls; installing sets, an index, a seed or streams over an installed library resets nothing.
 * Lifetime, index rule and errors as pg_set_plant_sets.  PG_ERR_INVALID (the handle is left unchanged; the message names the set and the field): mode outside 0..3;
 * hold_steps < 1; step_on < 0; a gain outside [0, 1] or not finite; a NaN limit, omega_max < 0, a_min > 0 or a_max < 0; a sigma or tau negative or not finite.
 * Without a library: nothing allocated, the launches of before; the read-only option "stat_human_steps" (rollout steps that ran under a library) stays 0. */
typedef struct pg_human {
    int32_t mode;                  /* 0 hold, 1 worst case (optimal_disturbance), 2 the caller's script, 3 seeded random */
    int32_t hold_steps;            /* >= 1: the driver decides at active steps with (k - step_on) % hold_steps == 0 and keeps (omega, a) in between */
    int32_t step_on, step_off;     /* active at clock steps k with step_on <= k and (step_off < 0 or k < step_off), as pg_disturbance */
    double  gain[2];               /* factor on the decided (omega, a), each in [0, 1] */
    double  omega_max;             /* |omega| <= omega_max; +Inf: no limit */
    double  a_min, a_max;          /* a_min <= a <= a_max, a_min <= 0 <= a_max; -Inf / +Inf: no limit */
    double  sigma[2];              /* mode 3: stationary standard deviation of (omega, a) */
    double  tau;                   /* mode 3: correlation time (s); 0 = white */
} pg_human;                        /* 80 bytes */
int pg_set_human_sets(pg_handle* h, int32_t n_sets, const pg_human* sets);
int pg_set_human_index(pg_handle* h, int32_t B, const int32_t* index);           /* index[b] in [0, n_sets) */
/* key of the mode-3 draws and the stream id per instance, as pg_set_disturbance_seed (stream == NULL: stream[b] = b); a library of its own seed: 0 until set */
int pg_set_human_seed(pg_handle* h, uint64_t seed, int32_t B, const uint64_t* stream);
int pg_clear_human_sets(pg_handle* h);                                           /* back to the rollouts' human_mode; the driver's state is dropped */
/* the installed library, as pg_get_plant_sets */
int pg_get_human_sets(pg_handle* h, int32_t* n_sets, pg_human* out, int32_t max_sets, int32_t* index, int32_t B);
/* u [B][2] = (omega, a) of the last rollout step under a library; PG_ERR_STATE before the first one since the inputs were installed */
int pg_get_human_state(pg_handle* h, double* u);
/* the NEXT rollout call writes (omega, a) of its step k < steps to buf[k][B][2] (library element type); one-shot -- that call consumes the registration whether it succeeds or
 * returns an error --; NULL cancels.  PG_ERR_STATE without a library.  (The node rollout has no human history of its own.) */
int pg_set_human_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps);
/* the law alone, ON THE DEVICE through the function k_human calls (k_human_response): x7 [steps][B][7] and vg8 [steps][B][8] (V, then the gradient) on the host, script
 * [steps][B][2] or NULL (required when an installed set has mode 2) -> u_out [steps][B][2] of the clock steps [step0, step0 + steps), with the installed library, index, seed
 * and streams over the current batch B (pg_set_inputs*), from a fresh state at step0.  Mode 1 reads the grid as the rollouts do (none, or a decoupled handle: (0, 0)).
 * Touches neither the rollout clock nor the handle's driver state.  step0 >= 0, steps >= 1, dt > 0; PG_ERR_STATE without inputs, without a library or with an index that
 * does not cover the batch */
int pg_human_response(pg_handle* h, int32_t step0, int32_t steps, double dt, const double* x7, const double* vg8, const double* script, double* u_out);

/* Route sets: the TRAJECTORY an instance tracks CHANGES DURING a rollout, per instance -- nominal_trajectory_callback of the node (src/ros_integration.jl:30-41: a /des_traj
 * message brings a new tube and time_offset = its stamp, a /des_path message a new tube and time_offset = NaN, either one sets mpc.solved = false) as a ninth library
 * beside the other eight axes: per instance a list of up to PG_ROUTE_EVENTS events "at clock step k, go to trajectory j of the installed library, anchored so".
 * With a library installed pg_simulate_dev, pg_simulate_safety_dev and pg_simulate_node_dev queue one launch (k_route, one wavefront per instance) on the clock steps that
 * carry an event in some installed set (and on every step of a call with a registered route history), behind the step's k_measure / k_estimate and ahead of the node gate
 * and the compute calls.  An event of instance b fires when the clock step (the step index of first_breach, first_exit and the sensor draws) equals ev.step; with t0[b] the
 * instance's clock time at that step it writes
 *   the trajectory index of b, in place     target_mode PG_ROUTE_ABSOLUTE: target; PG_ROUTE_RELATIVE: (current + target) mod n_traj, target may be negative
 *   time_offset[b]                          anchor PG_ROUTE_KEEP:    unchanged (the new trajectory shares the old one's time base: another plan set of the same path)
 *                                                  PG_ROUTE_PATH:    NaN, path-tracking mode (the /des_path callback, :30-35)
 *                                                  PG_ROUTE_STAMP:   t0[b] - t_join (t_join = 0: the /des_traj callback, :36-41 -- the new trajectory's t = 0 is now)
 *                                                  PG_ROUTE_PROJECT: t0[b] - (t_proj + t_join), t_proj = the third path coordinate (pg_get_path_coordinates) of the state
 *                                                                    the step's controller is handed (measured / estimated under those libraries) projected on the TARGET
 *                                                                    trajectory -- a planner that hands over a trajectory already in progress.  BUILD-DEFINED.  A non-finite
 *                                                                    pose gives time_offset = NaN; the index still switches
 *   with cold = 1: solved = false           as the reference's callback; cold = 0 keeps the warm start (BUILD-DEFINED: the previous solution belongs to the old trajectory)
 *   the route state (pg_get_route_state)    fired += 1, last_step = k, t_at, e_at
 * time_offset arithmetic is double in both libraries, the projection is the library's element type (the statements of the step's own projection: t_at and e_at of a PROJECT
 * event equal what pg_get_path_coordinates reports for that state on the target, bit for bit).  On a clock step that carries an event the host takes the launches of a batch
 * with a cold instance (as after pg_reset with a mask); the nodes kernels read `solved` per instance.
 * STATE.  The index pg_set_trajectory_index installed is the instance's HOME.  When the rollout clock restarts (new inputs, another dt) the next rollout under a library first
 * puts every instance back on its home trajectory with fired = 0 (time_offset is whatever the inputs carry); consecutive calls continue.  After a rollout pg_step* and the
 * phase calls run on the trajectory the instance switched to.  pg_set_trajectory_index installs home and current together; pg_clear_route_sets leaves the current index as
 * it is.  The other libraries' states (gust, streams, actuator ring, estimate, driver), the clock and the summaries do not restart at a switch; the tracking summary follows
 * the CURRENT trajectory (its "last s" and the tube test change trajectory with the instance).
 * IDENTITY: pg_default_route() (no event).  A library whose sets hold no event queues the launches of a handle without one and reproduces it bit for bit (the read-only option
 * "stat_route_steps" counts the k_route launches).
 * A rollout under a library wants a trajectory library of at least two trajectories whose index covers the batch, every absolute target < n_traj (checked when the rollout
 * starts: the trajectory library may be replaced after the route sets are installed), and with several sets pg_set_route_index covering the batch: PG_ERR_STATE otherwise.
 * Lifetime, index rule and errors as pg_set_plant_sets.  PG_ERR_INVALID (the handle is left unchanged; the message names the set): a used slot (step >= 0) behind an unused
 * one, steps of the used slots not strictly increasing, target_mode / anchor / cold out of range, t_join not finite or != 0 under KEEP / PATH, an absolute target < 0,
 * reserved != 0.  pg_abi_layout is unchanged (sizeof(pg_route) = 128 is asserted where the library is compiled). */
#define PG_ROUTE_EVENTS 4
enum pg_route_target_mode { PG_ROUTE_ABSOLUTE = 0, PG_ROUTE_RELATIVE = 1 };
enum pg_route_anchor { PG_ROUTE_KEEP = 0, PG_ROUTE_PATH = 1, PG_ROUTE_STAMP = 2, PG_ROUTE_PROJECT = 3 };
typedef struct pg_route_event {
    int32_t step;                  /* clock step at which it fires, ahead of that step's controller; < 0: unused slot */
    int32_t target;                /* PG_ROUTE_ABSOLUTE: library index; PG_ROUTE_RELATIVE: (current + target) mod n_traj, target may be negative */
    int32_t target_mode;           /* PG_ROUTE_ABSOLUTE 0 | PG_ROUTE_RELATIVE 1 */
    int32_t anchor;                /* PG_ROUTE_KEEP 0 | PG_ROUTE_PATH 1 | PG_ROUTE_STAMP 2 | PG_ROUTE_PROJECT 3 */
    int32_t cold;                  /* 1: solved = false, as the reference's callback (default); 0: keep the warm start */
    int32_t reserved;              /* 0 */
    double  t_join;                /* seconds, STAMP / PROJECT only (0 otherwise) */
} pg_route_event;                  /* 32 bytes */
typedef struct pg_route { pg_route_event ev[PG_ROUTE_EVENTS]; } pg_route;      /* 128 bytes */
pg_route pg_default_route(void);                                                 /* no event: the identity set (every slot {-1, 0, 0, PG_ROUTE_STAMP, 1, 0, 0.0}) */
int pg_set_route_sets(pg_handle* h, int32_t n_sets, const pg_route* sets);
int pg_set_route_index(pg_handle* h, int32_t B, const int32_t* index);           /* index[b] in [0, n_sets) */
int pg_clear_route_sets(pg_handle* h);                                           /* the current trajectory index stays as the events left it */
/* the installed library, as pg_get_plant_sets */
int pg_get_route_sets(pg_handle* h, int32_t* n_sets, pg_route* out, int32_t max_sets, int32_t* index, int32_t B);
/* [B] each, any may be NULL: traj = the trajectory the instance is on now; fired = events since the clock last restarted; last_step = clock step of the last one (-1: none);
 * t_at = where the new trajectory was joined at that event -- PROJECT: t_proj; STAMP: t_join; KEEP: t0 - time_offset; PATH: NaN --; e_at = the lateral offset of that
 * projection (NaN unless PROJECT).  Before the first rollout step since the clock restarted: fired 0, last_step -1, t_at and e_at NaN, and traj still the trajectory the
 * instance was left on -- the return home is applied when the next rollout starts, and until then pg_step* and the phase calls run on what traj reports.  PG_ERR_STATE without inputs or without a library */
int pg_get_route_state(pg_handle* h, int32_t* traj, int32_t* fired, int32_t* last_step, double* t_at, double* e_at);
/* the NEXT rollout call writes the trajectory the controller of its step k < steps ran on to buf[k][B] (int32, device memory); one-shot -- that call consumes the
 * registration whether it succeeds or returns an error --; (NULL, 0) cancels, NULL with steps != 0 and steps < 1 are PG_ERR_INVALID.  PG_ERR_STATE without a library */
int pg_set_route_history_dev(pg_handle* h, int32_t* buf, int32_t steps);

/* mpc.HJI_cache = HJICache(grid_knots, V_raw, gradV_raw)  src/HJI_computation.jl:26-57.  V is column-major (dim 1 fastest),
 * gradV is 7 floats per node in the same node order.  Without a grid the safety row is inactive (M = 0, b = 1).
 * An install first drops the installed grid and then builds the new table (never two tables side by side: the cell records of the real grid take 1.9 to 19 GB).
 * After an install that fails past the argument checks (PG_ERR_HIP: an allocation, a copy, the build launch) the handle has NO HJI grid, no device memory of the call
 * remains, and pg_last_error says why.  The same holds for pg_hji_solve with install != 0 once its sweeps have succeeded. */
int pg_set_hji_grid(pg_handle* h, const int32_t dims[7], const float* knots_concat, const float* V, const float* gradV);
int pg_clear_hji_grid(pg_handle* h);

/* Making a grid: the backward reachable tube of the relative system, computed on the device for the handle's vehicle or for any pg_vehicle.  Stands in for the external
 * level-set toolbox run whose result the reference downloads (deps/build.jl:1-4: BicycleCAvoid.jld2); the reference itself holds no solver, so the scheme is
 * build-defined (tests/hji_solve_numpy.py is its numpy twin).  The roles are those of src/HJI_computation.jl:74-158: the robot maximises with
 * optimal_control(X, x, p, :max, N = 50) (:133-158), the human minimises with optimal_disturbance(X, x, p, :min) (:90-131; (0, 0) at a knot V <= 0, where the
 * reference divides by zero), f = relative_dynamics(X, x, uR, uH) (:74-88).  V <= 0 is unsafe.
 *   Tube      V(0) = l0, dV/dtau = min(0, H), H(x, p) = p . f(x, uR*(p), uH*(p)), over tau in [0, horizon].
 *   One sweep at node i, dimension d: p-_d = (V_i - V_{i-e_d}) / (x_d[i_d] - x_d[i_d-1]), p+_d the forward counterpart (actual spacings); at a low face p- := p+, at a
 *             high face p+ := p-; pbar = (p+ + p-) / 2; Hhat = H(x_i, pbar) + sum_d alpha_d (p+_d - p-_d) / 2 with alpha_d = max over all nodes of |f_d| at this
 *             sweep's pbar; V_i <- float32(V_i + dt min(0, Hhat)).  dt = min(cfl / sum_d (alpha_d / min spacing_d), horizon - tau), or min(fixed_dt, horizon - tau)
 *             with fixed_dt > 0 (alpha is reduced all the same).  Arithmetic in the library's element type; V is float32 after every sweep in both libraries.
 *   PG_HJI_PERIODIC_PSI  dimension 3 wraps: first and last knot are the same angle (at least 3 knots).  The low neighbour of node 0 is node n-2 at spacing
 *             x[n-1] - x[n-2], the high neighbour of node n-1 is node 1 at spacing x[1] - x[0]; the last node's dynamics are evaluated at the first knot's angle, so the
 *             two end nodes, each computed on its own, stay bit-identical whenever l0 is.
 *   gradV     pbar of the final V, same face and wrap rules, 7 floats per node in node order.
 * max_sweeps bounds the loop; reaching it is reported (reached_horizon = 0), not an error.  A NaN or Inf in V after a sweep ends the solve with PG_ERR_INVALID and
 * the sweep's index in bad_sweep (-1 otherwise; the other fields describe the sweeps taken); nothing is installed. */
enum pg_hji_solve_flags { PG_HJI_PERIODIC_PSI = 1 };
typedef struct pg_hji_solve_opts {
    double horizon;                 /* s, >= 0 (0: no sweep, V = l0) */
    double cfl;                     /* in (0, 1]; default 0.8 */
    double fixed_dt;                /* > 0: replaces the CFL rule; 0 (default): the CFL rule */
    int32_t max_sweeps;             /* >= 0; default 100000 */
    int32_t flags;                  /* pg_hji_solve_flags */
} pg_hji_solve_opts;                /* 32 bytes */
typedef struct pg_hji_solve_stats {
    int32_t sweeps;                 /* sweeps taken */
    int32_t reached_horizon;        /* 1: tau == horizon; 0: max_sweeps ended the loop */
    int32_t bad_sweep;              /* index of the sweep after which V held a NaN or Inf (0-based; 0 too when l0 itself holds one), -1: none */
    int32_t reserved;
    double tau;                     /* time covered */
    double last_dt;                 /* step of the last sweep (0 without one) */
    double alpha[7];                /* the dissipation coefficients of the last sweep */
    double v_min, v_max;            /* over the nodes of the result */
} pg_hji_solve_stats;               /* 104 bytes */
/* { horizon 3, cfl 0.8, fixed_dt 0, max_sweeps 100000, flags 0 } */
pg_hji_solve_opts pg_default_hji_solve_opts(void);
/* dims, knots_concat as pg_set_hji_grid takes them; l0 [prod dims] the target, column-major.  vehicle NULL: pg_config.vehicle; opts NULL: the defaults.  V_out [prod dims]
 * and gradV_out [prod dims][7] (either may be NULL) are what pg_set_hji_grid takes.  install != 0 builds the handle's lookup table (the cell records of the current
 * "hji_cell_dims") from the device buffers, with no host round trip: the handle is then exactly as after pg_set_hji_grid(h, dims, knots_concat, V_out, gradV_out).
 * stats may be NULL.  Synchronous.  A handle that never calls this launches what it launched before.
 * PG_ERR_INVALID (the handle and its installed grid are left unchanged): a null dims, knots_concat or l0; a dimension below 2; knots that do not increase strictly; a
 * knot of dimension 4 (Ux) <= 0; PG_HJI_PERIODIC_PSI with fewer than 3 knots in dimension 3 or a span that is not 2 pi to float32 rounding (one ulp of 2 pi);
 * unknown flags; horizon < 0 or not finite; cfl outside (0, 1]; fixed_dt < 0; max_sweeps < 0; a vehicle pg_set_plant_sets would refuse.
 * PG_ERR_STATE: install on a decoupled handle (the safety row belongs to the coupled formulation). */
int pg_hji_solve(pg_handle* h, const int32_t dims[7], const float* knots_concat, const float* l0, const pg_vehicle* vehicle, const pg_hji_solve_opts* opts,
                 int32_t install, float* V_out, float* gradV_out, pg_hji_solve_stats* stats);

/* mpc.solved = false (src/ros_integration.jl:34,41,147): mask[b] != 0 resets instance b; mask == NULL resets all */
int pg_reset(pg_handle* h, const uint8_t* mask);

/* mpc.current_state / current_control / other_car_state / time_offset (src/ros_integration.jl:50-53,76-78,155):
 * state [B][6] (E,N,psi,Ux,Uy,r), control [B][3] (delta,Fxf,Fxr), t0 [B], other_car [B][4] (E,N,psi,V) or NULL (zeros),
 * time_offset [B] (NaN = path-tracking mode) or NULL (all NaN).  Copies host -> device. */
int pg_set_inputs(pg_handle* h, int32_t B, const double* state, const double* control, const double* t0, const double* other_car,
                  const double* time_offset);
/* same, inputs already resident in device memory (HBM) */
int pg_set_inputs_dev(pg_handle* h, int32_t B, const pg_real_dev* state_dev, const pg_real_dev* control_dev, const double* t0_dev,
                      const pg_real_dev* other_car_dev, const double* time_offset_dev);

/* the five reference calls, each over the whole batch, device-resident intermediates */
int pg_compute_time_steps(pg_handle* h);              /* compute_time_steps!           model_predictive_control.jl:17-30 */
int pg_compute_linearization_nodes(pg_handle* h);     /* compute_linearization_nodes!  coupled_lat_long.jl:62-142 */
int pg_update_qp(pg_handle* h);                       /* update_QP!                    coupled_lat_long.jl:315-368 (+ HJI_computation.jl:160-170) */
int pg_solve(pg_handle* h);                           /* solve!                        model_predictive_control.jl:76 */
int pg_get_next_control(pg_handle* h, double* u_out); /* get_next_control              coupled_lat_long.jl:370-374; u_out [B][3] (delta,Fxf,Fxr), host */
int pg_get_next_control_dev(pg_handle* h, pg_real_dev* u_out_dev);
/* The control the ROS loop actually sends (src/ros_integration.jl:114-124): when the instance is in trajectory mode (time_offset not NaN),
 * use_hji_policy is set and the looked-up value V <= HJI_eps, the HJI fallback policy optimal_control(...) (src/HJI_computation.jl:133-158:
 * bang-bang steer + 50-point Fx line search) replaces get_next_control(mpc).  Call after pg_update_qp/pg_solve (it reuses that step's lookup).
 * u_out [B][3] (delta,Fxf,Fxr); source [B] (may be NULL): 0 = MPC control, 1 = HJI policy, 2 = V <= eps but the policy is switched off
 * ("with a feather", :120-123); u2_policy [B][2] (may be NULL) = (delta_opt, Fx_opt) of optimal_control regardless of the selection.
 * Without a grid V = +Inf and the MPC control is returned.  Coupled formulation only. */
int pg_get_next_control_hji(pg_handle* h, int32_t use_hji_policy, double* u_out, int32_t* source, double* u2_policy);
int pg_get_next_control_hji_dev(pg_handle* h, int32_t use_hji_policy, pg_real_dev* u_out_dev, int32_t* source_dev);

/* all five for every instance: host buffers in, host buffers out (status/iters may be NULL).
 * A batch that fills the handle (B == batch_capacity) travels in one copy per direction.  Opt-in (pg_set_option "graph" = 1): when such a batch has at most 256
 * instances and every one of them is warm, the whole step -- copy in, the kernels of a warm step, copy out -- is captured once into a hipGraph and replayed
 * (re-captured whenever something its launches depend on has changed, a control-parameter library or index among them; results identical to the ordinary launches; pg_get_phase_ms has no timing for replayed
 * steps; with no stream installed the graph runs on a blocking stream of its own, ordered against the null stream).  Measured: 2-7 % per step, against ~7 ms for
 * every capture -- worth it for a long run on one path, not for a loop that re-installs its path every few steps; hence off by default. */
int pg_step(pg_handle* h, int32_t B, const double* state, const double* control, const double* t0, const double* other_car,
            const double* time_offset, double* u_out, int32_t* status, int32_t* iters);
/* the four compute phases + control extraction on the inputs last installed; nothing crosses PCIe.  u_out_dev may be NULL. */
int pg_step_dev(pg_handle* h, pg_real_dev* u_out_dev);

/* simulate(mpc, q0, u0, dt)  src/model_predictive_control.jl:80-100 for every instance, entirely on the device (no host round trip between
 * steps): per step  record -> the four compute calls -> state = propagate(dynamics, state, StepControl(dt, old control)) -> control = get_next_control
 * -> t = the next element of the loop's range (see pg_simulate_clock below).  Starts from the inputs last installed (pg_set_inputs*: state, control, t0, time_offset) and leaves the final ones there
 * (pg_get_state reads them).  state_hist_dev [steps][B][6] / control_hist_dev [steps][B][3] may be NULL.  Asynchronous on the handle's stream.
 * Under an actuator library (pg_set_actuator_sets) control_hist_dev records the APPLIED control a_k, the input the plant of step k integrates. */
int pg_simulate_dev(pg_handle* h, int32_t steps, double dt, pg_real_dev* state_hist_dev, pg_real_dev* control_hist_dev);
/* The loop variable of that rollout: `for t in 0:dt:mpc.trajectory.t[end]` (src/model_predictive_control.jl:87) is a Julia RANGE -- element k is ONE rounding of k dt with dt lifted
 * to its exact rational (0.01 = 1/100) when dt and the path's end time have one, `fl(k dt)` otherwise -- not the accumulation t += dt (which is 0.2900000000000001 at step 29 and
 * then puts the long horizon of :23 a whole dt_long later).  pg_simulate_dev forms each instance's time as (t_start .+ (0:dt:t_end))[k + 1] with t_start the time installed by
 * pg_set_inputs* and t_end the last time of the installed trajectory (trajectory 0 of a library); consecutive calls with the same dt continue the clock, pg_set_inputs* restarts it.
 * This entry point returns those times on the host, out[k * B + b] for k < steps, so that a host-driven loop (pg_step per step) can feed the same t0 the device loop uses.
 * Option "time_grid_naive" = 1: t_start + accumulated dt, as in rounds 1-5.  (A restatement of Julia 1.0's Base range arithmetic that could not be executed here.) */
int pg_simulate_clock(pg_handle* h, double dt, int32_t steps, int32_t B, const double* t_start, double* out);
/* current device-resident inputs: state [B][6], control [B][3], t0 [B] (host pointers, any may be NULL) */
int pg_get_state(pg_handle* h, double* state, double* control, double* t0);

/* Safety rollout: simulate (src/model_predictive_control.jl:80-100) with the control the ROS node sends fed back -- the HJI policy when use_hji_policy and V <= HJI_eps in
 * trajectory mode, else the MPC control (src/ros_integration.jl:114-124; the same decision and bits as pg_get_next_control_hji) -- against a MOVING other car, the human of
 * relative_dynamics (src/HJI_computation.jl:74-88): SimpleCarState (E, N, psi, V), control (omega, a).  Per step and instance: record state, control and other car (:88-89);
 * the four compute calls as pg_simulate_dev makes them (with a grid: the step's relative state and its lookup V, gradV); select the control; ego state = propagate(state, OLD
 * control, dt) as pg_simulate_dev; other car = RK4(other, (omega, a), dt) with rk4_substeps sub-steps of (-V sin psi, V cos psi, omega, a) (psi from North as for the ego,
 * src/vehicle_dynamics.jl:127-129); control = the selected control; t = the next element of the clock of pg_simulate_dev (same continuation and restart rules).
 * (omega, a) is held for the step; human_mode: 0 hold = (0, 0) (constant speed and heading: an other car of speed 0 is the frozen car of pg_simulate_dev), 1 worst case =
 * optimal_disturbance (dMode :min, src/HJI_computation.jl:90-131) at the step's relative state and gradient (no grid or out of the grid: gradV = 0 gives (0, 0)), 2 scripted =
 * human_u_dev [steps][B][2] = (omega, a).  Without a grid V = +Inf and the MPC control is applied.  Build-defined (the reference only receives the other car from ROS): the
 * other car's integrator, V <- max(V, 0) after each sub-step, and optimal_disturbance := (0, 0) where the other car's speed is <= 0 (the reference divides by it).
 * Histories may be NULL: state [steps][B][6], control [steps][B][3], other [steps][B][4], human [steps][B][2], V [steps][B] (library element type), source [steps][B] (int32:
 * 0 MPC, 1 HJI policy, 2 V <= eps with the policy off).  Coupled formulation only (PG_ERR_STATE); human_mode outside {0, 1, 2}, mode 2 without human_u_dev, steps < 1 or
 * dt <= 0: PG_ERR_INVALID.  Asynchronous on the handle's stream.  The gates of the node (pre_flag, the trajectory-time window, the low-speed pause), the NaN fallback and
 * the decoupled formulation are pg_simulate_node_dev's (below).  Under an actuator library (pg_set_actuator_sets) the control history is the APPLIED control a_k: the kernel
 * records the control it is handed, and it is handed the actuator's output. */
int pg_simulate_safety_dev(pg_handle* h, int32_t steps, double dt, int32_t use_hji_policy, int32_t human_mode, const pg_real_dev* human_u_dev,
                           pg_real_dev* state_hist_dev, pg_real_dev* control_hist_dev, pg_real_dev* other_hist_dev,
                           pg_real_dev* human_hist_dev, pg_real_dev* V_hist_dev, int32_t* source_hist_dev);
/* other car now [B][4]; per instance since the clock last restarted (pg_set_inputs*, or a rollout with another dt or path end): V_min [B] = the smallest V a safety step
 * looked up (+Inf: none), first_breach [B] = the first step index (the clock's, continuing across calls) with V <= 0 or -1, policy_steps [B] = steps whose control was the
 * HJI policy.  Host pointers, any may be NULL. */
int pg_get_safety_state(pg_handle* h, double* other_car, double* V_min, int32_t* first_breach, int32_t* policy_steps);

/* Node callback: the per-message decision of from_autobox_callback (src/ros_integration.jl:48-151) for every instance of the batch.  Per instance, in order: V, gradV looked
 * up (:55-57, before any gate); pre_flag == 0: return (:70-73); trajectory mode (time_offset not NaN) and t0 < 0 or t0 > trajectory.t[end] of the instance's trajectory:
 * return (:79-82); Ux < 1 (the literal 1 m/s, :84-87): return; else the four compute calls and heartbeat + 1 (:94-112), the selection of pg_get_next_control_hji (:114-124),
 * and the NaN fallback (:134-147): a NaN (not an Inf) in any published component publishes the current message instead, sets the message to 0 and starts the solver cold
 * (solved = false).  A return publishes nothing and leaves the instance's solver state exactly as it was.  Events: */
enum pg_node_event {
    PG_NODE_MPC = 0,                /* the MPC control was published */
    PG_NODE_HJI_POLICY = 1,         /* the HJI policy was published (trajectory mode, use_hji_policy, V <= HJI_eps) */
    PG_NODE_FEATHER = 2,            /* V <= HJI_eps in trajectory mode with the policy off: the MPC control was published */
    PG_NODE_NAN_FALLBACK = 3,       /* the selected control had a NaN: the previous message was published, the message is now 0 */
    PG_NODE_PRE_FLAG_OFF = 4,       /* gated out: pre_flag == 0 */
    PG_NODE_OUTSIDE_TRAJECTORY = 5, /* gated out: trajectory mode, t outside [0, trajectory.t[end]] */
    PG_NODE_LOW_SPEED = 6           /* gated out: Ux < 1 m/s */
};
/* One callback for every instance on the installed inputs.  The installed control plays current_control, the to_autobox message (:52); on return it is the message after
 * the callback (the published command, 0 after a fallback, unchanged when gated out).  Device outputs, each may be NULL: cmd_out [B][3] the published command (lanes that
 * publish nothing are not written), se_out [B][2] (s, e) of the step's projection (:114), event [B] (int32, pg_node_event).  pre_flag_dev [B] (uint8) or NULL = engaged.
 * The clock does not advance.  Decoupled handles: V = +Inf, use_hji_policy != 0 is PG_ERR_STATE.  Gated-out instances are computed too (their results are discarded):
 * the call costs a full step.  Asynchronous on the handle's stream.  PG_ERR_STATE while an actuator library is installed (pg_set_actuator_sets: out of scope). */
int pg_node_step_dev(pg_handle* h, int32_t use_hji_policy, const uint8_t* pre_flag_dev, pg_real_dev* cmd_out_dev, pg_real_dev* se_out_dev, int32_t* event_dev);
/* The node's closed loop.  Each instance keeps two controls: the message (the installed control) and the applied command (what the plant executes; initialised from the
 * installed control whenever the clock restarts).  Per step: the gates; the compute calls as pg_simulate_safety_dev makes them; the callback's decision as above; the records
 * (state and applied command at the step's start, the step's V, the event); ego state = propagate(state, applied command at the step's start, dt); applied command = the
 * published one where something was published; the other car as pg_simulate_safety_dev (human_mode, human_u_dev); the clock of pg_simulate_dev (continuing past the range's
 * end with the same element formula); the safety summary of pg_get_safety_state (V_min and first breach at every step, policy steps: published policy commands).
 * pre_flag_dev [steps][B] or NULL.  Histories may be NULL: state [steps][B][6], applied [steps][B][3], V [steps][B] (library element type), event [steps][B] (int32).
 * With every gate open and no NaN this is pg_simulate_safety_dev.  steps < 1, dt <= 0, human_mode outside {0, 1, 2}, mode 2 without human_u_dev: PG_ERR_INVALID;
 * use_hji_policy on a decoupled handle: PG_ERR_STATE.  Asynchronous on the handle's stream.  PG_ERR_STATE while an actuator library is installed (pg_set_actuator_sets:
 * the hand-back of the next command is not a plain copy here -- a gated-out instance leaves `applied` unwritten). */
int pg_simulate_node_dev(pg_handle* h, int32_t steps, double dt, int32_t use_hji_policy, int32_t human_mode, const pg_real_dev* human_u_dev, const uint8_t* pre_flag_dev,
                         pg_real_dev* state_hist_dev, pg_real_dev* applied_hist_dev, int32_t* event_hist_dev, pg_real_dev* V_hist_dev);
/* applied command [B][3]; heartbeat [B] (callbacks that ran the compute calls; zero at the first node call, never reset); counts [B][4] = steps with pre_flag off, outside
 * the window, low speed, NaN fallback since the clock last restarted (the restart rule of pg_get_safety_state).  Host pointers, any may be NULL. */
int pg_get_node_state(pg_handle* h, double* applied, int32_t* heartbeat, int32_t* counts);

/* Tracking summary of the rollouts (opt-in: option "tracking_summary" = 1; 0, the default, adds no launch anywhere).  With the option on, each step of pg_simulate_dev,
 * pg_simulate_safety_dev and pg_simulate_node_dev runs one small lane-per-instance kernel (k_track) behind the step's projection and ahead of the kernel that moves the plant.
 * per instance since the rollout clock last restarted (the restart rule of pg_get_safety_state): summary [B][6] =
 * (max |e|, sum e^2, max |Uy / Ux|, max |r|, min Ux, s of the last step), steps [B] = rollout steps counted,
 * first_exit [B] = first step index (the clock's) at which e lay outside [edge_R(s), edge_L(s)] of the instance's
 * trajectory, or -1.  (s, e) are the step's path_coordinates -- the s_m, e_m the node publishes
 * (ros_integration.jl:114,129-130) -- so step k describes the state recorded at step k.  Host pointers, any may be NULL.
 * The edges at s are the interp_by_s channels the wall rows read (a trajectory library: the instance's own tube).  In the node rollout every step counts, gated out or not
 * (the plant moves either way).  e is formed from differences to the knots of the projection's segment and its two neighbours, not from the foot point in map coordinates
 * as the projection forms it: the same distance, without that rounding (fp32 library: 1e-7 m instead of 1e-5 m on a path 300 m from the map's origin, which the squares double).
 * Before the first counted step: (0, 0, 0, 0, +Inf, NaN), steps 0, first_exit -1.  Sums are kept in the library's arithmetic type.
 * PG_ERR_STATE with the option off. */
int pg_get_tracking_state(pg_handle* h, double* summary, int32_t* steps, int32_t* first_exit);

/* stream to launch on (hipStream_t as void*); NULL = the null stream.  pg_set_inputs and pg_step are ASYNCHRONOUS on the handle's stream (copies from / into one pinned
 * staging buffer, synchronised at the next entry that needs it): switching streams first waits for whatever is still queued on the old one. */
int pg_set_stream(pg_handle* h, void* hip_stream);
/* Fused step: pg_step / pg_step_dev / pg_simulate_dev can run update_QP! and solve! of the coupled formulation (N <= 32) in ONE kernel -- the wavefront that
 * solves an instance linearises it first (same device functions: results are bit-identical either way; the QP data are still written and pg_get_qp reads them).
 * mode 0 = never (default), 1 = always, 2 = for batches of >= 1024 instances in which every instance is warm (closed loop).
 * Measured on MI355X: +7 % on the cold benchmark batch (skidpadoval), -5..-8 % on the other paths and in closed loop (EXPERIMENTS.md 4.1) -- it pays only where a few
 * slow instances dominate the solve kernel.  The four compute calls invoked one by one are never fused. */
int pg_set_fusion(pg_handle* h, int32_t mode);
/* Pipelined nodes + update_QP (build-defined; no counterpart in the reference): for batches of 2304..8192 instances with cold instances, coupled formulation,
 * pg_step / pg_step_dev / pg_simulate_dev run compute_linearization_nodes! and update_QP! as ONE launch in which the linearisation of
 * interval t starts as soon as nodes t, t + 1 of its instances are seeded (the cold seeding is a serial recurrence over the nodes: 0.18 ms of latency on 6 % of the
 * chip that the linearisation of the early intervals now runs under).  With a safety row installed its (M, b) are computed before that launch.  Same device
 * functions on the same arguments: nodes and QP data are bit-identical in fp64; in the fp32 library the nodes are, the QP data agree to fp32 rounding.
 * mode 1 = on where it applies (default), 0 = never.  The compute calls invoked one by one are never pipelined. */
int pg_set_pipeline(pg_handle* h, int32_t mode);
/* The wavefronts of that launch that linearise an interval WAIT for the wavefronts that seed its nodes.  The wait is bounded (20 ms of wall-clock time); a wavefront
 * that gives up -- the seeding wavefronts not resident before it: a dispatch order the launch does not control, a debugger, a time-sliced or counter-serialised run --
 * raises a device flag, and the launch-per-phase kernels queued behind the pipelined launch (predicated on that flag) redo update_QP! for the batch: such a step is
 * late, not wrong, and nothing is reported to the caller but this cumulative count of wavefronts that gave up (synchronises the handle's stream). */
int pg_get_pipeline_fallbacks(pg_handle* h, int64_t* count);
int pg_synchronize(pg_handle* h);

/* Build-defined options of a handle, by name (no counterpart in the reference; every one has a default under which the library behaves as documented above).  The library
 * reads NOTHING from the process environment: what a handle does depends on its pg_config and on the options set here.  Unknown name, read-only name or a value out of
 * range: PG_ERR_INVALID.  Integer options take integral values.  Options take effect at the next launch (hji_cell_dims: at the next pg_set_hji_grid).
 *   coupled solve kernel (k_solve):
 *     "solve_split" 0/1 (1)      rounds-only kernel + list-mode full kernel instead of one kernel (never with a safety row installed)
 *     "clip_guess" 0/1 (1)       first roll-out of a cold instance clips the steering rate; the clipped transitions are its first working set
 *     "clip_stops" 0/1 (0)       ... and at the steering stops too (measured: fewer rounds, a longer launch; EXPERIMENTS.md 11.3)
 *     "ck_riccati" 0/1 (1)       the matrix recursion of a later round restarts at a checkpoint behind the rows that changed (fp64)
 *     "warm_trivial_cold" 0/1 (1)  a warm instance whose previous working set was empty starts like a cold one
 *     "hji_seed" 0..4 (0), "hji_rounds" 0..64 (0)   seeded working sets for instances whose safety row is violated at the current control (experiment, off)
 *   launch shape:
 *     "pipe_min" (2304), "pipe_max" (8192, at most: 256 nodes wavefronts of 32 instances)  batch sizes the pipelined nodes + update_QP launch serves (pg_set_pipeline)
 *     "pipe_first" 0..64 (0)     short-horizon intervals whose wavefronts go first in that launch (0: as many as fill the SIMDs the recurrence leaves free -- all ten at B = 4096;
 *                                measured: fewer is slower, 0.317 / 0.323 / 0.328 / 0.344 ms for 10 / 8 / 6 / 2)
 *     "pipe_pub_short" (3), "pipe_pub_long" (5)   the recurrence of that launch publishes its progress after every n-th node of the short / long horizon (a publication is a
 *                                device-scope release, ~3 us on the serial chain: every node of the short horizon 0.317 -> 0.345 ms)
 *     "lin_lanes" 1/2 (1)        lanes per (instance, interval) of the large-batch linearisation
 *     "speed_plan_lanes" 0/16/32/64 (0)  sets per wavefront of pg_plan_speeds' kernel; 0 = by the size of the call (64, halved while the launch has fewer than 256
 *                                wavefronts).  The result does not depend on it
 *     "phase_timing" 0/1 (0)     1 = pg_step_dev records the HIP events pg_get_phase_ms reads (four event records per step on the handle's stream: measured 13-25 us per step, 2-4 % of a
 *                                4096-instance step); 0 = no instrumentation, pg_get_phase_ms returns PG_ERR_STATE
 *     "graph" 0/1 (0)            pg_step of a small warm batch as one hipGraph launch (see pg_step)
 *     "stat_sensor_steps"        (read-only) rollout steps that ran under a sensor library (k_measure launches) since pg_create
 *     "stat_actuator_steps"      (read-only) rollout steps whose plant launch ran under an actuator library (k_actuate launches) since pg_create
 *     "stat_disturbance_steps"   (read-only) rollout steps that ran under a disturbance library (k_disturb launches) since pg_create
 *     "stat_estimator_steps"     (read-only) rollout steps that ran under an estimator library (k_estimate launches) since pg_create
 *     "stat_human_steps"         (read-only) rollout steps that ran under a human library (k_human launches) since pg_create
 *     "stat_route_steps"         (read-only) k_route launches since pg_create: rollout steps that carried an event of an installed route set or recorded the route
 *     "tracking_summary" 0/1 (0) 1 = every rollout step runs k_track (pg_get_tracking_state); 0 = no such launch.  Switching it off and on again restarts the summary
 *     "time_grid_naive" 0/1 (0)  0 = the time axes as Julia's RANGES give them (src/model_predictive_control.jl:25-26: `t0 .+ dt_short*(0:N_short)`, `t0_long .+ dt_long*(1:N_long)`,
 *                                and :87, `for t in 0:dt:trajectory.t[end]` in pg_simulate_dev): reference value and step in twice the working precision, dt lifted to its exact
 *                                rational (0.01 = 1/100, 0.2 = 1/5), every element ONE rounding -- a restatement of Julia 1.0's Base that could not be executed here;
 *                                1 = `t0 + dt*i` with two roundings and `t += dt` in the closed loop (the form of rounds 1-5: differs by an ulp of ts now and then, which the
 *                                discontinuous `ceil` of :23 can turn into a different lattice point)
 *     "hji_cell_dims" 3/5/7 (3)  corners per cell record of the HJI table = 2^value (256 B / 1 KiB / 4 KiB records)
 *   lateral solve kernel (decoupled formulation):
 *     "lateral_solver" 0/1/2 (0) 0 = k_solve_lat beyond 20 intervals or with the polish off, else the embedding in k_solve; 1 = k_solve_lat; 2 = the embedding
 *     "lat_workspace" 0/1        k_solve_lat keeps its row state in the per-wavefront workspace at every horizon (default: beyond 32 intervals, or with walls beyond 16)
 *     "lat_pin" 0/1 (1)          a held steering-rate row pins the input of its stage exactly in the polish (0: held through the augmented Lagrangian like every other row)
 *     "lat_pack_only" 0/1 (1)    update_QP! of a handle solved by k_solve_lat writes the packed stage records only (the embedded block pg_get_qp returns is built on demand)
 *     "lat_split" 0/1 (1)        a step in which every instance is warm runs as two launches (warm attempts, then the cold solves of what they left)
 *     "lat_handover" 0/1 (1)     STRAGGLER HAND-OVER of a cold launch (batches of >= "lat_hand_batch" (1025) instances whose row state lives in the workspace: N > 16): the launch stops
 *                                after "lat_hand_cap" trips through the solver's loop (0 = 16 with the wall rows, 11 without), files its unfinished instances, and a second launch
 *                                resumes them with ONE instance per wavefront.  Same verified KKT points as the single launch (measured 4e-8 apart at most); 2.96-3.03 -> 2.61 ms on
 *                                the N = 50 + walls batch of 4096.  0 = one launch, as in round 5.  The trip rule depends on the data only: the same call returns the same bits.
 *     "lat_hand_target" (0)      > 0: stop the first launch once at most this many instances of the batch are unfinished instead (counted on the device, not before "lat_hand_min" (8)
 *                                trips).  Adapts to the batch (1500: 2.58 ms on the batch above, vail + walls 2.09 against 2.19) -- but WHEN a wavefront sees the count is a matter of
 *                                timing: answers then differ by ~1e-8 from run to run (two verified KKT points of the same QP, resumed a trip earlier or later)
 *                                ("lat_hand_work" > 0 with "lat_hand_w0": a third, deterministic rule kept for A/B -- stop when w0 + #unfinished instances, summed over the wavefront's
 *                                trips, reaches the budget: measured worse than the trip count at every weight, EXPERIMENTS 12.8)
 *     "lat_single_max" (1024)    cold lateral batches of at most this many instances (horizons beyond 16 intervals) run one instance per WAVEFRONT from the start: a trip through the
 *                                solver's loop costs 57 us instead of 84 (0: never).  The same arrangement serves the list a warm step's attempts leave, when it is that short (the length
 *                                is a device word: both arrangements are queued, one of them returns at once)
 *     "lat_aux_gate" 0/1 (1)     the serial passes write what a pinned row's multiplier is read from only while an instance of the wavefront is in a polish
 *     "nodes_serial" 0/1 (0)     1 = the cold node seeding (both formulations) commits ONE node per pass: the reference's serial recurrence exactly (the default runs 2 / 8 lanes per
 *                                instance ahead on the commanded acceleration and commits the nodes whose solve returned it: identical to 1e-12, 4e-6 in fp32; parity tests use this)
 *     "lat_rho_scale" (1e3 in fp64, 1 in fp32)  penalty of held rows = polish_rho x this;   "lat_mu0_cost" (10), "lat_far_cost" (3e4), "lat_polish2" 0/1 (1),
 *     "lat_polish_rounds" (3), "lat_settle" 0..2 (0), "lat_warm_rounds" (2), "lat_wipm" 0/1 (0), "lat_wmu" (1e-2), "lat_wtau" (1e-4)   see pg_solve_lat.hip
 *   read-only (pg_get_option): "stat_pipelined_launches", "stat_split_solve_launches", "stat_single_solve_launches", "stat_lat_two_launch_solves", "stat_lat_handover_solves", "stat_lat_one_per_wavefront_solves" -- how many launches of
 *     this handle took the path named (tests assert that the path they mean to cover is the one that ran); "stat_whole_batch_solves" -- counted ON THE DEVICE: launches in
 *     which the full k_solve took the whole batch because the previous launch had left instances for the interior point (reading it drains the stream);
 *     "lateral_solver_in_use" (1 = k_solve_lat, 2 = embedding).
 * The diagnostic build (libpigeon_hip_diag.so, -DPG_DIAG; never shipped) adds "diag_pipe_fault" (fault injection for the pipelined launch), "diag_instance",
 * "diag_lin_groups", "diag_timeline". */
int pg_set_option(pg_handle* h, const char* name, double value);
int pg_get_option(pg_handle* h, const char* name, double* value);

/* ---- read-backs for parity tests and logging (host pointers, any may be NULL) ---------------------------------- */
/* ts [B][N+1], dt [B][N], prev_ts [B][N+1] */
int pg_get_time_steps(pg_handle* h, double* ts, double* dt, double* prev_ts);
/* qs [B][N+1][6], us [B][N+1][2] (delta, Fx in physical units), ps [B][N+1][4] (V, kappa, 0, 0) */
int pg_get_nodes(pg_handle* h, double* qs, double* us, double* ps);
/* path_coordinates of the current states: sep [B][3] = (s, e, t)   src/trajectories.jl:71-94 */
int pg_get_path_coordinates(pg_handle* h, double* sep);
/* refreshed QP data of instances [b0, b0+n): n blocks of pg_qp_len() doubles laid out as
 * A[N][6][6] B0[N][6][2] Bf[N][6][2] c[N][6] H[N][4][2] G[N][4] dmin[N] dmax[N] fxmax[N] ddmin[N] ddmax[N] dt[N] q_curr[6] u_curr[2] M_hji[2] b_hji
 * (the numeric content update_QP! writes into the Parametron parameters, coupled_lat_long.jl:323-366; B's scaled by u_normalization) */
int pg_qp_len(const pg_handle* h);
int pg_get_qp(pg_handle* h, int32_t b0, int32_t n, double* out);
/* the inverse: install QP data for instances [b0, b0+n) in the same layout (what setting the Parametron parameters by hand is to the reference); pg_solve then solves
 * exactly these problems.  For replaying recorded QPs and for solver tests on constructed (e.g. degenerate) problems; a step (pg_update_qp, pg_step*) overwrites them. */
int pg_set_qp(pg_handle* h, int32_t b0, int32_t n, const double* in);
/* primal solution: x [B][N+1][8] = (q (6), normalised u (2)) per node; sigma [B][N][3] = (sigma1, sigma2, sigma_HJI of node k+1) */
int pg_get_solution(pg_handle* h, double* x, double* sigma);
/* status [B] (pg_solve_status), iters [B], active [B][N] bit masks over the 16 stage rows (row order in DESIGN.md), mu [B] final gap */
int pg_get_solve_info(pg_handle* h, int32_t* status, int32_t* iters, uint16_t* active, double* mu);
/* outcome of the active-set polish per instance, [B]: 0 = not run (polish off, or the interior point did not converge), k >= 1 = verified in round k (the
 * solution is the exact optimum on its active set), -1 = did not verify (the interior-point iterate at ipm_tol was kept) */
int pg_get_polish_info(pg_handle* h, int32_t* polish);
/* multipliers of the inequality rows as the last solve left them, lam [B][N][16], indexed like the bits of the `active` masks (the next step's warm start reads them).
 * A verified instance (pg_get_polish_info >= 1): the multipliers of its verified working set, 0 off the set -- with the masks, the dual half of the KKT point; the
 * CANONICAL active-set rule of the parity tests is "bit set AND multiplier > 1e-6" (a row held at its bound with a zero multiplier is degenerate: the QP does not say
 * which side of "active" it is on), the same rule the oracle applies to its own multipliers.  An unverified instance: the interior point's multipliers at the hand-over
 * (k_solve_lat) or the estimates of the last working set tried (k_solve) -- not a certificate. */
int pg_get_multipliers(pg_handle* h, double* lam);
/* milliseconds of the last pg_step_dev per phase: time_steps+nodes, update_qp (linearize, limits, HJI), solve (+extract); HIP events, recorded when the option
 * "phase_timing" is 1 (off by default: PG_ERR_STATE) */
int pg_get_phase_ms(pg_handle* h, float out3[3]);

/* cache[x] for a batch of relative states: HJI_computation.jl:66-72.  x7 [B][7] host; V [B], gradV [B][7] host.  Out of bounds => V=+Inf, gradV=0 */
int pg_hji_lookup(pg_handle* h, int32_t B, const double* x7, double* V, double* gradV);
int pg_hji_lookup_dev(pg_handle* h, int32_t B, const pg_real_dev* x7_dev, pg_real_dev* V_dev, pg_real_dev* gradV_dev);
/* packed form, no temporaries, asynchronous on the handle's stream: out8 [B][8] = (V, gradV[0..6]) per lookup (the kernel's native output) */
int pg_hji_lookup8_dev(pg_handle* h, int32_t B, const pg_real_dev* x7_dev, pg_real_dev* out8_dev);
/* dims of the installed grid (HJICache.grid_knots lengths) */
int pg_hji_grid_dims(pg_handle* h, int32_t dims[7]);
/* 2-D value slices for the RViz consumers, batched: src/rviz.jl:23-40 (update_HJI_values_marker!) and :60-69 (update_HJI_contour_marker!) evaluate
 * cache[HJIRelativeState(x, y, q[3..7])].V at every knot pair (x, y) of grid dimensions 1 and 2.  q7 [B][7] relative states (components 0, 1 are replaced by
 * the knots); V_out [B][n1][n2] = V(X[i], Y[j]);  rgb_out [B][n1][n2][3] or NULL = value_to_RGB(V) (rviz.jl:41-44);  zero-level crossings = the vertex set of
 * contour(X, Y, V, 0) (:63): cross_x [B][n1-1][n2] = x where V changes sign between (X[i], Y[j]) and (X[i+1], Y[j]), NaN where it does not;
 * cross_y [B][n1][n2-1] likewise along y (either may be NULL).  An edge carries a vertex iff exactly one end has V > 0 (Contour.jl's marching-squares rule). */
int pg_hji_slice(pg_handle* h, int32_t B, const double* q7, double* V_out, double* rgb_out, double* cross_x, double* cross_y);
/* compute_reachability_constraint for the installed inputs: M [B][2] (already multiplied by u_normalization), b [B], V [B] */
int pg_get_hji_constraint(pg_handle* h, double* M, double* b, double* V);
/* wall extension (pg_config.walls): (edge_L, edge_R) at nodes 2..N+1 of every instance, [B][N][2]; PG_ERR_STATE when walls are off.
 * The wall slack sw is returned in the third column of pg_get_solution's sigma [B][N][3]. */
int pg_get_walls(pg_handle* h, double* edges);

#ifdef __cplusplus
}
#endif
#endif
