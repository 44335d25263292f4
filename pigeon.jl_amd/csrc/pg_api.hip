// C ABI of libpigeon_hip.so (declared in include/pigeon_mpc.h).  Host-side handle, device buffers, kernel launches.
// The product path has NO CPU fallback: without a HIP device pg_create fails with PG_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>
#include "pg_kernels.hip"
#include "pg_own.hpp"

using namespace pg;

// One per-instance selection into a library: the device array [capacity] (entries beyond the covered batch select set 0) and the index as the caller installed it.
// `what` / `setter` name the library and its entry point in the messages
struct IndexArray {
    const char *what, *setter; int* d = nullptr; std::vector<int32_t> host;
    int covered() const { return (int)host.size(); }
};
// One library of per-instance sets: the sets as the caller installed them, their device records, the selection (setlib_install / setlib_clear / setlib_get below)
template <class Host, class Dev> struct SetLib {
    IndexArray idx; std::vector<Host> sets; Dev* d = nullptr;
    bool on() const { return !sets.empty(); }                                             // the host knows whether a library is installed: that alone adds its kernel to a rollout step
    const int* index() const { return sets.size() > 1 ? idx.d : (const int*)nullptr; }    // what the kernels are handed: a library of at most one set needs no index
};
// record k of a [steps][B][width] history on the device (nullptr: not recorded)
template <class T> static T* hist_at(T* hist, int k, int B, int width) { return hist ? hist + (size_t)k * B * width : nullptr; }
// One history registration (pg_set_*_history_dev): a device record [steps][B][width] of the caller's.  One-shot: the next rollout call takes it, whether it succeeds or not
struct HistSlot {
    real* buf = nullptr; int steps = 0;
    void clear() { buf = nullptr; steps = 0; }
    HistSlot take() { const HistSlot s = *this; clear(); return s; }
    real* at(int k, int B, int width) const { return k < steps ? hist_at(buf, k, B, width) : (real*)nullptr; }      // record k; nullptr: not recorded
};
// The streams of a seeded library: the ids as installed (instances they do not cover: stream[b] = b), their device copy [capacity] (sync: uploaded when a rollout or a
// *_response / pg_sensor_draws call first needs it and whenever the ids changed) and the seed, a launch argument
struct SeedStreams {
    unsigned long long* d = nullptr; bool dirty = true; std::vector<uint64_t> host; uint64_t seed = 0;
    int sync(pg_handle* h);
};

struct pg_handle {
    pg_config cfg;
    DevCfg dc;
    int B = 0;                       // current batch
    int warm_B = 0;                  // instances [0, warm_B) are known to carry a previous solution (solved = true): set by pg_solve, cleared by pg_reset
    hipStream_t stream = nullptr;
    int pipeline = 1;                                         // pg_set_pipeline: 1 = nodes + update_QP of a large batch with cold instances as one pipelined launch (k_nodes_linearize), 0 = never
    bool pipe_fault = false;                                  // -DPG_DIAG builds only (option "diag_pipe_fault"): fault injection for the pipelined launch (its nodes blocks never publish)
    int lin_groups = 0;                                       // -DPG_DIAG builds only (option "diag_lin_groups"): force the lane arrangement of launch_linearize (1, 2, 4, 8 lanes per interval)
    int speed_lanes = 0;                                      // option "speed_plan_lanes": sets per wavefront of k_speed_plan (64, 32, 16; 0 = by the size of the call: speed_plan_spw)
    int debug_timeline = 0;                                   // -DPG_DIAG builds only (option "diag_timeline"): pg_debug_solve_cycles records the timeline of the product's kernel
    int lateral_solver = 0;                                   // option "lateral_solver": 0 = by horizon (k_solve_lat beyond 20 intervals or with the polish off), 1 = k_solve_lat, 2 = the embedding in k_solve
    int hji_cell_dims = 3;                                    // option "hji_cell_dims": corners per cell record of the next pg_set_hji_grid = 2^3 (256 B, default), 2^5, 2^7
    int64_t stat_pipelined = 0, stat_split = 0, stat_single = 0, stat_lat_two = 0;      // read-only options "stat_*": launches that took the pipelined nodes + update_QP path / the split solve / the single solve kernel / the two-launch lateral solve
    // (these two are handle state, not arguments in disguise: pg_compute_linearization_nodes followed by a separate pg_solve relies on them across public calls)
    int solve_parity = 0;                                     // which of the two to-do counters the next solve launch counts into (the other one holds the previous launch's count: see launch_solve)
    bool cnt_cleared = false;                                 // this step's projection kernel has zeroed the counter launch_solve is about to use
    int* d_progress = nullptr;                                // progress and fault words of the pipelined launch (k_nodes_linearize): layout below (pipe_fault_word)
    int64_t fallback_total = 0; int fallback_seen = 0;        // pg_get_pipeline_fallbacks: 64-bit total kept on the host, last value of the device's 32-bit word
    int fuse = 0;                                             // pg_step_dev / pg_simulate_dev: linearisation fused into the solve kernel (pg_set_fusion): 0 never (default), 1 always, 2 for all-warm batches
    std::string err;
    // device buffers
    real *d_traj = nullptr; int traj_L = 0; int *d_traj_len = nullptr; IndexArray traj_idx{"trajectory", "pg_set_trajectory_index"};
    // control-parameter library (pg_set_control_param_sets / pg_set_control_param_index): device records (a library of several sets only) and index are what DevCfg points
    // to; cp_eff [capacity] is the set every instance currently runs under (an instance whose entry changes is reset)
    SetLib<pg_control_params, DevControlRec> cp{{"control-parameter", "pg_set_control_param_index"}}; std::vector<pg_control_params> cp_eff;
    // plant library (pg_set_plant_sets / pg_set_plant_index): the vehicles the ego plant of the rollouts integrates, per instance, read by the library kernels (k_*_lib).  Nothing on
    // the controller's side reads any of it
    SetLib<pg_vehicle, DevVehicle> plants{{"plant", "pg_set_plant_index"}};
    // tracking summary (option "tracking_summary"; pg_get_tracking_state): [cap][6] sums, steps [cap] then first_exit [cap] (k_track), allocated when the option is first used
    int tracking = 0; real* d_track = nullptr; int* d_track_i = nullptr;
    bool track_fresh = true;                                  // the tracking summary restarts at the next rollout step (the clock restarted since it was last written)
    // ---- the five rollout libraries that keep state beside their sets: one record each.  lib: the sets and the selection; streams: a seeded library's; hist: the one-shot
    // history registration(s); fresh: no state of the previous step exists, the law restarts at the next step under the library (restart_on_clock lists them); valid: the
    // record the getter reads was written by a rollout step since the inputs were installed (restart_on_inputs); steps_stat: read-only option "stat_<library>_steps";
    // cleared(): what pg_clear_*_sets resets beside the sets (the device buffers stay, and die with the handle: pg_handle::mem) ----
    // sensor library (pg_set_sensor_sets / pg_set_sensor_index / pg_set_sensor_seed): what the controller of a rollout step is handed in place of the true state.  Beside the
    // sets: the streams and the seed, the measured state meas [cap][6] and, with the tracking summary, the projection of the TRUE state sep_true [cap][4].  Nothing is
    // allocated without a library.  No `fresh`: the law has no state.  Clearing the sets leaves seed and streams as they are
    struct Sensor {
        SetLib<pg_sensor, DevSensor> lib{{"sensor", "pg_set_sensor_index"}}; SeedStreams streams; HistSlot hist;      // hist: pg_set_measured_history_dev
        real *meas = nullptr, *sep_true = nullptr; bool valid = false; int64_t steps_stat = 0;
        void cleared() { valid = false; hist.clear(); }
    } sensor;
    // actuator library (pg_set_actuator_sets / pg_set_actuator_index): what the plant of a rollout step is handed in place of the command.  Beside the sets, allocated when a
    // rollout first runs under a library: the actuator's position pos [cap][3], the command ring [PG_ACT_MAX_DELAY][cap][3], plant_u [cap][3] (the plant kernel's
    // `control`: a_k going in, the next command coming out) and, while some installed set has feedback == 1, seen [cap][3] (the compute kernels' current_control).
    // No `valid`: before the first step since the clock restarted the position is the command (pg_get_actuator_state)
    struct Actuator {
        SetLib<pg_actuator_set, DevActuator> lib{{"actuator", "pg_set_actuator_index"}}; HistSlot applied_hist, command_hist;      // pg_set_applied_history_dev / pg_set_command_history_dev
        real *pos = nullptr, *ring = nullptr, *plant_u = nullptr, *seen = nullptr;
        bool feedback = false;                                    // some installed set has feedback == 1
        bool fresh = true; int64_t steps_stat = 0;
        void cleared() { feedback = false; fresh = true; applied_hist.clear(); command_hist.clear(); }      // (a library installed later starts from the command it finds)
    } actuator;
    // disturbance library (pg_set_disturbance_sets / pg_set_disturbance_index / pg_set_disturbance_seed): what acts on the ego plant of a rollout step from outside.  Beside
    // the sets: the streams and the seed (its own, as the sensor library keeps its own), and, allocated when a rollout first runs under a library: the gust state
    // n [cap][2], this step's w [cap][4] (k_disturb writes it, the library kernel's <DistW> instantiation reads it) and veh, ONE record holding the handle's own vehicle:
    // the library of one that instantiation is handed when no plant library is installed
    struct Disturbance {
        SetLib<pg_disturbance, DevDisturbance> lib{{"disturbance", "pg_set_disturbance_index"}}; SeedStreams streams; HistSlot hist;      // hist: pg_set_disturbance_history_dev
        real *n = nullptr, *w = nullptr; DevVehicle* veh = nullptr; bool fresh = true, valid = false; int64_t steps_stat = 0;
        void cleared() { fresh = true; valid = false; hist.clear(); }      // (a library installed later starts a gust of its own)
    } disturbance;
    // estimator library (pg_set_estimator_sets / pg_set_estimator_index): a fixed-gain observer between the sensor and the controller of a rollout step.  Beside the sets,
    // allocated at the first install: the estimate x [cap][6] (what the gate and the compute calls of a step are handed as the state) and u [cap][3], the control
    // the controller was handed at the previous step (it drives the prior).  Nothing is allocated without a library
    struct Estimator {
        SetLib<pg_estimator, DevEstimator> lib{{"estimator", "pg_set_estimator_index"}}; HistSlot hist;      // hist: pg_set_estimated_history_dev
        real *x = nullptr, *u = nullptr; bool fresh = true, valid = false; int64_t steps_stat = 0;
        void cleared() { fresh = true; valid = false; hist.clear(); }      // (a library installed later starts from its first measurement)
    } estimator;
    // human library (pg_set_human_sets / pg_set_human_index / pg_set_human_seed): the driver of the other car in the safety and node rollouts.  Beside the sets: the streams
    // and the seed (its own), and, allocated when a rollout first runs under a library: the driver's control u [cap][2] (k_human writes it, the step's plant launch reads
    // it as the script of its human mode 2) and the random driver's state n [cap][2].  script: some installed set has mode 2 (the rollouts then want human_u_dev)
    struct Human {
        SetLib<pg_human, DevHuman> lib{{"human", "pg_set_human_index"}}; SeedStreams streams; HistSlot hist;      // hist: pg_set_human_history_dev
        real *u = nullptr, *n = nullptr; bool script = false, fresh = true, valid = false; int64_t steps_stat = 0;
        void cleared() { script = false; fresh = true; valid = false; hist.clear(); }      // (a library installed later starts a driver of its own)
    } human;
    // route library (pg_set_route_sets / pg_set_route_index): an instance changes trajectory during a rollout (k_route).  Beside the sets (the device records ARE the
    // caller's: no real in them): the clock steps that carry an event in some installed set (the host's branch choice and the launches follow them), and, allocated when a
    // rollout first runs under a library: fired [cap] then last_step [cap], t_at [cap], e_at [cap].  The trajectory index the events write is traj_idx.d; HOME is
    // traj_idx.host.  fresh: the clock restarted -- the next rollout under a library puts every instance back on its home trajectory with fired = 0 (route_start).
    // hist: pg_set_route_history_dev, one-shot, int32 [steps][B]
    struct Route {
        SetLib<pg_route, pg_route> lib{{"route", "pg_set_route_index"}}; std::vector<int> event_steps;
        int *fired = nullptr, *hist = nullptr; int hist_steps = 0; double* t_at = nullptr; real* e_at = nullptr; bool fresh = true; int64_t steps_stat = 0;
        bool event_at(int step) const { for (int s : event_steps) if (s == step) return true; return false; }
        void cleared() { event_steps.clear(); fresh = true; hist = nullptr; hist_steps = 0; }
    } route;
    // the inputs: the true state and the command, always -- assigned once, by pg_create.  What a step's controller is handed instead travels as a Seen (below)
    real *d_state = nullptr, *d_control = nullptr, *d_other = nullptr;
    double *d_t0 = nullptr, *d_toff = nullptr;            // absolute time stays fp64 in both builds (tdouble)
    // clock of pg_simulate_dev (model_predictive_control.jl:87, `for t in 0:dt:trajectory.t[end]`): start time per instance, the range, and the index of the element t0 holds.
    // pg_set_inputs* restarts it (sim_idx = 0); consecutive pg_simulate_dev calls with the same dt continue it, so 4 + 40 steps see the times of 44
    double* d_tstart = nullptr; JlRange sim_clk{}; int sim_idx = 0; double sim_dt = 0.0, sim_tend = 0.0; double traj_t_end = 0.0;
    int* d_solved = nullptr; uint8_t* d_mask = nullptr;     // d_mask: staging of pg_reset's per-instance mask
    double *d_ts = nullptr, *d_dt = nullptr, *d_prev_ts = nullptr;
    real *d_sep = nullptr, *d_nodes = nullptr, *d_qp = nullptr, *d_naux = nullptr;      // d_naux [cap][NN][4]: arguments of the angles k_nodes leaves to k_nodes_angles
    real *d_x7 = nullptr, *d_vg8 = nullptr, *d_Mb = nullptr;
    real *d_solx = nullptr, *d_sigma = nullptr, *d_u = nullptr, *d_mu = nullptr;
    real* d_lam = nullptr;                                      // [cap][N][16] multipliers of the last solve (warm start of the polish)
    int* d_wfail = nullptr;                                     // [cap] back-off of k_solve_lat's warm attempts (the second half of the d_solved allocation: pg_reset clears both with one fill)
    int pipe_pub_short = 3, pipe_pub_long = 5;                        // options: the recurrence of the pipelined launch publishes every n-th node of the short / long horizon
    int pipe_first = 0;                                               // option "pipe_first": short-horizon intervals that go first in the pipelined launch (0 = as many as fill the SIMDs the recurrence leaves free)
    int pipe_min = 2304, pipe_max = 256 * NODES_IPB;                    // batch sizes the pipelined launch serves (options "pipe_min" / "pipe_max"; its nodes blocks must be resident at once: <= 16384)
    int lin_lpi = 1;                                          // lanes per (instance, interval) of the large-batch linearisation (k_linearize_split / k_nodes_linearize): one lane with all eight
                                                              // directions (option "lin_lanes" = 2: the lane pair of rounds 1-3, for A/B runs; same bits in fp64, rounding-level differences in fp32)
    int* d_todo = nullptr; int split_solve = 1, split_lat = 1;      // d_todo: instances one solve launch leaves to the next; behind them the control words of the solve launches: layout below (solve_ctl)
    int phase_timing = 0;                                           // option "phase_timing": 1 = pg_step_dev records the four HIP events pg_get_phase_ms reads (13-25 us of stream time per step at B = 4096: 2-4 %); 0 (default) = no instrumentation on the stream
    int* d_order = nullptr; int order_B = 0;  // launch order filed by the nodes kernels of the current step (likely slow instances first): layout below (order_cnt); order_B = batch it is valid for
    real *d_pol_u2 = nullptr, *d_pol_u = nullptr; int* d_pol_src = nullptr;   // HJI fallback policy (HJI_computation.jl:133-158)
    real* d_vmin = nullptr; int* d_breach = nullptr;          // summary of pg_simulate_safety_dev: V_min [cap]; first_breach [cap] then policy_steps [cap] (k_advance_safety)
    bool sum_fresh = true;                                    // the summary restarts at the next safety step (the clock restarted since it was last written)
    // node callback (pg_node_step_dev / pg_simulate_node_dev), allocated at the first call of one of them: the keep buffer of gated-out instances' warm state (KeepView,
    // pg_kernels.hip), the node words d_node (layout below: node_cold; node_parity is the cold word the next recheck reads); the applied command [cap][3];
    // trajectory.t[end] per installed trajectory, fp64
    char* d_keep = nullptr; KeepView kv{}; int* d_node = nullptr; real* d_applied = nullptr; double* d_tend = nullptr;
    std::vector<double> traj_ends; bool tend_dirty = true;
    int node_parity = 0; bool node_recheck = false;           // node_recheck: the last step was a node step (some instance may have no solution: launch_nodes queues k_nodes_recheck)
    bool node_fresh = true;                                   // the node counts restart at the next node step (the clock restarted since they were last written)
    int *d_status = nullptr, *d_iters = nullptr, *d_polish = nullptr; uint16_t* d_active = nullptr;
    // HJI grid: the view the kernels are handed (knots and cells point into the two buffers, nodes is null: the node records die with the call that installs), the two
    // buffers, and whether a grid is installed (dc.has_hji mirrors `on` for the kernels).  Written by hji_table_clear and hji_table_build only
    struct HjiTable { HjiView hv; float *knots = nullptr, *cells = nullptr; bool on = false; HjiTable() { memset(&hv, 0, sizeof(hv)); } } hji;
    hipEvent_t ev[4]; bool ev_ok = false; float phase_ms[3] = {0, 0, 0}; bool timing_valid = false;
    size_t solve_lds = 0; bool solve_ring = false;
    real* d_walls = nullptr;                                    // [cap][N][2] wall extension
    char* d_lat_ws = nullptr; bool lat_mem = false, lat_mem_forced = false;            // k_solve_lat's workspace for horizons beyond 32 intervals (option "lat_workspace" = 1: at every horizon)
    real* d_lat_spc = nullptr;                                  // k_solve_lat's lane-contiguous stage constants (lat_spc_bytes)
    real* d_hand_r = nullptr; int* d_hand_i = nullptr;          // [cap][8] / [cap][16] hand-over records of k_solve_lat's unfinished instances (round 6: SolveOut::hand_mode)
    int lat_single_max = 1024;                                  // option "lat_single_max": cold lateral batches up to this size run ONE instance per wavefront from the start (k_solve_lat<.., 64, 0>)
    int lat_handover = 1, lat_hand_target = 0, lat_hand_min = 8, lat_hand_cap = 0, lat_hand_batch = 1025, lat_hand_work = 0, lat_hand_w0 = 3;      // options "lat_handover" (0 off, 1 = on), "lat_hand_target", "lat_hand_min", "lat_hand_cap", "lat_hand_batch" (smallest batch that hands over)
    int64_t stat_lat_single = 0;                                // read-only option "stat_lat_one_per_wavefront_solves"
    int64_t stat_lat_hand = 0;                                  // read-only option "stat_lat_handover_solves"
    real* d_lat_aux = nullptr;                                  // [cap][64][8] F, Bbar'P Bbar, Bbar'y per stage: what k_solve_lat reads the multiplier of a pinned rate row from
    real* d_lat = nullptr;                                      // [cap][N][LATP] packed stage records of the lateral formulation (k_qp_dec -> k_solve_lat)
    // hipGraph of a whole host-to-host warm step (pg_step of a small batch is launch-bound: one copy in, four kernels, one copy out; captured once, replayed while
    // nothing that the launches depend on has changed -- `sig` is compared field by field before every replay)
    struct StepGraph { hipGraph_t g = nullptr; hipGraphExec_t x = nullptr; hipStream_t own = nullptr; bool disabled = false; bool capturing = false;
                       DevCfg dc; HjiView hv; int B = 0, fuse = 0, pipeline = 0, has_hji = 0, traj_L = 0; hipStream_t user = nullptr; } sg;
    int graph_mode = 0;                                       // option "graph" = 1 turns it on.  OFF by default: capturing costs ~7 ms once and again whenever a launch parameter changes (a re-installed
                                                              // path: every `path` message of the ROS loop), a jitter that a 100 Hz loop minds more than the 4-20 us per step the replay saves
    char* d_in = nullptr; char* d_out = nullptr;             // the five input arrays / (u, status, iters) as ONE allocation each: a batch that fills the handle travels in one copy per direction
    size_t in_bytes = 0, out_bytes = 0, in_dbl_off = 0;        // (layout by capacity: [state 6][control 3][other 4] real, then at in_dbl_off [t0][time_offset] double; [u 3] real, [status][iters] int)
    char* h_stage = nullptr; size_t stage_bytes = 0;            // pinned host staging of pg_set_inputs / pg_step (one stream synchronisation per call instead of one per array)
    bool qp_embedded = true; int lat_pack_only = 1;            // lateral formulation: the embedded QP block is current (k_qp_dec wrote it) / option "lat_pack_only": steps write the packed records only
    bool qp_stale = false;                                    // the lateral solver was switched (option "lateral_solver") after the last update_QP!: pg_solve returns PG_ERR_STATE until the QP data are rebuilt
    bool solve_lat = false; size_t lat_lds = 0;               // lateral formulation: its own kernel k_solve_lat (option "lateral_solver" = 2 keeps the embedding in k_solve)
    pg_handle() = default; pg_handle(const pg_handle&) = delete; pg_handle& operator=(const pg_handle&) = delete;      // (never copied or moved: `mem` holds addresses of members)
    // what is not device memory; the device is current (pg_create set it, pg_destroy sets it)
    ~pg_handle() {
        if (h_stage) (void)hipHostFree(h_stage); if (sg.x) (void)hipGraphExecDestroy(sg.x); if (sg.g) (void)hipGraphDestroy(sg.g); if (sg.own) (void)hipStreamDestroy(sg.own);
        if (ev_ok) for (int i = 0; i < 4; i++) (void)hipEventDestroy(ev[i]);
    }
    // Every device buffer above is allocated through mem (ensure / adopt below) and freed by it, here or in a drop.  LAST member: destroyed first
    HandleBufs mem;
};

#define HIPCHK(h, call) do { const hipError_t e_ = (hipError_t)(call); if (e_ != hipSuccess) { (h)->err = std::string(#call) + ": " + hipGetErrorString(e_); return PG_ERR_HIP; } } while (0)
#define LAUNCH_CHECK(h) do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { (h)->err = std::string("kernel launch: ") + hipGetErrorString(e_); return PG_ERR_HIP; } } while (0)
#define REQUIRE(h, cond, msg) do { if (!(cond)) { if (h) (h)->err = (msg); return PG_ERR_INVALID; } } while (0)
// a *_problem check (why: its text, or nullptr when nothing is wrong) refuses with "<who><why>"; `who` carries its own ": "
#define REQUIRE_NO(h, who, why) do { const char* why_ = (why); if (why_) { (h)->err = std::string(who) + why_; return PG_ERR_INVALID; } } while (0)

static std::string g_create_error;

// what the two owners of pg_own.hpp allocate and free with: the library's only calls of either
int pg_dev_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
void pg_dev_free(void* p) { (void)hipFree(p); }
// The one way a buffer of the handle comes to be: `count` elements for member p, allocated when it is first needed and owned by h->mem from then on
template <class T> static int ensure(pg_handle* h, T*& p, size_t count) {
    const int e = h->mem.get(p, count);
    if (e) { h->err = "device allocation of " + std::to_string(count * sizeof(T)) + " bytes failed: " + hipGetErrorString((hipError_t)e); return PG_ERR_HIP; }
    return PG_OK;
}
// the stream ids of a seeded library on the device, [capacity]: the installed ones, then stream[b] = b
int SeedStreams::sync(pg_handle* h) {
    if (d && !dirty) return PG_OK;
    const size_t cap = (size_t)h->cfg.batch_capacity;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    { const int rc = ensure(h, d, cap); if (rc) return rc; }
    std::vector<unsigned long long> full(cap);
    for (size_t b = 0; b < cap; b++) full[b] = b < host.size() ? (unsigned long long)host[b] : (unsigned long long)b;
    HIPCHK(h, hipMemcpy(d, full.data(), cap * sizeof(unsigned long long), hipMemcpyHostToDevice));
    dirty = false;
    return PG_OK;
}
// The walk over the seven dimensions of an HJI grid, written here only (pg_set_hji_grid, pg_hji_solve; hji_table_build reads its result): nodes n, knots nk and, per
// dimension, the stride of its node index and the offset of its knots.  Refuses in the name of `who` fewer than 2 knots.  fill(): into a device view (HjiView, HjiSolveGrid)
struct HjiWalk {
    int dims[7], koff[7]; long stride[7]; size_t n; int nk;
    template <class Grid> void fill(Grid& G) const { for (int d = 0; d < 7; d++) { G.dims[d] = dims[d]; G.koff[d] = koff[d]; G.stride[d] = stride[d]; } }
};
static int hji_walk(pg_handle* h, const char* who, const int32_t dims[7], HjiWalk& W) {
    W.n = 1; W.nk = 0;
    for (int d = 0; d < 7; d++) { REQUIRE(h, dims[d] >= 2, std::string(who) + ": every dimension needs >= 2 knots"); W.dims[d] = dims[d]; W.koff[d] = W.nk; W.stride[d] = (long)W.n; W.n *= dims[d]; W.nk += dims[d]; }
    return PG_OK;
}

// ---- The device words the launches share: each layout is defined HERE only -- the allocations take their sizes from it, every launch its addresses. ----
// d_todo [cap + CTL_WORDS] (the words zeroed by pg_create): the to-do list [cap] one solve launch files for the next, then the control words of the solve launches
enum SolveCtl {
    CTL_TODO0 = 0, CTL_TODO1 = 1,      // k_solve's split launch: two to-do counters used alternately -- [solve_parity] is zeroed by k_project of the step (or a memset in launch_solve_coupled) and
                                       // counted by this launch, the other holds the previous launch's count (SolveOut::mode).  k_solve_lat's two-launch warm solve: [0] = length of the list the
                                       // warm attempts leave (memset, counted by them).  k_solve_lat's hand-over (memset of [0..2], counted by the launch that hands over): [0] listed from the
    CTL_HAND_BACK = 2,                 // front, [1] finished instances, [2] listed from the back
    CTL_TIMELINE = 4,                  // pg_debug_solve_cycles with "diag_timeline": the to-do counter of its rounds-only launch (memset there)
    CTL_WHOLE = 5,                     // launches in which the full k_solve took the whole batch (SolveOut::n_whole: counted by k_solve, read by option "stat_whole_batch_solves")
    CTL_WORDS = 8
};
// d_order [2 cap + ORDER_CNT_WORDS]: the launch order [cap]; two counters (filed from the front / from the back: zeroed by k_project of the step or by launch_hji_order, counted by
// the nodes kernels and k_order_hji); the verdict per instance [cap] (the same kernels)
// d_node [6 cap + NODE_COLD_WORDS], zeroed by node_prepare: gate [cap] (k_node_gate), heartbeat [cap] and counts [cap][4] (k_node_finish), two cold words used alternately (zeroed
// by k_node_gate, set by k_node_finish of the same step, read by k_nodes_recheck of the next)
// d_progress [cap / NODES_IPB + PIPE_WORDS], zeroed by pg_create: nodes completed per nodes wavefront [nbn <= cap / NODES_IPB + 1] of the pipelined launch (k_nodes_linearize), then the
// fault word of the launch (set by a waiting wavefront that gave up, read by the predicated repair) -- k_project of the step zeroes these nbn + 1 words --; last word: fall-backs so
// far (counted by the wavefronts that gave up, never reset: pg_get_pipeline_fallbacks)
enum { ORDER_CNT_WORDS = 2, NODE_COLD_WORDS = 2, PIPE_WORDS = 8 };
static size_t cap_of(const pg_handle* h) { return (size_t)h->cfg.batch_capacity; }
static int* solve_ctl(const pg_handle* h, int word) { return h->d_todo + cap_of(h) + word; }
static int* order_cnt(const pg_handle* h) { return h->d_order + cap_of(h); }                     static int* order_slow(const pg_handle* h) { return order_cnt(h) + ORDER_CNT_WORDS; }
static int* node_heartbeat(const pg_handle* h) { return h->d_node + cap_of(h); }                 static int* node_counts(const pg_handle* h) { return h->d_node + 2 * cap_of(h); }
static int* node_cold(const pg_handle* h, int parity) { return h->d_node + 6 * cap_of(h) + parity; }
static size_t pipe_words(const pg_handle* h) { return cap_of(h) / NODES_IPB + PIPE_WORDS; }
static int* pipe_fault_word(const pg_handle* h, int nbn) { return h->d_progress + nbn; }         static int* pipe_fallbacks(const pg_handle* h) { return h->d_progress + pipe_words(h) - 1; }
// ---- the solve kernels' launches (templates: ahead of the extern "C" block) ----
// the outputs every solve launch writes, `order` = the launch order (nullptr: index order); everything else zero -- each arrangement below sets the fields it uses
static SolveOut solve_out(const pg_handle* h, const int* order) {
    SolveOut O{}; O.sol_x = h->d_solx; O.sol_sigma = h->d_sigma; O.u_out = h->d_u; O.status = h->d_status; O.iters = h->d_iters; O.active = h->d_active; O.mu = h->d_mu;
    O.solved = h->d_solved; O.polish = h->d_polish; O.lam = h->d_lam; O.order_in = order; O.wfail = h->d_wfail;
    return O;
}
// pg_step_dev's control array (SolveOut::u_out2; nullptr: none) and whether a launch took it: every k_solve instantiation writes it itself, the lateral kernel does not
struct DirectOut { real* u = nullptr; bool written = false; };
static void take_direct(SolveOut& O, DirectOut& D) { if (D.u) { O.u_out2 = D.u; D.written = true; } }
// What the controller's side of a step is handed as current state and current control: the handle's own pair, except in a rollout step under a sensor, estimator or
// actuator library (rollout_compute).  Every launch on that side takes the two from here, never from the handle
struct Seen { const real* state; const real* control; };
static Seen seen_own(const pg_handle* h) { return Seen{h->d_state, h->d_control}; }
// one k_solve launch, one wavefront per instance, `n` blocks
template <bool PROF, bool RING, bool FUSE, bool IPM = true>
static void launch_k_solve(pg_handle* h, hipStream_t st, int n, const SolveOut& O, unsigned long long* prof = nullptr) {
    hipLaunchKernelGGL((k_solve<PROF, RING, FUSE, IPM>), dim3(n), dim3(64), h->solve_lds, st, h->dc, h->B, h->d_qp, h->d_nodes, O, prof, h->d_dt, h->d_Mb);
}
// one k_solve_lat launch: the instantiation with or without the wall rows, the row state in registers (MEM = 0), in the workspace (1) or where the handle keeps it (LAT_MEM_ANY)
enum { LAT_MEM_ANY = 2 };
template <int MEM, int LPI, int HAND>
static void launch_k_solve_lat(pg_handle* h, dim3 grid, size_t lds, hipStream_t st, const SolveOut& O, unsigned long long* prof) {
    if constexpr (MEM == LAT_MEM_ANY) { if (h->lat_mem) launch_k_solve_lat<1, LPI, HAND>(h, grid, lds, st, O, prof); else launch_k_solve_lat<0, LPI, HAND>(h, grid, lds, st, O, prof); }
    else if (h->dc.walls) hipLaunchKernelGGL((k_solve_lat<1, true, MEM != 0, LPI, HAND>), grid, dim3(64), lds, st, h->dc, h->B, h->d_qp, h->d_nodes, O, prof);
    else hipLaunchKernelGGL((k_solve_lat<1, false, MEM != 0, LPI, HAND>), grid, dim3(64), lds, st, h->dc, h->B, h->d_qp, h->d_nodes, O, prof);
}

// Host <-> device transfers of path data.  The ABI speaks double on the host side; device buffers are `real` (double in libpigeon_hip.so,
// float in libpigeon_hip_f32.so).  *_dev entry points take device pointers in the library's own element type (times are always double).
static int up(pg_handle* h, real* dst, const double* src, size_t n) {            // returns after the host buffer has been consumed
#ifdef PG_F32
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; i++) tmp[i] = (float)src[i];
    HIPCHK(h, hipMemcpyAsync(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, h->stream));
#else
    HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
#endif
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PG_OK;
}
static int down(pg_handle* h, double* dst, const real* src, size_t n) {          // returns after the copy has completed
    if (!dst) return PG_OK;
#ifdef PG_F32
    std::vector<float> tmp(n);
    HIPCHK(h, hipMemcpyAsync(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++) dst[i] = (double)tmp[i];
#else
    HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
#endif
    return PG_OK;
}
// `count` elements of a host array to a buffer of the same element type, under HIPCHK.  A plain synchronous copy: the host array is consumed when it returns, on every way out
template <class T> static hipError_t to_device(T* dst, const T* src, size_t count) { return hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice); }
static int down_raw(pg_handle* h, void* dst, const void* src, size_t bytes) {      // integer / time buffers: same type on both sides
    if (!dst) return PG_OK;
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PG_OK;
}
static void fill_dev_control(DevControl& U, const pg_control_params& u);
static void fill_dev_vehicle(DevVehicle& V, const pg_vehicle& v) {
    V.G = (real)v.G; V.m = (real)v.m; V.Izz = (real)v.Izz; V.L = (real)v.L; V.a = (real)v.a; V.b = (real)v.b; V.h = (real)v.h; V.mu = (real)v.mu;
    V.Caf = (real)v.Caf; V.Car = (real)v.Car; V.Cd0 = (real)v.Cd0; V.Cd1 = (real)v.Cd1; V.Cd2 = (real)v.Cd2;
    V.fwd_frac = (real)v.fwd_frac; V.rwd_frac = (real)v.rwd_frac; V.fwb_frac = (real)v.fwb_frac; V.rwb_frac = (real)v.rwb_frac;
    V.Fx_max = (real)v.Fx_max; V.Fx_min = (real)v.Fx_min; V.Px_max = (real)v.Px_max; V.delta_max = (real)v.delta_max; V.kappa_max = (real)v.kappa_max;
}
static void fill_dev_params(DevCfg& C, const pg_config* cfg) {
    fill_dev_vehicle(C.veh, cfg->vehicle);
    fill_dev_control(C.cp, cfg->control);
}
static void fill_dev_control(DevControl& U, const pg_control_params& u) {
    U.V_min = (real)u.V_min; U.V_max = (real)u.V_max; U.k_V = (real)u.k_V; U.k_s = (real)u.k_s; U.deltadot_max = (real)u.deltadot_max;
    U.Q_ds = (real)u.Q_ds; U.Q_dpsi = (real)u.Q_dpsi; U.Q_e = (real)u.Q_e; U.W_beta = (real)u.W_beta; U.W_r = (real)u.W_r; U.W_HJI = (real)u.W_HJI;
    U.R_delta = (real)u.R_delta; U.R_ddelta = (real)u.R_ddelta; U.R_Fx = (real)u.R_Fx; U.R_dFx = (real)u.R_dFx; U.N_HJI = u.N_HJI;
}

// One set of control parameters as the kernels read it, with what is derived from it: the inert slots of the embedded lateral problem pinned (decoupled formulation), and
// the value of its inert Ux slot, strictly inside [V_min, V_max] of THIS set.  pg_create makes the uniform set of the handle with it, the library every one of its sets.
static DevControlRec make_control_rec(int formulation, const pg_control_params& u) {
    DevControlRec r; fill_dev_control(r.cp, u);
    r.ux_dummy = (real)(0.5 * (u.V_min + u.V_max));
    if (formulation == PG_DECOUPLED) { r.cp.Q_ds = 0.0; r.cp.R_Fx = 0.0; r.cp.R_dFx = 1.0; r.cp.N_HJI = 0; r.cp.W_HJI = 0.0; }
    return r;
}

// Lateral formulation: which kernel solves it, and the buffers that kernel needs.  Called by pg_create and by pg_set_option("lateral_solver" / "lat_workspace").
// A failure says why in h->err
static int configure_lateral(pg_handle* h) {
    DevCfg& C = h->dc; const pg_config* cfg = &h->cfg; const int N = C.N; const size_t cap = (size_t)cfg->batch_capacity;
    const bool want = h->lateral_solver == 1 || (h->lateral_solver != 2 && !(cfg->polish && N <= 20));
    h->solve_lat = cfg->formulation == PG_DECOUPLED && want;
    if (!h->solve_lat) { C.lat_pack = nullptr; return PG_OK; }
    int rc;
    if ((rc = ensure(h, h->d_lat, cap * N * LATP))) return rc;                          // the packed lateral stage records
    C.lat_pack = h->d_lat;
    if ((rc = ensure(h, h->d_lat_aux, (cap + 1) * 64 * LAT_AUX + 8))) return rc;      // k_solve_lat's multiplier block (+ 1: the spare block idle lane groups of a resumed launch write)
    C.lat_aux = h->d_lat_aux;
    C.lat_zero = h->d_lat_aux + (cap + 1) * 64 * LAT_AUX;      // (+ 8 stored zeros: DevCfg::lat_zero)
    if (hipMemset((void*)C.lat_zero, 0, 8 * sizeof(real)) != hipSuccess) { h->err = "hipMemset failed"; return PG_ERR_HIP; }
    // (round 4: with the wall rows the two-slot register variant spills 720 B per lane since the warm start was added -- 1.57 ms at N = 30 against 1.36 ms through the
    // workspace; without them the registers still win, 0.94 against 1.01 ms)
    // (round 6: horizons of 17..32 intervals WITHOUT the wall rows used the two-slot register instantiation, k_solve_lat<2, .., false> -- 512 registers + 300 B of scratch, the
    // largest code of the kernel.  With this round's edits hipcc 7.2 allocated one accumulation register to two live values there (a debugger session, precise memory violations on: the
    // stage index of a slot visit read back from a76 was the high word of a double; memory access fault at the first launch).  Not a source bug that could be found: the
    // instantiation is retired, those horizons take the workspace variant like the longer ones -- and its straggler hand-over with it)
    h->lat_mem = N > 16 || h->lat_mem_forced;
    if (h->lat_mem) {
        if ((rc = ensure(h, h->d_lat_ws, lat_ws_bytes(cap)))) return rc;                              // k_solve_lat's workspace
        C.lat_ws = h->d_lat_ws;
        if ((rc = ensure(h, h->d_lat_spc, lat_spc_bytes((int)cap, N) / sizeof(real)))) return rc;      // ... its stage constants
        C.lat_spc = h->d_lat_spc;
        if ((rc = ensure(h, h->d_hand_r, cap * LAT_HAND_R)) || (rc = ensure(h, h->d_hand_i, cap * LAT_HAND_I))) return rc;      // ... its hand-over records
    } else C.lat_ws = nullptr;
    return PG_OK;
}

extern "C" {

int pg_default_config(pg_config* c) {
    if (!c) return PG_ERR_INVALID;
    memset(c, 0, sizeof(*c));
    pg_vehicle& P = c->vehicle;                      // vehicles.jl:1-59
    P.G = 9.80665;
    double mfl = 484, mfr = 455, mrl = 521, mrr = 504;
    P.m = mfl + mfr + mrl + mrr; P.Izz = 2900; P.L = 2.87;
    P.a = (mrl + mrr) / P.m * P.L; P.b = (mfl + mfr) / P.m * P.L;
    P.h = 0.1 * P.b / P.L + 0.1 * P.a / P.L + 0.37;
    P.mu = 0.92; P.Caf = 150e3; P.Car = 220e3; P.Fx_max = 5600; P.Px_max = 75e3; P.Cd0 = 241.0; P.Cd1 = 25.1; P.Cd2 = 0.0;
    P.fwd_frac = 0.0; P.rwd_frac = 1.0 - P.fwd_frac; P.fwb_frac = 0.6; P.rwb_frac = 1.0 - P.fwb_frac;
    double f1 = -P.m * P.G * P.a * P.mu / (P.L * P.rwb_frac + P.mu * P.h), f2 = -P.m * P.G * P.b * P.mu / (P.L * P.fwb_frac - P.mu * P.h);
    P.Fx_min = f1 > f2 ? f1 : f2;
    P.delta_max = 18 * M_PI / 180; P.kappa_max = tan(P.delta_max) / P.L;
    pg_control_params& U = c->control;               // coupled_lat_long.jl:23-38
    U.V_min = 1.0; U.V_max = 15.0; U.k_V = 10.0 / 4 / 100; U.k_s = 10.0 / 4 / 10000; U.deltadot_max = 0.344;
    U.Q_ds = 1.0; U.Q_dpsi = 1.0; U.Q_e = 1.0; U.W_beta = 50 / (10 * M_PI / 180); U.W_r = 50.0; U.W_HJI = 500.0; U.N_HJI = 3;
    U.R_delta = 0.0; U.R_ddelta = 0.1; U.R_Fx = 0.0; U.R_dFx = 0.5;
    c->N_short = 10; c->N_long = 20; c->dt_short = 0.01; c->dt_long = 0.2; c->use_correction_step = 1;   // coupled_lat_long.jl:42-43
    c->rk4_substeps = 10; c->hji_eps = 0.05; c->batch_capacity = 4096; c->device = 0;
    c->ipm_max_iter = 40; c->ipm_mu0 = 100.0; c->formulation = PG_COUPLED; c->walls = 0; c->wall_weight = 1000.0;
    c->polish = 1; c->warm_polish = 1; c->cold_guess = 8;
#ifdef PG_F32
    c->ipm_tol = 1e-5; c->polish_rho = 1e3; c->polish_tol = 1e-4; c->polish_ipm_tol = 1e-4;
#else
    c->ipm_tol = 1e-12; c->polish_rho = 1e7; c->polish_tol = 1e-9; c->polish_ipm_tol = 3e-6;
#endif
    return PG_OK;
}

int pg_default_config_decoupled(pg_config* c) {
    int rc = pg_default_config(c); if (rc) return rc;
    pg_control_params& U = c->control;               // decoupled_lat_long.jl:18-30
    const double d10 = 10 * M_PI / 180;
    U.Q_ds = 0.0; U.Q_dpsi = 1.0 / (d10 * d10); U.Q_e = 1.0; U.W_beta = 50 / d10; U.W_r = 50.0; U.W_HJI = 0.0; U.N_HJI = 0;
    U.R_delta = 0.0; U.R_ddelta = 0.01 / (d10 * d10); U.R_Fx = 0.0; U.R_dFx = 1.0;      // R_dFx only pins the inert Fx slot of the embedding
    c->formulation = PG_DECOUPLED;
    // polish ON (round 3; it used to be off here): with the interior point alone 5 (48 with the wall rows) of the 4096 N = 50 benchmark instances end 1e-6 .. 1e-4 from the
    // exact optimum of their own QP data -- rows that are nearly degenerate, on horizons whose optimum leaves the linearisation by kilometres --; behind the polish of
    // k_solve_lat every one of them is within 1.3e-7 (tests/test_gpu_decoupled.py::test_config5_as_shipped_every_instance_against_the_oracle)
    c->polish = 1;
#ifdef PG_F32
    c->ipm_tol = 1e-4;                               // the ill-conditioned 8 s lateral horizon stalls near 1e-4 in fp32 (tests/test_gpu_f32.py)
#endif
    return PG_OK;
}

const char* pg_last_error(const pg_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pg_create(const pg_config* cfg, pg_handle** out) {
    if (!cfg || !out) return PG_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_create_error = "no HIP device available (this library has no CPU path)"; return PG_ERR_NO_DEVICE; }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "device ordinal out of range"; return PG_ERR_INVALID; }
    if (cfg->formulation != PG_COUPLED && cfg->formulation != PG_DECOUPLED) { g_create_error = "unknown formulation"; return PG_ERR_INVALID; }
    if (cfg->walls != 0 && (cfg->walls != 1 || cfg->formulation != PG_DECOUPLED)) { g_create_error = "walls = 1 is an option of the decoupled formulation only"; return PG_ERR_INVALID; }
    if (cfg->polish && !(cfg->polish_rho > 0.0 && cfg->polish_tol > 0.0)) { g_create_error = "polish needs polish_rho > 0 and polish_tol > 0"; return PG_ERR_INVALID; }
    if (cfg->N_short < 1 || cfg->N_long < 0 || cfg->N_short + cfg->N_long + 1 > 64 || cfg->batch_capacity < 1 || cfg->rk4_substeps < 1) {
        g_create_error = "invalid horizon / capacity (need 1 <= N_short, N_short+N_long+1 <= 64)"; return PG_ERR_INVALID;
    }
#ifdef PG_F32
    if (cfg->formulation == PG_DECOUPLED && cfg->N_short + cfg->N_long > 32 && cfg->allow_f32_long_lateral != 1) {
        g_create_error = "the fp32 library refuses the decoupled formulation beyond 32 intervals (applied steering up to 6e-3 rad off on the N = 50 benchmark batch: use libpigeon_hip.so, "
                         "or set pg_config.allow_f32_long_lateral = 1 to run it anyway)";
        return PG_ERR_INVALID;
    }
#endif
    if (hipSetDevice(cfg->device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return PG_ERR_HIP; }
    std::unique_ptr<pg_handle> own(new pg_handle()); pg_handle* const h = own.get();      // (an exit below destroys the handle and, through h->mem, every buffer it has by then)
    h->cfg = *cfg;
    DevCfg& C = h->dc; memset(&C, 0, sizeof(C));
    fill_dev_params(C, cfg); C.Ns = cfg->N_short; C.Nl = cfg->N_long; C.N = C.Ns + C.Nl; C.NN = C.N + 1;
    C.dt_short = cfg->dt_short; C.dt_long = cfg->dt_long; C.use_correction_step = cfg->use_correction_step; C.nsub = cfg->rk4_substeps;
    C.alias_prev_ts = 1; C.has_hji = 0; C.hji_eps = (real)cfg->hji_eps;
    C.tg_short = jl_scalar_times_unitrange(cfg->dt_short, 0, cfg->N_short); C.tg_long = jl_scalar_times_unitrange(cfg->dt_long, 1, cfg->N_long); C.time_grid_naive = 0;
    C.un0 = (real)cfg->vehicle.delta_max; C.un1 = (real)fmax(-cfg->vehicle.Fx_min, cfg->vehicle.Fx_max);      // coupled_lat_long.jl:199
    C.fxmin_n = (real)(cfg->vehicle.Fx_min / fmax(-cfg->vehicle.Fx_min, cfg->vehicle.Fx_max));
    C.formulation = cfg->formulation;
    C.cp_sets = nullptr; C.cp_idx = nullptr; C.n_cp = 0; C.cp_epoch = 0;      // no control-parameter library: every kernel reads C.cp / C.ux_dummy
    C.dbg_poison = 0; C.dbg_instance = -1;                              // (-DPG_DIAG builds: option "diag_instance")
    if (cfg->formulation == PG_DECOUPLED) { C.un0 = 1.0; C.un1 = 1.0; C.fxmin_n = -1.0; }          // no u normalisation in the lateral QP (decoupled_lat_long.jl:134-226)
    { const DevControlRec r = make_control_rec(cfg->formulation, cfg->control); C.cp = r.cp; C.ux_dummy = r.ux_dummy; }
    h->cp_eff.assign((size_t)cfg->batch_capacity, cfg->control);
    C.qp_len = 84 * C.N + 11;
    C.ipm_max_iter = cfg->ipm_max_iter; C.ipm_tol = (real)cfg->ipm_tol; C.ipm_mu0 = (real)cfg->ipm_mu0;
    C.polish = cfg->polish != 0; C.polish_rho = (real)cfg->polish_rho; C.polish_tol = (real)cfg->polish_tol; C.polish_ipm_tol = (real)cfg->polish_ipm_tol; C.warm_polish = cfg->warm_polish != 0; C.cold_guess = cfg->cold_guess > 0 ? cfg->cold_guess : 0;
    const size_t cap = (size_t)cfg->batch_capacity; const int N = C.N, NN = C.NN;
#define ALLOC(ptr, count) do { if (ensure(h, ptr, (size_t)(count))) { g_create_error = h->err; return PG_ERR_HIP; } } while (0)
    h->in_dbl_off = (cap * 13 * sizeof(real) + 7) / 8 * 8; h->in_bytes = h->in_dbl_off + cap * 16; h->out_bytes = cap * (3 * sizeof(real) + 8);
    ALLOC(h->d_in, h->in_bytes); ALLOC(h->d_out, h->out_bytes);
    h->d_state = (real*)h->d_in; h->d_control = h->d_state + cap * 6; h->d_other = h->d_control + cap * 3; h->d_t0 = (double*)(h->d_in + h->in_dbl_off); h->d_toff = h->d_t0 + cap;
    h->d_u = (real*)h->d_out; h->d_status = (int*)(h->d_u + cap * 3); h->d_iters = h->d_status + cap;
    ALLOC(h->d_tstart, cap); ALLOC(h->d_solved, 2 * cap); h->d_wfail = h->d_solved + cap; ALLOC(h->d_mask, cap); ALLOC(h->d_ts, cap * NN); ALLOC(h->d_dt, cap * N); ALLOC(h->d_prev_ts, cap * NN);
    ALLOC(h->d_sep, cap * 4); ALLOC(h->d_nodes, cap * NN * 10); ALLOC(h->d_qp, cap * C.qp_len);
    ALLOC(h->d_x7, cap * 7); ALLOC(h->d_vg8, cap * 8); ALLOC(h->d_Mb, cap * 4);
    ALLOC(h->d_solx, cap * NN * 8); ALLOC(h->d_sigma, cap * N * 3); ALLOC(h->d_mu, cap);
    ALLOC(h->d_polish, cap); ALLOC(h->d_todo, cap + CTL_WORDS); ALLOC(h->d_lam, cap * N * 16); ALLOC(h->d_order, 2 * cap + ORDER_CNT_WORDS); ALLOC(h->d_naux, cap * NN * 4); ALLOC(h->d_progress, pipe_words(h)); ALLOC(h->d_active, cap * N);
    if (cfg->walls) { ALLOC(h->d_walls, cap * N * 2); C.walls = 1; C.wall_weight = (real)cfg->wall_weight; C.wall_edges = h->d_walls; }
    ALLOC(h->d_pol_u2, cap * 2); ALLOC(h->d_pol_u, cap * 3); ALLOC(h->d_pol_src, cap); ALLOC(h->d_vmin, cap); ALLOC(h->d_breach, 2 * cap);
    // The lateral formulation has a solve kernel of its own (k_solve_lat, pg_solve_lat.hip) for horizons beyond 20 intervals.  Shorter ones -- the reference's on-vehicle
    // N_short = 5, N_long = 10 among them -- stay with the embedding in k_solve when the polish is on: its active-set rounds from the empty set serve a short lateral QP
    // without any interior-point iteration (N = 15, 4096 instances: 0.12 ms against 0.37), an advantage that is gone at N = 30 (2.4 against 1.5 ms) and reversed at
    // N = 50 (12.6 against 5.9).  Option "lateral_solver" = 1 / 2 forces the choice (configure_lateral below).
    if (cfg->formulation == PG_DECOUPLED) {
        // defaults of k_solve_lat's tuning options (pg_set_option)
        C.lat_mu0_cost = real(10.0); C.lat_pin = 1; C.lat_polish2 = 1; C.lat_far_cost = real(3e4); C.lat_rho_scale = sizeof(real) == 8 ? real(1e3) : real(1.0); C.lat_polish_rounds = 3; C.lat_settle = 0;
        C.lat_warm_rounds = 2;      /* (2 since the two-launch warm step: an attempt that needs a third working set is cheaper to hand to the cold list: 2.03 -> 1.95 ms, 2.9 -> 2.7 with walls) */
        C.lat_wipm = 0; C.lat_wmu = real(1e-2); C.lat_wtau = real(1e-4); C.lat_aux_gate = 1;
        if (configure_lateral(h) != PG_OK) { g_create_error = h->err; return PG_ERR_HIP; }
    }
#undef ALLOC
    h->stage_bytes = h->in_bytes > h->out_bytes ? h->in_bytes : h->out_bytes;          // inputs: state 6 + control 3 + other 4 (real) + t0 + time_offset (double); outputs reuse the front of it
    if (hipHostMalloc((void**)&h->h_stage, h->stage_bytes, hipHostMallocDefault) != hipSuccess) { g_create_error = "hipHostMalloc failed for the staging buffer"; return PG_ERR_HIP; }
    // initial ts = 1..NN (model_predictive_control.jl:13), solved = false
    {
        std::vector<double> ts(cap * NN), dt(cap * N, 1.0);
        for (size_t b = 0; b < cap; b++) for (int i = 0; i < NN; i++) ts[b * NN + i] = i + 1;
        (void)hipMemcpy(h->d_ts, ts.data(), ts.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(h->d_prev_ts, ts.data(), ts.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(h->d_dt, dt.data(), dt.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemset(h->d_solved, 0, 2 * cap * sizeof(int));
        (void)hipMemset(h->d_progress, 0, pipe_words(h) * sizeof(int));
        (void)hipMemset(h->d_status, 0, cap * sizeof(int));
        (void)hipMemset(h->d_other, 0, cap * 4 * sizeof(real));
        (void)hipMemset(h->d_solx, 0, cap * NN * 8 * sizeof(real));
        (void)hipMemset(h->d_lam, 0, cap * N * 16 * sizeof(real));          // pg_get_multipliers promises 0 off the working set: the kernels write only the rows they own
        (void)hipMemset(h->d_active, 0, cap * N * sizeof(uint16_t));
        (void)hipMemset(solve_ctl(h, 0), 0, CTL_WORDS * sizeof(int));
        if (hipDeviceSynchronize() != hipSuccess) { g_create_error = "initial fills failed"; return PG_ERR_HIP; }   // hipMemset may return before the fill has run
    }
    for (int i = 0; i < 4; i++) if (hipEventCreate(&h->ev[i]) != hipSuccess) { g_create_error = "hipEventCreate failed"; return PG_ERR_HIP; }
    h->ev_ok = true;
    // defaults of the build-defined options (pg_set_option changes them per handle; nothing here reads the process environment)
    C.hji_seed = 0; C.clip_guess = 1; C.clip_stops = 0; C.ck_riccati = 1; C.warm_trivial_cold = 1; C.hji_rounds = 0;
    // horizons up to 32 intervals keep their dynamics blocks resident in LDS (one pass over the QP data); longer ones stream them through a 4-slot ring
    h->solve_ring = N > 32;
    h->solve_lds = (size_t)((h->solve_ring ? 4 : N) * SB + 10 * NN + 8 * NN + 2 * N + 2 * N + 16 * N + 4 * N + 8 * N + 2 * N + 8 * NN + 2 * N + 72 + 100 + 8 + 72 + 4 + 32 + 2 * N + 11 * N) * sizeof(real);
    if (h->solve_lds > 160 * 1024) { g_create_error = "horizon too long for LDS staging"; return PG_ERR_INVALID; }
    // hipFuncSetAttribute applies to the CURRENT DEVICE's copy of a kernel, and a later handle with a shorter horizon must not lower the limit an earlier handle of the same
    // device relies on: the largest size asked for so far is kept per device ordinal
    static size_t lds_attr_max[64] = {0};
    const int dev_slot = cfg->device < 64 ? cfg->device : 63;
    if (lds_attr_max[dev_slot] < 48 * 1024) lds_attr_max[dev_slot] = 48 * 1024;
    if (h->solve_lds > lds_attr_max[dev_slot])
    {
        lds_attr_max[dev_slot] = h->solve_lds;
        (void)hipFuncSetAttribute((const void*)k_solve<false, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->solve_lds);
        (void)hipFuncSetAttribute((const void*)k_solve<false, false, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->solve_lds);
        (void)hipFuncSetAttribute((const void*)k_solve<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->solve_lds);
        (void)hipFuncSetAttribute((const void*)k_solve<false, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->solve_lds);
#ifdef PG_DIAG      // (the PROF instantiations exist in the diagnostic library only: pg_debug_solve_cycles)
        (void)hipFuncSetAttribute((const void*)k_solve<true, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->solve_lds);
        (void)hipFuncSetAttribute((const void*)k_solve<true, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->solve_lds);
#endif
    }
    h->lat_lds = lat_lds_doubles(N) * sizeof(real);
    // (N + 1 <= 64 nodes: at most 4 x 63 x 24 doubles + 72 = 48,960 B, below the 64 KB a launch may ask for without raising the function attribute)
    if (h->solve_lat && h->lat_lds > 64 * 1024) { g_create_error = "horizon too long for k_solve_lat's LDS staging"; return PG_ERR_INVALID; }
    *out = own.release();
    return PG_OK;
}

int pg_destroy(pg_handle* h) { if (!h) return PG_ERR_INVALID; (void)hipSetDevice(h->cfg.device); delete h; return PG_OK; }
int pg_get_config(const pg_handle* h, pg_config* out) { if (!h || !out) return PG_ERR_INVALID; *out = h->cfg; return PG_OK; }
int pg_get_u_normalization(const pg_handle* h, double out[2]) {
    if (!h || !out) return PG_ERR_INVALID;
    const bool dec = h->cfg.formulation == PG_DECOUPLED;      // reported in full precision (the host de-normalises with it)
    out[0] = dec ? 1.0 : h->cfg.vehicle.delta_max; out[1] = dec ? 1.0 : fmax(-h->cfg.vehicle.Fx_min, h->cfg.vehicle.Fx_max);
    return PG_OK;
}
int pg_precision_bits(void) { return (int)(8 * sizeof(real)); }
// Layout of the configuration structs as THIS library was compiled: the ctypes mirror (pigeon.jl_amd/_lib.py) and the Julia mirror (julia/PigeonMI355X.jl)
// are hand-written copies of include/pigeon_mpc.h; they compare their own sizeof / field offsets with these numbers before the first pg_create.
int pg_abi_layout(int32_t* out, int32_t n) {
#define OFF(f) (int32_t)offsetof(pg_config, f)
    const int32_t v[] = {(int32_t)sizeof(pg_config), (int32_t)sizeof(pg_vehicle), (int32_t)sizeof(pg_control_params), OFF(control), OFF(N_short), OFF(dt_short), OFF(use_correction_step),
                         OFF(hji_eps), OFF(batch_capacity), OFF(ipm_max_iter), OFF(formulation), OFF(ipm_tol), OFF(ipm_mu0), OFF(walls), OFF(wall_weight), OFF(polish), OFF(polish_rho),
                         OFF(polish_tol), OFF(polish_ipm_tol), OFF(warm_polish), OFF(cold_guess), (int32_t)offsetof(pg_control_params, N_HJI), (int32_t)offsetof(pg_vehicle, kappa_max)};
#undef OFF
    const int32_t cnt = (int32_t)(sizeof(v) / sizeof(v[0]));
    if (out) for (int32_t i = 0; i < cnt && i < n; i++) out[i] = v[i];
    return cnt;
}
int pg_qp_len(const pg_handle* h) { return h ? h->dc.qp_len : PG_ERR_INVALID; }
int pg_set_stream(pg_handle* h, void* s) {
    if (!h) return PG_ERR_INVALID;
    // pg_set_inputs / pg_step leave asynchronous copies from (and into) the ONE pinned staging buffer queued on the old stream: they must have landed before kernels on
    // the new stream read the inputs or the next call overwrites the buffer
    if ((hipStream_t)s != h->stream) { (void)hipSetDevice(h->cfg.device); HIPCHK(h, hipStreamSynchronize(h->stream)); }
    h->stream = (hipStream_t)s;
    return PG_OK;
}
int pg_set_pipeline(pg_handle* h, int32_t mode) { if (!h || mode < 0 || mode > 1) return PG_ERR_INVALID; h->pipeline = mode; return PG_OK; }
int pg_set_fusion(pg_handle* h, int32_t mode) { if (!h || mode < 0 || mode > 2) return PG_ERR_INVALID; h->fuse = mode; return PG_OK; }
// ---- build-defined options by name (include/pigeon_mpc.h lists them).  One table serves pg_set_option and pg_get_option. ----
namespace {
struct OptRef { int* i; real* r; int64_t* stat; double lo, hi; bool integer; };
static bool find_option(pg_handle* h, const char* name, OptRef* o) {
    DevCfg& C = h->dc;
    *o = OptRef{nullptr, nullptr, nullptr, 0.0, 0.0, true};
    auto I = [&](int* p, double lo, double hi) { o->i = p; o->lo = lo; o->hi = hi; o->integer = true; return true; };
    auto R = [&](real* p, double lo, double hi) { o->r = p; o->lo = lo; o->hi = hi; o->integer = false; return true; };
    auto S = [&](int64_t* p) { o->stat = p; return true; };
    const std::string n(name);
    // k_solve (coupled QP)
    if (n == "clip_guess") return I(&C.clip_guess, 0, 1);
    if (n == "clip_stops") return I(&C.clip_stops, 0, 1);
    if (n == "ck_riccati") return I(&C.ck_riccati, 0, 1);
    if (n == "warm_trivial_cold") return I(&C.warm_trivial_cold, 0, 1);
    if (n == "hji_seed") return I(&C.hji_seed, 0, 4);
    if (n == "hji_rounds") return I(&C.hji_rounds, 0, 64);
    if (n == "solve_split") return I(&h->split_solve, 0, 1);
    // launch shape
    if (n == "pipe_min") return I(&h->pipe_min, 0, 1 << 30);
    if (n == "pipe_first") return I(&h->pipe_first, 0, 64);
    if (n == "pipe_pub_short") return I(&h->pipe_pub_short, 1, 64);
    if (n == "pipe_pub_long") return I(&h->pipe_pub_long, 1, 64);
    if (n == "pipe_max") return I(&h->pipe_max, 0, 256 * NODES_IPB);
    if (n == "lin_lanes") return I(&h->lin_lpi, 1, 2);
    if (n == "graph") return I(&h->graph_mode, 0, 1);
    if (n == "phase_timing") return I(&h->phase_timing, 0, 1);
    if (n == "hji_cell_dims") return I(&h->hji_cell_dims, 3, 7);
    if (n == "time_grid_naive") return I(&C.time_grid_naive, 0, 1);
    if (n == "tracking_summary") return I(&h->tracking, 0, 1);
    if (n == "speed_plan_lanes") return I(&h->speed_lanes, 0, 64);
    // k_solve_lat (lateral QP)
    if (n == "lateral_solver") return I(&h->lateral_solver, 0, 2);
    if (n == "lat_split") return I(&h->split_lat, 0, 1);
    if (n == "lat_handover") return I(&h->lat_handover, 0, 1);
    if (n == "nodes_serial") return I(&C.nodes_serial, 0, 1);
    if (n == "lat_aux_gate") return I(&C.lat_aux_gate, 0, 1);
    if (n == "lat_hand_target") return I(&h->lat_hand_target, 0, 1 << 30);
    if (n == "lat_hand_min") return I(&h->lat_hand_min, 1, 1 << 20);
    if (n == "lat_hand_cap") return I(&h->lat_hand_cap, 0, 1 << 20);
    if (n == "lat_hand_work") return I(&h->lat_hand_work, 0, 1 << 20);
    if (n == "lat_hand_w0") return I(&h->lat_hand_w0, 0, 1 << 10);
    if (n == "lat_hand_batch") return I(&h->lat_hand_batch, 1, 1 << 30);
    if (n == "lat_single_max") return I(&h->lat_single_max, 0, 1 << 30);
    if (n == "lat_pack_only") return I(&h->lat_pack_only, 0, 1);
    if (n == "lat_polish2") return I(&C.lat_polish2, 0, 1);
    if (n == "lat_pin") return I(&C.lat_pin, 0, 1);
    if (n == "lat_polish_rounds") return I(&C.lat_polish_rounds, 2, 64);
    if (n == "lat_settle") return I(&C.lat_settle, 0, 2);
    if (n == "lat_warm_rounds") return I(&C.lat_warm_rounds, 0, 64);
    if (n == "lat_wipm") return I(&C.lat_wipm, 0, 1);
    if (n == "lat_mu0_cost") return R(&C.lat_mu0_cost, 1e-300, 1e300);
    if (n == "lat_far_cost") return R(&C.lat_far_cost, 1e-300, 1e300);
    if (n == "lat_rho_scale") return R(&C.lat_rho_scale, 1e-300, 1e12);
    if (n == "lat_wmu") return R(&C.lat_wmu, 1e-300, 1e300);
    if (n == "lat_wtau") return R(&C.lat_wtau, 1e-300, 1e300);
    // read-only launch statistics of this handle
    if (n == "stat_pipelined_launches") return S(&h->stat_pipelined);
    if (n == "stat_sensor_steps") return S(&h->sensor.steps_stat);
    if (n == "stat_actuator_steps") return S(&h->actuator.steps_stat);
    if (n == "stat_disturbance_steps") return S(&h->disturbance.steps_stat);
    if (n == "stat_estimator_steps") return S(&h->estimator.steps_stat);
    if (n == "stat_human_steps") return S(&h->human.steps_stat);
    if (n == "stat_route_steps") return S(&h->route.steps_stat);
    if (n == "stat_split_solve_launches") return S(&h->stat_split);
    if (n == "stat_single_solve_launches") return S(&h->stat_single);
    if (n == "stat_lat_two_launch_solves") return S(&h->stat_lat_two);
    if (n == "stat_lat_handover_solves") return S(&h->stat_lat_hand);
    if (n == "stat_lat_one_per_wavefront_solves") return S(&h->stat_lat_single);
#ifdef PG_DIAG      // diagnostic build only (libpigeon_hip_diag.so): fault injection and traces have no place in the shipped libraries
    if (n == "diag_instance") return I(&C.dbg_instance, -1, 1 << 30);
    if (n == "diag_lat_poison") return I(&C.dbg_poison, 0, 1);
    if (n == "diag_lin_groups") return I(&h->lin_groups, 0, 8);
    if (n == "diag_timeline") return I(&h->debug_timeline, 0, 1);
#endif
    return false;
}
}  // namespace
int pg_set_option(pg_handle* h, const char* name, double value) {
    if (!h || !name) return PG_ERR_INVALID;
#ifdef PG_DIAG
    if (strcmp(name, "diag_pipe_fault") == 0) { h->pipe_fault = value != 0.0; return PG_OK; }
#endif
    if (strcmp(name, "lat_workspace") == 0 || strcmp(name, "lateral_solver") == 0) {      // these two decide buffers: applied through configure_lateral, with the stream drained
        REQUIRE(h, h->cfg.formulation == PG_DECOUPLED, "pg_set_option: an option of the decoupled formulation");
        const bool which_solver = strcmp(name, "lateral_solver") == 0;
        REQUIRE(h, value == 0.0 || value == 1.0 || (value == 2.0 && which_solver), "pg_set_option: value out of range");
        HIPCHK(h, hipSetDevice(h->cfg.device)); HIPCHK(h, hipStreamSynchronize(h->stream));
        // (validated BEFORE anything changes, and a configure_lateral that fails -- an allocation -- leaves the handle as it was: ADVICE r5)
        if (which_solver && value == 1.0 && lat_lds_doubles(h->dc.N) * sizeof(real) > 64 * 1024) { h->err = "horizon too long for k_solve_lat's LDS staging"; return PG_ERR_INVALID; }
        const int old_solver = h->lateral_solver; const bool old_forced = h->lat_mem_forced, old_lat = h->solve_lat;
        if (which_solver) h->lateral_solver = (int)value; else h->lat_mem_forced = value != 0.0;
        if (configure_lateral(h) != PG_OK) {
            const std::string why = h->err;
            h->lateral_solver = old_solver; h->lat_mem_forced = old_forced; (void)configure_lateral(h);
            h->err = why; return PG_ERR_HIP;
        }
        // the two solve kernels read different QP records (k_solve: the embedded block, k_solve_lat: the packed stage records) and the last update_QP! wrote what the OLD
        // choice needed: pg_solve refuses until pg_update_qp (or a whole-batch pg_set_qp) has run again
        if (h->solve_lat != old_lat) h->qp_stale = true;
        return PG_OK;
    }
    OptRef o;
    if (!find_option(h, name, &o)) { h->err = std::string("pg_set_option: unknown option '") + name + "'"; return PG_ERR_INVALID; }
    if (o.stat) { h->err = std::string("pg_set_option: '") + name + "' is read-only"; return PG_ERR_INVALID; }
    if (!(value >= o.lo && value <= o.hi) || (o.integer && value != (double)(long long)value)) { h->err = std::string("pg_set_option: value out of range for '") + name + "'"; return PG_ERR_INVALID; }
    if (strcmp(name, "hji_cell_dims") == 0 && !(value == 3 || value == 5 || value == 7)) { h->err = "pg_set_option: hji_cell_dims is 3, 5 or 7"; return PG_ERR_INVALID; }
    if (strcmp(name, "speed_plan_lanes") == 0 && !(value == 0 || value == 16 || value == 32 || value == 64)) { h->err = "pg_set_option: speed_plan_lanes is 0, 16, 32 or 64"; return PG_ERR_INVALID; }
    if (o.i) *o.i = (int)value; else *o.r = (real)value;
    return PG_OK;
}
int pg_get_option(pg_handle* h, const char* name, double* value) {
    if (!h || !name || !value) return PG_ERR_INVALID;
#ifdef PG_DIAG
    if (strcmp(name, "diag_pipe_fault") == 0) { *value = h->pipe_fault ? 1.0 : 0.0; return PG_OK; }
#endif
    if (strcmp(name, "lat_workspace") == 0) { *value = h->lat_mem ? 1.0 : 0.0; return PG_OK; }
    if (strcmp(name, "stat_whole_batch_solves") == 0) {      // counted ON THE DEVICE by the full k_solve whenever it takes the whole batch (SolveOut::mode): drains the stream
        HIPCHK(h, hipSetDevice(h->cfg.device)); HIPCHK(h, hipStreamSynchronize(h->stream));
        int v = 0; HIPCHK(h, hipMemcpy(&v, solve_ctl(h, CTL_WHOLE), sizeof(int), hipMemcpyDeviceToHost));
        *value = (double)v; return PG_OK;
    }
    if (strcmp(name, "lateral_solver_in_use") == 0) { *value = h->solve_lat ? 1.0 : (h->cfg.formulation == PG_DECOUPLED ? 2.0 : 0.0); return PG_OK; }
    OptRef o;
    if (!find_option(h, name, &o)) { h->err = std::string("pg_get_option: unknown option '") + name + "'"; return PG_ERR_INVALID; }
    *value = o.stat ? (double)*o.stat : (o.i ? (double)*o.i : (double)*o.r);
    return PG_OK;
}
int pg_get_pipeline_fallbacks(pg_handle* h, int64_t* count) {
    if (!h || !count) return PG_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));                 // (a multi-GPU process: the copy below must not depend on whichever device happens to be current)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int v = 0;
    HIPCHK(h, hipMemcpy(&v, pipe_fallbacks(h), sizeof(int), hipMemcpyDeviceToHost));
    // the device word is a 32-bit counter of waiting wavefronts that gave up: the host keeps the 64-bit total and folds the device word into it (a wrap of the 32-bit
    // word between two calls would need 2^31 fall-backs -- at one per 20 ms wait, more than a year of nothing but fall-backs)
    h->fallback_total += (int64_t)(uint32_t)((uint32_t)v - (uint32_t)h->fallback_seen);
    h->fallback_seen = v;
    *count = h->fallback_total;
    return PG_OK;
}
int pg_synchronize(pg_handle* h) { if (!h) return PG_ERR_INVALID; HIPCHK(h, hipStreamSynchronize(h->stream)); return PG_OK; }

// ---- what the nine libraries share (trajectories, control parameters, plants, sensors, actuators, disturbances, estimators, humans, routes): one index rule and one install / clear / get protocol ----
// Installs the selection of `B` instances into a library of `n_sets`.  The WHOLE [capacity] array is written, entries beyond B as 0: never an address outside the library,
// whatever an earlier, larger library left there
static int index_install(pg_handle* h, int n_sets, IndexArray& arr, int32_t B, const int32_t* index) {
    const std::string who(arr.setter);
    REQUIRE(h, n_sets >= 1, who + ": no " + arr.what + " library installed");
    REQUIRE(h, B >= 1 && B <= h->cfg.batch_capacity && index, who + ": need 1 <= B <= batch_capacity and an index array");
    for (int b = 0; b < B; b++) REQUIRE(h, index[b] >= 0 && index[b] < n_sets, who + ": index out of range of the installed library");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    { const int rc = ensure(h, arr.d, cap_of(h)); if (rc) return rc; }
    std::vector<int> full(cap_of(h), 0);
    for (int b = 0; b < B; b++) full[(size_t)b] = index[b];
    HIPCHK(h, hipMemcpy(arr.d, full.data(), full.size() * sizeof(int), hipMemcpyHostToDevice));
    arr.host.assign(index, index + B);
    return PG_OK;
}
// a library of several sets wants an index that covers the batch
static int index_covers(pg_handle* h, size_t n_sets, const IndexArray& arr) {
    if (n_sets <= 1 || arr.covered() >= h->B) return PG_OK;
    h->err = std::string("a ") + arr.what + " library is installed but " + arr.setter + " does not cover the batch";
    return PG_ERR_STATE;
}
}  // extern "C" (the set library's templates have C++ linkage)
// problem(set): why a set is refused, or nullptr; fill(record, set): the device record of a set.  The new records replace the old ones only once they are on the device
// (on_device = false: a library that needs none); installing a library drops the previous index
template <class Host, class Dev, class Problem, class Fill>
static int setlib_install(pg_handle* h, const char* who_, SetLib<Host, Dev>& L, int32_t n_sets, const Host* sets, Problem problem, Fill fill, bool on_device = true) {
    const std::string who(who_);
    REQUIRE(h, n_sets >= 1 && sets, who + ": need n_sets >= 1 and the sets");
    for (int k = 0; k < n_sets; k++) REQUIRE_NO(h, who + ": ", problem(sets[k]));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));                 // (a rollout still queued reads the library it was launched with)
    CallBufs D; Dev* d_new = nullptr;
    if (on_device) {
        std::vector<Dev> recs((size_t)n_sets);
        for (int k = 0; k < n_sets; k++) fill(recs[(size_t)k], sets[k]);
        HIPCHK(h, D.alloc(d_new, recs.size()));
        if (hipMemcpy(d_new, recs.data(), recs.size() * sizeof(Dev), hipMemcpyHostToDevice) != hipSuccess) { h->err = who + ": copy failed"; return PG_ERR_HIP; }
    }
    h->mem.adopt(L.d, D.give(d_new)); L.sets.assign(sets, sets + n_sets); L.idx.host.clear();
    return PG_OK;
}
template <class Host, class Dev>
static int setlib_clear(pg_handle* h, SetLib<Host, Dev>& L) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->mem.drop(L.d); L.sets.clear(); h->mem.drop(L.idx.d); L.idx.host.clear();
    return PG_OK;
}
// the sets and the index as installed: *n_sets always, up to max_sets sets, index[b] = -1 where no index covers instance b
template <class Host, class Dev>
static int setlib_get(pg_handle* h, const char* who, const SetLib<Host, Dev>& L, int32_t* n_sets, Host* out, int32_t max_sets, int32_t* index, int32_t B) {
    REQUIRE(h, (!out || max_sets >= 0) && (!index || (B >= 0 && B <= h->cfg.batch_capacity)), std::string(who) + ": need max_sets >= 0 and 0 <= B <= batch_capacity");
    const int n = (int)L.sets.size();
    if (n_sets) *n_sets = n;
    if (out) for (int k = 0; k < n && k < max_sets; k++) out[k] = L.sets[(size_t)k];
    if (index) for (int b = 0; b < B; b++) index[b] = b < L.idx.covered() ? L.idx.host[(size_t)b] : -1;
    return PG_OK;
}
template <class Host, class Dev> static int index_covers(pg_handle* h, const SetLib<Host, Dev>& L) { return index_covers(h, L.sets.size(), L.idx); }
// field_problem(set) names the field that is wrong; the refusal of the install names the set as well: "set k: field" (`why` keeps the text while setlib_install reads it)
template <class Host, class FieldProblem>
static auto numbered_problem(FieldProblem field_problem, const Host* sets, std::string& why) {
    return [field_problem, sets, &why](const Host& s) -> const char* {
        const char* f = field_problem(s);
        if (!f) return nullptr;
        why = "set " + std::to_string((int)(&s - sets)) + ": " + f;
        return why.c_str();
    };
}
// ---- what the rollout libraries keep beside their sets (pg_handle: one record per library) ----
// pg_set_*_history_dev: registers buf [steps][B][width] with the next rollout call (nullptr: drops the registration).  hint: what to record without the library
template <class Host, class Dev>
static int history_register(pg_handle* h, const char* who_, const SetLib<Host, Dev>& L, const char* hint, HistSlot& slot, pg_real_dev* buf, int32_t steps) {
    if (!buf) { slot.clear(); return PG_OK; }
    const std::string who(who_);
    REQUIRE(h, steps >= 1, who + ": steps >= 1 required");
    if (!L.on()) { h->err = who + ": no " + L.idx.what + " library installed " + hint; return PG_ERR_STATE; }
    slot = HistSlot{(real*)buf, steps};
    return PG_OK;
}
// pg_set_*_seed: the seed and the stream ids of the first B instances (nullptr: stream[b] = b for all)
static int seed_install(pg_handle* h, const char* who, SeedStreams& S, uint64_t seed, int32_t B, const uint64_t* stream) {
    REQUIRE(h, B >= 1 && B <= h->cfg.batch_capacity, std::string(who) + ": need 1 <= B <= batch_capacity");
    S.seed = seed;                                              // (a launch argument: a rollout already queued keeps the seed it was launched with)
    if (stream) S.host.assign(stream, stream + B); else S.host.clear();      // instances the array does not cover: stream[b] = b
    S.dirty = true;
    return PG_OK;
}
// The only two places that list what restarts.  The rollouts' clock restarted (clock_start; new inputs restart it too): every law starts from no previous step, and
// the safety summary, the node counts and the tracking summary with it.  New inputs (set_inputs) also void what the *_state getters read.  The sensor's law has no
// state, and the actuator's getter falls back to the command
static void restart_on_clock(pg_handle* h) {
    h->sum_fresh = true; h->node_fresh = true; h->track_fresh = true;
    h->actuator.fresh = true; h->disturbance.fresh = true; h->estimator.fresh = true; h->human.fresh = true; h->route.fresh = true;
}
static void restart_on_inputs(pg_handle* h) {
    restart_on_clock(h);
    h->sensor.valid = false; h->disturbance.valid = false; h->estimator.valid = false; h->human.valid = false;
}
// The scaffold of the four pg_*_response calls (the law of one library alone, on scratch memory of the call).  The shared preconditions in their order: inputs, a library,
// `refuse` (the entry point's own reason for PG_ERR_INVALID, or nullptr), an index that covers the batch.  Then the streams of a seeded library (S, or nullptr) and
// `scratch` reals; body(d, result) uploads, launches and names the n_out reals to download.  A failure is waited out before the scratch memory is freed
template <class Host, class Dev, class Body>
static int response_call(pg_handle* h, const char* who_, const SetLib<Host, Dev>& L, const char* refuse, SeedStreams* S, size_t scratch, double* out, size_t n_out, Body body) {
    const std::string who(who_);
    if (h->B <= 0) { h->err = who + ": no inputs installed (the batch size is the one of pg_set_inputs)"; return PG_ERR_STATE; }
    if (!L.on()) { h->err = who + ": no " + L.idx.what + " library installed"; return PG_ERR_STATE; }
    REQUIRE(h, !refuse, refuse);
    if (index_covers(h, L)) return PG_ERR_STATE;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = S ? S->sync(h) : PG_OK; if (rc) return rc;
    CallBufs D; real* d = nullptr;
    HIPCHK(h, D.alloc(d, scratch));
    const real* result = nullptr;
    rc = body(d, result);
    if (!rc) { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { h->err = who + ": " + hipGetErrorString(e); rc = PG_ERR_HIP; } }
    if (!rc) rc = down(h, out, result, n_out);
    else (void)hipStreamSynchronize(h->stream);
    return rc;
}
extern "C" {

// The ONE routine that replaces the handle's trajectory library (install_trajectories for pg_set_trajectory / pg_set_trajectories after their upload, finish_library for
// the six makers -- pg_plan_speeds, pg_make_paths, pg_fit_paths, pg_offset_paths, pg_clip_tubes, pg_refine_paths -- after their kernels).  The rule: h->d_traj [n_traj][10][Lmax] and h->d_traj_len [n_traj] are device memory the handle owns, and h->dc.traj / traj_len / n_traj / traj_stride
// describe exactly that pair.  The caller hands in a FINISHED library held by its CallBufs, with trajectory.t[end] of every trajectory in fp64; no call touches the
// handle's library before this point, so one that fails earlier leaves it whole.  In this order: wait for the stream (a launch still queued reads the old pair), free
// the old pair and take the new one (HandleBufs::adopt; the caller's pointers are nulled), fill the view, drop the index
static int replace_trajectories(pg_handle* h, CallBufs& D, real*& traj, int*& len, int n_traj, int Lmax, int L0, std::vector<double>&& t_ends) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->mem.adopt(h->d_traj, D.give(traj)); h->mem.adopt(h->d_traj_len, D.give(len));
    const size_t stride = (size_t)10 * Lmax;
    h->traj_t_end = t_ends[0];                           // trajectory.t[end] of trajectory 0 (channel 0 = t): the stop of pg_simulate_dev's clock range
    h->traj_ends = std::move(t_ends); h->tend_dirty = true;      // ... and of every trajectory, fp64 (the window gate of the node callback)
    TrajView& T = h->dc.traj; T.L = L0;
    const real* p = h->d_traj; const size_t c = (size_t)Lmax;
    T.t = p; T.s = p + c; T.V = p + 2 * c; T.A = p + 3 * c; T.E = p + 4 * c; T.N = p + 5 * c; T.psi = p + 6 * c; T.kappa = p + 7 * c; T.edge_L = p + 8 * c; T.edge_R = p + 9 * c;
    h->dc.n_traj = n_traj; h->dc.traj_stride = (long)stride; h->dc.traj_len = h->d_traj_len;
    h->traj_L = L0;
    h->traj_idx.host.clear(); h->dc.traj_idx = nullptr;
    return PG_OK;
}
// install a trajectory library: channels[n_traj][10][Lmax] (t, s, V, A, E, N, psi, kappa, edge_L, edge_R), L[k] valid nodes of trajectory k.  Built in fresh buffers
// beside the installed library, which stays whole and in place until both uploads have succeeded
static int install_trajectories(pg_handle* h, int n_traj, int Lmax, const int32_t* L, const double* channels) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t stride = (size_t)10 * Lmax;
    CallBufs D; real* traj = nullptr; int* len = nullptr;
    HIPCHK(h, D.alloc(traj, (size_t)n_traj * stride));
    { int rc = up(h, traj, channels, (size_t)n_traj * stride); if (rc) return rc; }
    HIPCHK(h, D.alloc(len, (size_t)n_traj));
    HIPCHK(h, to_device(len, L, (size_t)n_traj));
    std::vector<double> ends((size_t)n_traj);
    for (int k = 0; k < n_traj; k++) ends[(size_t)k] = channels[(size_t)k * stride + (size_t)L[k] - 1];
    return replace_trajectories(h, D, traj, len, n_traj, Lmax, L[0], std::move(ends));
}

// ---- what the six makers of a trajectory library share on the host (pg_plan_speeds, pg_make_paths, pg_fit_paths, pg_offset_paths, pg_clip_tubes, pg_refine_paths below) ----
// One path of a source library (the four pair makers): L valid knots of Lmax, c = its channels [10][Lmax].  What is wrong with it (nullptr: nothing), tested in this
// order.  t, V and A are not geometry: each maker says after this what it needs of them
static const char* source_path_problem(int L, int Lmax, bool closed, const double* c) {
    if (!(L >= 2 && L <= Lmax)) return "every path needs 2 <= L[k] <= Lmax";
    if (closed && L < 3) return "a closed path needs >= 3 knots";
    for (int ch = 0; ch < 10; ch++) {
        if (ch == CH_T || ch == CH_V || ch == CH_A) continue;
        for (int i = 0; i < L; i++) if (!std::isfinite(c[(size_t)ch * Lmax + i])) return "a geometry value of a valid knot is not finite";
    }
    const double* s = c + (size_t)CH_S * Lmax;
    for (int i = 1; i < L; i++) if (!((real)s[i] > (real)s[i - 1])) return "s must increase strictly over the valid knots";      // (as the library's element type holds s)
    return nullptr;
}
// A pair is one (path, set) combination of a pair maker, numbered path * n_sets + set.  Its number has to fit an int, and the largest buffer of the call, n_path * n_sets *
// 10 * Lmax elements, has a size in bytes that has to fit the size arithmetic with room for the sums around it
static const char* pair_count_problem(int n_path, int n_sets, int Lmax) {
    if (!((double)n_path * (double)n_sets <= 2147483647.0)) return "n_path * n_sets must fit 31 bits";
    if (!((double)n_path * (double)n_sets * 10.0 * (double)Lmax * 8.0 < 4611686018427387904.0)) return "n_path * n_sets * 10 * Lmax elements are more than the allocation arithmetic holds";
    return nullptr;
}
// lens[pair] = L[path] of every pair, cls[path] = closed[path] (no array: every path is open)
static void pair_vectors(int n_path, int n_sets, const int32_t* L, const int32_t* closed, std::vector<int>& lens, std::vector<int>& cls) {
    lens.resize((size_t)n_path * n_sets); cls.resize((size_t)n_path);
    for (size_t k = 0; k < lens.size(); k++) lens[k] = L[k / (size_t)n_sets];
    for (int k = 0; k < n_path; k++) cls[(size_t)k] = closed ? closed[k] : 0;
}
// a turn reduced to (-pi, pi]: the IEEE remainder is exact
static double turn_in_pi(double turn) {
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    const double r = std::remainder(turn, two_pi);
    return r <= -pi ? r + two_pi : r;
}
// The end of every maker's call, after its one hipStreamSynchronize: the finished library d_out [lens.size()][10][Lmax] goes to the caller -- channels_out, L_out and
// closed_out, each where given; cls holds one flag per n_sets trajectories (a spec maker: n_sets = 1) -- and, with install, to the handle together with d_len.
// ends, read with install only: t of the last knot of every trajectory as stored, as a double (what pg_set_trajectories reads from channels_out)
static int finish_library(pg_handle* h, CallBufs& D, real*& d_out, int*& d_len, const std::vector<int>& lens, const std::vector<int>& cls, int n_sets, int Lmax,
                          int install, int32_t* L_out, int32_t* closed_out, double* channels_out, std::vector<double>&& ends) {
    const size_t n_traj = lens.size();
    { int rc = down(h, channels_out, d_out, n_traj * 10 * (size_t)Lmax); if (rc) return rc; }
    for (size_t k = 0; k < n_traj; k++) {
        if (L_out) L_out[k] = lens[k];
        if (closed_out) closed_out[k] = cls[k / (size_t)n_sets];
    }
    if (!install) return PG_OK;
    return replace_trajectories(h, D, d_out, d_len, (int)n_traj, Lmax, lens[0], std::move(ends));
}

int pg_set_trajectory(pg_handle* h, int32_t L, const double* t, const double* s, const double* V, const double* A, const double* E, const double* N,
                      const double* psi, const double* kappa, const double* theta, const double* phi, const double* edge_L, const double* edge_R) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, L >= 2 && t && s && V && A && E && N && psi && kappa, "pg_set_trajectory: need L >= 2 and the eight read channels");
    (void)theta; (void)phi;                                   // carried by TrajectoryTube (trajectories.jl:17-18) but read by nothing on this path
    std::vector<double> pack((size_t)10 * L);
    const double* src[8] = {t, s, V, A, E, N, psi, kappa};
    for (int k = 0; k < 8; k++) memcpy(pack.data() + (size_t)k * L, src[k], (size_t)L * 8);
    for (int i = 0; i < L; i++) { pack[(size_t)8 * L + i] = edge_L ? edge_L[i] : 4.0; pack[(size_t)9 * L + i] = edge_R ? edge_R[i] : -4.0; }   // defaults: trajectories.jl:42
    const int32_t Ls = L;
    return install_trajectories(h, 1, L, &Ls, pack.data());
}

int pg_set_trajectories(pg_handle* h, int32_t n_traj, int32_t Lmax, const int32_t* L, const double* channels) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, n_traj >= 1 && Lmax >= 2 && L && channels, "pg_set_trajectories: need n_traj >= 1, Lmax >= 2, lengths and channels");
    for (int k = 0; k < n_traj; k++) REQUIRE(h, L[k] >= 2 && L[k] <= Lmax, "pg_set_trajectories: every trajectory needs 2 <= L[k] <= Lmax");
    return install_trajectories(h, n_traj, Lmax, L, channels);
}

int pg_set_trajectory_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    const int rc = index_install(h, h->d_traj ? h->dc.n_traj : 0, h->traj_idx, B, index); if (rc) return rc;
    h->dc.traj_idx = h->traj_idx.d;
    return PG_OK;
}

__global__ void k_reset(int B, const uint8_t* mask, int* solved, int* wfail) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (!mask || mask[b])) { solved[b] = 0; wfail[b] = 0; }
}

// ---- control-parameter library: control_params of one controller per instance (coupled_lat_long.jl:42-60, decoupled_lat_long.jl:32-50) ----
static const char* control_set_problem(const pg_handle* h, const pg_control_params& u) {
    const double f[15] = {u.V_min, u.V_max, u.k_V, u.k_s, u.deltadot_max, u.Q_ds, u.Q_dpsi, u.Q_e, u.W_beta, u.W_r, u.W_HJI, u.R_delta, u.R_ddelta, u.R_Fx, u.R_dFx};
    for (double v : f) if (!std::isfinite(v)) return "a set has a non-finite field";
    if (!(u.V_min < u.V_max)) return "a set needs V_min < V_max";
    if (!(u.deltadot_max > 0.0)) return "a set needs deltadot_max > 0";
    for (int i = 5; i < 15; i++) if (f[i] < 0.0) return "a set has a negative weight";
    if (!(u.R_ddelta > 0.0)) return "a set needs R_ddelta > 0 (the rate weights make the optimum unique)";
    if (h->cfg.formulation == PG_COUPLED && !(u.R_dFx > 0.0)) return "a set of a coupled handle needs R_dFx > 0 (the rate weights make the optimum unique)";
    if (u.N_HJI != h->cfg.control.N_HJI) return "N_HJI of a set differs from the handle's (it decides which rows exist: structure, not tuning)";
    return nullptr;
}
static bool same_control(const pg_control_params& a, const pg_control_params& b) {
    return a.V_min == b.V_min && a.V_max == b.V_max && a.k_V == b.k_V && a.k_s == b.k_s && a.deltadot_max == b.deltadot_max && a.Q_ds == b.Q_ds && a.Q_dpsi == b.Q_dpsi && a.Q_e == b.Q_e &&
           a.W_beta == b.W_beta && a.W_r == b.W_r && a.W_HJI == b.W_HJI && a.R_delta == b.R_delta && a.R_ddelta == b.R_ddelta && a.R_Fx == b.R_Fx && a.R_dFx == b.R_dFx && a.N_HJI == b.N_HJI;
}
// instances [0, n) now run under eff(b): those whose set changed start cold, as pg_reset leaves them (their warm start belonged to another QP); the others keep their state
// (eff(b): the one set `single`, or set index[b] of the installed library)
static int control_sets_changed(pg_handle* h, int n, const pg_control_params* single, const int32_t* index) {
    auto eff = [&](int b) -> const pg_control_params& { return index ? h->cp.sets[(size_t)index[b]] : *single; };
    std::vector<uint8_t> mask((size_t)n, 0); bool any = false;
    for (int b = 0; b < n; b++) if (!same_control(eff(b), h->cp_eff[(size_t)b])) { mask[(size_t)b] = 1; any = true; }
    h->dc.cp_epoch++;                                          // (the captured step compares DevCfg: re-captured)
    if (!any) return PG_OK;
    h->warm_B = 0; h->order_B = 0;
    HIPCHK(h, hipMemcpyAsync(h->d_mask, mask.data(), (size_t)n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_reset, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->d_mask, h->d_solved, h->d_wfail);
    LAUNCH_CHECK(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int b = 0; b < n; b++) if (mask[(size_t)b]) h->cp_eff[(size_t)b] = eff(b);      // (only now: a failed reset leaves the instances marked as running under their old set, and the next install resets them)
    return PG_OK;
}
int pg_set_control_param_sets(pg_handle* h, int32_t n_sets, const pg_control_params* sets) {
    if (!h) return PG_ERR_INVALID;
    // (device records for a library of several sets only: a library of one is the uniform set of the handle)
    const int rc = setlib_install(h, "pg_set_control_param_sets", h->cp, n_sets, sets, [h](const pg_control_params& u) { return control_set_problem(h, u); },
                                  [h](DevControlRec& r, const pg_control_params& u) { r = make_control_rec(h->cfg.formulation, u); }, n_sets > 1);
    if (rc) return rc;
    DevCfg& C = h->dc; C.n_cp = n_sets; C.cp_sets = h->cp.d; C.cp_idx = nullptr;
    if (n_sets > 1) { C.cp_epoch++; return PG_OK; }            // (which instance runs under which set is known once the index arrives)
    // a library of one: the set becomes the uniform set of the handle -- every kernel reads it as the launch argument
    { const DevControlRec r = make_control_rec(h->cfg.formulation, sets[0]); C.cp = r.cp; C.ux_dummy = r.ux_dummy; }
    return control_sets_changed(h, h->cfg.batch_capacity, &h->cp.sets[0], nullptr);
}
int pg_set_control_param_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    const int rc = index_install(h, h->dc.n_cp, h->cp.idx, B, index); if (rc) return rc;
    if (h->dc.n_cp > 1) h->dc.cp_idx = h->cp.idx.d;            // (a library of one needs no index: every entry is 0)
    return control_sets_changed(h, B, nullptr, index);
}
int pg_clear_control_param_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->cp); if (rc) return rc;
    DevCfg& C = h->dc; C.n_cp = 0; C.cp_sets = nullptr; C.cp_idx = nullptr;
    { const DevControlRec r = make_control_rec(h->cfg.formulation, h->cfg.control); C.cp = r.cp; C.ux_dummy = r.ux_dummy; }
    return control_sets_changed(h, h->cfg.batch_capacity, &h->cfg.control, nullptr);
}
int pg_get_control_param_sets(pg_handle* h, int32_t* n_sets, pg_control_params* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_control_param_sets", h->cp, n_sets, out, max_sets, index, B);
}

// ---- plant library: the vehicle the ego plant of a rollout step integrates, per instance (model_predictive_control.jl:94).  No part of any QP: nothing is reset ----
static const char* plant_set_problem(const pg_vehicle& v) {
    const double f[22] = {v.G, v.m, v.Izz, v.L, v.a, v.b, v.mu, v.Caf, v.Car, v.Fx_max, v.Px_max, v.delta_max,      // [0, 12): must be > 0
                          v.h, v.Cd0, v.Cd1, v.Cd2, v.fwd_frac, v.rwd_frac, v.fwb_frac, v.rwb_frac, v.Fx_min, v.kappa_max};
    for (double x : f) if (!std::isfinite(x)) return "a set has a non-finite field";
    for (int i = 0; i < 12; i++) if (!(f[i] > 0.0)) return "a set needs G, m, Izz, L, a, b, mu, Caf, Car, Fx_max, Px_max and delta_max > 0";
    if (!(v.Fx_min < 0.0)) return "a set needs Fx_min < 0";
    return nullptr;
}
int pg_set_plant_sets(pg_handle* h, int32_t n_sets, const pg_vehicle* sets) {
    if (!h) return PG_ERR_INVALID;
    return setlib_install(h, "pg_set_plant_sets", h->plants, n_sets, sets, plant_set_problem, fill_dev_vehicle);
}
int pg_set_plant_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->plants.sets.size(), h->plants.idx, B, index);
}
int pg_clear_plant_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    return setlib_clear(h, h->plants);
}
int pg_get_plant_sets(pg_handle* h, int32_t* n_sets, pg_vehicle* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_plant_sets", h->plants, n_sets, out, max_sets, index, B);
}

// ---- pg_plan_speeds: friction-limited speed profiles of a path library x a plan-set library (pg_speed_plan.hip).  Two launches (copy, plan); no loop on the host ----
pg_speed_plan pg_default_speed_plan(void) {
    pg_speed_plan p; p.mu_scale = 1.0; p.V_max = 30.0; p.V_floor = 1.0; p.V_start = NAN; p.V_end = NAN; p.ax_max = INFINITY; p.ax_min = -INFINITY; p.ay_max = INFINITY;
    return p;
}
static const char* speed_plan_problem(const pg_speed_plan& p) {
    if (!(std::isfinite(p.mu_scale) && p.mu_scale > 0.0)) return "a set needs a finite mu_scale > 0";
    if (!(std::isfinite(p.V_max) && p.V_max > 0.0)) return "a set needs a finite V_max > 0";
    if (!(p.V_floor > 0.0 && p.V_floor <= p.V_max)) return "a set needs 0 < V_floor <= V_max";
    for (double v : {p.V_start, p.V_end}) if (!std::isnan(v) && !(std::isfinite(v) && v >= 0.0)) return "V_start / V_end of a set are NaN (free) or finite and >= 0";
    if (!(p.ax_min <= 0.0 && p.ax_max >= 0.0)) return "a set needs ax_min <= 0 <= ax_max";
    if (!(p.ay_max > 0.0)) return "a set needs ay_max > 0";
    return nullptr;
}
// the constants of one (set, vehicle) as the kernel reads them: every product rounded on its own in the library's element type, as the scheme states it
static void fill_speed_set(SpeedSet& S, const pg_speed_plan& p, const pg_vehicle& v) {
#pragma clang fp contract(off)
    const real mu_scale = (real)p.mu_scale, mu = (real)v.mu, G = (real)v.G, V_max = (real)p.V_max, V_floor = (real)p.V_floor;
    const real mm = mu_scale * mu;
    S.a_lim = mm * G;
    const real ay_max = (real)p.ay_max;
    S.ay = ay_max < S.a_lim ? ay_max : S.a_lim;
    S.Wmax = V_max * V_max; S.Wfloor = V_floor * V_floor;
    auto end = [&](double x) -> real { if (std::isnan(x)) return (real)NAN; real e = (real)x; if (V_floor > e) e = V_floor; return e * e; };
    S.Wstart = end(p.V_start); S.Wend = end(p.V_end);
    S.ax_max = (real)p.ax_max; S.nax_min = -(real)p.ax_min;
    S.m = (real)v.m; S.Fx_max = (real)v.Fx_max; S.nFx_min = -(real)v.Fx_min; S.Px_max = (real)v.Px_max;
    S.Cd0 = (real)v.Cd0; S.Cd1 = (real)v.Cd1; S.Cd2 = (real)v.Cd2; S.pad = real(0.0);
}
// sets per wavefront of k_speed_plan: option "speed_plan_lanes" (64, 32, 16), or 0 = the fewest wavefronts that still give every CU one (the passes are latency-bound and
// a lane's stores are strided: fewer live lanes per wavefront cost nothing while CUs are idle, EXPERIMENTS 27).  The result does not depend on it: a lane owns its trajectory
static int speed_plan_spw(const pg_handle* h, int n_path, int n_sets) {
    if (h->speed_lanes) return h->speed_lanes;
    int spw = 64;
    while (spw > 16 && (long)n_path * ((n_sets + spw - 1) / spw) < 256) spw /= 2;
    return spw;
}
int pg_plan_speeds(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in, int32_t n_sets,
                   const pg_speed_plan* sets, const pg_vehicle* vehicles, int32_t install, double* channels_out, pg_speed_plan_stats* stats) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, L && channels_in && sets, "pg_plan_speeds: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && Lmax >= 2, "pg_plan_speeds: need n_path >= 1, n_sets >= 1 and Lmax >= 2");
    REQUIRE(h, (n_sets + 15) / 16 <= 65535, "pg_plan_speeds: at most 65535 x 16 sets");
    REQUIRE(h, (double)n_path * (double)n_sets <= 2147483647.0, "pg_plan_speeds: n_path * n_sets must fit 31 bits");
    const size_t stride = (size_t)10 * Lmax;
    std::vector<int> i0((size_t)n_path, -1);
    for (int k = 0; k < n_path; k++) {
        const bool cl = closed && closed[k] != 0;
        const double* c = channels_in + (size_t)k * stride;
        REQUIRE_NO(h, "pg_plan_speeds: ", source_path_problem(L[k], Lmax, cl, c));
        if (cl) {                                          // i0: the first knot of largest |kappa| among knots 0 .. L-2, as the library's element type holds them
            const double* kap = c + (size_t)CH_KAPPA * Lmax;
            int best = 0;
            for (int i = 1; i < L[k] - 1; i++) if (fabs((real)kap[i]) > fabs((real)kap[best])) best = i;
            i0[(size_t)k] = best;
        }
    }
    for (int j = 0; j < n_sets; j++) {
        REQUIRE_NO(h, "pg_plan_speeds: ", speed_plan_problem(sets[j]));
        if (vehicles) REQUIRE_NO(h, "pg_plan_speeds: the vehicle: ", plant_set_problem(vehicles[j]));
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t n_traj = (size_t)n_path * n_sets, total = n_traj * stride;
    std::vector<SpeedSet> recs((size_t)n_sets);
    for (int j = 0; j < n_sets; j++) fill_speed_set(recs[(size_t)j], sets[j], vehicles ? vehicles[j] : h->cfg.vehicle);
    std::vector<int> lens, cls;
    pair_vectors(n_path, n_sets, L, closed, lens, cls);
    CallBufs D; real *d_in = nullptr, *d_out = nullptr; int *d_L = nullptr, *d_i0 = nullptr, *d_len = nullptr; SpeedSet* d_sets = nullptr; pg_speed_plan_stats* d_stats = nullptr;
    HIPCHK(h, D.alloc(d_in, (size_t)n_path * stride));
    HIPCHK(h, D.alloc(d_out, total));
    HIPCHK(h, D.alloc(d_L, (size_t)n_path));
    HIPCHK(h, D.alloc(d_i0, (size_t)n_path));
    HIPCHK(h, D.alloc(d_len, n_traj));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_stats, n_traj));
    { int rc = up(h, d_in, channels_in, (size_t)n_path * stride); if (rc) return rc; }
    HIPCHK(h, to_device(d_L, L, (size_t)n_path));
    HIPCHK(h, to_device(d_i0, i0.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_len, lens.data(), n_traj));
    HIPCHK(h, to_device(d_sets, recs.data(), (size_t)n_sets));
    SpeedPlanArgs A; A.n_path = n_path; A.n_sets = n_sets; A.Lmax = Lmax; A.spw = speed_plan_spw(h, n_path, n_sets); A.L = d_L; A.i0 = d_i0; A.in = d_in; A.sets = d_sets; A.out = d_out; A.stats = d_stats;
    hipLaunchKernelGGL(k_speed_plan_copy, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, A, total);
    LAUNCH_CHECK(h);
    const dim3 grid((unsigned)n_path, (unsigned)((n_sets + A.spw - 1) / A.spw));
    hipLaunchKernelGGL(k_speed_plan, grid, dim3(64), 0, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_speed_plan_stats> st(n_traj);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_traj * sizeof(pg_speed_plan_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the host arrays have been consumed, the kernels have run)
    if (stats) memcpy(stats, st.data(), n_traj * sizeof(pg_speed_plan_stats));
    std::vector<double> ends(install ? n_traj : 0);
    for (size_t k = 0; k < ends.size(); k++) ends[k] = st[k].t_end;      // (the rounded t of the last knot, as a double)
    return finish_library(h, D, d_out, d_len, lens, cls, n_sets, Lmax, install, nullptr, nullptr, channels_out, std::move(ends));
}

// ---- pg_make_paths: a path library from line, arc and clothoid segments (pg_path_make.hip).  One launch, one workgroup per path; no loop on the host ----
static_assert(sizeof(pg_path_segment) == 64 && sizeof(pg_path_spec) == 48 && sizeof(pg_path_stats) == 48, "the sizes include/pigeon_mpc.h states");
pg_path_segment pg_default_path_segment(void) {
    pg_path_segment s; s.length = 1.0; s.kappa0 = 0.0; s.kappa1 = 0.0; s.edge_L0 = 4.0; s.edge_L1 = 4.0; s.edge_R0 = -4.0; s.edge_R1 = -4.0; s.reserved = 0.0;
    return s;
}
static const char* path_segment_problem(const pg_path_segment& g) {
    if (!(std::isfinite(g.length) && g.length > 0.0)) return "a segment needs a finite length > 0";
    for (double v : {g.kappa0, g.kappa1, g.edge_L0, g.edge_L1, g.edge_R0, g.edge_R1}) if (!std::isfinite(v)) return "a curvature or an edge of a segment is not finite";
    if (!(g.edge_L0 > g.edge_R0 && g.edge_L1 > g.edge_R1)) return "a segment needs edge_L > edge_R at both ends";
    if (g.reserved != 0.0) return "reserved of a segment must be 0";
    return nullptr;
}
// the segment bounds of one path as the scheme states them: b_0 = 0, b_{j+1} = b_j + length_j; psib_0 = psi0, psib_{j+1} = psib_j + 0.5 (kappa0_j + kappa1_j) length_j,
// every operation rounded once.  Returns total = b_{n_seg}
static double path_bounds(const pg_path_spec& p, const pg_path_segment* seg, PathSeg* out) {
#pragma clang fp contract(off)
    double b = 0.0, psib = p.psi0;
    for (int j = 0; j < p.n_seg; j++) {
        const pg_path_segment& g = seg[p.seg0 + j];
        PathSeg& o = out[j];
        o.b = b; o.psib = psib; o.length = g.length; o.kappa0 = g.kappa0; o.kappa1 = g.kappa1; o.eL0 = g.edge_L0; o.eL1 = g.edge_L1; o.eR0 = g.edge_R0; o.eR1 = g.edge_R1; o.pad = 0.0;
        const double ksum = g.kappa0 + g.kappa1;
        const double kmid = 0.5 * ksum;
        const double dpsi = kmid * g.length;
        b = b + g.length; psib = psib + dpsi;
    }
    return b;
}
// s_i = i (total / (n_knots - 1)), s_last = total, as the library's element type holds them: do they increase strictly?  Two neighbours are ds apart before the two
// roundings (to double, to real), each of which moves a value by at most half an ulp at `total`: with ds >= 4 eps total they cannot meet, and only denser knots are walked
static bool path_s_increases(double total, int n_knots) {
#pragma clang fp contract(off)
    const double ds = total / (double)(n_knots - 1);
    if (!(std::isfinite(total) && ds > 0.0)) return false;
    const double eps = sizeof(real) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
    if (ds >= 4.0 * eps * total) return true;
    real prev = (real)0.0;
    for (int i = 1; i < n_knots; i++) {
        const real s = (real)(i == n_knots - 1 ? total : (double)i * ds);
        if (!(s > prev)) return false;
        prev = s;
    }
    return true;
}
int pg_make_paths(pg_handle* h, int32_t n_path, const pg_path_spec* specs, int32_t n_seg_total, const pg_path_segment* segments, int32_t Lmax,
                  int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_path_stats* stats) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, specs && segments, "pg_make_paths: null argument");
    REQUIRE(h, n_path >= 1 && n_seg_total >= 1 && Lmax >= 2, "pg_make_paths: need n_path >= 1, n_seg_total >= 1 and Lmax >= 2");
    // (the largest buffer of the call holds n_path * 10 * Lmax doubles: its size in bytes has to fit the size arithmetic, with room for the sums around it)
    REQUIRE(h, (double)n_path * 10.0 * (double)Lmax * 8.0 < 4611686018427387904.0, "pg_make_paths: n_path * 10 * Lmax elements are more than the allocation arithmetic holds");
    size_t n_rows = 0;
    for (int k = 0; k < n_path; k++) {
        const pg_path_spec& p = specs[k];
        REQUIRE(h, p.n_knots >= 2 && p.n_knots <= Lmax, "pg_make_paths: every path needs 2 <= n_knots <= Lmax");
        REQUIRE(h, !p.closed || p.n_knots >= 3, "pg_make_paths: a closed path needs >= 3 knots");
        REQUIRE(h, p.n_seg >= 1 && p.seg0 >= 0 && p.seg0 < n_seg_total && p.n_seg <= n_seg_total - p.seg0, "pg_make_paths: the segments of a path must lie inside [0, n_seg_total)");
        REQUIRE(h, std::isfinite(p.E0) && std::isfinite(p.N0) && std::isfinite(p.psi0), "pg_make_paths: the pose of a path is not finite");
        REQUIRE(h, std::isfinite(p.V_ref) && p.V_ref > 0.0, "pg_make_paths: a path needs a finite V_ref > 0");
        for (int j = 0; j < p.n_seg; j++) REQUIRE_NO(h, "pg_make_paths: ", path_segment_problem(segments[p.seg0 + j]));
        n_rows += (size_t)p.n_seg;
    }
    std::vector<PathSeg> rows(n_rows);
    std::vector<PathSpec> recs((size_t)n_path);
    std::vector<int> lens((size_t)n_path);
    {
        size_t at = 0;
        for (int k = 0; k < n_path; k++) {
            const pg_path_spec& p = specs[k];
            REQUIRE(h, at + (size_t)p.n_seg <= 2147483647u, "pg_make_paths: the segments of all paths together must fit 31 bits");
            PathSpec& r = recs[(size_t)k];
            r.E0 = p.E0; r.N0 = p.N0; r.psi0 = p.psi0; r.V_ref = p.V_ref; r.seg0 = (int)at; r.n_seg = p.n_seg; r.n_knots = p.n_knots; r.pad = 0;
            r.total = path_bounds(p, segments, rows.data() + at);
            REQUIRE(h, path_s_increases(r.total, p.n_knots), "pg_make_paths: the knots are so dense that s does not increase strictly in the library's element type");
            lens[(size_t)k] = p.n_knots;
            at += (size_t)p.n_seg;
        }
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t stride = (size_t)10 * Lmax, total = (size_t)n_path * stride;
    CallBufs D; real* d_out = nullptr; int* d_len = nullptr; PathSpec* d_specs = nullptr; PathSeg* d_segs = nullptr; double* d_scratch = nullptr; pg_path_stats* d_stats = nullptr;
    HIPCHK(h, D.alloc(d_out, total));
    HIPCHK(h, D.alloc(d_len, (size_t)n_path));
    HIPCHK(h, D.alloc(d_specs, (size_t)n_path));
    HIPCHK(h, D.alloc(d_segs, n_rows));
    HIPCHK(h, D.alloc(d_scratch, (size_t)n_path * 2 * (size_t)Lmax));
    HIPCHK(h, D.alloc(d_stats, (size_t)n_path));
    HIPCHK(h, to_device(d_len, lens.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_specs, recs.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_segs, rows.data(), n_rows));
    PathMakeArgs A; A.Lmax = Lmax; A.specs = d_specs; A.segs = d_segs; A.out = d_out; A.scratch = d_scratch; A.stats = d_stats;
    hipLaunchKernelGGL(k_path_make, dim3((unsigned)n_path), dim3(PM_THREADS), 0, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_path_stats> st((size_t)n_path);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, (size_t)n_path * sizeof(pg_path_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    std::vector<int> cls((size_t)n_path); std::vector<double> ends(install ? (size_t)n_path : 0);
    for (size_t k = 0; k < cls.size(); k++) { st[k].closure_psi = turn_in_pi(st[k].turn); cls[k] = specs[k].closed; }
    for (size_t k = 0; k < ends.size(); k++) ends[k] = (double)(real)(recs[k].total / recs[k].V_ref);
    if (stats) memcpy(stats, st.data(), (size_t)n_path * sizeof(pg_path_stats));
    return finish_library(h, D, d_out, d_len, lens, cls, 1, Lmax, install, L_out, closed_out, channels_out, std::move(ends));
}

// ---- pg_fit_paths: a path library fitted to waypoints (pg_path_fit.hip).  One launch, one workgroup per path; no loop on the host ----
static_assert(sizeof(pg_waypoint) == 32 && sizeof(pg_fit_spec) == 24 && sizeof(pg_fit_stats) == 80, "the sizes include/pigeon_mpc.h states");
pg_waypoint pg_default_waypoint(void) {
    pg_waypoint w; w.E = 0.0; w.N = 0.0; w.edge_L = 4.0; w.edge_R = -4.0;
    return w;
}
// the waypoints of one path: what is wrong with them (nullptr: nothing); C = the sum of the chords as the scheme rounds each of them
static const char* fit_waypoints_problem(const pg_fit_spec& p, const pg_waypoint* wp, double& C) {
#pragma clang fp contract(off)
    const pg_waypoint* w = wp + p.wp0;
    for (int i = 0; i < p.n_wp; i++) {
        for (double v : {w[i].E, w[i].N, w[i].edge_L, w[i].edge_R}) if (!std::isfinite(v)) return "a field of a waypoint is not finite";
        if (!(w[i].edge_L > w[i].edge_R)) return "a waypoint needs edge_L > edge_R";
    }
    C = 0.0;
    const int n_span = p.closed ? p.n_wp : p.n_wp - 1;
    for (int j = 0; j < n_span; j++) {
        const pg_waypoint &a = w[j], &b = w[j + 1 == p.n_wp ? 0 : j + 1];
        const double dE = b.E - a.E, dN = b.N - a.N;
        const double ee = dE * dE, nn = dN * dN;
        const double h = sqrt(ee + nn);
        if (!(std::isfinite(h) && h > 0.0)) return "two neighbouring waypoints of a path lie at the same point (a chord must be finite and > 0)";
        C += h;
    }
    return nullptr;
}
int pg_fit_paths(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints, int32_t Lmax,
                 int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_fit_stats* stats) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, specs && waypoints, "pg_fit_paths: null argument");
    REQUIRE(h, n_path >= 1 && n_wp_total >= 1 && Lmax >= 2, "pg_fit_paths: need n_path >= 1, n_wp_total >= 1 and Lmax >= 2");
    REQUIRE(h, (double)n_path * 10.0 * (double)Lmax * 8.0 < 4611686018427387904.0, "pg_fit_paths: n_path * 10 * Lmax elements are more than the allocation arithmetic holds");
    const double eps = sizeof(real) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16, range = 1.2676506002282294e30;      // 2^100
    double span_doubles = 0.0;
    for (int k = 0; k < n_path; k++) {
        const pg_fit_spec& p = specs[k];
        REQUIRE(h, p.n_knots >= 2 && p.n_knots <= Lmax, "pg_fit_paths: every path needs 2 <= n_knots <= Lmax");
        REQUIRE(h, p.closed ? (p.n_wp >= 3 && p.n_knots >= 3) : p.n_wp >= 2, "pg_fit_paths: an open path needs >= 2 waypoints, a closed one >= 3 waypoints and >= 3 knots");
        REQUIRE(h, p.wp0 >= 0 && p.wp0 < n_wp_total && p.n_wp <= n_wp_total - p.wp0, "pg_fit_paths: the waypoints of a path must lie inside [0, n_wp_total)");
        REQUIRE(h, std::isfinite(p.V_ref) && p.V_ref > 0.0, "pg_fit_paths: a path needs a finite V_ref > 0");
        double C = 0.0;
        REQUIRE_NO(h, "pg_fit_paths: ", fit_waypoints_problem(p, waypoints, C));
        const double per = (double)(p.n_knots - 1);
        REQUIRE(h, per <= 1.0 / (4.0 * eps) && C / per >= 1.0 / range && C <= range,
                "pg_fit_paths: the knots are so dense that s cannot be shown to increase strictly in the library's element type");
        span_doubles += (double)PF_ARRAYS * ((double)p.n_wp + 1.0);
    }
    REQUIRE(h, span_doubles * 8.0 < 4611686018427387904.0, "pg_fit_paths: the spans of all paths together are more than the allocation arithmetic holds");
    std::vector<FitSpec> recs((size_t)n_path);
    std::vector<int> lens((size_t)n_path);
    size_t n_span_doubles = 0;
    for (int k = 0; k < n_path; k++) {
        const pg_fit_spec& p = specs[k];
        FitSpec& r = recs[(size_t)k];
        r.V_ref = p.V_ref; r.soff = (long long)n_span_doubles; r.wp0 = p.wp0; r.n_wp = p.n_wp; r.n_knots = p.n_knots; r.closed = p.closed ? 1 : 0;
        n_span_doubles += (size_t)PF_ARRAYS * ((size_t)p.n_wp + 1);
        lens[(size_t)k] = p.n_knots;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t stride = (size_t)10 * Lmax, total = (size_t)n_path * stride, n_knot_slots = (size_t)n_path * (size_t)Lmax;
    CallBufs D; real* d_out = nullptr; int* d_len = nullptr; FitSpec* d_specs = nullptr; pg_waypoint* d_wps = nullptr; double* d_span = nullptr; double* d_raw = nullptr;
    int* d_runk = nullptr; pg_fit_stats* d_stats = nullptr;
    HIPCHK(h, D.alloc(d_out, total));
    HIPCHK(h, D.alloc(d_len, (size_t)n_path));
    HIPCHK(h, D.alloc(d_specs, (size_t)n_path));
    HIPCHK(h, D.alloc(d_wps, (size_t)n_wp_total));
    HIPCHK(h, D.alloc(d_span, n_span_doubles));
    HIPCHK(h, D.alloc(d_raw, n_knot_slots));
    HIPCHK(h, D.alloc(d_runk, n_knot_slots));
    HIPCHK(h, D.alloc(d_stats, (size_t)n_path));
    HIPCHK(h, to_device(d_len, lens.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_specs, recs.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_wps, waypoints, (size_t)n_wp_total));      // (waypoints no path refers to travel with the rest and are read by no thread)
    PathFitArgs A; A.Lmax = Lmax; A.specs = d_specs; A.wps = d_wps; A.out = d_out; A.span = d_span; A.psi_raw = d_raw; A.runk = d_runk; A.stats = d_stats;
    hipLaunchKernelGGL(k_path_fit, dim3((unsigned)n_path), dim3(PF_THREADS), 0, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_fit_stats> st((size_t)n_path);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, (size_t)n_path * sizeof(pg_fit_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    std::vector<int> cls((size_t)n_path); std::vector<double> ends(install ? (size_t)n_path : 0);
    for (size_t k = 0; k < cls.size(); k++) { st[k].closure_psi = turn_in_pi(st[k].turn); cls[k] = specs[k].closed; }
    for (size_t k = 0; k < ends.size(); k++) ends[k] = (double)(real)(st[k].length / recs[k].V_ref);
    if (stats) memcpy(stats, st.data(), (size_t)n_path * sizeof(pg_fit_stats));
    return finish_library(h, D, d_out, d_len, lens, cls, 1, Lmax, install, L_out, closed_out, channels_out, std::move(ends));
}

// ---- pg_offset_paths: every (path, offset set) pair of a path library x a library of offset sets (pg_path_offset.hip).  One launch, one workgroup per pair ----
static_assert(sizeof(pg_offset_set) == 64 && sizeof(pg_offset_stats) == 64, "the sizes include/pigeon_mpc.h states");
pg_offset_set pg_default_offset_set(void) {
    pg_offset_set s; s.d0 = 0.0; s.d1 = 0.0; s.s_a = INFINITY; s.s_b = INFINITY; s.s_c = INFINITY; s.s_d = INFINITY; s.x_min = 0.1; s.edge_mode = 0; s.reserved = 0;
    return s;
}
static const char* offset_set_problem(const pg_offset_set& s) {
    if (!(std::isfinite(s.d0) && std::isfinite(s.d1))) return "d0 or d1 of a set is not finite";
    const bool rise = std::isfinite(s.s_a), fall = std::isfinite(s.s_c);
    if (!(rise || s.s_a == INFINITY) || !(fall || s.s_c == INFINITY)) return "s_a and s_c of a set are finite or +Inf";
    if (rise && !(std::isfinite(s.s_b) && s.s_b > s.s_a)) return "a rise of a set needs a finite s_b > s_a";
    if (fall && !(std::isfinite(s.s_d) && s.s_d > s.s_c)) return "a fall of a set needs a finite s_d > s_c";
    if (!rise && std::isnan(s.s_b)) return "s_b of a set is NaN";
    if (!fall && std::isnan(s.s_d)) return "s_d of a set is NaN";
    if (fall && !rise) return "a set has a fall without a rise";
    if (rise && fall && s.s_c < s.s_b) return "a set needs s_c >= s_b (the fall starts after the rise has ended)";
    if (!(s.x_min > 0.0 && s.x_min <= 1.0)) return "a set needs x_min in (0, 1]";
    if (s.edge_mode != 0 && s.edge_mode != 1) return "edge_mode of a set is 0 or 1";
    if (s.reserved != 0) return "reserved of a set must be 0";
    return nullptr;
}
int pg_offset_paths(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,
                    int32_t n_sets, const pg_offset_set* sets, int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_offset_stats* stats) {
#pragma clang fp contract(off)
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, L && channels_in && sets, "pg_offset_paths: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && Lmax >= 2, "pg_offset_paths: need n_path >= 1, n_sets >= 1 and Lmax >= 2");
    REQUIRE_NO(h, "pg_offset_paths: ", pair_count_problem(n_path, n_sets, Lmax));
    const size_t stride = (size_t)10 * Lmax;
    for (int k = 0; k < n_path; k++) {
        const double* c = channels_in + (size_t)k * stride;
        REQUIRE_NO(h, "pg_offset_paths: ", source_path_problem(L[k], Lmax, closed && closed[k] != 0, c));
        const double* V = c + (size_t)CH_V * Lmax;
        for (int i = 0; i < L[k]; i++) REQUIRE(h, std::isfinite(V[i]) && V[i] > 0.0, "pg_offset_paths: V of a valid knot is not finite and > 0");
        REQUIRE(h, std::isfinite(c[(size_t)CH_T * Lmax]), "pg_offset_paths: t of the first knot is not finite");
    }
    for (int j = 0; j < n_sets; j++) REQUIRE_NO(h, "pg_offset_paths: ", offset_set_problem(sets[j]));
    // the pairs: x = 1 - kappa_i d_i at every valid knot, in the kernel's own arithmetic (po_offset is one function for host and device); the ends of a closed path
    for (int k = 0; k < n_path; k++) {
        const double* c = channels_in + (size_t)k * stride;
        const double* s = c + (size_t)CH_S * Lmax; const double* kap = c + (size_t)CH_KAPPA * Lmax;
        const bool cl = closed && closed[k] != 0;
        for (int j = 0; j < n_sets; j++) {
            const pg_offset_set& S = sets[j];
            if (cl) {
                const OffsetEval a = po_offset(S, 0.0), z = po_offset(S, s[L[k] - 1] - s[0]);
                if (!(a.d1 == 0.0 && a.d2 == 0.0 && z.d1 == 0.0 && z.d2 == 0.0 && a.d == z.d)) {
                    h->err = "pg_offset_paths: path " + std::to_string(k) + " is closed and its first or last knot lies inside a window of set " + std::to_string(j) +
                             ", or its two ends lie on different plateaus (the offset curve does not close)";
                    return PG_ERR_INVALID;
                }
            }
            if (S.d0 == 0.0 && S.d1 == 0.0) continue;         // (x = 1 at every knot)
            for (int i = 0; i < L[k]; i++) {
                const OffsetEval D = po_offset(S, s[i] - s[0]);
                const double kd = kap[i] * D.d;
                const double x = 1.0 - kd;
                if (!(x >= S.x_min)) {
                    h->err = "pg_offset_paths: path " + std::to_string(k) + ", set " + std::to_string(j) + ", knot " + std::to_string(i) + ": 1 - kappa d = " + std::to_string(x) +
                             " is below x_min (the offset reaches the centre of curvature)";
                    return PG_ERR_INVALID;
                }
            }
        }
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t n_traj = (size_t)n_path * n_sets, total = n_traj * stride, n_in = (size_t)n_path * stride;
    std::vector<int> lens, cls;
    pair_vectors(n_path, n_sets, L, closed, lens, cls);
    CallBufs D; double *d_in = nullptr, *d_sp = nullptr, *d_run = nullptr, *d_tend = nullptr; real* d_out = nullptr; int *d_L = nullptr, *d_cl = nullptr, *d_len = nullptr, *d_bad = nullptr;
    pg_offset_set* d_sets = nullptr; pg_offset_stats* d_stats = nullptr;
    HIPCHK(h, D.alloc(d_in, n_in));
    HIPCHK(h, D.alloc(d_out, total));
    HIPCHK(h, D.alloc(d_sp, n_traj * (size_t)Lmax));
    HIPCHK(h, D.alloc(d_run, n_traj * (size_t)Lmax));
    HIPCHK(h, D.alloc(d_tend, n_traj));
    HIPCHK(h, D.alloc(d_L, (size_t)n_path));
    HIPCHK(h, D.alloc(d_cl, (size_t)n_path));
    HIPCHK(h, D.alloc(d_len, n_traj));
    HIPCHK(h, D.alloc(d_bad, n_traj));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_stats, n_traj));
    HIPCHK(h, to_device(d_in, channels_in, n_in));            // (the source travels as the doubles given)
    HIPCHK(h, to_device(d_L, L, (size_t)n_path));
    HIPCHK(h, to_device(d_cl, cls.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_len, lens.data(), n_traj));
    HIPCHK(h, to_device(d_sets, sets, (size_t)n_sets));
    PathOffsetArgs A; A.n_sets = n_sets; A.Lmax = Lmax; A.L = d_L; A.closed = d_cl; A.in = d_in; A.sets = d_sets; A.out = d_out; A.sp = d_sp; A.run = d_run; A.t_end = d_tend; A.stats = d_stats; A.bad = d_bad;
    hipLaunchKernelGGL(k_path_offset, dim3((unsigned)n_traj), dim3(PO_THREADS), 0, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_offset_stats> st(n_traj);
    std::vector<int> bad(n_traj);
    std::vector<double> ends(n_traj);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_traj * sizeof(pg_offset_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ends.data(), d_tend, n_traj * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad.data(), d_bad, n_traj * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    for (size_t k = 0; k < n_traj; k++) if (bad[k]) {
        h->err = "pg_offset_paths: path " + std::to_string(k / (size_t)n_sets) + ", set " + std::to_string(k % (size_t)n_sets) +
                 ": the offset knots are so dense that s does not increase strictly in the library's element type (ds_min " + std::to_string(st[k].ds_min) + ")";
        return PG_ERR_INVALID;
    }
    if (stats) memcpy(stats, st.data(), n_traj * sizeof(pg_offset_stats));
    return finish_library(h, D, d_out, d_len, lens, cls, n_sets, Lmax, install, L_out, closed_out, channels_out, std::move(ends));
}

// ---- pg_clip_tubes: every (path, obstacle set) pair of a path library x a library of obstacle sets (pg_tube_clip.hip).  One launch, one workgroup per pair ----
static_assert(sizeof(pg_obstacle) == 32 && sizeof(pg_obstacle_set) == 64 && sizeof(pg_clip_stats) == 64 && sizeof(pg_obstacle_report) == 64, "the sizes include/pigeon_mpc.h states");
pg_obstacle_set pg_default_obstacle_set(void) {
    pg_obstacle_set s; s.first = 0; s.count = 0; s.margin = 0.0; s.taper = INFINITY; s.min_width = 0.0; s.policy = PG_PASS_CENTRE; s.reserved = 0; s.pad[0] = 0.0; s.pad[1] = 0.0; s.pad[2] = 0.0;
    return s;
}
static const char* obstacle_set_problem(const pg_obstacle_set& s, int n_obs, const pg_obstacle* obs) {
    if (!(s.count >= 0 && s.count <= 64)) return "count of a set is outside [0, 64]";
    if (!(s.first >= 0 && (long long)s.first + s.count <= (long long)n_obs)) return "first .. first + count of a set lies outside the obstacle array";
    if (s.count > 0 && !obs) return "a set has obstacles and the obstacle array is null";
    if (!(std::isfinite(s.margin) && s.margin >= 0.0)) return "margin of a set is not finite and >= 0";
    if (!(s.taper > 0.0)) return "taper of a set is not > 0 (+Inf: no taper)";
    if (!(std::isfinite(s.min_width) && s.min_width >= 0.0)) return "min_width of a set is not finite and >= 0";
    if (s.policy < 0 || s.policy > 3) return "policy of a set is outside 0 .. 3";
    if (s.reserved != 0 || s.pad[0] != 0.0 || s.pad[1] != 0.0 || s.pad[2] != 0.0) return "reserved and pad of a set must be 0";
    for (int j = 0; j < s.count; j++) {
        const pg_obstacle& o = obs[s.first + j];
        if (!(std::isfinite(o.E) && std::isfinite(o.N) && std::isfinite(o.radius))) return "E, N or radius of an obstacle is not finite";
        if (!(o.radius >= 0.0)) return "radius of an obstacle is < 0";
        if (o.reserved != 0.0) return "reserved of an obstacle must be 0";
        const double R = o.radius + s.margin;
        if (!(R > 0.0)) return "radius + margin of an obstacle is not > 0";
    }
    return nullptr;
}
int pg_clip_tubes(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,
                  int32_t n_sets, const pg_obstacle_set* sets, int32_t n_obs, const pg_obstacle* obstacles, int32_t install,
                  int32_t* L_out, int32_t* closed_out, double* channels_out, pg_clip_stats* stats, pg_obstacle_report* report) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, L && channels_in && sets, "pg_clip_tubes: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && Lmax >= 2, "pg_clip_tubes: need n_path >= 1, n_sets >= 1 and Lmax >= 2");
    REQUIRE(h, n_obs >= 0, "pg_clip_tubes: n_obs < 0");
    REQUIRE_NO(h, "pg_clip_tubes: ", pair_count_problem(n_path, n_sets, Lmax));
    const size_t stride = (size_t)10 * Lmax;
    for (int k = 0; k < n_path; k++) REQUIRE_NO(h, "pg_clip_tubes: ", source_path_problem(L[k], Lmax, closed && closed[k] != 0, channels_in + (size_t)k * stride));
    int max_count = 0;
    for (int j = 0; j < n_sets; j++) {
        REQUIRE_NO(h, "pg_clip_tubes: ", obstacle_set_problem(sets[j], n_obs, obstacles));
        max_count = std::max(max_count, (int)sets[j].count);
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t n_traj = (size_t)n_path * n_sets, total = n_traj * stride, n_in = (size_t)n_path * stride, n_rep = n_traj * (size_t)max_count;
    std::vector<int> lens, cls;
    pair_vectors(n_path, n_sets, L, closed, lens, cls);
    CallBufs D; double *d_in = nullptr, *d_scr = nullptr, *d_tend = nullptr; real* d_out = nullptr; int *d_L = nullptr, *d_cl = nullptr, *d_len = nullptr;
    pg_obstacle_set* d_sets = nullptr; pg_obstacle* d_obs = nullptr; pg_clip_stats* d_stats = nullptr; pg_obstacle_report* d_rep = nullptr;
    HIPCHK(h, D.alloc(d_in, n_in));
    HIPCHK(h, D.alloc(d_out, total));
    HIPCHK(h, D.alloc(d_scr, 6 * n_traj * (size_t)Lmax));
    HIPCHK(h, D.alloc(d_tend, n_traj));
    HIPCHK(h, D.alloc(d_L, (size_t)n_path));
    HIPCHK(h, D.alloc(d_cl, (size_t)n_path));
    HIPCHK(h, D.alloc(d_len, n_traj));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_obs, (size_t)std::max(n_obs, 1)));
    HIPCHK(h, D.alloc(d_stats, n_traj));
    HIPCHK(h, D.alloc(d_rep, std::max(n_rep, (size_t)1)));
    HIPCHK(h, to_device(d_in, channels_in, n_in));            // (the source travels as the doubles given)
    HIPCHK(h, to_device(d_L, L, (size_t)n_path));
    HIPCHK(h, to_device(d_cl, cls.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_len, lens.data(), n_traj));
    HIPCHK(h, to_device(d_sets, sets, (size_t)n_sets));
    if (n_obs > 0 && obstacles) HIPCHK(h, to_device(d_obs, obstacles, (size_t)n_obs));
    TubeClipArgs A; A.n_sets = n_sets; A.Lmax = Lmax; A.max_count = max_count; A.L = d_L; A.closed = d_cl; A.in = d_in; A.sets = d_sets; A.obs = d_obs; A.out = d_out; A.scratch = d_scr;
    A.t_end = d_tend; A.stats = d_stats; A.report = d_rep;
    hipLaunchKernelGGL(k_tube_clip, dim3((unsigned)n_traj), dim3(TC_THREADS), 0, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_clip_stats> st(n_traj);
    std::vector<pg_obstacle_report> rp(n_rep);
    std::vector<double> ends(n_traj);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_traj * sizeof(pg_clip_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ends.data(), d_tend, n_traj * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (report && n_rep > 0) HIPCHK(h, hipMemcpyAsync(rp.data(), d_rep, n_rep * sizeof(pg_obstacle_report), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    if (stats) memcpy(stats, st.data(), n_traj * sizeof(pg_clip_stats));
    if (report && n_rep > 0) memcpy(report, rp.data(), n_rep * sizeof(pg_obstacle_report));
    return finish_library(h, D, d_out, d_len, lens, cls, n_sets, Lmax, install, L_out, closed_out, channels_out, std::move(ends));
}

// ---- pg_refine_paths: every (path, refine set) pair of a path library x a library of refine sets (pg_path_refine.hip).  One launch, one workgroup per pair; the one pair
// maker whose output has its own knot counts and its own Lmax_out ----
static_assert(sizeof(pg_refine_set) == 128 && sizeof(pg_refine_stats) == 64, "the sizes include/pigeon_mpc.h states");
pg_refine_set pg_default_refine_set(void) {
    pg_refine_set s; s.ds = INFINITY;
    for (int j = 0; j < 4; j++) { s.s_lo[j] = INFINITY; s.s_hi[j] = INFINITY; s.ds_w[j] = INFINITY; }
    s.reserved[0] = 0.0; s.reserved[1] = 0.0; s.reserved[2] = 0.0;
    return s;
}
static const char* refine_set_problem(const pg_refine_set& s) {
    if (!(s.ds == INFINITY || (std::isfinite(s.ds) && s.ds > 0.0))) return "ds of a set is +Inf or finite and > 0";
    for (int j = 0; j < 4; j++) {
        const bool used = std::isfinite(s.s_lo[j]);
        if (!(used || s.s_lo[j] == INFINITY)) return "s_lo of a window is finite or +Inf";
        if (used && !(std::isfinite(s.s_hi[j]) && s.s_hi[j] > s.s_lo[j])) return "a window of a set needs a finite s_hi > s_lo";
        if (used && !(std::isfinite(s.ds_w[j]) && s.ds_w[j] > 0.0)) return "a window of a set needs a finite ds_w > 0";
        if (!used && (std::isnan(s.s_hi[j]) || std::isnan(s.ds_w[j]))) return "s_hi or ds_w of an unused window is NaN";
    }
    if (s.reserved[0] != 0.0 || s.reserved[1] != 0.0 || s.reserved[2] != 0.0) return "reserved of a set must be 0";
    return nullptr;
}
int pg_refine_paths(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,
                    int32_t n_sets, const pg_refine_set* sets, int32_t Lmax_out, int32_t install,
                    int32_t* L_out, int32_t* closed_out, double* channels_out, pg_refine_stats* stats) {
#pragma clang fp contract(off)
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, L && channels_in && sets, "pg_refine_paths: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && Lmax >= 2, "pg_refine_paths: need n_path >= 1, n_sets >= 1 and Lmax >= 2");
    REQUIRE(h, Lmax_out >= 2, "pg_refine_paths: need Lmax_out >= 2");
    REQUIRE_NO(h, "pg_refine_paths: ", pair_count_problem(n_path, n_sets, std::max(Lmax, Lmax_out)));
    const size_t stride = (size_t)10 * Lmax, stride_out = (size_t)10 * Lmax_out;
    for (int k = 0; k < n_path; k++) {
        const double* c = channels_in + (size_t)k * stride;
        REQUIRE_NO(h, "pg_refine_paths: ", source_path_problem(L[k], Lmax, closed && closed[k] != 0, c));
        const double* V = c + (size_t)CH_V * Lmax; const double* t = c + (size_t)CH_T * Lmax;
        for (int i = 0; i < L[k]; i++) REQUIRE(h, std::isfinite(V[i]) && V[i] > 0.0, "pg_refine_paths: V of a valid knot is not finite and > 0");
        for (int i = 0; i < L[k]; i++) REQUIRE(h, std::isfinite(t[i]), "pg_refine_paths: t of a valid knot is not finite");
    }
    for (int j = 0; j < n_sets; j++) REQUIRE_NO(h, "pg_refine_paths: ", refine_set_problem(sets[j]));
    // the pairs: L_out = 1 + sum of m_i in the kernel's own arithmetic (rf_parts is one function for host and device)
    const size_t n_traj = (size_t)n_path * n_sets;
    std::vector<int> lens, cls;
    pair_vectors(n_path, n_sets, L, closed, lens, cls);
    for (int k = 0; k < n_path; k++) {
        const double* s = channels_in + (size_t)k * stride + (size_t)CH_S * Lmax;
        for (int j = 0; j < n_sets; j++) {
            long long count = 1;
            for (int i = 0; i + 1 < L[k]; i++) {
                const int m = rf_parts(sets[j], s[i + 1] - s[i], s[i] - s[0], s[i + 1] - s[0]);
                if (m > RF_M_MAX) {
                    h->err = "pg_refine_paths: path " + std::to_string(k) + ", set " + std::to_string(j) + ", interval " + std::to_string(i) + " would be cut into more than " +
                             std::to_string((int)RF_M_MAX) + " parts";
                    return PG_ERR_INVALID;
                }
                count += m;
            }
            if (count > (long long)Lmax_out) {
                h->err = "pg_refine_paths: path " + std::to_string(k) + ", set " + std::to_string(j) + " has " + std::to_string(count) + " knots, more than Lmax_out = " +
                         std::to_string(Lmax_out);
                return PG_ERR_INVALID;
            }
            lens[(size_t)k * n_sets + j] = (int)count;
        }
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t total = n_traj * stride_out, n_in = (size_t)n_path * stride;
    CallBufs D; double *d_in = nullptr, *d_clos = nullptr, *d_tend = nullptr; real* d_out = nullptr; int *d_L = nullptr, *d_len = nullptr, *d_off = nullptr, *d_bad = nullptr;
    pg_refine_set* d_sets = nullptr; pg_refine_stats* d_stats = nullptr;
    HIPCHK(h, D.alloc(d_in, n_in));
    HIPCHK(h, D.alloc(d_out, total));
    HIPCHK(h, D.alloc(d_off, n_traj * (size_t)Lmax));
    HIPCHK(h, D.alloc(d_clos, 2 * n_traj * (size_t)Lmax));
    HIPCHK(h, D.alloc(d_tend, n_traj));
    HIPCHK(h, D.alloc(d_L, (size_t)n_path));
    HIPCHK(h, D.alloc(d_len, n_traj));
    HIPCHK(h, D.alloc(d_bad, n_traj));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_stats, n_traj));
    HIPCHK(h, to_device(d_in, channels_in, n_in));            // (the source travels as the doubles given)
    HIPCHK(h, to_device(d_L, L, (size_t)n_path));
    HIPCHK(h, to_device(d_len, lens.data(), n_traj));
    HIPCHK(h, to_device(d_sets, sets, (size_t)n_sets));
    PathRefineArgs A; A.n_sets = n_sets; A.Lmax = Lmax; A.Lmax_out = Lmax_out; A.L = d_L; A.len = d_len; A.in = d_in; A.sets = d_sets; A.out = d_out; A.off = d_off; A.clos = d_clos;
    A.t_end = d_tend; A.stats = d_stats; A.bad = d_bad;
    hipLaunchKernelGGL(k_path_refine, dim3((unsigned)n_traj), dim3(RF_THREADS), 0, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_refine_stats> st(n_traj);
    std::vector<int> bad(n_traj);
    std::vector<double> ends(n_traj);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_traj * sizeof(pg_refine_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ends.data(), d_tend, n_traj * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad.data(), d_bad, n_traj * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    for (size_t k = 0; k < n_traj; k++) if (bad[k]) {
        h->err = "pg_refine_paths: path " + std::to_string(k / (size_t)n_sets) + ", set " + std::to_string(k % (size_t)n_sets) +
                 ": the refined knots are so dense that s does not increase strictly in the library's element type (ds_min " + std::to_string(st[k].ds_min) + ")";
        return PG_ERR_INVALID;
    }
    if (stats) memcpy(stats, st.data(), n_traj * sizeof(pg_refine_stats));
    return finish_library(h, D, d_out, d_len, lens, cls, n_sets, Lmax_out, install, L_out, closed_out, channels_out, std::move(ends));
}

// ---- pg_smooth_waypoints: every (path, smoothing set) pair of a waypoint library x a library of smoothing sets (pg_waypoint_smooth.hip).  One launch, one workgroup per
// pair; waypoints in, waypoints out: no trajectory library is made, so nothing is installed ----
static_assert(sizeof(pg_smooth_set) == 120 && sizeof(pg_smooth_stats) == 72, "the sizes include/pigeon_mpc.h states");
pg_smooth_set pg_default_smooth_set(void) {
    pg_smooth_set s; s.lambda = 0.0;
    for (int j = 0; j < 4; j++) { s.u_lo[j] = 0.0; s.u_hi[j] = 0.0; s.factor[j] = 1.0; }
    s.n_win = 0; s.pin_ends = 0; s.keep_walls = 0; s.reserved = 0;
    return s;
}
static const char* smooth_set_problem(const pg_smooth_set& s) {
    if (!(std::isfinite(s.lambda) && s.lambda >= 0.0)) return "lambda of a set is finite and >= 0";
    if (!(s.n_win >= 0 && s.n_win <= 4)) return "n_win of a set lies in [0, 4]";
    for (int j = 0; j < s.n_win; j++) {
        if (std::isnan(s.u_lo[j]) || std::isnan(s.u_hi[j]) || s.u_lo[j] > s.u_hi[j]) return "a window of a set needs u_lo <= u_hi";
        if (!(std::isfinite(s.factor[j]) && s.factor[j] >= 0.0)) return "factor of a window is finite and >= 0";
    }
    if (s.reserved != 0) return "reserved of a set must be 0";
    return nullptr;
}
// two writers of one output waypoint: the paths in the order of their first waypoint, neighbours compared (empty: none)
static std::string wp_overlap_problem(int n_path, const pg_fit_spec* specs) {
    std::vector<int> order((size_t)n_path);
    for (int k = 0; k < n_path; k++) order[(size_t)k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return specs[a].wp0 != specs[b].wp0 ? specs[a].wp0 < specs[b].wp0 : a < b; });
    for (int k = 0; k + 1 < n_path; k++) {
        const int a = order[(size_t)k], b = order[(size_t)k + 1];
        if (specs[a].wp0 + specs[a].n_wp > specs[b].wp0)
            return "the waypoint ranges of path " + std::to_string(std::min(a, b)) + " and path " + std::to_string(std::max(a, b)) + " overlap";
    }
    return std::string();
}
// what a pair's final solve can report after the launch, in the order of the kernel's bad [4]
static const char* const smooth_bad_text[4] = {"a pivot of the factorisation is not > 0", "the output is not finite", "edge_L <= edge_R after keep_walls",
                                               "this output waypoint and the next lie at the same point"};
int pg_smooth_waypoints(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,
                        int32_t n_sets, const pg_smooth_set* sets, pg_waypoint* waypoints_out, pg_smooth_stats* stats) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, specs && waypoints && sets, "pg_smooth_waypoints: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && n_wp_total >= 1, "pg_smooth_waypoints: need n_path >= 1, n_sets >= 1 and n_wp_total >= 1");
    REQUIRE_NO(h, "pg_smooth_waypoints: ", pair_count_problem(n_path, n_sets, 2));
    for (int k = 0; k < n_path; k++) {
        const pg_fit_spec& p = specs[k];
        REQUIRE(h, p.closed ? p.n_wp >= 5 : p.n_wp >= 2, "pg_smooth_waypoints: an open path needs >= 2 waypoints, a closed one >= 5");
        REQUIRE(h, p.wp0 >= 0 && p.wp0 < n_wp_total && p.n_wp <= n_wp_total - p.wp0, "pg_smooth_waypoints: the waypoints of a path must lie inside [0, n_wp_total)");
        double C = 0.0;
        REQUIRE_NO(h, "pg_smooth_waypoints: ", fit_waypoints_problem(p, waypoints, C));
    }
    {
        const std::string why = wp_overlap_problem(n_path, specs);
        if (!why.empty()) { h->err = "pg_smooth_waypoints: " + why; return PG_ERR_INVALID; }
    }
    for (int j = 0; j < n_sets; j++) REQUIRE_NO(h, "pg_smooth_waypoints: ", smooth_set_problem(sets[j]));
    std::vector<SmoothSpec> recs((size_t)n_path);
    size_t n_used = 0;
    int lds_rows = 1;                                         // the rows of the longest path, at most WS_LDS_ROWS: what the launch keeps of the recurrence in LDS
    for (int k = 0; k < n_path; k++) {
        lds_rows = std::max(lds_rows, std::min(specs[k].n_wp - 2, (int)WS_LDS_ROWS));
        SmoothSpec& r = recs[(size_t)k];
        r.soff = (long long)n_used; r.wp0 = specs[k].wp0; r.n_wp = specs[k].n_wp; r.closed = specs[k].closed ? 1 : 0; r.pad = 0;
        n_used += (size_t)specs[k].n_wp;                          // (<= n_wp_total: the ranges do not overlap)
    }
    REQUIRE(h, (double)n_sets * (double)n_wp_total * (double)WS_ARRAYS * 8.0 < 4611686018427387904.0,
            "pg_smooth_waypoints: the scratch of all pairs is more than the allocation arithmetic holds");
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t n_pair = (size_t)n_path * n_sets, n_all = (size_t)n_wp_total;
    CallBufs D; pg_waypoint *d_in = nullptr, *d_out = nullptr; SmoothSpec* d_specs = nullptr; pg_smooth_set* d_sets = nullptr; double* d_scr = nullptr;
    pg_smooth_stats* d_stats = nullptr; int* d_bad = nullptr;
    HIPCHK(h, D.alloc(d_in, n_all));
    HIPCHK(h, D.alloc(d_out, (size_t)n_sets * n_all));
    HIPCHK(h, D.alloc(d_specs, (size_t)n_path));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_scr, (size_t)n_sets * n_used * WS_ARRAYS));
    HIPCHK(h, D.alloc(d_stats, n_pair));
    HIPCHK(h, D.alloc(d_bad, 4 * n_pair));
    HIPCHK(h, to_device(d_in, waypoints, n_all));
    for (int j = 0; j < n_sets; j++)                          // (every block starts as the input, copied on the device: a pair writes its own path's waypoints alone)
        HIPCHK(h, hipMemcpyAsync(d_out + (size_t)j * n_all, d_in, n_all * sizeof(pg_waypoint), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, to_device(d_specs, recs.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_sets, sets, (size_t)n_sets));
    WpSmoothArgs A; A.n_sets = n_sets; A.n_wp_total = n_wp_total; A.lds_rows = lds_rows; A.n_used = (long long)n_used; A.specs = d_specs; A.sets = d_sets; A.in = d_in; A.out = d_out; A.scratch = d_scr;
    A.stats = d_stats; A.bad = d_bad;
    hipLaunchKernelGGL(k_wp_smooth, dim3((unsigned)n_pair), dim3(WS_THREADS), (size_t)7 * lds_rows * sizeof(double), h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_smooth_stats> st(n_pair);
    std::vector<int> bad(4 * n_pair);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_pair * sizeof(pg_smooth_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad.data(), d_bad, 4 * n_pair * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    for (size_t k = 0; k < n_pair; k++) for (int c = 0; c < 4; c++) if (bad[4 * k + c] >= 0) {
        h->err = "pg_smooth_waypoints: path " + std::to_string(k / (size_t)n_sets) + ", set " + std::to_string(k % (size_t)n_sets) + ", waypoint " + std::to_string(bad[4 * k + c]) +
                 ": " + smooth_bad_text[c];
        return PG_ERR_INVALID;
    }
    if (stats) memcpy(stats, st.data(), n_pair * sizeof(pg_smooth_stats));
    return down_raw(h, waypoints_out, d_out, (size_t)n_sets * n_all * sizeof(pg_waypoint));
}

// ---- pg_tune_smoothing: the smoothing weight of every (path, tune set) pair searched on the device and the pair smoothed under it (pg_waypoint_tune.hip).  One launch,
// one workgroup per pair; waypoints in, waypoints out: nothing is installed ----
static_assert(sizeof(pg_tune_set) == 152 && sizeof(pg_tune_stats) == 72, "the sizes include/pigeon_mpc.h states");
pg_tune_set pg_default_tune_set(void) {
    pg_tune_set s; s.base = pg_default_smooth_set(); s.target = 1e-3; s.lambda_lo = 1e-6; s.lambda_hi = 1e3; s.rounds = 3; s.reserved = 0;
    return s;
}
static const char* tune_set_problem(const pg_tune_set& s) {
    if (const char* why = smooth_set_problem(s.base)) return why;
    if (s.base.lambda != 0.0) return "base.lambda of a set must be 0 (the weight is what the call chooses)";
    if (!(std::isfinite(s.target) && s.target > 0.0)) return "target of a set is finite and > 0";
    if (!(std::isfinite(s.lambda_lo) && std::isfinite(s.lambda_hi) && 0.0 < s.lambda_lo && s.lambda_lo < s.lambda_hi)) return "the bounds of a set are finite with 0 < lambda_lo < lambda_hi";
    if (!(s.rounds >= 1 && s.rounds <= 8)) return "rounds of a set lies in [1, 8]";
    if (s.reserved != 0) return "reserved of a set must be 0";
    return nullptr;
}
int pg_tune_smoothing(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,
                      int32_t n_sets, const pg_tune_set* sets, pg_waypoint* waypoints_out, pg_smooth_stats* stats, pg_tune_stats* tune) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, specs && waypoints && sets, "pg_tune_smoothing: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && n_wp_total >= 1, "pg_tune_smoothing: need n_path >= 1, n_sets >= 1 and n_wp_total >= 1");
    REQUIRE_NO(h, "pg_tune_smoothing: ", pair_count_problem(n_path, n_sets, 2));
    for (int k = 0; k < n_path; k++) {
        const pg_fit_spec& p = specs[k];
        REQUIRE(h, p.closed ? p.n_wp >= 5 : p.n_wp >= 2, "pg_tune_smoothing: an open path needs >= 2 waypoints, a closed one >= 5");
        REQUIRE(h, p.wp0 >= 0 && p.wp0 < n_wp_total && p.n_wp <= n_wp_total - p.wp0, "pg_tune_smoothing: the waypoints of a path must lie inside [0, n_wp_total)");
        double C = 0.0;
        REQUIRE_NO(h, "pg_tune_smoothing: ", fit_waypoints_problem(p, waypoints, C));
    }
    {
        const std::string why = wp_overlap_problem(n_path, specs);
        if (!why.empty()) { h->err = "pg_tune_smoothing: " + why; return PG_ERR_INVALID; }
    }
    for (int j = 0; j < n_sets; j++) REQUIRE_NO(h, "pg_tune_smoothing: ", tune_set_problem(sets[j]));
    std::vector<SmoothSpec> recs((size_t)n_path);
    size_t n_used = 0;
    int rows_max = 1;                                         // the rows of the longest path
    for (int k = 0; k < n_path; k++) {
        rows_max = std::max(rows_max, specs[k].n_wp - 2);
        SmoothSpec& r = recs[(size_t)k];
        r.soff = (long long)n_used; r.wp0 = specs[k].wp0; r.n_wp = specs[k].n_wp; r.closed = specs[k].closed ? 1 : 0; r.pad = 0;
        n_used += (size_t)specs[k].n_wp;                          // (<= n_wp_total: the ranges do not overlap)
    }
    // the search keeps its state in LDS where a path has at most WT_LDS_ROWS rows, the final solve where it has at most WS_LDS_ROWS; the scratch holds the search's
    // state only where some path of the call is longer
    const int tune_rows = std::min(rows_max, (int)WT_LDS_ROWS), lds_rows = std::min(rows_max, (int)WS_LDS_ROWS);
    const int n_arr = rows_max <= (int)WT_LDS_ROWS ? (int)WT_ARRAYS_LDS : (int)WT_ARRAYS_SCRATCH;
    REQUIRE(h, (double)n_sets * (double)n_wp_total * (double)WT_ARRAYS_SCRATCH * 8.0 < 4611686018427387904.0,
            "pg_tune_smoothing: the scratch of all pairs is more than the allocation arithmetic holds");
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t n_pair = (size_t)n_path * n_sets, n_all = (size_t)n_wp_total;
    CallBufs D; pg_waypoint *d_in = nullptr, *d_out = nullptr; SmoothSpec* d_specs = nullptr; pg_tune_set* d_sets = nullptr; double* d_scr = nullptr;
    pg_smooth_stats* d_stats = nullptr; pg_tune_stats* d_tune = nullptr; int *d_bad = nullptr, *d_bad_tune = nullptr;
    HIPCHK(h, D.alloc(d_in, n_all));
    HIPCHK(h, D.alloc(d_out, (size_t)n_sets * n_all));
    HIPCHK(h, D.alloc(d_specs, (size_t)n_path));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_scr, (size_t)n_sets * n_used * (size_t)n_arr));
    HIPCHK(h, D.alloc(d_stats, n_pair));
    HIPCHK(h, D.alloc(d_tune, n_pair));
    HIPCHK(h, D.alloc(d_bad, 4 * n_pair));
    HIPCHK(h, D.alloc(d_bad_tune, 2 * n_pair));
    HIPCHK(h, to_device(d_in, waypoints, n_all));
    for (int j = 0; j < n_sets; j++)                          // (every block starts as the input, copied on the device: a pair writes its own path's waypoints alone)
        HIPCHK(h, hipMemcpyAsync(d_out + (size_t)j * n_all, d_in, n_all * sizeof(pg_waypoint), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, to_device(d_specs, recs.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_sets, sets, (size_t)n_sets));
    WpTuneArgs A; A.n_sets = n_sets; A.n_wp_total = n_wp_total; A.lds_rows = lds_rows; A.tune_rows = tune_rows; A.n_arr = n_arr; A.n_used = (long long)n_used; A.specs = d_specs;
    A.sets = d_sets; A.in = d_in; A.out = d_out; A.scratch = d_scr; A.stats = d_stats; A.tune = d_tune; A.bad = d_bad; A.bad_tune = d_bad_tune;
    const size_t lds = std::max((size_t)WT_STATE * WT_CAND * (size_t)tune_rows, (size_t)7 * (size_t)lds_rows) * sizeof(double);      // (at most 60928 bytes)
    hipLaunchKernelGGL(k_wp_tune, dim3((unsigned)n_pair), dim3(WS_THREADS), lds, h->stream, A);
    LAUNCH_CHECK(h);
    std::vector<pg_smooth_stats> st(n_pair);
    std::vector<pg_tune_stats> tn(n_pair);
    std::vector<int> bad(4 * n_pair), bad_tune(2 * n_pair);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_pair * sizeof(pg_smooth_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(tn.data(), d_tune, n_pair * sizeof(pg_tune_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad.data(), d_bad, 4 * n_pair * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad_tune.data(), d_bad_tune, 2 * n_pair * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    for (size_t k = 0; k < n_pair; k++) {
        const std::string who = "pg_tune_smoothing: path " + std::to_string(k / (size_t)n_sets) + ", set " + std::to_string(k % (size_t)n_sets);
        if (bad_tune[2 * k] >= 0) {
            h->err = who + ", round " + std::to_string(bad_tune[2 * k]) + ": " + (bad_tune[2 * k + 1] == 0 ? "a pivot of the factorisation is not > 0 at a candidate" : "dev_rms is not finite at a candidate");
            return PG_ERR_INVALID;
        }
        for (int c = 0; c < 4; c++) if (bad[4 * k + c] >= 0) {
            h->err = who + ", waypoint " + std::to_string(bad[4 * k + c]) + ": " + smooth_bad_text[c];
            return PG_ERR_INVALID;
        }
    }
    if (stats) memcpy(stats, st.data(), n_pair * sizeof(pg_smooth_stats));
    if (tune) memcpy(tune, tn.data(), n_pair * sizeof(pg_tune_stats));
    return down_raw(h, waypoints_out, d_out, (size_t)n_sets * n_all * sizeof(pg_waypoint));
}

// ---- pg_optimize_line: every (path, line set) pair of a waypoint library x a library of line sets moved along its normals to the least bending energy the walls allow
// (pg_line_opt.hip).  One launch, one workgroup per pair; waypoints in, waypoints out: nothing is installed ----
static_assert(sizeof(pg_line_set) == 176 && sizeof(pg_line_stats) == 96, "the sizes include/pigeon_mpc.h states");
pg_line_set pg_default_line_set(void) {
    pg_line_set s; s.mu = 1e-6; s.rho = 0.1; s.margin = 0.5; s.alpha_max = 2.0; s.tol = 0.0;
    for (int j = 0; j < 4; j++) { s.u_lo[j] = 0.0; s.u_hi[j] = 0.0; s.win_margin[j] = 0.0; s.win_pin[j] = 0; }
    s.iters = 1000; s.n_win = 0; s.pin_ends = 0; s.keep_walls = 0; s.reserved[0] = 0; s.reserved[1] = 0;
    return s;
}
static const char* line_set_problem(const pg_line_set& s) {
    if (!(std::isfinite(s.mu) && s.mu > 0.0)) return "mu of a set is finite and > 0";
    if (!(std::isfinite(s.rho) && s.rho > 0.0)) return "rho of a set is finite and > 0";
    if (!(std::isfinite(s.margin) && s.margin >= 0.0)) return "margin of a set is finite and >= 0";
    if (!(std::isfinite(s.alpha_max) && s.alpha_max > 0.0)) return "alpha_max of a set is finite and > 0";
    if (!(std::isfinite(s.tol) && s.tol >= 0.0)) return "tol of a set is finite and >= 0";
    if (!(s.iters >= 1 && s.iters <= 4096)) return "iters of a set lies in [1, 4096]";
    if (!(s.n_win >= 0 && s.n_win <= 4)) return "n_win of a set lies in [0, 4]";
    for (int j = 0; j < s.n_win; j++) {
        if (std::isnan(s.u_lo[j]) || std::isnan(s.u_hi[j]) || s.u_lo[j] > s.u_hi[j]) return "a window of a set needs u_lo <= u_hi";
        if (!(std::isfinite(s.win_margin[j]) && s.win_margin[j] >= 0.0)) return "the margin of a window is finite and >= 0";
    }
    if (s.reserved[0] != 0 || s.reserved[1] != 0) return "reserved of a set must be 0";
    return nullptr;
}
// what a pair can report after the launch, in the order of the kernel's bad [3]
static const char* const line_bad_text[3] = {"a pivot of the factorisation is not > 0", "the output is not finite", "this output waypoint and the next lie at the same point"};
int pg_optimize_line(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,
                     int32_t n_sets, const pg_line_set* sets, pg_waypoint* waypoints_out, pg_line_stats* stats) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, specs && waypoints && sets, "pg_optimize_line: null argument");
    REQUIRE(h, n_path >= 1 && n_sets >= 1 && n_wp_total >= 1, "pg_optimize_line: need n_path >= 1, n_sets >= 1 and n_wp_total >= 1");
    REQUIRE_NO(h, "pg_optimize_line: ", pair_count_problem(n_path, n_sets, 2));
    for (int k = 0; k < n_path; k++) {
        const pg_fit_spec& p = specs[k];
        REQUIRE(h, p.closed ? p.n_wp >= 5 : p.n_wp >= 2, "pg_optimize_line: an open path needs >= 2 waypoints, a closed one >= 5");
        REQUIRE(h, p.wp0 >= 0 && p.wp0 < n_wp_total && p.n_wp <= n_wp_total - p.wp0, "pg_optimize_line: the waypoints of a path must lie inside [0, n_wp_total)");
        double C = 0.0;
        REQUIRE_NO(h, "pg_optimize_line: ", fit_waypoints_problem(p, waypoints, C));
    }
    {
        const std::string why = wp_overlap_problem(n_path, specs);
        if (!why.empty()) { h->err = "pg_optimize_line: " + why; return PG_ERR_INVALID; }
    }
    for (int j = 0; j < n_sets; j++) REQUIRE_NO(h, "pg_optimize_line: ", line_set_problem(sets[j]));
    // the box of every pair in the kernel's own arithmetic (the chords, the blocked prefix U, lo_box: one text for host and device)
    for (int k = 0; k < n_path; k++) {
        const pg_fit_spec& p = specs[k];
        const pg_waypoint* w = waypoints + p.wp0;
        std::vector<double> hh((size_t)p.n_wp, 0.0), U((size_t)p.n_wp, 0.0);
        for (int j = 0; j + 1 < p.n_wp; j++) {
#pragma clang fp contract(off)
            const double dE = w[j + 1].E - w[j].E, dN = w[j + 1].N - w[j].N;
            const double ee = dE * dE, nn = dN * dN;
            hh[(size_t)j] = sqrt(ee + nn);
        }
        lo_prefix_host(p.n_wp - 1, hh.data(), U.data());
        for (int j = 0; j < n_sets; j++) for (int i = 0; i < p.n_wp; i++) {
            double lo, hi;
            lo_box(sets[j].margin, sets[j].alpha_max, sets[j].n_win, sets[j].u_lo, sets[j].u_hi, sets[j].win_margin, sets[j].win_pin, U[(size_t)i], w[i].edge_L, w[i].edge_R,
                   sets[j].pin_ends && !p.closed && (i == 0 || i == p.n_wp - 1), lo, hi);
            if (lo > hi) {
                h->err = "pg_optimize_line: path " + std::to_string(k) + ", set " + std::to_string(j) + ", waypoint " + std::to_string(i) +
                         ": the margins leave no room between the edges (lo > hi)";
                return PG_ERR_INVALID;
            }
        }
    }
    std::vector<SmoothSpec> recs((size_t)n_path);
    size_t n_used = 0;
    int lds_rows = 1;                                         // the rows of the longest path, at most LO_LDS_ROWS: what the launch keeps of the recurrence in LDS
    for (int k = 0; k < n_path; k++) {
        lds_rows = std::max(lds_rows, std::min(specs[k].closed ? specs[k].n_wp - 2 : specs[k].n_wp, (int)LO_LDS_ROWS));
        SmoothSpec& r = recs[(size_t)k];
        r.soff = (long long)n_used; r.wp0 = specs[k].wp0; r.n_wp = specs[k].n_wp; r.closed = specs[k].closed ? 1 : 0; r.pad = 0;
        n_used += (size_t)specs[k].n_wp;                          // (<= n_wp_total: the ranges do not overlap)
    }
    REQUIRE(h, (double)n_sets * (double)n_wp_total * (double)LO_ARRAYS * 8.0 < 4611686018427387904.0,
            "pg_optimize_line: the scratch of all pairs is more than the allocation arithmetic holds");
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t n_pair = (size_t)n_path * n_sets, n_all = (size_t)n_wp_total;
    CallBufs D; pg_waypoint *d_in = nullptr, *d_out = nullptr; SmoothSpec* d_specs = nullptr; pg_line_set* d_sets = nullptr; double* d_scr = nullptr;
    pg_line_stats* d_stats = nullptr; int* d_bad = nullptr;
    HIPCHK(h, D.alloc(d_in, n_all));
    HIPCHK(h, D.alloc(d_out, (size_t)n_sets * n_all));
    HIPCHK(h, D.alloc(d_specs, (size_t)n_path));
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(d_scr, (size_t)n_sets * n_used * LO_ARRAYS));
    HIPCHK(h, D.alloc(d_stats, n_pair));
    HIPCHK(h, D.alloc(d_bad, 3 * n_pair));
    HIPCHK(h, to_device(d_in, waypoints, n_all));
    for (int j = 0; j < n_sets; j++)                          // (every block starts as the input, copied on the device: a pair writes its own path's waypoints alone)
        HIPCHK(h, hipMemcpyAsync(d_out + (size_t)j * n_all, d_in, n_all * sizeof(pg_waypoint), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, to_device(d_specs, recs.data(), (size_t)n_path));
    HIPCHK(h, to_device(d_sets, sets, (size_t)n_sets));
    LineOptArgs A; A.n_sets = n_sets; A.n_wp_total = n_wp_total; A.lds_rows = lds_rows; A.n_used = (long long)n_used; A.specs = d_specs; A.sets = d_sets; A.in = d_in; A.out = d_out; A.scratch = d_scr;
    A.stats = d_stats; A.bad = d_bad;
    hipLaunchKernelGGL(k_line_opt, dim3((unsigned)n_pair), dim3(WS_THREADS), (size_t)6 * lds_rows * sizeof(double), h->stream, A);      // (at most 49152 bytes)
    LAUNCH_CHECK(h);
    std::vector<pg_line_stats> st(n_pair);
    std::vector<int> bad(3 * n_pair);
    HIPCHK(h, hipMemcpyAsync(st.data(), d_stats, n_pair * sizeof(pg_line_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad.data(), d_bad, 3 * n_pair * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the kernel has run)
    for (size_t k = 0; k < n_pair; k++) for (int c = 0; c < 3; c++) if (bad[3 * k + c] >= 0) {
        h->err = "pg_optimize_line: path " + std::to_string(k / (size_t)n_sets) + ", set " + std::to_string(k % (size_t)n_sets) + ", waypoint " + std::to_string(bad[3 * k + c]) +
                 ": " + line_bad_text[c];
        return PG_ERR_INVALID;
    }
    if (stats) memcpy(stats, st.data(), n_pair * sizeof(pg_line_stats));
    return down_raw(h, waypoints_out, d_out, (size_t)n_sets * n_all * sizeof(pg_waypoint));
}

// ---- sensor library: the state the CONTROLLER of a rollout step reads, measured = true + bias + sigma z per channel (k_measure).  No part of any QP's structure and no
// solver state: nothing is reset ----
static const char* sensor_set_problem(const pg_sensor& s) {
    for (int c = 0; c < 6; c++) {
        if (!std::isfinite(s.sigma[c]) || !std::isfinite(s.bias[c])) return "a set has a non-finite field";
        if (s.sigma[c] < 0.0) return "a set needs sigma >= 0";
    }
    return nullptr;
}
static void fill_dev_sensor(DevSensor& S, const pg_sensor& s) { for (int c = 0; c < 6; c++) { S.sigma[c] = (real)s.sigma[c]; S.bias[c] = (real)s.bias[c]; } }
int pg_set_sensor_sets(pg_handle* h, int32_t n_sets, const pg_sensor* sets) {
    if (!h) return PG_ERR_INVALID;
    return setlib_install(h, "pg_set_sensor_sets", h->sensor.lib, n_sets, sets, sensor_set_problem, fill_dev_sensor);      // (seed and streams persist)
}
int pg_set_sensor_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->sensor.lib.sets.size(), h->sensor.lib.idx, B, index);
}
int pg_set_sensor_seed(pg_handle* h, uint64_t seed, int32_t B, const uint64_t* stream) {
    if (!h) return PG_ERR_INVALID;
    return seed_install(h, "pg_set_sensor_seed", h->sensor.streams, seed, B, stream);
}
int pg_clear_sensor_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->sensor.lib); if (rc) return rc;
    h->sensor.cleared();
    return PG_OK;
}
int pg_get_sensor_sets(pg_handle* h, int32_t* n_sets, pg_sensor* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_sensor_sets", h->sensor.lib, n_sets, out, max_sets, index, B);
}
int pg_sensor_draws(pg_handle* h, int32_t step0, int32_t steps, int32_t B, double* z) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, step0 >= 0 && steps >= 1 && z, "pg_sensor_draws: need step0 >= 0, steps >= 1 and the output array");
    REQUIRE(h, B >= 1 && B <= h->cfg.batch_capacity, "pg_sensor_draws: need 1 <= B <= batch_capacity");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = h->sensor.streams.sync(h); if (rc) return rc;
    const size_t n = (size_t)steps * (size_t)B * 6;
    CallBufs D; real* d = nullptr;
    HIPCHK(h, D.alloc(d, n));
    hipLaunchKernelGGL(k_sensor_draws, dim3((unsigned)(((size_t)steps * B + 63) / 64)), dim3(64), 0, h->stream, (int)B, (int)step0, (int)steps, h->sensor.streams.d, (unsigned long long)h->sensor.streams.seed, d);
    std::vector<real> tmp(n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(tmp.data(), d, n * sizeof(real), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("pg_sensor_draws: ") + hipGetErrorString(e); return PG_ERR_HIP; }
    for (size_t i = 0; i < n; i++) z[i] = (double)tmp[i];
    return PG_OK;
}
int pg_set_measured_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    return history_register(h, "pg_set_measured_history_dev", h->sensor.lib, "(the measured state is the true one: record state_hist)", h->sensor.hist, buf, steps);
}
static int check_ready(pg_handle* h);
int pg_get_measured_state(pg_handle* h, double* measured) {
    int rc = check_ready(h); if (rc) return rc;
    if (!h->sensor.valid || !h->sensor.meas) { h->err = "pg_get_measured_state: no rollout step under a sensor library since the inputs were installed"; return PG_ERR_STATE; }
    return down(h, measured, h->sensor.meas, (size_t)h->B * 6);
}

// ---- actuator library: the control the PLANT of a rollout step integrates, a_k = actuator(c_{k - delay}, a_{k-1}) per channel (k_actuate).  Build-defined (the reference
// applies the command exactly, model_predictive_control.jl:94-95; ros_integration.jl:51-52 is the choice `feedback` restates).  No part of any QP's structure: nothing is reset ----
static const char* actuator_field_problem(const pg_actuator_set& s) {
    if (s.delay_steps < 0 || s.delay_steps > PG_ACT_MAX_DELAY) return "delay_steps outside [0, PG_ACT_MAX_DELAY = 16]";
    if (!std::isfinite(s.tau_delta) || s.tau_delta < 0.0) return "tau_delta must be finite and >= 0";
    if (!std::isfinite(s.tau_fx) || s.tau_fx < 0.0) return "tau_fx must be finite and >= 0";
    if (!(s.rate_delta > 0.0)) return "rate_delta must be > 0 or +Inf";
    if (!(s.rate_fx > 0.0)) return "rate_fx must be > 0 or +Inf";
    if (s.feedback != 0 && s.feedback != 1) return "feedback must be 0 or 1";
    return nullptr;
}
static void fill_dev_actuator(DevActuator& A, const pg_actuator_set& s) {
    A.delay = s.delay_steps; A.feedback = s.feedback; A.tau_delta = (real)s.tau_delta; A.tau_fx = (real)s.tau_fx; A.rate_delta = (real)s.rate_delta; A.rate_fx = (real)s.rate_fx;
}
int pg_set_actuator_sets(pg_handle* h, int32_t n_sets, const pg_actuator_set* sets) {
    if (!h) return PG_ERR_INVALID;
    std::string why;                                            // (the message names the field and the set)
    const int rc = setlib_install(h, "pg_set_actuator_sets", h->actuator.lib, n_sets, sets, numbered_problem(actuator_field_problem, sets, why), fill_dev_actuator);
    if (rc) return rc;
    h->actuator.feedback = false;
    for (const pg_actuator_set& s : h->actuator.lib.sets) h->actuator.feedback = h->actuator.feedback || s.feedback == 1;
    return PG_OK;
}
int pg_set_actuator_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->actuator.lib.sets.size(), h->actuator.lib.idx, B, index);
}
int pg_clear_actuator_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->actuator.lib); if (rc) return rc;
    h->actuator.cleared();
    return PG_OK;
}
int pg_get_actuator_sets(pg_handle* h, int32_t* n_sets, pg_actuator_set* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_actuator_sets", h->actuator.lib, n_sets, out, max_sets, index, B);
}
int pg_set_applied_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    return history_register(h, "pg_set_applied_history_dev", h->actuator.lib, "(applied = command: record control_hist)", h->actuator.applied_hist, buf, steps);
}
int pg_set_command_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    return history_register(h, "pg_set_command_history_dev", h->actuator.lib, "(applied = command: record control_hist)", h->actuator.command_hist, buf, steps);
}
int pg_get_actuator_state(pg_handle* h, double* applied) {
    int rc = check_ready(h); if (rc) return rc;
    const bool stepped = h->actuator.lib.on() && !h->actuator.fresh && h->actuator.pos;      // (else: no step under a library since the clock restarted -- the position is the command)
    return down(h, applied, stepped ? h->actuator.pos : h->d_control, (size_t)h->B * 3);
}
int pg_actuator_response(pg_handle* h, int32_t steps, double dt, const double* commands, double* applied) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, steps >= 1 && dt > 0.0 && commands && applied, "pg_actuator_response: steps >= 1, dt > 0 and both arrays required");
    const int B = h->B;
    const size_t n = (size_t)steps * (size_t)B * 3;
    // scratch of the call: commands, applied, ring
    return response_call(h, "pg_actuator_response", h->actuator.lib, nullptr, nullptr, 2 * n + (size_t)PG_ACT_MAX_DELAY * B * 3, applied, n, [&](real* d, const real*& result) -> int {
        const int rc = up(h, d, commands, n); if (rc) return rc;
        hipLaunchKernelGGL(k_actuator_response, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, (int)steps, (real)dt, h->actuator.lib.d, h->actuator.lib.index(), d + 2 * n, d, d + n);
        result = d + n;
        return PG_OK;
    });
}

// ---- disturbance library: what acts on the EGO PLANT of a rollout step from outside, w = (wFx, wFy, wMz, wmu) per instance (k_disturb; the <DistW> instantiations of the library kernels).
// Build-defined (the reference integrates the nominal model, model_predictive_control.jl:94).  No part of any QP and invisible to the controller: nothing is reset ----
static const char* disturbance_field_problem(const pg_disturbance& s) {
    const struct { const char* name; double v; } f[8] = {{"Fx", s.Fx}, {"Fy", s.Fy}, {"Mz", s.Mz}, {"sigma_Fx", s.sigma_Fx}, {"sigma_Fy", s.sigma_Fy}, {"x_cp", s.x_cp},
                                                         {"tau_gust", s.tau_gust}, {"mu_scale", s.mu_scale}};
    static thread_local std::string msg;
    for (const auto& x : f) if (!std::isfinite(x.v)) { msg = std::string(x.name) + " is not finite"; return msg.c_str(); }
    if (s.sigma_Fx < 0.0) return "sigma_Fx must be >= 0";
    if (s.sigma_Fy < 0.0) return "sigma_Fy must be >= 0";
    if (s.tau_gust < 0.0) return "tau_gust must be >= 0";
    if (!(s.mu_scale > 0.0)) return "mu_scale must be > 0";
    if (s.step_on < 0) return "step_on must be >= 0";
    return nullptr;
}
static void fill_dev_disturbance(DevDisturbance& D, const pg_disturbance& s) {
    D.step_on = s.step_on; D.step_off = s.step_off; D.Fx = (real)s.Fx; D.Fy = (real)s.Fy; D.Mz = (real)s.Mz; D.sigma_Fx = (real)s.sigma_Fx; D.sigma_Fy = (real)s.sigma_Fy;
    D.x_cp = (real)s.x_cp; D.tau_gust = (real)s.tau_gust; D.mu_scale = (real)s.mu_scale;
}
int pg_set_disturbance_sets(pg_handle* h, int32_t n_sets, const pg_disturbance* sets) {
    if (!h) return PG_ERR_INVALID;
    std::string why;                                            // (the message names the field and the set; seed, streams and the gust state persist)
    return setlib_install(h, "pg_set_disturbance_sets", h->disturbance.lib, n_sets, sets, numbered_problem(disturbance_field_problem, sets, why), fill_dev_disturbance);
}
int pg_set_disturbance_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->disturbance.lib.sets.size(), h->disturbance.lib.idx, B, index);
}
int pg_set_disturbance_seed(pg_handle* h, uint64_t seed, int32_t B, const uint64_t* stream) {
    if (!h) return PG_ERR_INVALID;
    return seed_install(h, "pg_set_disturbance_seed", h->disturbance.streams, seed, B, stream);
}
int pg_clear_disturbance_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->disturbance.lib); if (rc) return rc;
    h->disturbance.cleared();
    return PG_OK;
}
int pg_get_disturbance_sets(pg_handle* h, int32_t* n_sets, pg_disturbance* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_disturbance_sets", h->disturbance.lib, n_sets, out, max_sets, index, B);
}
int pg_set_disturbance_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    return history_register(h, "pg_set_disturbance_history_dev", h->disturbance.lib, "(w = (0, 0, 0, 1) at every step)", h->disturbance.hist, buf, steps);
}
int pg_get_disturbance_state(pg_handle* h, double* w) {
    int rc = check_ready(h); if (rc) return rc;
    if (!h->disturbance.lib.on() || !h->disturbance.valid || !h->disturbance.w) { h->err = "pg_get_disturbance_state: no rollout step under a disturbance library since the inputs were installed"; return PG_ERR_STATE; }
    return down(h, w, h->disturbance.w, (size_t)h->B * 4);
}
int pg_disturbance_response(pg_handle* h, int32_t step0, int32_t steps, double dt, double* w_out) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, step0 >= 0 && steps >= 1 && dt > 0.0 && w_out, "pg_disturbance_response: step0 >= 0, steps >= 1, dt > 0 and the output array required");
    const int B = h->B;
    const size_t n = (size_t)steps * (size_t)B * 4;
    // scratch of the call: w (the gust state lives in the lanes' registers)
    return response_call(h, "pg_disturbance_response", h->disturbance.lib, nullptr, &h->disturbance.streams, n, w_out, n, [&](real* d, const real*& result) -> int {
        hipLaunchKernelGGL(k_disturbance_response, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, (int)step0, (int)steps, (real)dt, h->disturbance.lib.d, h->disturbance.lib.index(),
                           h->disturbance.streams.d, (unsigned long long)h->disturbance.streams.seed, d);
        result = d;
        return PG_OK;
    });
}

// ---- estimator library: the state the CONTROLLER of a rollout step reads, a fixed-gain observer on the sensor's output, xh = p + gain (y - p) per channel with p one step
// of the controller's own model from the previous estimate (k_estimate).  Build-defined (the reference's node receives its estimate from the car).  No part of any QP's
// structure: installing sets or an index resets nothing ----
static const char* estimator_set_problem(const pg_estimator& s) {
    static const char* const outside[6] = {"gain[0] (E) is outside [0, 1] or not finite", "gain[1] (N) is outside [0, 1] or not finite", "gain[2] (psi) is outside [0, 1] or not finite",
                                           "gain[3] (Ux) is outside [0, 1] or not finite", "gain[4] (Uy) is outside [0, 1] or not finite", "gain[5] (r) is outside [0, 1] or not finite"};
    for (int c = 0; c < 6; c++) if (!(s.gain[c] >= 0.0 && s.gain[c] <= 1.0)) return outside[c];      // (false for NaN as well)
    if (s.predict != 0 && s.predict != 1) return "predict must be 0 or 1";
    if (s.reserved != 0) return "reserved must be 0";
    return nullptr;
}
static void fill_dev_estimator(DevEstimator& E, const pg_estimator& s) { E.predict = s.predict; for (int c = 0; c < 6; c++) E.gain[c] = (real)s.gain[c]; }
int pg_set_estimator_sets(pg_handle* h, int32_t n_sets, const pg_estimator* sets) {
    if (!h) return PG_ERR_INVALID;
    // the buffers first: a library is never installed without them (a failed allocation leaves the handle as it was)
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc;
    if ((rc = ensure(h, h->estimator.x, cap_of(h) * 6)) || (rc = ensure(h, h->estimator.u, cap_of(h) * 3))) return rc;
    std::string why;                                            // (the message names the set and the field; the estimate persists)
    return setlib_install(h, "pg_set_estimator_sets", h->estimator.lib, n_sets, sets, numbered_problem(estimator_set_problem, sets, why), fill_dev_estimator);
}
int pg_set_estimator_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->estimator.lib.sets.size(), h->estimator.lib.idx, B, index);
}
int pg_clear_estimator_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->estimator.lib); if (rc) return rc;
    h->estimator.cleared();
    return PG_OK;
}
int pg_get_estimator_sets(pg_handle* h, int32_t* n_sets, pg_estimator* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_estimator_sets", h->estimator.lib, n_sets, out, max_sets, index, B);
}
int pg_set_estimated_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    return history_register(h, "pg_set_estimated_history_dev", h->estimator.lib, "(the controller reads the sensor's output: record that)", h->estimator.hist, buf, steps);
}
int pg_get_estimated_state(pg_handle* h, double* estimated) {
    int rc = check_ready(h); if (rc) return rc;
    if (!h->estimator.lib.on() || !h->estimator.valid || !h->estimator.x) { h->err = "pg_get_estimated_state: no rollout step under an estimator library since the inputs were installed"; return PG_ERR_STATE; }
    return down(h, estimated, h->estimator.x, (size_t)h->B * 6);
}
int pg_estimator_response(pg_handle* h, int32_t steps, double dt, const double* y, const double* u, double* xhat) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, steps >= 1 && dt > 0.0 && y && u && xhat, "pg_estimator_response: steps >= 1, dt > 0, the measurements, the controls and the output array required");
    const int B = h->B;
    const size_t ny = (size_t)steps * (size_t)B * 6, nu = (size_t)steps * (size_t)B * 3;
    // scratch of the call: y, xhat [steps][B][6], u [steps][B][3] (the estimate lives in the lanes' registers)
    return response_call(h, "pg_estimator_response", h->estimator.lib, nullptr, nullptr, 2 * ny + nu, xhat, ny, [&](real* d, const real*& result) -> int {
        int rc;
        if ((rc = up(h, d, y, ny)) || (rc = up(h, d + 2 * ny, u, nu))) return rc;
        hipLaunchKernelGGL(k_estimator_response, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, (int)steps, (real)(dt / h->dc.nsub), h->estimator.lib.d, h->estimator.lib.index(),
                           (const real*)d, (const real*)(d + 2 * ny), d + ny);
        result = d + ny;
        return PG_OK;
    });
}

// ---- human library: the driver of the OTHER CAR in the safety and node rollouts, (omega, a) per instance (k_human; the plant kernels take it through their scripted mode).
// Build-defined (the reference only receives the other car from ROS).  No part of any QP: installing sets, an index, a seed or streams resets nothing ----
static const char* human_field_problem(const pg_human& s) {
    if (s.mode < 0 || s.mode > 3) return "mode must be 0 (hold), 1 (worst case), 2 (scripted) or 3 (seeded random)";
    if (s.hold_steps < 1) return "hold_steps must be >= 1";
    if (s.step_on < 0) return "step_on must be >= 0";
    if (!(s.gain[0] >= 0.0 && s.gain[0] <= 1.0)) return "gain[0] (omega) is outside [0, 1] or not finite";      // (false for NaN as well)
    if (!(s.gain[1] >= 0.0 && s.gain[1] <= 1.0)) return "gain[1] (a) is outside [0, 1] or not finite";
    if (!(s.omega_max >= 0.0)) return "omega_max must be >= 0 (+Inf: no limit) and not NaN";
    if (!(s.a_min <= 0.0)) return "a_min must be <= 0 (-Inf: no limit) and not NaN";
    if (!(s.a_max >= 0.0)) return "a_max must be >= 0 (+Inf: no limit) and not NaN";
    if (!(std::isfinite(s.sigma[0]) && s.sigma[0] >= 0.0)) return "sigma[0] (omega) must be >= 0 and finite";
    if (!(std::isfinite(s.sigma[1]) && s.sigma[1] >= 0.0)) return "sigma[1] (a) must be >= 0 and finite";
    if (!(std::isfinite(s.tau) && s.tau >= 0.0)) return "tau must be >= 0 and finite";
    return nullptr;
}
static void fill_dev_human(DevHuman& H, const pg_human& s) {
    H.mode = s.mode; H.hold_steps = s.hold_steps; H.step_on = s.step_on; H.step_off = s.step_off; H.gain[0] = (real)s.gain[0]; H.gain[1] = (real)s.gain[1];
    H.omega_max = (real)s.omega_max; H.a_min = (real)s.a_min; H.a_max = (real)s.a_max; H.sigma[0] = (real)s.sigma[0]; H.sigma[1] = (real)s.sigma[1]; H.tau = (real)s.tau;
}
int pg_set_human_sets(pg_handle* h, int32_t n_sets, const pg_human* sets) {
    if (!h) return PG_ERR_INVALID;
    std::string why;                                            // (the message names the set and the field; seed, streams and the driver's state persist)
    const int rc = setlib_install(h, "pg_set_human_sets", h->human.lib, n_sets, sets, numbered_problem(human_field_problem, sets, why), fill_dev_human);
    if (rc) return rc;
    h->human.script = false;
    for (const pg_human& s : h->human.lib.sets) h->human.script = h->human.script || s.mode == 2;
    return PG_OK;
}
int pg_set_human_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->human.lib.sets.size(), h->human.lib.idx, B, index);
}
int pg_set_human_seed(pg_handle* h, uint64_t seed, int32_t B, const uint64_t* stream) {
    if (!h) return PG_ERR_INVALID;
    return seed_install(h, "pg_set_human_seed", h->human.streams, seed, B, stream);
}
int pg_clear_human_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->human.lib); if (rc) return rc;
    h->human.cleared();
    return PG_OK;
}
int pg_get_human_sets(pg_handle* h, int32_t* n_sets, pg_human* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_human_sets", h->human.lib, n_sets, out, max_sets, index, B);
}
int pg_set_human_history_dev(pg_handle* h, pg_real_dev* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    return history_register(h, "pg_set_human_history_dev", h->human.lib, "(the rollouts' human_mode decides: human_hist_dev of pg_simulate_safety_dev records that)", h->human.hist, buf, steps);
}
int pg_get_human_state(pg_handle* h, double* u) {
    int rc = check_ready(h); if (rc) return rc;
    if (!h->human.lib.on() || !h->human.valid || !h->human.u) { h->err = "pg_get_human_state: no rollout step under a human library since the inputs were installed"; return PG_ERR_STATE; }
    return down(h, u, h->human.u, (size_t)h->B * 2);
}
// what mode 1 is handed as has_hji: a grid on a coupled handle (the safety rollout is coupled only; the node rollout passes its plant kernel the same word)
static int has_hji_row(const pg_handle* h) { return (int)(h->hji.on && h->dc.formulation == PG_COUPLED); }
int pg_human_response(pg_handle* h, int32_t step0, int32_t steps, double dt, const double* x7, const double* vg8, const double* script, double* u_out) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, step0 >= 0 && steps >= 1 && dt > 0.0 && x7 && vg8 && u_out, "pg_human_response: step0 >= 0, steps >= 1, dt > 0, x7, vg8 and the output array required");
    const char* const refuse = (h->human.script && !script) ? "pg_human_response: an installed set has mode 2 and needs script [steps][B][2]" : nullptr;
    const int B = h->B;
    const size_t sb = (size_t)steps * (size_t)B, nx = sb * 7, nv = sb * 8, nu = sb * 2;
    // scratch of the call: x7, vg8, script, u (the driver's state lives in the lanes' registers)
    return response_call(h, "pg_human_response", h->human.lib, refuse, &h->human.streams, nx + nv + 2 * nu, u_out, nu, [&](real* d, const real*& result) -> int {
        real *dx = d, *dv = d + nx, *ds = dv + nv, *du = ds + nu;
        int rc;
        if ((rc = up(h, dx, x7, nx)) || (rc = up(h, dv, vg8, nv)) || (script && (rc = up(h, ds, script, nu)))) return rc;
        hipLaunchKernelGGL(k_human_response, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc.veh, B, (int)step0, (int)steps, has_hji_row(h), (real)dt, h->human.lib.d,
                           h->human.lib.index(), h->human.streams.d, (unsigned long long)h->human.streams.seed, (const real*)dx, (const real*)dv,
                           script ? (const real*)ds : (const real*)nullptr, du);
        result = du;
        return PG_OK;
    });
}

// ---- route library: the trajectory an instance tracks changes DURING a rollout (nominal_trajectory_callback, ros_integration.jl:30-41; k_route).  The events write the
// device trajectory index in place; what pg_set_trajectory_index installed (IndexArray::host) is the instance's home ----
static_assert(sizeof(pg_route_event) == 32 && sizeof(pg_route) == 128 && offsetof(pg_route_event, t_join) == 24, "the sizes include/pigeon_mpc.h states");
pg_route pg_default_route(void) {
    pg_route r; memset(&r, 0, sizeof(r));
    for (pg_route_event& e : r.ev) { e.step = -1; e.anchor = PG_ROUTE_STAMP; e.cold = 1; }
    return r;
}
static const char* route_set_problem(const pg_route& r) {
    bool unused_seen = false; int last = -1;
    for (const pg_route_event& e : r.ev) {
        if (e.target_mode != PG_ROUTE_ABSOLUTE && e.target_mode != PG_ROUTE_RELATIVE) return "target_mode must be 0 (absolute) or 1 (relative)";
        if (e.anchor < PG_ROUTE_KEEP || e.anchor > PG_ROUTE_PROJECT) return "anchor must be 0 (keep), 1 (path), 2 (stamp) or 3 (project)";
        if (e.cold != 0 && e.cold != 1) return "cold must be 0 or 1";
        if (e.reserved != 0) return "reserved must be 0";
        if (!std::isfinite(e.t_join)) return "t_join must be finite";
        if ((e.anchor == PG_ROUTE_KEEP || e.anchor == PG_ROUTE_PATH) && e.t_join != 0.0) return "t_join must be 0 under the anchors keep and path";
        if (e.step < 0) { unused_seen = true; continue; }
        if (unused_seen) return "a used slot (step >= 0) stands behind an unused one";
        if (e.step <= last) return "the steps of the used slots must be strictly increasing";
        last = e.step;
        if (e.target_mode == PG_ROUTE_ABSOLUTE && e.target < 0) return "an absolute target must be >= 0";
    }
    return nullptr;
}
int pg_set_route_sets(pg_handle* h, int32_t n_sets, const pg_route* sets) {
    if (!h) return PG_ERR_INVALID;
    std::string why;                                            // (the message names the set; the route state persists: it restarts with the clock)
    const int rc = setlib_install(h, "pg_set_route_sets", h->route.lib, n_sets, sets, numbered_problem(route_set_problem, sets, why), [](pg_route& d, const pg_route& s) { d = s; });
    if (rc) return rc;
    auto& steps = h->route.event_steps; steps.clear();
    for (const pg_route& r : h->route.lib.sets) for (const pg_route_event& e : r.ev) if (e.step >= 0 && !h->route.event_at(e.step)) steps.push_back(e.step);
    return PG_OK;
}
int pg_set_route_index(pg_handle* h, int32_t B, const int32_t* index) {
    if (!h) return PG_ERR_INVALID;
    return index_install(h, (int)h->route.lib.sets.size(), h->route.lib.idx, B, index);
}
int pg_clear_route_sets(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    const int rc = setlib_clear(h, h->route.lib); if (rc) return rc;
    h->route.cleared();
    return PG_OK;
}
int pg_get_route_sets(pg_handle* h, int32_t* n_sets, pg_route* out, int32_t max_sets, int32_t* index, int32_t B) {
    if (!h) return PG_ERR_INVALID;
    return setlib_get(h, "pg_get_route_sets", h->route.lib, n_sets, out, max_sets, index, B);
}
int pg_set_route_history_dev(pg_handle* h, int32_t* buf, int32_t steps) {
    if (!h) return PG_ERR_INVALID;
    auto& U = h->route;
    if (!buf && steps == 0) { U.hist = nullptr; U.hist_steps = 0; return PG_OK; }
    REQUIRE(h, buf, "pg_set_route_history_dev: a device buffer [steps][B] of int32 is required ((NULL, 0) drops the registration)");
    REQUIRE(h, steps >= 1, "pg_set_route_history_dev: steps >= 1 required");
    if (!U.lib.on()) { h->err = "pg_set_route_history_dev: no route library installed (every instance stays on the trajectory pg_set_trajectory_index gave it)"; return PG_ERR_STATE; }
    U.hist = buf; U.hist_steps = steps;
    return PG_OK;
}
int pg_get_route_state(pg_handle* h, int32_t* traj, int32_t* fired, int32_t* last_step, double* t_at, double* e_at) {
    int rc = check_ready(h); if (rc) return rc;
    auto& U = h->route;
    if (!U.lib.on()) { h->err = "pg_get_route_state: no route library installed"; return PG_ERR_STATE; }
    const size_t B = (size_t)h->B, cap = cap_of(h);
    if (U.fresh || !U.fired) {                                  // no rollout step under the library since the clock (re)started: nothing fired.  The return home is
        // applied when the next rollout starts (route_start): until then pg_step* and the phase calls run on what the device index holds, and that is what is reported
        if (h->dc.n_traj > 1 && h->traj_idx.d) { if ((rc = down_raw(h, traj, h->traj_idx.d, B * sizeof(int32_t)))) return rc; }
        else if (traj) memset(traj, 0, B * sizeof(int32_t));
        for (size_t b = 0; b < B; b++) {
            if (fired) fired[b] = 0;
            if (last_step) last_step[b] = -1;
            if (t_at) t_at[b] = NAN;
            if (e_at) e_at[b] = NAN;
        }
        return PG_OK;
    }
    if ((rc = down_raw(h, traj, h->traj_idx.d, B * sizeof(int32_t))) || (rc = down_raw(h, fired, U.fired, B * sizeof(int32_t))) ||
        (rc = down_raw(h, last_step, U.fired + cap, B * sizeof(int32_t))) || (rc = down_raw(h, t_at, U.t_at, B * sizeof(double))) || (rc = down(h, e_at, U.e_at, B))) return rc;
    return PG_OK;
}

// ---- the handle's HJI table (pg_handle::hji, dc.has_hji): these two routines are the only code that writes it.  An install is "clear, then build": the old table is gone
// before the new one is allocated (never two tables side by side: the cell records are 1.9 to 19 GB for the real grid), so AFTER A FAILED INSTALL the handle has no HJI
// grid, no device memory of the call remains (the call's CallBufs held all of it), and pg_last_error says why ----
static void hji_table_clear(pg_handle* h) {
    (void)hipStreamSynchronize(h->stream);                      // (a launch still queued reads the old table)
    h->mem.drop(h->hji.knots); h->mem.drop(h->hji.cells);
    memset(&h->hji.hv, 0, sizeof(HjiView)); h->hji.on = false; h->dc.has_hji = 0;
}
// The lookup table from the node records and the knots of walk W, both on the device and held by D.  The cell records (8 corners of dims 1..3 contiguous) are built in D
// on a view of the call's; only after the kernel has run do knots and cells pass to the handle and the record is filled.  The node records stay in D and die with the call
static int hji_table_build(pg_handle* h, const HjiWalk& W, CallBufs& D, float*& nodes, float*& knots) {
    HjiView V; memset(&V, 0, sizeof(V)); W.fill(V); V.knots = knots; V.nodes = nodes;
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    // Device layout: 256 B cell records (cdims = 3: sixteen per lookup; 6 x the node table -- 1.9 GB for the 13 x 13 x 9^5 grid).  Since the lookup reads every record 256
    // contiguous bytes per instruction and lane group (round 4), the three layouts stream at the same rate -- 0.77 / 0.76 / 0.69-0.74 of the HBM peak for 256 B / 1 KiB /
    // 4 KiB records -- so the smallest table is the default (rounds 1-3: 4 KiB records, 19.3 GB).  Option "hji_cell_dims" = 5 / 7 selects the larger records (bench, tests).
    int cd = h->hji_cell_dims; long ncell = 0;
    for (;; cd -= 2) {        // (a larger record asked for must fit a quarter of the free HBM)
        long cs = 1; ncell = 1;
        for (int d = 0; d < 7; d++) { int ext = d < cd ? W.dims[d] - 1 : W.dims[d]; V.cstride[d] = cs; cs *= ext; ncell *= ext; }
        if (cd == 3 || ((size_t)ncell << cd) * 32 <= free_b / 4) break;
    }
    float* cells = nullptr;
    HIPCHK(h, D.alloc(cells, ((size_t)ncell << cd) * 8));
    V.cdims = cd; V.cells = cells;
    hipLaunchKernelGGL(k_hji_build_cells, dim3((unsigned)((((size_t)ncell << cd) + 255) / 256)), dim3(256), 0, h->stream, V, ncell, cells);
    LAUNCH_CHECK(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    V.nodes = nullptr;
    h->mem.adopt(h->hji.knots, D.give(knots)); h->mem.adopt(h->hji.cells, D.give(cells));
    memcpy(&h->hji.hv, &V, sizeof(HjiView)); h->hji.on = true; h->dc.has_hji = 1;      // (a byte copy: the captured step compares the view with memcmp, padding included)
    return PG_OK;
}

int pg_clear_hji_grid(pg_handle* h) { if (!h) return PG_ERR_INVALID; hji_table_clear(h); return PG_OK; }
int pg_set_hji_grid(pg_handle* h, const int32_t dims[7], const float* knots_concat, const float* V, const float* gradV) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, dims && knots_concat && V && gradV, "pg_set_hji_grid: null argument");
    REQUIRE(h, h->dc.formulation == PG_COUPLED, "the HJI safety row belongs to the coupled formulation only (coupled_lat_long.jl:341-346)");
    HjiWalk W; { const int rc = hji_walk(h, "pg_set_hji_grid", dims, W); if (rc) return rc; }
    const size_t n = W.n; const int nk = W.nk;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hji_table_clear(h);
    // interleave (V, gradV[7]) into 8-float node records: one 32 B aligned read per corner instead of a 4 B + a 28 B unaligned one
    std::vector<float> rec(n * 8);
    for (size_t i = 0; i < n; i++) { rec[8 * i] = V[i]; for (int k = 0; k < 7; k++) rec[8 * i + 1 + k] = gradV[7 * i + k]; }
    CallBufs D; float *d_rec = nullptr, *d_kn = nullptr;
    HIPCHK(h, D.alloc(d_rec, rec.size())); HIPCHK(h, D.alloc(d_kn, (size_t)nk));
    HIPCHK(h, hipMemcpy(d_rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_kn, knots_concat, (size_t)nk * sizeof(float), hipMemcpyHostToDevice));
    return hji_table_build(h, W, D, d_rec, d_kn);
}

// ---- pg_hji_solve: the reachable-tube sweeps (pg_hji_solve.hip).  The host owns the only loop over sweeps: eval -> alpha to the host -> dt -> update ----
pg_hji_solve_opts pg_default_hji_solve_opts(void) {
    pg_hji_solve_opts o; o.horizon = 3.0; o.cfl = 0.8; o.fixed_dt = 0.0; o.max_sweeps = 100000; o.flags = 0;
    return o;
}
namespace {
float hji_key_float(unsigned int k) { unsigned int b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; memcpy(&f, &b, 4); return f; }
}  // namespace
int pg_hji_solve(pg_handle* h, const int32_t dims[7], const float* knots_concat, const float* l0, const pg_vehicle* vehicle, const pg_hji_solve_opts* opts,
                 int32_t install, float* V_out, float* gradV_out, pg_hji_solve_stats* stats) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, dims && knots_concat && l0, "pg_hji_solve: null argument");
    const pg_hji_solve_opts O = opts ? *opts : pg_default_hji_solve_opts();
    HjiWalk W; { const int rc = hji_walk(h, "pg_hji_solve", dims, W); if (rc) return rc; }
    const size_t n = W.n; const int nk = W.nk;
    double minsp[7];
    {
        const float* k = knots_concat;
        for (int d = 0; d < 7; d++) {
            minsp[d] = INFINITY;
            for (int i = 0; i < dims[d]; i++) REQUIRE(h, std::isfinite(k[i]), "pg_hji_solve: a knot is not finite");
            for (int i = 1; i < dims[d]; i++) {
                REQUIRE(h, k[i] > k[i - 1], "pg_hji_solve: knots must increase strictly");
                minsp[d] = std::min(minsp[d], (double)k[i] - (double)k[i - 1]);
            }
            if (d == 3) REQUIRE(h, k[0] > 0.0f, "pg_hji_solve: the knots of dimension 4 (Ux) must be positive");
            if (d == 2 && (O.flags & PG_HJI_PERIODIC_PSI)) {
                REQUIRE(h, dims[d] >= 3, "pg_hji_solve: a periodic dimension 3 needs >= 3 knots");
                REQUIRE(h, fabs(((double)k[dims[d] - 1] - (double)k[0]) - 2.0 * M_PI) <= 4.76837158203125e-07, "pg_hji_solve: a periodic dimension 3 spans 2 pi");
            }
            k += dims[d];
        }
    }
    REQUIRE(h, (O.flags & ~(int32_t)PG_HJI_PERIODIC_PSI) == 0, "pg_hji_solve: unknown flags");
    REQUIRE(h, std::isfinite(O.horizon) && O.horizon >= 0.0, "pg_hji_solve: horizon must be finite and >= 0");
    REQUIRE(h, O.cfl > 0.0 && O.cfl <= 1.0, "pg_hji_solve: cfl must lie in (0, 1]");
    REQUIRE(h, std::isfinite(O.fixed_dt) && O.fixed_dt >= 0.0, "pg_hji_solve: fixed_dt must be finite and >= 0");
    REQUIRE(h, O.max_sweeps >= 0, "pg_hji_solve: max_sweeps must be >= 0");
    if (vehicle) REQUIRE_NO(h, "pg_hji_solve: the vehicle: ", plant_set_problem(*vehicle));
    if (install && h->dc.formulation != PG_COUPLED) { h->err = "pg_hji_solve: install: the HJI safety row belongs to the coupled formulation only (coupled_lat_long.jl:341-346)"; return PG_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    HjiSolveGrid G; W.fill(G);
    G.n = (long)n; G.periodic = (O.flags & PG_HJI_PERIODIC_PSI) ? 1 : 0;
    DevVehicle P; fill_dev_vehicle(P, vehicle ? *vehicle : h->cfg.vehicle);
    CallBufs D; float *d_kn = nullptr, *d_V[2] = {nullptr, nullptr}, *d_rec = nullptr; real *d_Hc = nullptr, *d_alpha = nullptr; int* d_bad = nullptr; unsigned int* d_vkeys = nullptr;
    HIPCHK(h, D.alloc(d_kn, (size_t)nk));
    HIPCHK(h, D.alloc(d_V[0], n));
    HIPCHK(h, D.alloc(d_V[1], n));
    HIPCHK(h, D.alloc(d_Hc, n));
    HIPCHK(h, D.alloc(d_rec, n * 8));
    HIPCHK(h, D.alloc(d_alpha, 7));
    HIPCHK(h, D.alloc(d_bad, 1));
    HIPCHK(h, D.alloc(d_vkeys, 2));
    G.knots = d_kn;
    HIPCHK(h, hipMemcpyAsync(d_kn, knots_concat, (size_t)nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_V[0], l0, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_bad, 0, sizeof(int), h->stream));
    const unsigned int keys0[2] = {0xffffffffu, 0u};
    HIPCHK(h, hipMemcpyAsync(d_vkeys, keys0, sizeof(keys0), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                 // (the host arrays have been consumed)

    pg_hji_solve_stats S; memset(&S, 0, sizeof(S)); S.bad_sweep = -1;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    int cur = 0, bad = 0;
    bool reached = !(O.horizon > 0.0);
    while (!reached && S.sweeps < O.max_sweeps) {
        real a[7];
        HIPCHK(h, hipMemsetAsync(d_alpha, 0, 7 * sizeof(real), h->stream));
        hipLaunchKernelGGL(k_hji_sweep_eval, grid, block, 0, h->stream, G, P, (const float*)d_V[cur], d_Hc, d_alpha);
        LAUNCH_CHECK(h);
        HIPCHK(h, hipMemcpyAsync(a, d_alpha, sizeof(a), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));      // (the flag of the previous sweep's update)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (bad) break;
        double sum = 0.0;
        for (int d = 0; d < 7; d++) { S.alpha[d] = (double)a[d]; sum += (double)a[d] / minsp[d]; }
        double dt = O.fixed_dt > 0.0 ? O.fixed_dt : O.cfl / sum;          // (sum = 0: nothing moves, dt = +Inf and the step below is the whole remainder)
        const double rem = O.horizon - S.tau;
        const bool last = !(dt < rem);
        if (last) dt = rem;
        hipLaunchKernelGGL(k_hji_sweep_update, grid, block, 0, h->stream, G, (const float*)d_V[cur], (const real*)d_Hc, (const real*)d_alpha, (real)dt, d_V[cur ^ 1], d_bad);
        LAUNCH_CHECK(h);
        cur ^= 1; S.sweeps++; S.last_dt = dt; S.tau = last ? O.horizon : S.tau + dt; reached = last;
    }
    if (!bad) {
        hipLaunchKernelGGL(k_hji_finish, grid, block, 0, h->stream, G, (const float*)d_V[cur], d_rec, d_vkeys, d_bad);
        LAUNCH_CHECK(h);
        unsigned int keys[2];
        HIPCHK(h, hipMemcpyAsync(keys, d_vkeys, sizeof(keys), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        S.v_min = (double)hji_key_float(keys[0]); S.v_max = (double)hji_key_float(keys[1]);
    }
    S.reached_horizon = (int32_t)(reached && !bad);
    if (bad) {
        S.bad_sweep = S.sweeps > 0 ? S.sweeps - 1 : 0;
        if (stats) *stats = S;
        h->err = "pg_hji_solve: V holds a NaN or Inf after sweep " + std::to_string(S.bad_sweep) + " (nothing was installed)";
        return PG_ERR_INVALID;
    }
    if (V_out) HIPCHK(h, hipMemcpy(V_out, d_V[cur], n * sizeof(float), hipMemcpyDeviceToHost));
    if (gradV_out) {                                    // the records hold (V, gradV[7]): 28 of every 32 bytes
        std::vector<float> rec(n * 8);
        HIPCHK(h, hipMemcpy(rec.data(), d_rec, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) for (int k = 0; k < 7; k++) gradV_out[7 * i + k] = rec[8 * i + 1 + k];
    }
    if (stats) *stats = S;
    if (install) {
        hji_table_clear(h);
        return hji_table_build(h, W, D, d_rec, d_kn);
    }
    return PG_OK;
}

int pg_reset(pg_handle* h, const uint8_t* mask) {
    if (!h) return PG_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int cap = h->cfg.batch_capacity;
    h->warm_B = 0; h->order_B = 0;
    if (!mask) { HIPCHK(h, hipMemsetAsync(h->d_solved, 0, (size_t)2 * cap * sizeof(int), h->stream)); return PG_OK; }      // (solved flags and the back-off words behind them: one fill)
    REQUIRE(h, h->B > 0, "pg_reset with a mask needs inputs installed (B known)");
    HIPCHK(h, hipMemcpyAsync(h->d_mask, mask, h->B, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_reset, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->B, h->d_mask, h->d_solved, h->d_wfail);
    LAUNCH_CHECK(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));            // the caller may reuse `mask`
    return PG_OK;
}

static void stage_block(pg_handle* h, int32_t B, const double* s_, const double* c_, const double* t0, const double* o_, const double* toff);
static int set_inputs(pg_handle* h, int32_t B, const void* state, const void* control, const double* t0, const void* other, const double* toff, bool host) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, B >= 1 && B <= h->cfg.batch_capacity, "batch size outside [1, batch_capacity]");
    REQUIRE(h, state && control && t0, "state, control and t0 are required");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->B = B; h->sim_idx = 0; restart_on_inputs(h);      // (new times: the clock of pg_simulate_dev restarts from them, and the safety summary and node counts with it)
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (host) {
        // the caller's arrays are converted / copied into the pinned staging buffer here and now (so they may be reused as soon as this returns) and travel
        // from there with asynchronous copies ordered before the kernels on the handle's stream: no synchronisation on the way in.  A previous call's
        // copies must have left the buffer first.
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const double* s_ = (const double*)state; const double* c_ = (const double*)control; const double* o_ = (const double*)other;
        if (B == h->cfg.batch_capacity) {
            // the batch fills the handle: the staging buffer takes the layout of the device block and ONE copy carries all five arrays (a single controller at
            // 100 Hz -- B = capacity = 1 -- used to pay five copies and two memsets of a few bytes each per step)
            stage_block(h, B, s_, c_, t0, o_, toff);
            HIPCHK(h, hipMemcpyAsync(h->d_in, h->h_stage, h->in_bytes, kind, h->stream));
            return PG_OK;
        }
        real* st = (real*)h->h_stage; real* ct = st + (size_t)B * 6; real* ot = ct + (size_t)B * 3; double* tt = (double*)(h->h_stage + ((size_t)B * 13 * sizeof(real) + 7) / 8 * 8); double* ft = tt + B;
        for (size_t i = 0; i < (size_t)B * 6; i++) st[i] = (real)s_[i];
        for (size_t i = 0; i < (size_t)B * 3; i++) ct[i] = (real)c_[i];
        if (o_) for (size_t i = 0; i < (size_t)B * 4; i++) ot[i] = (real)o_[i];
        memcpy(tt, t0, (size_t)B * 8);
        if (toff) memcpy(ft, toff, (size_t)B * 8);
        state = st; control = ct; t0 = tt; if (o_) other = ot; if (toff) toff = ft;      // (the five copies below, from the staging buffer)
    }
    HIPCHK(h, hipMemcpyAsync(h->d_state, state, (size_t)B * 6 * sizeof(real), kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_control, control, (size_t)B * 3 * sizeof(real), kind, h->stream));
    if (other) HIPCHK(h, hipMemcpyAsync(h->d_other, other, (size_t)B * 4 * sizeof(real), kind, h->stream));
    else HIPCHK(h, hipMemsetAsync(h->d_other, 0, (size_t)B * 4 * sizeof(real), h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_t0, t0, (size_t)B * 8, kind, h->stream));
    if (toff) HIPCHK(h, hipMemcpyAsync(h->d_toff, toff, (size_t)B * 8, kind, h->stream));
    else HIPCHK(h, hipMemsetAsync(h->d_toff, 0xFF, (size_t)B * 8, h->stream));      // all-ones bit pattern is a NaN: path-tracking mode
    return PG_OK;
}
int pg_set_inputs(pg_handle* h, int32_t B, const double* state, const double* control, const double* t0, const double* other, const double* toff) {
    return set_inputs(h, B, state, control, t0, other, toff, true);
}
int pg_set_inputs_dev(pg_handle* h, int32_t B, const void* state, const void* control, const double* t0, const void* other, const double* toff) {
    return set_inputs(h, B, state, control, t0, other, toff, false);
}

// ---- pg_make_starts: the inputs of a batch placed on the installed trajectory library under a library of start sets (pg_start_make.hip).  One launch, one lane per
// instance; the install is pg_set_inputs_dev from the call's own buffers ----
static_assert(sizeof(pg_start_set) == 240 && offsetof(pg_start_set, s_mode) == 208, "the size include/pigeon_mpc.h states; the 26 range fields lead the structure");
pg_start_set pg_default_start_set(void) {
    pg_start_set s; memset(&s, 0, sizeof(s)); s.v_lo = 1.0; s.v_hi = 1.0;
    return s;
}
static const char* start_set_problem(const pg_start_set& s) {
    const double* r = &s.s_lo;
    for (int c = 0; c < ST_CHANNELS; c++) {
        if (!(std::isfinite(r[2 * c]) && std::isfinite(r[2 * c + 1]))) return "a range field is not finite";
        if (r[2 * c] > r[2 * c + 1]) return "a range needs lo <= hi";
    }
    if (!(s.v_lo > 0.0)) return "the speed factor needs v_lo > 0";
    for (int32_t m : {s.s_mode, s.e_mode, s.steady, s.time_mode, s.other_mode}) if (m != 0 && m != 1) return "a mode is 0 or 1";
    for (int32_t z : s.reserved) if (z != 0) return "reserved must be 0";
    return nullptr;
}
int pg_make_starts(pg_handle* h, int32_t B, int32_t n_sets, const pg_start_set* sets, const int32_t* set_index, uint64_t seed, const uint64_t* stream, int32_t install,
                   double* state_out, double* control_out, double* t0_out, double* other_out, double* time_offset_out, double* placed_out) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, sets, "pg_make_starts: null argument");
    REQUIRE(h, n_sets >= 1, "pg_make_starts: need n_sets >= 1");
    REQUIRE(h, B >= 1 && B <= h->cfg.batch_capacity, "pg_make_starts: batch size outside [1, batch_capacity]");
    std::string why;
    auto problem = numbered_problem(start_set_problem, sets, why);
    for (int k = 0; k < n_sets; k++) REQUIRE_NO(h, "pg_make_starts: ", problem(sets[k]));
    if (set_index) for (int b = 0; b < B; b++) REQUIRE(h, set_index[b] >= 0 && set_index[b] < n_sets, "pg_make_starts: index out of range of the start sets");
    if (!h->d_traj) { h->err = "pg_make_starts: no trajectory installed (the starts are placed on the installed library)"; return PG_ERR_STATE; }
    if (h->dc.n_traj > 1 && h->traj_idx.covered() < B) { h->err = "pg_make_starts: a trajectory library is installed but pg_set_trajectory_index does not cover B (an instance is placed on its own tube)"; return PG_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->cfg.device));

    const size_t nb = (size_t)B;
    CallBufs D; StartMakeArgs A{}; pg_start_set* d_sets = nullptr; int* d_idx = nullptr; unsigned long long* d_stream = nullptr;
    HIPCHK(h, D.alloc(d_sets, (size_t)n_sets));
    HIPCHK(h, D.alloc(A.state, nb * 6)); HIPCHK(h, D.alloc(A.control, nb * 3)); HIPCHK(h, D.alloc(A.other, nb * 4));
    HIPCHK(h, D.alloc(A.t0, nb)); HIPCHK(h, D.alloc(A.toff, nb)); HIPCHK(h, D.alloc(A.placed, nb * 4));
    // (plain copies: the caller's arrays are consumed when each returns, on every way out)
    HIPCHK(h, hipMemcpy(d_sets, sets, (size_t)n_sets * sizeof(pg_start_set), hipMemcpyHostToDevice));
    if (set_index && n_sets > 1) { HIPCHK(h, D.alloc(d_idx, nb)); HIPCHK(h, hipMemcpy(d_idx, set_index, nb * sizeof(int), hipMemcpyHostToDevice)); }
    if (stream) { HIPCHK(h, D.alloc(d_stream, nb)); HIPCHK(h, hipMemcpy(d_stream, stream, nb * sizeof(unsigned long long), hipMemcpyHostToDevice)); }
    A.B = B; A.n_sets = n_sets; A.sets = d_sets; A.set_index = d_idx; A.stream = d_stream; A.seed = (unsigned long long)seed;
    hipLaunchKernelGGL(k_make_starts, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, h->dc, A);
    LAUNCH_CHECK(h);
    int rc = down(h, state_out, A.state, nb * 6);                  // (each waits for the stream: the kernel has run)
    if (!rc) rc = down(h, control_out, A.control, nb * 3);
    if (!rc) rc = down(h, other_out, A.other, nb * 4);
    if (!rc) rc = down_raw(h, t0_out, A.t0, nb * 8);
    if (!rc) rc = down_raw(h, time_offset_out, A.toff, nb * 8);
    if (!rc) rc = down_raw(h, placed_out, A.placed, nb * 4 * 8);
    if (!rc && install) rc = set_inputs(h, B, A.state, A.control, A.t0, A.other, A.toff, false);      // pg_set_inputs_dev: the same buffers, the restarted clock, the restart of every library state
    const hipError_t e = hipStreamSynchronize(h->stream);          // the copies out of the call's buffers have landed before they are freed, on every way out
    if (!rc && e != hipSuccess) { h->err = std::string("pg_make_starts: ") + hipGetErrorString(e); rc = PG_ERR_HIP; }
    return rc;
}

static int check_ready(pg_handle* h) {
    if (!h) return PG_ERR_INVALID;
    if (h->B <= 0) { h->err = "no inputs installed (call pg_set_inputs first)"; return PG_ERR_STATE; }
    if (!h->d_traj) { h->err = "no trajectory installed (call pg_set_trajectory first)"; return PG_ERR_STATE; }
    if (index_covers(h, (size_t)h->dc.n_traj, h->traj_idx) || index_covers(h, (size_t)h->dc.n_cp, h->cp.idx)) return PG_ERR_STATE;
    if (hipSetDevice(h->cfg.device) != hipSuccess) { h->err = "hipSetDevice failed"; return PG_ERR_HIP; }
    return PG_OK;
}

int pg_compute_time_steps(pg_handle* h) {
    int rc = check_ready(h); if (rc) return rc;
    const int B = h->B;
    hipLaunchKernelGGL(k_time_steps, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, h->d_t0, h->d_ts, h->d_dt, h->d_prev_ts);
    LAUNCH_CHECK(h);
    return PG_OK;
}
static int launch_nodes(pg_handle* h, const Seen& seen, bool with_time_grid, bool& lin_done);
int pg_compute_linearization_nodes(pg_handle* h) {
    int rc = check_ready(h); if (rc) return rc;
    bool lin_done;      // (false: without the time grid the pipelined launch never applies)
    return launch_nodes(h, seen_own(h), false, lin_done);
}
// compute_time_steps! + compute_linearization_nodes! of pg_step_dev / pg_simulate_dev: the time grid rides in the projection kernel (one launch fewer)
// the pipelined nodes + update_QP launch (k_nodes_linearize) serves the steps of pg_step_dev / pg_simulate_dev when: coupled formulation, some instance is cold (an
// all-warm batch has no recurrence: k_nodes_warm), the batch is large enough for the linearisation to need more than one round of wavefronts (one lane per interval:
// 2048 x 29 / 64 = 928 wavefronts are one round and the two launches are shorter -- 0.310 against 0.315 ms; 2560: 0.386 against 0.317) and small enough for the nodes
// wavefronts to be resident at once (<= 16384 instances = 256 of the 1024 SIMD slots; measured with the one-lane linearisation: 12288: 0.72 against 0.86 ms, 16384: 1.02 against 1.07), and the
// linearisation is not fused into the solve kernel.  With a safety row, its (M, b) -- functions of the measured states only -- are computed BEFORE the launch and the
// launch order is re-filed after it (k_order_hji needs the verdicts the recurrence files).
static int launch_hji_rows_compute(pg_handle* h, const Seen& seen);
static int launch_hji_order(pg_handle* h, const Seen& seen);
static bool pipeline_applies(const pg_handle* h) {
    const DevCfg& C = h->dc;
    const bool fuse_wanted = h->fuse == 1;
    return h->pipeline == 1 && C.formulation != PG_DECOUPLED && h->warm_B < h->B && h->B >= h->pipe_min && h->B <= h->pipe_max && C.Ns > 0 && C.Ns < C.N && !fuse_wanted;
}
// the nodes kernels' view of the launch order: what the previous solve left per instance, and where the order of this step is filed (order == nullptr: not filed)
static OrderOut order_out(const pg_handle* h, int* order) {
    OrderOut F{}; F.prev_status = h->d_status; F.prev_iters = h->d_iters; F.prev_polish = h->d_polish; F.order = order; F.cnt = order_cnt(h); F.slow = order_slow(h);
    return F;
}
// The four branches of launch_nodes behind the projection.  staged / traj_lds: the trajectory travels through LDS; F: where the launch order of the step is filed.
static int launch_nodes_decoupled(pg_handle* h, const Seen& seen, bool staged, size_t traj_lds) {
    const int B = h->B;
    auto kern = staged ? k_nodes_dec<true> : k_nodes_dec<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((B + NODES_DEC_IPB - 1) / NODES_DEC_IPB)), dim3(64), traj_lds, h->stream, h->dc, B, seen.state, seen.control, h->d_toff, h->d_sep, h->d_ts, h->d_dt, h->d_nodes, h->d_naux);      // (NODES_DEC_LPN lanes per instance)
    LAUNCH_CHECK(h);
    const long nn = (long)B * h->dc.NN;
    hipLaunchKernelGGL(k_nodes_angles, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, h->stream, h->dc, B, h->d_naux, h->d_nodes, (const int*)nullptr);
    LAUNCH_CHECK(h);
    return PG_OK;
}
// every instance takes the warm branch: lane = (instance, node)
static int launch_nodes_warm(pg_handle* h, const Seen& seen, bool staged, size_t traj_lds, const OrderOut& F, bool recheck) {
    const int B = h->B;
    auto kern = staged ? k_nodes_warm<true> : k_nodes_warm<false>;
    const long nth = (long)B * h->dc.NN;
    hipLaunchKernelGGL(kern, dim3((unsigned)((nth + 255) / 256)), dim3(256), traj_lds, h->stream, h->dc, B, seen.state, seen.control, h->d_sep, h->d_ts, h->d_prev_ts, h->d_solx,
                       h->d_nodes, F);
    if (recheck) {          // behind a node step: instances without a solution are known on the device only (k_nodes_recheck, predicated on the word k_node_finish filed)
        LAUNCH_CHECK(h);
        const int* cold = node_cold(h, h->node_parity);
        OrderOut Fr = order_out(h, nullptr); Fr.cnt = nullptr; Fr.slow = nullptr;      // (the launch order stays as k_nodes_warm filed it)
        auto rk = staged ? k_nodes_recheck<true> : k_nodes_recheck<false>;
        hipLaunchKernelGGL(rk, dim3((B + NODES_IPB - 1) / NODES_IPB), dim3(64), traj_lds, h->stream, h->dc, B, cold, seen.state, seen.control, h->d_toff, h->d_solved, h->d_sep,
                           h->d_ts, h->d_dt, h->d_prev_ts, h->d_solx, h->d_nodes, Fr, h->d_naux);
        LAUNCH_CHECK(h);
        hipLaunchKernelGGL(k_nodes_angles, dim3(64), dim3(256), 0, h->stream, h->dc, B, h->d_naux, h->d_nodes, cold);
    }
    LAUNCH_CHECK(h);
    return PG_OK;
}
// nodes + update_QP! as one pipelined launch (k_nodes_linearize), its predicated repair, and the rate rows of a control-parameter library
static int launch_nodes_pipelined(pg_handle* h, const Seen& seen, bool staged, size_t traj_lds, const OrderOut& F) {
    const int B = h->B;
    { int rc = launch_hji_rows_compute(h, seen); if (rc) return rc; }      // (M, b) of the safety row: read by the lanes that linearise interval 0
    const int lpi = h->lin_lpi, ipb = 64 / lpi;
    const int nbn = (B + NODES_IPB - 1) / NODES_IPB, nbt = (B + ipb - 1) / ipb;
    const size_t lds = traj_lds > 64 * 20 * sizeof(real) ? traj_lds : 64 * 20 * sizeof(real);
    auto kern = lpi == 1 ? (staged ? k_nodes_linearize<true, 1> : k_nodes_linearize<false, 1>) : (staged ? k_nodes_linearize<true, 2> : k_nodes_linearize<false, 2>);
#ifdef PG_F32
    if (lpi == 1 && B >= 6144) kern = staged ? k_nodes_linearize<true, 1, 2> : k_nodes_linearize<false, 1, 2>;      // (two waves per SIMD once the linearisation is more than one round of them)
#endif
    int nzf = (1024 - nbn + nbt - 1) / nbt;               // short-horizon intervals that go first: one wavefront for every SIMD the recurrence leaves free
    if (h->pipe_first > 0) nzf = h->pipe_first;
    if (nzf > h->dc.Ns) nzf = h->dc.Ns;
    if (nzf < 1) nzf = 1;
    // nodes after which the recurrence publishes its progress (each publication is a device-scope release, i.e. an L2 write-back): every third node of the
    // short horizon, every fifth of the long one (N = 30, Ns = 10: nodes 3, 6, 9, 14, 19, 24); the end of the recurrence always publishes
    unsigned long long pub = 0ull;
    for (int i = 1; i < h->dc.N - 2 && i < 63; i++)
        if (i <= h->dc.Ns ? i % h->pipe_pub_short == 0 : (i - h->dc.Ns) % h->pipe_pub_long == h->pipe_pub_long - 1) pub |= 1ull << i;
    if (h->pipe_fault) pub = 1ull << 63;                  // test hook: nothing is ever published (tests/test_gpu_api_contract.py)
    hipLaunchKernelGGL(kern, dim3((unsigned)(nbn + nbt * h->dc.N)), dim3(64), lds, h->stream, h->dc, B, nbn, nzf, pub, seen.state, seen.control, h->d_toff, h->d_solved, h->d_sep, h->d_ts,
                       h->d_dt, h->d_prev_ts, h->d_solx, h->d_nodes, F, h->d_naux, h->d_progress, h->d_Mb, h->d_qp, pipe_fault_word(h, nbn), pipe_fallbacks(h));
    LAUNCH_CHECK(h);
    // repair, queued unconditionally and predicated on the device: if any waiting wavefront of the launch above gave up (its fault word, zeroed by the
    // projection kernel of the step), the deferred angles and update_QP! of the WHOLE batch run launch per phase -- the same kernels on the same nodes, so the QP
    // data are the ones the pipeline would have written.  When nothing gave up the two launches return at once (~3 us together).
    {
        const int* flt = pipe_fault_word(h, nbn);
        hipLaunchKernelGGL(k_nodes_angles, dim3(64), dim3(256), 0, h->stream, h->dc, B, h->d_naux, h->d_nodes, flt);               // (small grids, striding over the work:
        const long nz = (long)B * h->dc.Ns * lpi, nr = (long)B * (h->dc.N - h->dc.Ns) * lpi;                                           //  an empty launch is cheap)
        const int nbz = (int)((nz + 63) / 64), nbr = (int)((nr + 63) / 64);
        auto ksplit = lpi == 1 ? k_linearize_split<1> : k_linearize_split<2>;
        hipLaunchKernelGGL(ksplit, dim3(512), dim3(64), 0, h->stream, h->dc, B, nbz, h->d_nodes, h->d_dt, h->d_Mb, h->d_qp, flt, nbz + nbr);
    }
    // Under a library (n_cp > 1) the pipelined launch has written the steering-rate rows of the QP data from DevCfg::cp -- pg_config.control, or the set of a
    // one-set library installed earlier: NOT any instance's set -- and k_rate_limits overwrites them per instance, on the same stream, behind the predicated repair
    // launches (which read the library themselves) and before anything reads the QP data.  Nothing may be queued between the two that consumes ddmin / ddmax.
    if (h->dc.n_cp > 1) {
        const long nt = (long)B * h->dc.N;
        hipLaunchKernelGGL(k_rate_limits, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, h->stream, h->dc, B, h->d_qp);
    }
    h->stat_pipelined++;
    LAUNCH_CHECK(h);
    return PG_OK;
}
// some instance is cold: the recurrence, one lane group per instance, then the deferred angles
static int launch_nodes_cold(pg_handle* h, const Seen& seen, bool staged, size_t traj_lds, const OrderOut& F) {
    const int B = h->B;
    auto kern = staged ? k_nodes<true> : k_nodes<false>;
    hipLaunchKernelGGL(kern, dim3((B + NODES_IPB - 1) / NODES_IPB), dim3(64), traj_lds, h->stream, h->dc, B, seen.state, seen.control, h->d_toff, h->d_solved, h->d_sep, h->d_ts,
                       h->d_dt, h->d_prev_ts, h->d_solx, h->d_nodes, F, h->d_naux);
    LAUNCH_CHECK(h);
    const long nn = (long)B * h->dc.NN;
    hipLaunchKernelGGL(k_nodes_angles, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, h->stream, h->dc, B, h->d_naux, h->d_nodes);
    LAUNCH_CHECK(h);
    return PG_OK;
}
static int launch_nodes(pg_handle* h, const Seen& seen, bool with_time_grid, bool& lin_done) {
    const int B = h->B;
    const bool recheck = h->node_recheck && !h->sg.capturing; h->node_recheck = false;
    const bool pipelined = with_time_grid && pipeline_applies(h);
    lin_done = pipelined;      // the pipelined branch (taken whenever pipeline_applies: coupled, some instance cold) writes this step's QP data too: update_and_solve skips update_QP!
    const bool file = h->dc.formulation != PG_DECOUPLED && h->dc.polish;
    int* const cnt = file ? order_cnt(h) : (int*)nullptr;                      // the two counters of the launch order start from zero: the projection kernel clears them (no memset of its own)
    int* const ctl = solve_ctl(h, CTL_TODO0);                                  // ... and the control words of this step's solve launches (launch_solve_coupled): the to-do counter it counts into
    h->cnt_cleared = !h->sg.capturing;
    if (with_time_grid) hipLaunchKernelGGL(k_project<true>, dim3((B * 64 + 255) / 256), dim3(256), 0, h->stream, h->dc, B, seen.state, h->d_sep, h->d_t0, h->d_ts, h->d_dt, h->d_prev_ts,
                                           pipelined ? h->d_progress : (int*)nullptr, (B + NODES_IPB - 1) / NODES_IPB + 1, cnt, ctl, h->solve_parity);      // (+ 1: the fault word of the pipelined launch)
    else hipLaunchKernelGGL(k_project<false>, dim3((B * 64 + 255) / 256), dim3(256), 0, h->stream, h->dc, B, seen.state, h->d_sep, (const double*)nullptr, (double*)nullptr, (double*)nullptr,
                            (double*)nullptr, (int*)nullptr, 0, cnt, ctl, h->solve_parity);
    LAUNCH_CHECK(h);
    const bool staged = h->dc.n_traj == 1 && h->traj_L <= 2048;
    const size_t traj_lds = staged ? (size_t)2 * h->traj_L * sizeof(real) : 0;
    const OrderOut F = order_out(h, file ? h->d_order : nullptr);
    h->order_B = file ? B : 0;
    if (h->dc.formulation == PG_DECOUPLED) return launch_nodes_decoupled(h, seen, staged, traj_lds);
    if (h->warm_B >= B) return launch_nodes_warm(h, seen, staged, traj_lds, F, recheck);
    if (pipelined) return launch_nodes_pipelined(h, seen, staged, traj_lds, F);
    return launch_nodes_cold(h, seen, staged, traj_lds, F);
}
static int launch_hji_lookup(pg_handle* h, int B, const real* x7_dev, real* out8_dev) {
    dim3 grid((unsigned)(((size_t)B * 16 + 255) / 256));
    if (h->hji.hv.cdims == 7) hipLaunchKernelGGL(k_hji_lookup<7>, grid, dim3(256), 0, h->stream, h->hji.hv, B, x7_dev, out8_dev);
    else if (h->hji.hv.cdims == 5) hipLaunchKernelGGL(k_hji_lookup<5>, grid, dim3(256), 0, h->stream, h->hji.hv, B, x7_dev, out8_dev);
    else hipLaunchKernelGGL(k_hji_lookup<3>, grid, dim3(256), 0, h->stream, h->hji.hv, B, x7_dev, out8_dev);
    LAUNCH_CHECK(h);
    return PG_OK;
}
// the safety row of update_QP! (coupled_lat_long.jl:345-346): relative state, value / gradient look-up, (M, b) per instance
// (two halves: the rows themselves read the measured states only and may run before the nodes -- the pipelined launch needs (M, b) when it linearises interval 0 --,
// the re-filed launch order needs the verdicts the nodes kernel filed)
static int launch_hji_rows_compute(pg_handle* h, const Seen& seen) {
    if (!h->hji.on) return PG_OK;
    const int B = h->B;
    hipLaunchKernelGGL(k_hji_relstate, dim3((B + 255) / 256), dim3(256), 0, h->stream, B, seen.state, h->d_other, h->d_x7);
    LAUNCH_CHECK(h);
    int rc = launch_hji_lookup(h, B, h->d_x7, h->d_vg8); if (rc) return rc;
    hipLaunchKernelGGL(k_hji_constraint, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, h->d_x7, h->d_vg8, seen.control, h->d_Mb);
    LAUNCH_CHECK(h);
    return PG_OK;
}
static int launch_hji_order(pg_handle* h, const Seen& seen) {
    if (!h->hji.on) return PG_OK;
    const int B = h->B;
    if (h->dc.polish && h->order_B == B) {              // launch order again, now that the safety rows are known (k_order_hji)
        const OrderOut F = order_out(h, h->d_order);
        HIPCHK(h, hipMemsetAsync(order_cnt(h), 0, ORDER_CNT_WORDS * sizeof(int), h->stream));
        hipLaunchKernelGGL(k_order_hji, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->dc, B, seen.control, h->d_Mb, F);
        LAUNCH_CHECK(h);
    }
    return PG_OK;
}
static int launch_hji_rows(pg_handle* h, const Seen& seen) {
    int rc = launch_hji_rows_compute(h, seen); if (rc) return rc;
    return launch_hji_order(h, seen);
}
#define PG_LIN_PAIR_MAX 1024
static int launch_linearize(pg_handle* h, int n) {
    // two lanes per (instance, interval) with four tangent directions each; small batches -- a handful of wavefronts whose duration is the latency of one lane --
    // spread the eight directions over four or eight lanes instead (same arithmetic per direction)
    // Large batches (several rounds of wavefronts): ONE lane per interval with all eight directions (k_linearize_split<1>) -- the fewest instructions per interval.
    // While every lane pair is resident at once (n <= 1024: 2 x 29 x 1024 / 64 = 928 wavefronts on 1024 SIMDs) the pair is the shorter chain.
    const int g_env = h->lin_groups;       // (-DPG_DIAG builds: option "diag_lin_groups" forces the lane arrangement; 0 otherwise)
#ifdef PG_F32
    const int G_small = 2;   // (fp32: the instantiations differ at rounding level -- the compiler contracts them differently --, so only the two classes n <= 1024 / above exist:
                             //  shards and whole batch agree bit for bit when they fall in the same class)
#else
    const int G_small = n <= 256 ? 8 : (n <= 512 ? 4 : 2);
#endif
    // fp64: bit-identical across K (tests/test_gpu_multiprocess.py steps 1024 = 2 x 512, 1001 = 501 + 500, 400 = 2 x 200; tests/test_gpu_full_size.py 4096 against 4 x 1024)
    const int G = (g_env == 1 || g_env == 2 || g_env == 4 || g_env == 8) ? g_env : ((n <= PG_LIN_PAIR_MAX || h->lin_lpi == 2) ? G_small : 1);
    if (G <= 2 && h->dc.Ns > 0 && h->dc.Ns < h->dc.N) {     // short-horizon intervals without the two uf directions (k_linearize_split)
        const long nz = (long)n * h->dc.Ns * G, nr = (long)n * (h->dc.N - h->dc.Ns) * G;
        const int nbz = (int)((nz + 63) / 64), nbr = (int)((nr + 63) / 64);
        auto ksplit = G == 1 ? k_linearize_split<1> : k_linearize_split<2>;
        hipLaunchKernelGGL(ksplit, dim3((unsigned)(nbz + nbr)), dim3(64), 0, h->stream, h->dc, n, nbz, h->d_nodes, h->d_dt, h->d_Mb, h->d_qp, (const int*)nullptr, 0);
        LAUNCH_CHECK(h);
        return PG_OK;
    }
    const long nl = (long)n * h->dc.N * G;
    const dim3 grid((unsigned)((nl + 63) / 64)), block(64);
    if (G == 1) hipLaunchKernelGGL(k_linearize<8>, grid, block, 0, h->stream, h->dc, n, h->d_nodes, h->d_dt, h->d_Mb, h->d_qp);
    else if (G == 8) hipLaunchKernelGGL(k_linearize<1>, grid, block, 0, h->stream, h->dc, n, h->d_nodes, h->d_dt, h->d_Mb, h->d_qp);
    else if (G == 4) hipLaunchKernelGGL(k_linearize<2>, grid, block, 0, h->stream, h->dc, n, h->d_nodes, h->d_dt, h->d_Mb, h->d_qp);
    else hipLaunchKernelGGL(k_linearize<4>, grid, block, 0, h->stream, h->dc, n, h->d_nodes, h->d_dt, h->d_Mb, h->d_qp);
    LAUNCH_CHECK(h);
    return PG_OK;
}
static int update_qp(pg_handle* h, const Seen& seen) {
    int rc;
    const int B = h->B; const DevCfg& C = h->dc;
    if (C.formulation == PG_DECOUPLED) {
        long nt = (long)B * C.N;
        // (a handle whose solver is k_solve_lat needs the packed stage records only: the embedded block is built when pg_get_qp asks for it)
        const int embed = (h->solve_lat && h->lat_pack_only) ? 0 : 1;
        hipLaunchKernelGGL(k_qp_dec, dim3((unsigned)((nt + 127) / 128)), dim3(128), 0, h->stream, h->dc, B, h->d_nodes, h->d_dt, h->d_qp, embed);
        LAUNCH_CHECK(h);
        h->qp_embedded = embed != 0; h->qp_stale = false;
        return PG_OK;
    }
    if ((rc = launch_hji_rows(h, seen))) return rc;
    return launch_linearize(h, B);
}
int pg_update_qp(pg_handle* h) { const int rc = check_ready(h); return rc ? rc : update_qp(h, seen_own(h)); }
static const int* solve_order(const pg_handle* h) { return (h->dc.polish && h->order_B == h->B) ? h->d_order : nullptr; }      // the launch order the nodes kernels of this step filed (likely slow instances first)
static void mark_solved(pg_handle* h) { if (h->B > h->warm_B) h->warm_B = h->B; }      // model_predictive_control.jl:76: solved = true for every instance of the batch
static dim3 lat_grid4(const pg_handle* h) { return dim3((unsigned)((h->B + 3) / 4)); }                              // four instances per wavefront
static size_t lat_lds1(const pg_handle* h) { return lat_lds_doubles(h->dc.N, 1) * sizeof(real); }                  // LDS of one instance per wavefront

// ---- the arrangements of the lateral solve (k_solve_lat), always the whole batch in index order; the plain one (one launch, four instances per wavefront) closes launch_solve_lat ----
// A batch in which every instance carries a previous solution (a closed loop after its first step) is solved in TWO launches: the warm attempts, then -- over the
// list the first launch leaves -- the cold solves of what they did not serve, packed four per wavefront again (see k_solve_lat).  Option "lat_split" = 0: one launch.
// (queues the warm attempts and leaves O in list mode for the plain launch behind them)
static int lat_solve_warm_attempts(pg_handle* h, hipStream_t st, SolveOut& O, unsigned long long* prof) {
    int* const n_list = solve_ctl(h, CTL_TODO0);
    HIPCHK(h, hipMemsetAsync(n_list, 0, sizeof(int), st)); h->stat_lat_two++;
    O.todo = h->d_todo; O.n_todo = n_list;
    launch_k_solve_lat<LAT_MEM_ANY, 16, 0>(h, lat_grid4(h), h->lat_lds, st, O, prof);
    LAUNCH_CHECK(h);
    O.todo = nullptr; O.n_todo = nullptr; O.list = h->d_todo; O.n_list = n_list;
    // (round 6) a list of up to `lat_single_max` instances is solved ONE instance per wavefront (see "small batches" below: 871 unserved instances of the benchmark
    // batch 1.5 instead of 2.1 ms); the host does not know the length, so both arrangements are queued and the device word picks one (an idle launch: ~4 us)
    if (h->lat_single_max > 0 && h->dc.N > 16) {
        const unsigned nb1 = (unsigned)(h->B < h->lat_single_max ? h->B : h->lat_single_max);
        O.list_lo = 0; O.list_hi = h->lat_single_max;
        launch_k_solve_lat<0, 64, 0>(h, dim3(nb1), lat_lds1(h), st, O, prof);
        LAUNCH_CHECK(h);
        O.list_lo = h->lat_single_max + 1; O.list_hi = 0;
    }
    return PG_OK;
}
// Small batches (round 6): with at most one wavefront per SIMD to fill anyway, every instance gets a wavefront of its own from the start -- the mapping of the resuming
// launch (lane = stage in the stage-parallel passes, one slot visit instead of four, the row state in registers): a trip costs 57 us instead of 84.  Not behind warm
// attempts (their launches are a round or two of the polish: four per wavefront is the cheaper shape there).
static int lat_solve_one_per_wavefront(pg_handle* h, hipStream_t st, const SolveOut& O, unsigned long long* prof) {
    launch_k_solve_lat<0, 64, 0>(h, dim3((unsigned)h->B), lat_lds1(h), st, O, prof);
    LAUNCH_CHECK(h); h->stat_lat_single++;
    return PG_OK;
}
// Straggler hand-over (round 6, see k_solve_lat): a batch that starts cold interior points runs as TWO launches -- the first stops at a trip boundary once at most
// `lat_hand_target` instances of the batch are unfinished and files them, the second resumes those, ONE instance per wavefront (option "lat_handover" = 0: one launch
// as in round 5.  Measured and removed: resuming four per wavefront again, i.e. compaction only -- 3.34 against 3.25 ms for the single launch).  Only where the row
// state lives in the workspace (N > 16, or option "lat_workspace"), and not behind the warm attempts' own two launches.
static int lat_solve_handover(pg_handle* h, hipStream_t st, SolveOut O, unsigned long long* prof) {
    int* const ctl = solve_ctl(h, CTL_TODO0);
    HIPCHK(h, hipMemsetAsync(ctl, 0, (CTL_HAND_BACK + 1) * sizeof(int), st)); h->stat_lat_hand++;      // [0] listed from the front, [1] finished instances, [2] listed from the back
    O.todo = h->d_todo; O.n_todo = ctl; O.hand_mode = 1;
    // When to stop the first launch.  Default: after a fixed number of trips (16 with the wall rows, 11 without: mean interior-point iterations + 2..3 on the benchmark
    // batches) -- a rule that depends on the data only, so that the same call gives the same bits.  Option "lat_hand_target" > 0 stops when that few instances of the
    // batch are unfinished instead (counted on the device: adapts to the batch -- vail + walls 2.09 against 2.19 ms -- but WHEN a wavefront sees the count is a matter
    // of timing, and an instance resumed one trip earlier or later ends 1e-8 away: two verified KKT points of the same QP, not the same bits).
    O.hand_cap = h->lat_hand_cap > 0 ? h->lat_hand_cap : ((h->lat_hand_target > 0 || h->lat_hand_work > 0) ? 0 : (h->dc.walls ? 16 : 11)); O.hand_target = h->lat_hand_target; O.hand_min = h->lat_hand_min; O.hand_done = solve_ctl(h, CTL_TODO1); O.hand_work = h->lat_hand_work; O.hand_w0 = h->lat_hand_w0;
    O.hand_r = h->d_hand_r; O.hand_i = h->d_hand_i;
    launch_k_solve_lat<1, 16, 1>(h, lat_grid4(h), h->lat_lds, st, O, prof);
    LAUNCH_CHECK(h);
    O.todo = nullptr; O.n_todo = nullptr; O.list = h->d_todo; O.n_list = ctl; O.hand_mode = 2;
    launch_k_solve_lat<0, 64, 2>(h, dim3((unsigned)h->B), lat_lds1(h), st, O, prof);          // one wavefront per listed instance; blocks beyond the list return at once
    LAUNCH_CHECK(h);
    return PG_OK;
}
// lateral formulation: four instances per wavefront unless an arrangement above says otherwise
static int launch_solve_lat(pg_handle* h, hipStream_t st, unsigned long long* lat_prof) {
    SolveOut O = solve_out(h, nullptr);
#ifdef PG_DIAG
    if (h->dc.dbg_poison) {      // (every byte 0xFF: NaN in both precisions)
        const size_t cap = (size_t)h->cfg.batch_capacity;
        if (h->d_lat_ws) HIPCHK(h, hipMemsetAsync(h->d_lat_ws, 0xFF, lat_ws_bytes(cap), st));
        if (h->d_lat_aux) HIPCHK(h, hipMemsetAsync(h->d_lat_aux, 0xFF, (cap + 1) * 64 * LAT_AUX * sizeof(real), st));
        if (h->d_lat_spc) HIPCHK(h, hipMemsetAsync(h->d_lat_spc, 0xFF, lat_spc_bytes((int)cap, h->dc.N), st));
    }
#endif
    const bool two = h->split_lat && h->dc.polish && h->dc.warm_polish && h->dc.lat_warm_rounds > 0 && h->warm_B >= h->B && !lat_prof && !h->sg.capturing;
    if (two) { const int rc = lat_solve_warm_attempts(h, st, O, lat_prof); if (rc) return rc; }
    else if (!h->sg.capturing && h->warm_B < h->B && h->B <= h->lat_single_max && h->dc.N > 16) return lat_solve_one_per_wavefront(h, st, O, lat_prof);
    else if (!h->sg.capturing && h->lat_handover != 0 && h->lat_mem && h->B >= h->lat_hand_batch) return lat_solve_handover(h, st, O, lat_prof);
    launch_k_solve_lat<LAT_MEM_ANY, 16, 0>(h, lat_grid4(h), h->lat_lds, st, O, lat_prof);
    LAUNCH_CHECK(h);
    return PG_OK;
}
// coupled formulation (and the lateral one embedded in it), one wavefront per instance: `n` instances, the whole batch in index order (order == nullptr) or the
// sub-range order[0..n) of the launch order
static int launch_solve_coupled(pg_handle* h, hipStream_t st, const int* order, int n, DirectOut& direct) {
    SolveOut O = solve_out(h, order);
    take_direct(O, direct);
    if (h->solve_ring) launch_k_solve<false, true, false>(h, st, n, O);
    else if (h->split_solve && h->dc.polish && (h->dc.cold_guess > 0 || h->dc.warm_polish) && !h->hji.on && !h->sg.capturing) {
        // Two launches: the rounds-only instantiation (no scratch: the interior point's state and code are not in it) serves the instances an active-set attempt
        // verifies -- all of them on the tracking batches --; what it leaves (SolveOut::todo) goes through the full kernel in list mode, its blocks returning at once
        // when the list is empty.  Not with a safety row installed: there the instances whose row is violated NEED the interior point (9-17 % of config 3), and in one
        // kernel they start first (launch order) instead of after everyone else.  For the same reason a launch of this handle that has left something for the interior
        // point changes the NEXT launch: the full kernel then takes the whole batch in its launch order and the rounds-only kernel returns at once -- an instance that needs
        // the interior point runs it right behind its rounds, under the rest of the batch, instead of after it (`vail`, two such instances of 4096: 1.38 ms per cold step
        // split, 1.07 ms in one kernel).  The full kernel counts its interior-point instances the same way, so the split returns when they are gone.
        // The decision is taken ON THE DEVICE from the previous launch's count (SolveOut::mode), i.e. from stream-ordered state only: the same sequence of calls gives the
        // same launches whatever the host's timing (round 4 read a pinned copy of the count that an asynchronous copy filled "whenever it arrived").  Two counters are used
        // alternately -- this launch counts into one while the other still holds the previous launch's count --; the projection kernel of the step zeroes the one about to be
        // used (a solve without a nodes phase in front -- replayed QPs -- zeroes it here).
        int* const cnt = solve_ctl(h, CTL_TODO0 + h->solve_parity); const int* const prev = solve_ctl(h, CTL_TODO0 + (h->solve_parity ^ 1));
        if (!h->cnt_cleared) HIPCHK(h, hipMemsetAsync(cnt, 0, sizeof(int), st));
        h->cnt_cleared = false; h->solve_parity ^= 1; h->stat_split++;
        O.todo = h->d_todo; O.n_todo = cnt; O.mode = prev; O.n_whole = solve_ctl(h, CTL_WHOLE);
        launch_k_solve<false, false, false, false>(h, st, n, O);
        LAUNCH_CHECK(h);
        SolveOut O2 = O; O2.todo = nullptr; O2.list = h->d_todo; O2.n_list = cnt;      // (order_in stays: the whole-batch mode uses the launch order)
        launch_k_solve<false, false, false, true>(h, st, n, O2);
    }
    else {
        h->stat_single++;
        launch_k_solve<false, false, false>(h, st, n, O);
    }
    LAUNCH_CHECK(h);
    return PG_OK;
}
static int launch_solve(pg_handle* h, hipStream_t st, const int* order, int n, DirectOut& direct) { return h->solve_lat ? launch_solve_lat(h, st, nullptr) : launch_solve_coupled(h, st, order, n, direct); }
static int solve_qp(pg_handle* h, DirectOut& direct) {
    int rc;
    if (h->qp_stale) { h->err = "pg_solve: the lateral solver was switched (pg_set_option \"lateral_solver\") after the last update_QP!: call pg_update_qp first"; return PG_ERR_STATE; }
    if ((rc = launch_solve(h, h->stream, solve_order(h), h->B, direct))) return rc;
    mark_solved(h);
    return PG_OK;
}
int pg_solve(pg_handle* h) { DirectOut none; const int rc = check_ready(h); return rc ? rc : solve_qp(h, none); }
// update_QP! + solve! of one step.  For the coupled formulation with N <= 32 both run in ONE kernel (k_solve<.., FUSE = true>): the wavefront that solves an instance
// first linearises it (two lanes per interval = 60 of its 64 lanes), writes the QP data (still readable through pg_get_qp) and goes on to the solve.  k_solve ends
// with its slowest wave -- an instance that needs the interior point takes 0.5 ms whatever the batch size -- and as a separate kernel it leaves part of the machine
// idle for the last third of its run; fused, the SIMDs that are done with their quick instances linearise and solve the next ones meanwhile.  Same device
// functions, same per-instance arithmetic: results are bit-identical to the two-kernel sequence.  MEASURED (B = 4096, MI355X): 1.23 vs 1.30 ms per cold step on
// skidpadoval, but 1.52 vs 1.40 on vail and 1.13 vs 1.05 on EastPaddock -- the linearisation runs ~15 % slower inside the big kernel (the waves of a CU are then
// spread over 85 KB of code instead of sharing one loop in the 64 KB instruction cache), and where no straggler tail exists there is nothing to win.  Closed
// loops were 5-8 % faster fused as long as a few instances per step fell back to the interior point; with those stragglers gone (the polish rules of k_solve)
// the two-kernel sequence wins there too (0.91 vs 0.99, 1.06 vs 1.11, 0.87 vs 0.98 ms per closed-loop step).  Hence OFF by default (pg_set_fusion:
// 0 never, 1 always, 2 for all-warm batches of >= 1024 instances).
static int update_and_solve(pg_handle* h, const Seen& seen, bool lin_done, hipEvent_t after_update, DirectOut& direct) {
    const bool want = h->fuse == 1 || (h->fuse == 2 && h->warm_B >= h->B && h->B >= 1024);
    const bool fused = !lin_done && want && h->dc.formulation != PG_DECOUPLED && !h->solve_ring && 2 * h->dc.N <= 64;
    const int rc = lin_done ? launch_hji_order(h, seen) : (fused ? launch_hji_rows(h, seen) : update_qp(h, seen));
    if (rc) return rc;
    if (after_update) HIPCHK(h, hipEventRecord(after_update, h->stream));
    if (!fused) return solve_qp(h, direct);
    SolveOut O = solve_out(h, solve_order(h));
    take_direct(O, direct);
    launch_k_solve<false, false, true>(h, h->stream, h->B, O);
    LAUNCH_CHECK(h);
    mark_solved(h);
    return PG_OK;
}
#ifdef PG_DIAG
// debug (-DPG_DIAG library only; not part of the public header, not in the shipped libraries -- nor are the PROF instantiations of k_solve it launches): per-phase shader-clock
// cycles of one solve launch, out [B][6] = (stage assembly+step, sync, matrix pass, vector passes, forward passes, prologue); diagnostic build of the kernel, never timed
int pg_debug_solve_cycles(pg_handle* h, unsigned long long* out) {
    int rc = check_ready(h); if (rc) return rc;
    CallBufs D; unsigned long long* d = nullptr;
    HIPCHK(h, D.alloc(d, (size_t)h->B * 9 + 1024));
    HIPCHK(h, hipMemset(d, 0, ((size_t)h->B * 9 + 1024) * 8));
    SolveOut O = solve_out(h, solve_order(h));            // (the launch order pg_solve would use: the timeline is the product's)
    if (h->solve_lat) { if ((rc = launch_solve_lat(h, h->stream, d))) return rc; }
    else if (h->solve_ring) launch_k_solve<true, true, false>(h, h->stream, h->B, O, d);
    else if (h->debug_timeline) {      // the product's kernel (the rounds-only instantiation of the split launch): timeline only
        int* const cnt = solve_ctl(h, CTL_TIMELINE);
        HIPCHK(h, hipMemsetAsync(cnt, 0, sizeof(int), h->stream));
        O.todo = h->d_todo; O.n_todo = cnt;
        launch_k_solve<false, false, false, false>(h, h->stream, h->B, O, d);
    }
    else launch_k_solve<true, false, false>(h, h->stream, h->B, O, d);
    LAUNCH_CHECK(h);
    HIPCHK(h, hipMemcpy(out, d, ((size_t)h->B * 9 + 1024) * 8, hipMemcpyDeviceToHost));      // out: [B][6] cycles + 1024-double trace of the "diag_instance" instance + [B][3] timeline (k_solve: entry, exit on the 100 MHz wall clock, HW_ID | XCC_ID << 32)
    return PG_OK;
}
#endif
#ifdef PG_TIMELINE
// debug (timeline build only, not part of the public header): per block of the last pipelined launch (entry, end of the wait, exit on the 100 MHz wall clock; interval, 1000 = a nodes block)
extern "C" int pg_debug_pipeline_timeline(pg_handle* h, unsigned long long* out, int n_blocks) {
    int rc = check_ready(h); if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nl_timeline), (size_t)(n_blocks < 8192 ? n_blocks : 8192) * 8 * sizeof(unsigned long long)));
    return PG_OK;
}
#endif
int pg_get_next_control_dev(pg_handle* h, void* u_out_dev) {
    int rc = check_ready(h); if (rc) return rc;
    if (u_out_dev) HIPCHK(h, hipMemcpyAsync(u_out_dev, h->d_u, (size_t)h->B * 3 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));
    return PG_OK;
}
int pg_get_next_control(pg_handle* h, double* u_out) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, u_out, "u_out is null");
    return down(h, u_out, h->d_u, (size_t)h->B * 3);
}
// ros_integration.jl:114-124: the HJI fallback policy takes the wheel when the value function says the situation is unsafe
static int launch_hji_policy(pg_handle* h, int use_policy) {
    const int B = h->B;
    if (h->dc.formulation != PG_COUPLED) { h->err = "the HJI policy belongs to the coupled controller (ros_integration.jl:56,114)"; return PG_ERR_STATE; }
    if (!h->hji.on) {                      // no grid: V = +Inf everywhere, the MPC control always wins
        HIPCHK(h, hipMemcpyAsync(h->d_pol_u, h->d_u, (size_t)B * 3 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_pol_src, 0, (size_t)B * sizeof(int), h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_pol_u2, 0, (size_t)B * 2 * sizeof(real), h->stream));
        return PG_OK;
    }
    hipLaunchKernelGGL(k_hji_policy, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, use_policy, h->d_x7, h->d_vg8, h->d_toff, h->d_u, h->d_pol_u2, h->d_pol_u, h->d_pol_src);
    LAUNCH_CHECK(h);
    return PG_OK;
}
int pg_get_next_control_hji_dev(pg_handle* h, int32_t use_hji_policy, void* u_out_dev, int32_t* source_dev) {
    int rc = check_ready(h); if (rc) return rc;
    if ((rc = launch_hji_policy(h, use_hji_policy))) return rc;
    if (u_out_dev) HIPCHK(h, hipMemcpyAsync(u_out_dev, h->d_pol_u, (size_t)h->B * 3 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));
    if (source_dev) HIPCHK(h, hipMemcpyAsync(source_dev, h->d_pol_src, (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    return PG_OK;
}
int pg_get_next_control_hji(pg_handle* h, int32_t use_hji_policy, double* u_out, int32_t* source, double* u2_policy) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, u_out, "u_out is null");
    if ((rc = launch_hji_policy(h, use_hji_policy))) return rc;
    if ((rc = down(h, u_out, h->d_pol_u, (size_t)h->B * 3)) || (rc = down_raw(h, source, h->d_pol_src, (size_t)h->B * sizeof(int))) ||
        (rc = down(h, u2_policy, h->d_pol_u2, (size_t)h->B * 2))) return rc;
    return PG_OK;
}
int pg_step_dev(pg_handle* h, void* u_out_dev) {
    int rc = check_ready(h); if (rc) return rc;
    const bool ev = !h->sg.capturing && h->phase_timing != 0;     // (a step that is being captured into a graph carries no timing events; option "phase_timing" = 0: none at all)
    if (ev) HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    const Seen seen = seen_own(h); bool lin_done; DirectOut direct{(real*)u_out_dev};
    if ((rc = launch_nodes(h, seen, true, lin_done))) return rc;
    if (ev) HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if ((rc = update_and_solve(h, seen, lin_done, ev ? h->ev[2] : nullptr, direct))) return rc;       // (chunked: ev[2] marks the end of the LAST update_QP chunk; earlier solve chunks run under it)
    if (!direct.written && (rc = pg_get_next_control_dev(h, u_out_dev))) return rc;      // (k_solve writes the caller's array itself; the lateral kernel's controls are copied)
    if (ev) HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
    h->timing_valid = ev;
    return PG_OK;
}
// the loop's clock (:87): t takes the elements of 0:dt:trajectory.t[end], here shifted by each instance's start time.  A call continues the clock of the previous one
// (same dt, same path end, no pg_set_inputs in between); otherwise it restarts from the times the inputs carry (and so does the safety summary)
// the compute calls of one closed-loop step (model_predictive_control.jl:90-93; the time grid rides in the projection launch): fusion, pipelining and the split solve as pg_step_dev has them
static int step_compute(pg_handle* h, const Seen& seen) {
    bool lin_done; DirectOut none;
    const int rc = launch_nodes(h, seen, true, lin_done);
    return rc ? rc : update_and_solve(h, seen, lin_done, nullptr, none);
}
// the arguments the rollouts share (`who`: the entry point, for the message; a rollout without a human passes mode 0)
// human_lib: the rollout runs under a human library -- the sets decide, and the script is wanted exactly when one of them has mode 2
static int check_rollout_args(pg_handle* h, const char* who, int32_t steps, double dt, int32_t human_mode, const void* human_u_dev, bool human_lib) {
    const std::string w(who);
    REQUIRE(h, steps >= 1 && dt > 0.0, w + ": steps >= 1 and dt > 0 required");
    REQUIRE(h, human_mode >= 0 && human_mode <= 2, w + ": human_mode is 0 (hold), 1 (worst case) or 2 (scripted)");
    if (human_lib) REQUIRE(h, !h->human.script || human_u_dev, w + ": a set of the human library has mode 2 and needs human_u_dev [steps][B][2]");
    else REQUIRE(h, human_mode != 2 || human_u_dev, w + ": human_mode 2 needs human_u_dev [steps][B][2]");
    return PG_OK;
}
// what a rollout needs beyond check_ready: a plant library of several sets wants an index that covers the batch; the tracking summary its buffers
static int rollout_ready(pg_handle* h, bool human_lib) {
    int rc;
    const size_t cap = cap_of(h);
    if (index_covers(h, h->plants)) return PG_ERR_STATE;
    if (human_lib) {                                             // (a rollout with another car, under a human library)
        auto& U = h->human;
        if (index_covers(h, U.lib)) return PG_ERR_STATE;
        if ((rc = ensure(h, U.u, cap * 2)) || (rc = ensure(h, U.n, cap * 2)) || (rc = U.streams.sync(h))) return rc;
    }
    if (h->tracking && ((rc = ensure(h, h->d_track, cap * 6)) || (rc = ensure(h, h->d_track_i, cap * 2)))) return rc;
    if (h->sensor.lib.on()) {
        if (index_covers(h, h->sensor.lib)) return PG_ERR_STATE;
        if ((rc = ensure(h, h->sensor.meas, cap * 6)) || (rc = h->sensor.streams.sync(h))) return rc;
    }
    if (index_covers(h, h->estimator.lib)) return PG_ERR_STATE;
    // (under either of the two the controller's (s, e) is not the truth's: launch_track projects the true state once more)
    if (h->tracking && (h->sensor.lib.on() || h->estimator.lib.on()) && (rc = ensure(h, h->sensor.sep_true, cap * 4))) return rc;
    if (h->actuator.lib.on()) {
        auto& A = h->actuator;
        if (index_covers(h, A.lib)) return PG_ERR_STATE;
        if ((rc = ensure(h, A.pos, cap * 3)) || (rc = ensure(h, A.ring, (size_t)PG_ACT_MAX_DELAY * cap * 3)) || (rc = ensure(h, A.plant_u, cap * 3)) || (A.feedback && (rc = ensure(h, A.seen, cap * 3)))) return rc;
    }
    if (h->disturbance.lib.on()) {
        auto& D = h->disturbance;
        if (index_covers(h, D.lib)) return PG_ERR_STATE;
        if ((rc = ensure(h, D.n, cap * 2)) || (rc = ensure(h, D.w, cap * 4))) return rc;
        if (!D.veh) {                                            // (the controller's vehicle as the kernels hold it: DevCfg's record, bit for bit)
            if ((rc = ensure(h, D.veh, 1))) return rc;
            HIPCHK(h, hipMemcpy(D.veh, &h->dc.veh, sizeof(DevVehicle), hipMemcpyHostToDevice));
        }
        if ((rc = D.streams.sync(h))) return rc;
    }
    if (h->route.lib.on()) {
        auto& U = h->route;
        if (h->dc.n_traj < 2) { h->err = "a route library is installed but the handle has no trajectory library of at least two trajectories (pg_set_trajectories)"; return PG_ERR_STATE; }
        if (h->traj_idx.covered() < h->B || !h->traj_idx.d) { h->err = "a route library is installed but pg_set_trajectory_index does not cover the batch (it is every instance's home)"; return PG_ERR_STATE; }
        for (const pg_route& r : U.lib.sets) for (const pg_route_event& e : r.ev)      // (here, not at the install: the trajectory library may have been replaced since)
            if (e.step >= 0 && e.target_mode == PG_ROUTE_ABSOLUTE && e.target >= h->dc.n_traj) {
                h->err = "a route set has an absolute target " + std::to_string(e.target) + " outside the installed trajectory library of " + std::to_string(h->dc.n_traj); return PG_ERR_STATE;
            }
        if (index_covers(h, U.lib)) return PG_ERR_STATE;
        if ((rc = ensure(h, U.fired, cap * 2)) || (rc = ensure(h, U.t_at, cap)) || (rc = ensure(h, U.e_at, cap))) return rc;
    }
    return PG_OK;
}
// The one-shot history registrations a rollout call consumes (pg_set_*_history_dev), taken from the handle when the call starts
struct RolloutHist { HistSlot measured, applied, command, disturbance, estimated, human; int* route = nullptr; int route_steps = 0; };
static RolloutHist take_histories(pg_handle* h) {
    RolloutHist r{h->sensor.hist.take(), h->actuator.applied_hist.take(), h->actuator.command_hist.take(), h->disturbance.hist.take(), h->estimator.hist.take(), h->human.hist.take(),
                  h->route.hist, h->route.hist_steps};
    h->route.hist = nullptr; h->route.hist_steps = 0;
    return r;
}
// the disturbance library (installed: k_disturb joins a rollout step, and the step's last launch is the <DistW> instantiation of the library kernel).
// The top of a rollout step under a library: w of clock step `step` into disturbance.w, the gust state advanced (fresh: the host knows that no state of step - 1 exists)
static int launch_disturb(pg_handle* h, int step, int k, double dt, const HistSlot& hist) {
    const int B = h->B; auto& D = h->disturbance;
    const DisturbanceLib lib{D.lib.d, D.lib.index(), D.streams.d, (unsigned long long)D.streams.seed, D.n, D.w};
    hipLaunchKernelGGL(k_disturb, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, step, (int)D.fresh, (real)dt, lib, hist.at(k, B, 4));
    LAUNCH_CHECK(h);
    D.fresh = false; D.valid = true; D.steps_stat++;
    return PG_OK;
}
// the human library (installed: k_human joins a step of the rollouts that have another car, ahead of the plant launch, which is handed human.u as the script of its human
// mode 2).  Behind the compute calls of a rollout step under a library (mode 1 reads the step's d_x7, d_vg8): (omega, a) of clock step `step` into human.u, the driver's state
// advanced (fresh: the host knows that no state of step - 1 exists).  script: human_u_dev of the call, [steps][B][2] or nullptr
static int launch_human(pg_handle* h, int step, int k, double dt, const void* script, const HistSlot& hist) {
    const int B = h->B; auto& U = h->human;
    const HumanLib lib{U.lib.d, U.lib.index(), U.streams.d, (unsigned long long)U.streams.seed, U.n, U.u};
    hipLaunchKernelGGL(k_human, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc.veh, B, step, (int)U.fresh, has_hji_row(h), (real)dt, lib, (const real*)h->d_x7,
                       (const real*)h->d_vg8, hist_at((const real*)script, k, B, 2), hist.at(k, B, 2));
    LAUNCH_CHECK(h);
    U.fresh = false; U.valid = true; U.steps_stat++;
    return PG_OK;
}
// the actuator library (installed: k_actuate and the copy-back join a rollout step).  The top of a rollout step under a library: a_k of clock step `step` from the command
// the handle's control buffer holds, into actuator.pos, plant_u (and seen)
static int launch_actuate(pg_handle* h, int step, int k, double dt, const HistSlot& applied, const HistSlot& command) {
    const int B = h->B; auto& A = h->actuator;
    const ActuatorLib lib{A.lib.d, A.lib.index(), A.pos, A.ring, A.plant_u, A.feedback ? A.seen : (real*)nullptr, (int)cap_of(h)};
    hipLaunchKernelGGL(k_actuate, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, step, (int)A.fresh, (real)dt, lib, h->d_control, applied.at(k, B, 3), command.at(k, B, 3));
    LAUNCH_CHECK(h);
    A.fresh = false;
    return PG_OK;
}
// the controller's side of one rollout step: the node gate (node rollout) and the compute calls, on the view built here.  State: under a sensor library k_measure writes the
// measured state of clock step `step` and the view names that; under an estimator library k_estimate follows (on the measured state, or on the true one without a sensor
// library) and the view names estimator.x -- the gates, the projection, the nodes, the QP's q_curr, the HJI relative state and the policy selection all follow it; without
// either, the true state.  Control: `control`, as the rollout hands it in (the command, or actuator.seen).  The summary, the records and the plant never see the view
static int node_gate(pg_handle* h, const Seen& seen, const uint8_t* pre_flag);
// the route library (installed: k_route joins the rollout steps whose clock step carries an event in some installed set, and every step of a call that records the route).
// Behind k_measure / k_estimate -- a PROJECT event projects the state the controller is handed -- and ahead of the gate and the compute calls, which then read the new
// index, the new offset and the cleared solved flag.  On an event step the host takes the launches of a batch with a cold instance, exactly as control_sets_changed does
// (k_nodes / k_nodes_linearize read solved[b] per instance); mark_solved makes the batch warm again behind the step's solve
static int launch_route(pg_handle* h, const Seen& seen, int step, int* hist) {
    auto& U = h->route;
    const bool event = U.event_at(step);
    if (!event && !hist) return PG_OK;
    const int B = h->B;
    const RouteLib lib{U.lib.d, U.lib.index(), h->traj_idx.d, U.fired, U.fired + cap_of(h), U.t_at, U.e_at};
    hipLaunchKernelGGL(k_route, dim3((B * 64 + 255) / 256), dim3(256), 0, h->stream, h->dc, B, step, lib, seen.state, (const double*)h->d_t0, h->d_toff, h->d_solved, h->d_wfail, hist);
    LAUNCH_CHECK(h);
    U.steps_stat++;
    if (event) { h->warm_B = 0; h->order_B = 0; }
    return PG_OK;
}
// The clock restarted (route.fresh): every instance back on its home trajectory, nothing fired.  Once per restart, at the start of a rollout call: the copy waits for the stream
static int route_start(pg_handle* h) {
    auto& U = h->route;
    if (!U.lib.on() || !U.fresh) return PG_OK;
    const size_t cap = cap_of(h);
    std::vector<int> home(cap, 0), last(cap, -1);
    for (size_t b = 0; b < h->traj_idx.host.size(); b++) home[b] = h->traj_idx.host[b];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->traj_idx.d, home.data(), cap * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(U.fired, 0, cap * sizeof(int)));
    HIPCHK(h, hipMemcpy(U.fired + cap, last.data(), cap * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(U.t_at, 0xFF, cap * sizeof(double)));      // (all-ones: a NaN in either element type)
    HIPCHK(h, hipMemset(U.e_at, 0xFF, cap * sizeof(real)));
    U.fresh = false;
    return PG_OK;
}
static int rollout_compute(pg_handle* h, const real* control, int step, int k, double dt, const HistSlot& measured, const HistSlot& estimated, int* route_hist, bool gate, const uint8_t* pre_flag) {
    int rc;
    auto& S = h->sensor; auto& E = h->estimator;
    const int B = h->B;
    Seen seen{h->d_state, control};
    if (S.lib.on()) {
        const SensorLib lib{S.lib.d, S.lib.index(), S.streams.d, (unsigned long long)S.streams.seed};
        hipLaunchKernelGGL(k_measure, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, step, lib, h->d_state, S.meas, measured.at(k, B, 6));
        LAUNCH_CHECK(h);
        S.valid = true; S.steps_stat++;
        seen.state = S.meas;
    }
    if (E.lib.on()) {
        const EstimatorLib lib{E.lib.d, E.lib.index(), E.x, E.u};
        hipLaunchKernelGGL(k_estimate, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, (int)E.fresh, (real)(dt / h->dc.nsub), lib, seen.state, seen.control, estimated.at(k, B, 6));
        LAUNCH_CHECK(h);
        E.fresh = false; E.valid = true; E.steps_stat++;
        seen.state = E.x;
    }
    if (h->route.lib.on() && (rc = launch_route(h, seen, step, route_hist))) return rc;
    if (gate && (rc = node_gate(h, seen, pre_flag))) return rc;
    return step_compute(h, seen);
}
// the plant library as the library kernels (k_*_lib) take it (the host knows whether one is installed: that alone picks the kernel)
static PlantLib plant_lib(const pg_handle* h) { return PlantLib{h->plants.d, h->plants.index()}; }
// the step's tracking summary (option "tracking_summary"): behind the projection of this step (step_compute), ahead of the kernel that moves the plant
static int launch_track(pg_handle* h, int step) {
    if (!h->tracking) { h->track_fresh = true; return PG_OK; }      // (off: no launch; steps that went unseen must not be continued when it comes back on)
    const int B = h->B;
    const real* sep = h->d_sep;
    if (h->sensor.lib.on() || h->estimator.lib.on()) {      // d_sep holds the projection of the MEASURED / ESTIMATED state (the node publishes its (s, e)): the summary describes the true one, projected once more
        hipLaunchKernelGGL(k_project<false>, dim3((B * 64 + 255) / 256), dim3(256), 0, h->stream, h->dc, B, h->d_state, h->sensor.sep_true, (const double*)nullptr, (double*)nullptr, (double*)nullptr,
                           (double*)nullptr, (int*)nullptr, 0, (int*)nullptr, (int*)nullptr, 0);
        LAUNCH_CHECK(h);
        sep = h->sensor.sep_true;
    }
    hipLaunchKernelGGL(k_track, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, (int)h->track_fresh, step, h->d_state, sep, h->d_track, h->d_track_i, h->d_track_i + cap_of(h));
    LAUNCH_CHECK(h);
    h->track_fresh = false;
    return PG_OK;
}
static int clock_start(pg_handle* h, double dt) {
    if (h->sim_idx == 0 || h->sim_dt != dt || h->sim_tend != h->traj_t_end) {
        HIPCHK(h, hipMemcpyAsync(h->d_tstart, h->d_t0, (size_t)h->B * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        h->sim_clk = jl_colon(0.0, dt, h->traj_t_end); h->sim_idx = 1; h->sim_dt = dt; h->sim_tend = h->traj_t_end; restart_on_clock(h);
    }
    return PG_OK;
}
static int node_start(pg_handle* h, double dt);
}  // extern "C" (the rollouts' templates have C++ linkage)
// the last launch of a rollout step, one lane per instance: `uniform`, or the family's library kernel -- under a plant library its instantiation `with_plant`, the same
// arguments and the library behind them; under a disturbance library its instantiation `with_dist` (W = DistW), the plant library (without one: the library of one made of
// the handle's own vehicle) and w of this step behind them
template <class K, class KP, class KD, class... A>
static void launch_plant_step(pg_handle* h, K uniform, KP with_plant, KD with_dist, const A&... args) {
    const dim3 grid((h->B + 63) / 64), block(64);
    if (h->disturbance.lib.on()) hipLaunchKernelGGL(with_dist, grid, block, 0, h->stream, args..., h->plants.on() ? plant_lib(h) : PlantLib{h->disturbance.veh, nullptr}, (const real*)h->disturbance.w);
    else if (h->plants.on()) hipLaunchKernelGGL(with_plant, grid, block, 0, h->stream, args..., plant_lib(h));
    else hipLaunchKernelGGL(uniform, grid, block, 0, h->stream, args...);
}
// The rollouts' shared driver.  Prologue, in this order: the one-shot history registrations (measured, applied / command, disturbance, estimated, human, route) are taken (THIS call consumes them, also when it fails below), check_ready,
// the entry point's own precondition (coupled_only: the message for a lateral handle, nullptr: none), the shared arguments, rollout_ready, the node's buffers (node: the
// rollout of the node callback, its steps run behind the gate with pre_flag [steps][B]), the loop's clock (:87), the route library's return home when that clock restarted.  Per step: records ahead of the compute calls, the
// controller's side (:90-93, rollout_compute), the tracking summary, the clock index, then finish: the step's last launch, which moves the plant
static const char* const ACTUATOR_NODE_REFUSAL = "an actuator library is installed and the node callback is outside its scope (k_node_finish keeps message and applied command "
                                                 "apart and leaves `applied` unwritten for a gated-out instance: no plain hand-back of the next command); pg_clear_actuator_sets first";
// one step as records and finish see it: k within the call, the clock step (index of the clock element t0 held -- steps continue across calls), the control they read
struct RolloutStep { int k, step; real* control; };
struct RolloutArgs { const char* who; int32_t steps; double dt; int32_t human_mode; const void* human_u; const char* coupled_only; bool node; const uint8_t* pre_flag; bool other_car; };
template <class Records, class Finish>
static int rollout(pg_handle* h, const RolloutArgs& a, Records records, Finish finish) {
    const RolloutHist hist = h ? take_histories(h) : RolloutHist{};
    int rc = check_ready(h); if (rc) return rc;
    if (a.coupled_only && h->dc.formulation != PG_COUPLED) { h->err = a.coupled_only; return PG_ERR_STATE; }
    if (a.node && h->actuator.lib.on()) { h->err = std::string(a.who) + ": " + ACTUATOR_NODE_REFUSAL; return PG_ERR_STATE; }
    const bool human = a.other_car && h->human.lib.on();         // (pg_simulate_dev has no other car: it never reads the human library)
    if ((rc = check_rollout_args(h, a.who, a.steps, a.dt, a.human_mode, a.human_u, human)) || (rc = rollout_ready(h, human)) || (a.node && (rc = node_start(h, a.dt))) || (rc = clock_start(h, a.dt)) || (rc = route_start(h))) return rc;
    // Who reads which control.  The records and the plant launch: actuator.plant_u (= a_k) under an actuator library, else the command.  The compute calls -- k_nodes*, the
    // QP's u_curr, the steering-rate rows, k_estimate --: actuator.seen when some set has feedback == 1, else the command.  k_actuate: the command (the handle's own buffer).
    // The plant kernel leaves the next command in plant_u: one copy moves it to the control buffer
    auto& A = h->actuator;
    const bool act = A.lib.on(), dist = h->disturbance.lib.on();
    real* const command = h->d_control;
    real* const plant_u = act ? A.plant_u : command;
    const real* const seen_u = act && A.feedback ? A.seen : command;
    for (int k = 0; k < a.steps; k++) {
        const RolloutStep s{k, h->sim_idx - 1, plant_u};
        if (act && (rc = launch_actuate(h, s.step, k, a.dt, hist.applied, hist.command))) return rc;
        if (dist && (rc = launch_disturb(h, s.step, k, a.dt, hist.disturbance))) return rc;      // (w of this step: read by the step's last launch only)
        if ((rc = records(s)) || (rc = rollout_compute(h, seen_u, s.step, k, a.dt, hist.measured, hist.estimated, k < hist.route_steps ? hist_at(hist.route, k, h->B, 1) : (int*)nullptr, a.node, a.pre_flag ? a.pre_flag + (size_t)k * h->B : nullptr)) ||
            (rc = launch_track(h, s.step)) || (human && (rc = launch_human(h, s.step, k, a.dt, a.human_u, hist.human)))) return rc;
        h->sim_idx++;                                                     // (t0 now holds element sim_idx of the clock)
        finish(s);
        LAUNCH_CHECK(h);
        if (act) {
            HIPCHK(h, hipMemcpyAsync(command, plant_u, (size_t)h->B * 3 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));
            A.steps_stat++;
        }
    }
    return PG_OK;
}
static int no_records(const RolloutStep&) { return PG_OK; }
extern "C" {
int pg_simulate_dev(pg_handle* h, int32_t steps, double dt, void* state_hist_dev, void* control_hist_dev) {
    return rollout(h, RolloutArgs{"pg_simulate_dev", steps, dt, 0, nullptr, nullptr, false, nullptr, false},
        [&](const RolloutStep& s) -> int {
            const int B = h->B, k = s.k;
            if (state_hist_dev) HIPCHK(h, hipMemcpyAsync(hist_at((real*)state_hist_dev, k, B, 6), h->d_state, (size_t)B * 6 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));          // push!(qs, state) :88
            if (control_hist_dev) HIPCHK(h, hipMemcpyAsync(hist_at((real*)control_hist_dev, k, B, 3), s.control, (size_t)B * 3 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));  // push!(us, control) :89
            return PG_OK;
        },
        [&](const RolloutStep& s) { launch_plant_step(h, k_advance, k_advance_lib<>, k_advance_lib<DistW>, h->dc, h->B, dt, h->d_state, s.control, h->d_u, h->d_t0, h->d_tstart, h->sim_clk, h->sim_idx); });      // :94-95
}
// simulate (:80-100) with the control the ROS node sends (ros_integration.jl:114-124) fed back and the other car moving (k_advance_safety, pg_kernels.hip).  Per step: the four
// compute calls exactly as pg_simulate_dev makes them (fusion, pipelining and the split solve unchanged; with a grid they leave the step's relative state d_x7 and its
// lookup d_vg8), then ONE launch for the records, the selection, both plants, the new control, the clock and the summary
int pg_simulate_safety_dev(pg_handle* h, int32_t steps, double dt, int32_t use_hji_policy, int32_t human_mode, const void* human_u_dev,
                           void* state_hist_dev, void* control_hist_dev, void* other_hist_dev, void* human_hist_dev, void* V_hist_dev, int32_t* source_hist_dev) {
    return rollout(h, RolloutArgs{"pg_simulate_safety_dev", steps, dt, human_mode, human_u_dev,
                                  "the safety rollout belongs to the coupled controller (ros_integration.jl:56,114): the lateral formulation has no safety row", false, nullptr, true},
        no_records,
        [&](const RolloutStep& s) {
            const int B = h->B, k = s.k;
            const bool lib = h->human.lib.on();                  // (under a human library the kernel is handed this step's human.u as its script: it records and integrates that)
            const int hmode = lib ? 2 : (int)human_mode;
            SafetyIO io{lib ? (const real*)h->human.u : (human_mode == 2 ? hist_at((const real*)human_u_dev, k, B, 2) : nullptr), hist_at((real*)state_hist_dev, k, B, 6), hist_at((real*)control_hist_dev, k, B, 3),
                        hist_at((real*)other_hist_dev, k, B, 4), hist_at((real*)human_hist_dev, k, B, 2), hist_at((real*)V_hist_dev, k, B, 1), hist_at(source_hist_dev, k, B, 1),
                        h->d_vmin, h->d_breach, h->d_breach + h->cfg.batch_capacity};
            launch_plant_step(h, k_advance_safety, k_advance_safety_lib<>, k_advance_safety_lib<DistW>, h->dc, B, dt, (int)(use_hji_policy != 0), hmode, (int)h->hji.on, (int)h->sum_fresh, s.step,
                              h->d_state, s.control, h->d_other, h->d_u, h->d_x7, h->d_vg8, h->d_toff, h->d_t0, h->d_tstart, h->sim_clk, h->sim_idx, io);
            h->sum_fresh = false;
        });
}
int pg_get_safety_state(pg_handle* h, double* other_car, double* V_min, int32_t* first_breach, int32_t* policy_steps) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B;
    if ((rc = down(h, other_car, h->d_other, B * 4))) return rc;
    if (h->sum_fresh) {                  // no safety step since the clock (re)started
        for (size_t b = 0; b < B; b++) {
            if (V_min) V_min[b] = INFINITY;
            if (first_breach) first_breach[b] = -1;
            if (policy_steps) policy_steps[b] = 0;
        }
        return PG_OK;
    }
    if ((rc = down(h, V_min, h->d_vmin, B)) || (rc = down_raw(h, first_breach, h->d_breach, B * sizeof(int32_t))) ||
        (rc = down_raw(h, policy_steps, h->d_breach + h->cfg.batch_capacity, B * sizeof(int32_t)))) return rc;
    return PG_OK;
}
int pg_get_tracking_state(pg_handle* h, double* summary, int32_t* steps, int32_t* first_exit) {
    int rc = check_ready(h); if (rc) return rc;
    if (!h->tracking) { h->err = "the tracking summary is off: pg_set_option(h, \"tracking_summary\", 1), then a rollout"; return PG_ERR_STATE; }
    const size_t B = h->B;
    if (h->track_fresh || !h->d_track) {             // no rollout step since the clock (re)started
        for (size_t b = 0; b < B; b++) {
            if (summary) { double* S = summary + b * 6; S[0] = S[1] = S[2] = S[3] = 0.0; S[4] = INFINITY; S[5] = NAN; }
            if (steps) steps[b] = 0;
            if (first_exit) first_exit[b] = -1;
        }
        return PG_OK;
    }
    if ((rc = down(h, summary, h->d_track, B * 6)) || (rc = down_raw(h, steps, h->d_track_i, B * sizeof(int32_t))) ||
        (rc = down_raw(h, first_exit, h->d_track_i + cap_of(h), B * sizeof(int32_t)))) return rc;
    return PG_OK;
}
// ---- node callback (from_autobox_callback, ros_integration.jl:48-151) --------------------------------------------
// first call: the keep buffer at batch capacity (one carve-up of one allocation), the node words, the applied command (zeroed: heartbeat and counts start at 0).
// A call that failed here is not a first call that happened: the next one takes up whichever of the three buffers is missing and fills again
static int node_prepare(pg_handle* h) {
    const size_t cap = (size_t)h->cfg.batch_capacity; const int N = h->dc.N, NN = h->dc.NN;
    const int naux_cap = h->dc.formulation == PG_DECOUPLED ? 64 * LAT_AUX : 0;
    KeepView& K = h->kv;
    if (!h->d_applied) {                                      // (the last of the three)
        const size_t dbl = cap * (size_t)(NN + N + NN), rl = cap * (size_t)(NN * 8 + N * 3 + N * 16 + 3 + 1 + naux_cap), it = cap * 5, u16 = cap * (size_t)N;
        const size_t bytes = dbl * sizeof(double) + rl * sizeof(real) + it * sizeof(int) + u16 * sizeof(uint16_t);
        int rc;
        if ((rc = ensure(h, h->d_keep, bytes))) return rc;
        char* p = h->d_keep;
        auto take = [&](auto*& dst, size_t n) { dst = (std::remove_reference_t<decltype(dst)>)p; p += n * sizeof(*dst); };
        take(K.k_ts, cap * NN); take(K.k_dt, cap * N); take(K.k_prev_ts, cap * NN);
        take(K.k_solx, cap * NN * 8); take(K.k_sigma, cap * N * 3); take(K.k_lam, cap * N * 16); take(K.k_u, cap * 3); take(K.k_mu, cap); take(K.k_aux, cap * naux_cap);
        take(K.k_solved, cap); take(K.k_wfail, cap); take(K.k_status, cap); take(K.k_iters, cap); take(K.k_polish, cap); take(K.k_active, cap * N);
        if ((rc = ensure(h, h->d_node, cap * 6 + NODE_COLD_WORDS))) return rc;
        HIPCHK(h, hipMemset(h->d_node, 0, (cap * 6 + NODE_COLD_WORDS) * sizeof(int)));
        if ((rc = ensure(h, h->d_applied, cap * 3))) return rc;
        HIPCHK(h, hipMemset(h->d_applied, 0, cap * 3 * sizeof(real)));
    }
    if (h->tend_dirty) {
        if (h->d_tend) { HIPCHK(h, hipStreamSynchronize(h->stream)); h->mem.drop(h->d_tend); }
        { const int rc = ensure(h, h->d_tend, h->traj_ends.size()); if (rc) return rc; }
        HIPCHK(h, hipMemcpy(h->d_tend, h->traj_ends.data(), h->traj_ends.size() * sizeof(double), hipMemcpyHostToDevice));
        h->tend_dirty = false;
    }
    // the live side (k_solve_lat's multiplier block exists while that kernel is the handle's solver: option "lateral_solver" may change it)
    K.NN = NN; K.N = N; K.naux = (h->solve_lat && h->d_lat_aux) ? 64 * LAT_AUX : 0;
    K.ts = h->d_ts; K.dt = h->d_dt; K.prev_ts = h->d_prev_ts; K.solx = h->d_solx; K.sigma = h->d_sigma; K.lam = h->d_lam; K.u = h->d_u; K.mu = h->d_mu; K.aux = h->d_lat_aux;
    K.solved = h->d_solved; K.wfail = h->d_wfail; K.status = h->d_status; K.iters = h->d_iters; K.polish = h->d_polish; K.active = h->d_active;
    return PG_OK;
}
static int node_gate(pg_handle* h, const Seen& seen, const uint8_t* pre_flag) {
    const int B = h->B;
    hipLaunchKernelGGL(k_node_gate, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, seen.state, h->d_t0, h->d_toff, h->d_tend, pre_flag, h->d_node,
                       node_cold(h, h->node_parity ^ 1), h->kv);
    LAUNCH_CHECK(h);
    return PG_OK;
}
static NodeIO node_io(pg_handle* h) {
    NodeIO io{};
    io.gate = h->d_node; io.heartbeat = node_heartbeat(h); io.counts = node_counts(h); io.cold = node_cold(h, h->node_parity ^ 1); io.applied = h->d_applied; io.sep = h->d_sep;
    return io;
}
static void node_done(pg_handle* h) { h->node_parity ^= 1; h->node_recheck = true; h->node_fresh = false; }

int pg_node_step_dev(pg_handle* h, int32_t use_hji_policy, const uint8_t* pre_flag_dev, void* cmd_out_dev, void* se_out_dev, int32_t* event_dev) {
    int rc = check_ready(h); if (rc) return rc;
    if (h->dc.formulation != PG_COUPLED && use_hji_policy) { h->err = "pg_node_step_dev: the HJI policy belongs to the coupled controller (the lateral formulation has no safety row)"; return PG_ERR_STATE; }
    if (h->actuator.lib.on()) { h->err = std::string("pg_node_step_dev: ") + ACTUATOR_NODE_REFUSAL; return PG_ERR_STATE; }
    if ((rc = node_prepare(h)) || (rc = node_gate(h, seen_own(h), pre_flag_dev)) || (rc = step_compute(h, seen_own(h)))) return rc;
    NodeIO io = node_io(h);
    io.cmd_out = (real*)cmd_out_dev; io.se_out = (real*)se_out_dev; io.event = event_dev;
    const int B = h->B;
    hipLaunchKernelGGL(k_node_finish<false>, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->dc, B, 0.0, (int)(use_hji_policy != 0), 0, has_hji_row(h),
                       (int)h->node_fresh, 0, 0, h->d_state, h->d_control, h->d_other, h->d_u, h->d_x7, h->d_vg8, h->d_toff, h->d_t0, h->d_tstart, h->sim_clk, 0, h->kv, io);
    LAUNCH_CHECK(h);
    node_done(h);
    return PG_OK;
}
// the node rollout's buffers, and the applied command of a clock that is about to restart: it starts as the message
static int node_start(pg_handle* h, double dt) {
    int rc = node_prepare(h); if (rc) return rc;
    if (h->sim_idx == 0 || h->sim_dt != dt || h->sim_tend != h->traj_t_end) HIPCHK(h, hipMemcpyAsync(h->d_applied, h->d_control, (size_t)h->B * 3 * sizeof(real), hipMemcpyDeviceToDevice, h->stream));
    return PG_OK;
}
// the node's closed loop: per step gate, the compute calls, then ONE launch for the restore, the selection, the fallback, the message, the records, both plants, the applied
// command, the clock, the summary and the counts (k_node_finish<true>); every step counts for the tracking summary, gated out or not: the plant moves either way
int pg_simulate_node_dev(pg_handle* h, int32_t steps, double dt, int32_t use_hji_policy, int32_t human_mode, const void* human_u_dev, const uint8_t* pre_flag_dev,
                         void* state_hist_dev, void* applied_hist_dev, int32_t* event_hist_dev, void* V_hist_dev) {
    return rollout(h, RolloutArgs{"pg_simulate_node_dev", steps, dt, human_mode, human_u_dev,
                                  use_hji_policy ? "pg_simulate_node_dev: the HJI policy belongs to the coupled controller (the lateral formulation has no safety row)" : nullptr, true, pre_flag_dev, true},
        no_records,
        [&](const RolloutStep& s) {
            const int B = h->B, k = s.k;
            NodeIO io = node_io(h);
            const bool lib = h->human.lib.on();                  // (as pg_simulate_safety_dev: human.u of this step is the script)
            const int hmode = lib ? 2 : (int)human_mode;
            io.human_u = lib ? (const real*)h->human.u : (human_mode == 2 ? hist_at((const real*)human_u_dev, k, B, 2) : nullptr);
            io.state_h = hist_at((real*)state_hist_dev, k, B, 6); io.applied_h = hist_at((real*)applied_hist_dev, k, B, 3); io.V_h = hist_at((real*)V_hist_dev, k, B, 1);
            io.event_h = hist_at(event_hist_dev, k, B, 1);
            io.V_min = h->d_vmin; io.first_breach = h->d_breach; io.policy_steps = h->d_breach + h->cfg.batch_capacity;
            launch_plant_step(h, k_node_finish<true>, k_node_finish_lib<>, k_node_finish_lib<DistW>, h->dc, B, dt, (int)(use_hji_policy != 0), hmode, has_hji_row(h),
                              (int)h->node_fresh, (int)h->sum_fresh, s.step, h->d_state, s.control, h->d_other, h->d_u, h->d_x7, h->d_vg8, h->d_toff, h->d_t0, h->d_tstart, h->sim_clk,
                              h->sim_idx, h->kv, io);
            h->sum_fresh = false;
            node_done(h);
        });
}
int pg_get_node_state(pg_handle* h, double* applied, int32_t* heartbeat, int32_t* counts) {
    int rc = check_ready(h); if (rc) return rc;
    if ((rc = node_prepare(h))) return rc;
    const size_t B = h->B;
    if ((rc = down(h, applied, h->d_applied, B * 3)) || (rc = down_raw(h, heartbeat, node_heartbeat(h), B * sizeof(int32_t)))) return rc;
    if (h->node_fresh) { if (counts) memset(counts, 0, B * 4 * sizeof(int32_t)); return PG_OK; }      // no node step since the clock (re)started
    return down_raw(h, counts, node_counts(h), B * 4 * sizeof(int32_t));
}
int pg_simulate_clock(pg_handle* h, double dt, int32_t steps, int32_t B, const double* t_start, double* out) {
#pragma clang fp contract(off)
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, steps >= 1 && dt > 0.0 && B >= 1 && t_start && out, "pg_simulate_clock: steps >= 1, dt > 0, B >= 1 and both arrays required");
    REQUIRE(h, h->d_traj, "pg_simulate_clock: no trajectory installed (its last time is the stop of the range)");
    const JlRange clk = jl_colon(0.0, dt, h->traj_t_end);
    for (int b = 0; b < B; b++) {
        double acc = t_start[b];
        for (int k = 0; k < steps; k++) { out[(size_t)k * B + b] = h->dc.time_grid_naive ? acc : jl_shifted_elem(clk, t_start[b], k + 1); acc = acc + dt; }
    }
    return PG_OK;
}
int pg_get_state(pg_handle* h, double* state, double* control, double* t0) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B;
    if ((rc = down(h, state, h->d_state, B * 6)) || (rc = down(h, control, h->d_control, B * 3)) || (rc = down_raw(h, t0, h->d_t0, B * 8))) return rc;
    return PG_OK;
}
int pg_get_phase_ms(pg_handle* h, float out3[3]) {
    if (!h || !out3) return PG_ERR_INVALID;
    if (!h->timing_valid) {
        h->err = h->phase_timing == 0 ? "phase timing is off (the default since round 5): pg_set_option(h, \"phase_timing\", 1), then pg_step_dev" : "no pg_step_dev recorded yet";
        return PG_ERR_STATE;
    }
    HIPCHK(h, hipEventSynchronize(h->ev[3]));
    for (int i = 0; i < 3; i++) HIPCHK(h, hipEventElapsedTime(&out3[i], h->ev[i], h->ev[i + 1]));
    return PG_OK;
}
// the five input arrays in the staging buffer, in the layout of the device block (batch == capacity)
static void stage_block(pg_handle* h, int32_t B, const double* s_, const double* c_, const double* t0, const double* o_, const double* toff) {
    real* st = (real*)h->h_stage; real* ct = st + (size_t)B * 6; real* ot = ct + (size_t)B * 3; double* tt = (double*)(h->h_stage + h->in_dbl_off); double* ft = tt + B;
    for (size_t i = 0; i < (size_t)B * 6; i++) st[i] = (real)s_[i];
    for (size_t i = 0; i < (size_t)B * 3; i++) ct[i] = (real)c_[i];
    for (size_t i = 0; i < (size_t)B * 4; i++) ot[i] = o_ ? (real)o_[i] : real(0.0);
    memcpy(tt, t0, (size_t)B * 8);
    if (toff) memcpy(ft, toff, (size_t)B * 8); else memset(ft, 0xFF, (size_t)B * 8);      // all-ones bit pattern is a NaN: path-tracking mode
}
// pg_step of a small warm batch as ONE graph launch.  Returns PG_OK with *done = true when the step ran through the graph; *done = false means "not eligible / not
// possible": the caller takes the ordinary path.  Eligible: graphs on, the batch fills the handle (one copy per direction), <= 256 instances (beyond, the kernels
// dominate the launches), every instance warm (the cold branch picks other kernels), nothing fused or chunked.
static int step_by_graph(pg_handle* h, int32_t B, const double* state, const double* control, const double* t0, const double* other, const double* toff, bool* done) {
    *done = false;
    auto& G = h->sg;
    if (!h->graph_mode || G.disabled || B != h->cfg.batch_capacity || B > 256 || h->B != B || h->warm_B < B || h->fuse != 0 || !h->d_traj || h->node_recheck) return PG_OK;
    if (index_covers(h, (size_t)h->dc.n_traj, h->traj_idx) || index_covers(h, (size_t)h->dc.n_cp, h->cp.idx)) return PG_OK;      // (h->B == B; the ordinary path reports it)
    if (hipSetDevice(h->cfg.device) != hipSuccess) return PG_OK;
    const bool same = G.x && G.B == B && G.user == h->stream && G.fuse == h->fuse && G.pipeline == h->pipeline && G.has_hji == (int)h->hji.on && G.traj_L == h->traj_L &&
                      memcmp(&G.dc, &h->dc, sizeof(DevCfg)) == 0 && memcmp(&G.hv, &h->hji.hv, sizeof(HjiView)) == 0;
    hipStream_t run = h->stream ? h->stream : G.own;
    if (!same) {
        if (G.x) { (void)hipGraphExecDestroy(G.x); G.x = nullptr; }
        if (G.g) { (void)hipGraphDestroy(G.g); G.g = nullptr; }
        if (!h->stream && !G.own && hipStreamCreate(&G.own) != hipSuccess) { G.disabled = true; (void)hipGetLastError(); return PG_OK; }      // (a blocking stream: ordered against the null stream)
        run = h->stream ? h->stream : G.own;
        if (hipStreamSynchronize(h->stream) != hipSuccess) return PG_OK;
        hipStream_t user = h->stream;
        bool ok = hipStreamBeginCapture(run, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            h->stream = run; G.capturing = true;
            ok = hipMemcpyAsync(h->d_in, h->h_stage, h->in_bytes, hipMemcpyHostToDevice, run) == hipSuccess && pg_step_dev(h, nullptr) == PG_OK &&
                 hipMemcpyAsync(h->h_stage, h->d_out, h->out_bytes, hipMemcpyDeviceToHost, run) == hipSuccess;
            h->stream = user; G.capturing = false;
            hipGraph_t g = nullptr;
            const bool ended = hipStreamEndCapture(run, &g) == hipSuccess && g != nullptr;
            ok = ok && ended;
            if (ok) { G.g = g; ok = hipGraphInstantiate(&G.x, G.g, nullptr, nullptr, 0) == hipSuccess; }
            else if (g) (void)hipGraphDestroy(g);
        }
        if (!ok) {           // this runtime / this configuration cannot be captured: never again for this handle, the ordinary path takes over
            if (G.x) { (void)hipGraphExecDestroy(G.x); G.x = nullptr; }
            if (G.g) { (void)hipGraphDestroy(G.g); G.g = nullptr; }
            G.disabled = true; (void)hipGetLastError();
            return PG_OK;
        }
        memcpy(&G.dc, &h->dc, sizeof(DevCfg)); memcpy(&G.hv, &h->hji.hv, sizeof(HjiView)); G.B = B;      // (byte copies: the signature is compared with memcmp, padding included)
         G.user = user; G.fuse = h->fuse; G.pipeline = h->pipeline; G.has_hji = (int)h->hji.on; G.traj_L = h->traj_L;
    } else if (hipStreamSynchronize(h->stream) != hipSuccess) return PG_OK;
    stage_block(h, B, state, control, t0, other, toff);
    HIPCHK(h, hipGraphLaunch(G.x, run));
    HIPCHK(h, hipStreamSynchronize(run));
    h->timing_valid = false;
    *done = true;
    return PG_OK;
}
int pg_step(pg_handle* h, int32_t B, const double* state, const double* control, const double* t0, const double* other, const double* toff,
            double* u_out, int32_t* status, int32_t* iters) {
    if (h && state && control && t0) {
        bool done = false;
        int rc = step_by_graph(h, B, state, control, t0, other, toff, &done); if (rc) return rc;
        if (done) {
            const real* us = (const real*)h->h_stage; const int* ss = (const int*)(us + (size_t)B * 3); const int* is = ss + B;
            if (u_out) for (size_t i = 0; i < (size_t)B * 3; i++) u_out[i] = (double)us[i];
            if (status) memcpy(status, ss, (size_t)B * sizeof(int));
            if (iters) memcpy(iters, is, (size_t)B * sizeof(int));
            return PG_OK;
        }
    }
    int rc = pg_set_inputs(h, B, state, control, t0, other, toff); if (rc) return rc;
    if ((rc = pg_step_dev(h, nullptr))) return rc;
    // controls, status and iteration counts come back through the pinned staging buffer: three asynchronous copies behind k_solve on the handle's stream
    // (ordered even when the caller installed a non-blocking stream), ONE synchronisation, then the conversion into the caller's arrays
    real* us = (real*)h->h_stage; int* ss = (int*)(us + (size_t)B * 3); int* is = ss + B;
    if (B == h->cfg.batch_capacity) {          // (u, status, iters) are one block on the device: one copy
        HIPCHK(h, hipMemcpyAsync(h->h_stage, h->d_out, h->out_bytes, hipMemcpyDeviceToHost, h->stream));
    } else {
        if (u_out) HIPCHK(h, hipMemcpyAsync(us, h->d_u, (size_t)B * 3 * sizeof(real), hipMemcpyDeviceToHost, h->stream));
        if (status) HIPCHK(h, hipMemcpyAsync(ss, h->d_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (iters) HIPCHK(h, hipMemcpyAsync(is, h->d_iters, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (u_out) for (size_t i = 0; i < (size_t)B * 3; i++) u_out[i] = (double)us[i];
    if (status) memcpy(status, ss, (size_t)B * sizeof(int));
    if (iters) memcpy(iters, is, (size_t)B * sizeof(int));
    return PG_OK;
}

// ---- read-backs --------------------------------------------------------------------------------------------------
int pg_get_time_steps(pg_handle* h, double* ts, double* dt, double* prev_ts) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B; const DevCfg& C = h->dc;
    if ((rc = down_raw(h, ts, h->d_ts, B * C.NN * 8)) || (rc = down_raw(h, dt, h->d_dt, B * C.N * 8)) || (rc = down_raw(h, prev_ts, h->d_prev_ts, B * C.NN * 8))) return rc;
    return PG_OK;
}
int pg_get_nodes(pg_handle* h, double* qs, double* us, double* ps) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B; const DevCfg& C = h->dc;
    std::vector<double> nd(B * C.NN * 10);
    if ((rc = down(h, nd.data(), h->d_nodes, nd.size()))) return rc;
    for (size_t i = 0; i < B * C.NN; i++) {
        const double* r = &nd[i * 10];
        if (qs) for (int k = 0; k < 6; k++) qs[i * 6 + k] = r[k];
        if (us) { us[i * 2] = r[6]; us[i * 2 + 1] = r[7]; }
        if (ps) { ps[i * 4] = r[8]; ps[i * 4 + 1] = r[9]; ps[i * 4 + 2] = 0.0; ps[i * 4 + 3] = 0.0; }
    }
    return PG_OK;
}
int pg_get_path_coordinates(pg_handle* h, double* sep) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, sep, "sep is null");
    const size_t B = h->B;
    std::vector<double> s4(B * 4);
    if ((rc = down(h, s4.data(), h->d_sep, s4.size()))) return rc;
    for (size_t b = 0; b < B; b++) for (int k = 0; k < 3; k++) sep[b * 3 + k] = s4[b * 4 + k];
    return PG_OK;
}
// the last update_QP! of a lateral handle may have written the packed records only: the embedded block now, from the same nodes
static int embed_lateral_qp(pg_handle* h) {
    if (h->dc.formulation != PG_DECOUPLED || h->qp_embedded) return PG_OK;
    const long nt = (long)h->B * h->dc.N;
    hipLaunchKernelGGL(k_qp_dec, dim3((unsigned)((nt + 127) / 128)), dim3(128), 0, h->stream, h->dc, h->B, h->d_nodes, h->d_dt, h->d_qp, 1);
    LAUNCH_CHECK(h);
    h->qp_embedded = true;
    return PG_OK;
}
int pg_get_qp(pg_handle* h, int32_t b0, int32_t n, double* out) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, out && b0 >= 0 && n >= 1 && b0 + n <= h->B, "pg_get_qp: range outside the batch");
    if ((rc = embed_lateral_qp(h))) return rc;
    return down(h, out, h->d_qp + (size_t)b0 * h->dc.qp_len, (size_t)n * h->dc.qp_len);
}
int pg_set_qp(pg_handle* h, int32_t b0, int32_t n, const double* in) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, in && b0 >= 0 && n >= 1 && b0 + n <= h->B, "pg_set_qp: range outside the batch");
    if ((rc = embed_lateral_qp(h))) return rc;      // (a partial install on top of a step that wrote the packed records only: complete the embedded block first)
    if ((rc = up(h, h->d_qp + (size_t)b0 * h->dc.qp_len, in, (size_t)n * h->dc.qp_len))) return rc;
    if (h->solve_lat) {      // k_solve_lat reads the packed stage records: refresh them from the installed block
        const long nt = (long)n * h->dc.N;
        hipLaunchKernelGGL(k_lat_pack, dim3((unsigned)((nt + 127) / 128)), dim3(128), 0, h->stream, h->dc, b0, n, h->d_qp);
        LAUNCH_CHECK(h);
    }
    if (b0 == 0 && n == h->B) h->qp_stale = false;      // (both record forms of the whole batch are current now)
    return PG_OK;
}
int pg_get_solution(pg_handle* h, double* x, double* sigma) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B; const DevCfg& C = h->dc;
    if ((rc = down(h, x, h->d_solx, B * C.NN * 8)) || (rc = down(h, sigma, h->d_sigma, B * C.N * 3))) return rc;
    return PG_OK;
}
int pg_get_solve_info(pg_handle* h, int32_t* status, int32_t* iters, uint16_t* active, double* mu) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B; const DevCfg& C = h->dc;
    if ((rc = down_raw(h, status, h->d_status, B * 4)) || (rc = down_raw(h, iters, h->d_iters, B * 4)) || (rc = down_raw(h, active, h->d_active, B * C.N * 2)) ||
        (rc = down(h, mu, h->d_mu, B))) return rc;
    return PG_OK;
}
int pg_get_polish_info(pg_handle* h, int32_t* polish) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, polish, "polish is null");
    return down_raw(h, polish, h->d_polish, (size_t)h->B * 4);
}
int pg_get_multipliers(pg_handle* h, double* lam) {
    int rc = check_ready(h); if (rc) return rc;
    REQUIRE(h, lam, "lam is null");
    return down(h, lam, h->d_lam, (size_t)h->B * h->dc.N * 16);
}
int pg_get_walls(pg_handle* h, double* edges) {
    int rc = check_ready(h); if (rc) return rc;
    if (!h->dc.walls) { h->err = "walls are off (pg_config.walls = 0)"; return PG_ERR_STATE; }
    REQUIRE(h, edges, "edges is null");
    return down(h, edges, h->d_walls, (size_t)h->B * h->dc.N * 2);
}
int pg_get_hji_constraint(pg_handle* h, double* M, double* b, double* V) {
    int rc = check_ready(h); if (rc) return rc;
    const size_t B = h->B;
    std::vector<double> mb(B * 4);
    if (h->hji.on && (rc = down(h, mb.data(), h->d_Mb, mb.size()))) return rc;
    for (size_t i = 0; i < B; i++) {
        if (!h->hji.on) { mb[4 * i] = 0; mb[4 * i + 1] = 0; mb[4 * i + 2] = 1; mb[4 * i + 3] = INFINITY; }
        if (M) { M[2 * i] = mb[4 * i]; M[2 * i + 1] = mb[4 * i + 1]; }
        if (b) b[i] = mb[4 * i + 2];
        if (V) V[i] = mb[4 * i + 3];
    }
    return PG_OK;
}

int pg_hji_lookup_dev(pg_handle* h, int32_t B, const void* x7_dev, void* V_dev, void* gradV_dev) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, h->hji.on, "no HJI grid installed");
    REQUIRE(h, B >= 1 && x7_dev, "pg_hji_lookup_dev: bad arguments");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    CallBufs D; real* out8 = nullptr; const size_t R = sizeof(real);
    HIPCHK(h, D.alloc(out8, (size_t)B * 8));
    const int rc = launch_hji_lookup(h, B, (const real*)x7_dev, out8); if (rc) return rc;
    if (V_dev) HIPCHK(h, hipMemcpy2DAsync(V_dev, R, out8, 8 * R, R, B, hipMemcpyDeviceToDevice, h->stream));
    if (gradV_dev) HIPCHK(h, hipMemcpy2DAsync(gradV_dev, 7 * R, out8 + 1, 8 * R, 7 * R, B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PG_OK;
}
int pg_hji_lookup8_dev(pg_handle* h, int32_t B, const void* x7_dev, void* out8_dev) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, h->hji.on, "no HJI grid installed");
    REQUIRE(h, B >= 1 && x7_dev && out8_dev, "pg_hji_lookup8_dev: bad arguments");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return launch_hji_lookup(h, B, (const real*)x7_dev, (real*)out8_dev);
}
int pg_hji_grid_dims(pg_handle* h, int32_t dims[7]) {
    if (!h || !dims) return PG_ERR_INVALID;
    REQUIRE(h, h->hji.on, "no HJI grid installed");
    for (int d = 0; d < 7; d++) dims[d] = h->hji.hv.dims[d];
    return PG_OK;
}
int pg_hji_slice(pg_handle* h, int32_t B, const double* q7, double* V_out, double* rgb_out, double* cross_x, double* cross_y) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, h->hji.on, "no HJI grid installed");
    REQUIRE(h, B >= 1 && q7 && V_out, "pg_hji_slice: need B >= 1, the relative states and V_out");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int n1 = h->hji.hv.dims[0], n2 = h->hji.hv.dims[1]; const size_t npt = (size_t)B * n1 * n2;
    CallBufs D; real *dq = nullptr, *dx = nullptr, *dv = nullptr, *dV = nullptr, *drgb = nullptr, *dcx = nullptr, *dcy = nullptr; int rc = PG_OK;
    HIPCHK(h, D.alloc(dq, (size_t)B * 7)); HIPCHK(h, D.alloc(dx, npt * 7)); HIPCHK(h, D.alloc(dv, npt * 8)); HIPCHK(h, D.alloc(dV, npt));
    if (rgb_out) HIPCHK(h, D.alloc(drgb, npt * 3));
    if (cross_x) HIPCHK(h, D.alloc(dcx, (size_t)B * (n1 - 1) * n2));
    if (cross_y) HIPCHK(h, D.alloc(dcy, (size_t)B * n1 * (n2 - 1)));
    if ((rc = up(h, dq, q7, (size_t)B * 7))) return rc;
    const dim3 grid((unsigned)((npt + 255) / 256));
    hipLaunchKernelGGL(k_hji_slice_queries, grid, dim3(256), 0, h->stream, h->hji.hv, B, dq, dx);
    if ((rc = launch_hji_lookup(h, (int)npt, dx, dv))) return rc;
    hipLaunchKernelGGL(k_hji_slice_post, grid, dim3(256), 0, h->stream, h->hji.hv, B, dv, dV, drgb, dcx, dcy);
    if (hipGetLastError() != hipSuccess) { h->err = "pg_hji_slice: kernel launch failed"; return PG_ERR_HIP; }
    if ((rc = down(h, V_out, dV, npt)) || (rc = down(h, rgb_out, drgb, npt * 3)) || (rc = down(h, cross_x, dcx, (size_t)B * (n1 - 1) * n2)) ||
        (rc = down(h, cross_y, dcy, (size_t)B * n1 * (n2 - 1)))) return rc;
    return PG_OK;
}
int pg_hji_lookup(pg_handle* h, int32_t B, const double* x7, double* V, double* gradV) {
    if (!h) return PG_ERR_INVALID;
    REQUIRE(h, h->hji.on, "no HJI grid installed");
    REQUIRE(h, B >= 1 && x7, "pg_hji_lookup: bad arguments");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    CallBufs D; real *dx = nullptr, *dout = nullptr;
    HIPCHK(h, D.alloc(dx, (size_t)B * 7));
    HIPCHK(h, D.alloc(dout, (size_t)B * 8));
    std::vector<double> out((size_t)B * 8);
    int rc;
    if ((rc = up(h, dx, x7, (size_t)B * 7)) || (rc = launch_hji_lookup(h, B, dx, dout)) || (rc = down(h, out.data(), dout, out.size()))) return rc;
    for (int i = 0; i < B; i++) { if (V) V[i] = out[8 * (size_t)i]; if (gradV) for (int k = 0; k < 7; k++) gradV[7 * (size_t)i + k] = out[8 * (size_t)i + 1 + k]; }
    return PG_OK;
}

}  // extern "C"
