// Route sets: an instance changes trajectory during a rollout (nominal_trajectory_callback, ros_integration.jl:30-41).  Stated in include/pigeon_mpc.h at
// pg_set_route_sets and in DESIGN.md 4.20; tests/route_numpy.py is the numpy twin of the event resolution and the anchors.  Included by pg_kernels.hip inside namespace pg.
//
// k_route: one wavefront per instance, the launch shape of k_project.  Lane 0 resolves the event of the clock step -- at most PG_ROUTE_EVENTS compares against the steps of
// the instance's set -- and the result is wave-uniform (readfirstlane), so every branch below is taken by the whole wavefront or by none of it.  A wavefront without an
// event writes its history word and leaves.  A PROJECT event projects the state the controller is handed on the TARGET trajectory with the statements of k_project in
// their order (restated, not shared: k_project's code stays what it was): seg_dist2 per segment with i striding by 64, strict '<' with the lowest index winning in the
// lane and in the __shfl_xor reduction, the rationalised ds / dt.  The projection is in `real`, the time offset in double in both builds (tdouble).  Every write -- the
// index, the offset, the solved flag and back-off word, the route state, the history word -- is a plain store of lane 0.  No LDS, no atomics.

struct RouteLib {
    const pg_route* sets;          // [n_sets] as the caller installed them
    const int* idx;                // [B] per-instance selection, or nullptr: set 0
    int* traj_idx;                 // [B] the device trajectory index (DevCfg::traj_idx), written in place
    int* fired;                    // [B] events since the clock restarted
    int* last_step;                // [B] clock step of the last one
    tdouble* t_at;                 // [B] where the new trajectory was joined
    real* e_at;                    // [B] lateral offset of a PROJECT event's projection (NaN otherwise)
};
// trajectory k of the installed library (traj_of for an explicit index: nothing is read through C.traj_idx)
PG_DEV TrajView route_traj(const DevCfg& C, int k) {
    TrajView T = C.traj;
    const long off = (long)k * C.traj_stride;
    T.L = C.traj_len[k];
    T.t += off; T.s += off; T.V += off; T.A += off; T.E += off; T.N += off; T.psi += off; T.kappa += off; T.edge_L += off; T.edge_R += off;
    return T;
}

__global__ __launch_bounds__(256) void k_route(DevCfg C, int B, int step, RouteLib R, const real* __restrict__ state, const tdouble* __restrict__ t0, tdouble* __restrict__ toff,
                                               int* __restrict__ solved, int* __restrict__ wfail, int* __restrict__ hist) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= B) return;
    int slot = -1, cur = 0, set = 0;
    if (lane == 0) {
        set = R.idx ? R.idx[wave] : 0;
        cur = R.traj_idx[wave];
        const pg_route_event* ev = R.sets[set].ev;
#pragma unroll
        for (int k = 0; k < PG_ROUTE_EVENTS; k++) if (ev[k].step == step) slot = k;      // (the steps of a set are strictly increasing: at most one matches)
    }
    slot = __builtin_amdgcn_readfirstlane(slot); cur = __builtin_amdgcn_readfirstlane(cur); set = __builtin_amdgcn_readfirstlane(set);
    if (slot < 0) { if (lane == 0 && hist) hist[wave] = cur; return; }
    const pg_route_event ev = R.sets[set].ev[slot];                                       // (a wave-uniform address)
    int tgt = ev.target;
    if (ev.target_mode == PG_ROUTE_RELATIVE) { tgt = (cur + ev.target) % C.n_traj; if (tgt < 0) tgt += C.n_traj; }
    // (the host refuses a rollout whose absolute targets do not fit the library: never an address outside it, whatever reached this point)
    if (tgt < 0 || tgt >= C.n_traj) { if (lane == 0 && hist) hist[wave] = cur; return; }
    real t_proj = NAN, e_proj = NAN;
    if (ev.anchor == PG_ROUTE_PROJECT) {
        const TrajView T = route_traj(C, tgt);
        real x = state[(size_t)wave * 6 + 0], y = state[(size_t)wave * 6 + 1];
        real best = INFINITY; int bi = 0x7fffffff;
        for (int i = lane; i < T.L - 1; i += 64) {
            real d2 = seg_dist2(T.E[i], T.N[i], T.E[i + 1], T.N[i + 1], x, y);
            if (d2 < best) { best = d2; bi = i; }           // i increases within a lane, so strict '<' keeps the lowest index
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            real ob = __shfl_xor(best, off); int oi = __shfl_xor(bi, off);
            if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            int i = bi;
            // non-finite pose: no segment ever wins and bi keeps its sentinel -- NaN coordinates, NaN offset, and no address is formed from the sentinel (k_project)
            if (!(i < 0 || i > T.L - 2)) {
                real vx = T.E[i + 1] - T.E[i], vy = T.N[i + 1] - T.N[i], wx = x - T.E[i], wy = y - T.N[i];
                real vw = vx * wx + vy * wy, vv = vx * vx + vy * vy;
                real lam = vw / vv; lam = lam < real(0.0) ? real(0.0) : (lam > real(1.0) ? real(1.0) : lam);
                real ds = sqrt(fmax(lam * (real(2.0) * vw - lam * vv), real(0.0)));
                real cr = vx * wy - vy * wx;
                real Ai = (T.V[i + 1] - T.V[i]) / (T.t[i + 1] - T.t[i]);
                real dt = fabs(Ai) < real(1e-3) ? ds / T.V[i] : real(2.0) * ds / (sqrt(real(2.0) * Ai * ds + T.V[i] * T.V[i]) + T.V[i]);
                e_proj = sqrt(best) * sgn(cr); t_proj = T.t[i] + dt;
            }
        }
    }
    if (lane != 0) return;
    const tdouble now = t0[wave];
    tdouble off_new = toff[wave], at;
    if (ev.anchor == PG_ROUTE_PATH) { off_new = __builtin_nan(""); at = off_new; }
    else if (ev.anchor == PG_ROUTE_STAMP) { off_new = now - ev.t_join; at = ev.t_join; }
    else if (ev.anchor == PG_ROUTE_PROJECT) { at = (tdouble)t_proj; off_new = now - (at + ev.t_join); }
    else at = now - off_new;
    R.traj_idx[wave] = tgt;
    toff[wave] = off_new;
    if (ev.cold) { solved[wave] = 0; wfail[wave] = 0; }
    R.fired[wave] = R.fired[wave] + 1; R.last_step[wave] = step; R.t_at[wave] = at; R.e_at[wave] = e_proj;
    if (hist) hist[wave] = tgt;
}
