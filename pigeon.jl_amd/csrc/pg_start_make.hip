// pg_make_starts: the inputs of a batch (state, control, t0, other car, time offset) placed on the installed trajectory library under a library of start sets, on the
// device.  The reference receives its state from the car (ros_integration.jl:48-99), so the scheme is build-defined: stated in include/pigeon_mpc.h at pg_make_starts and
// in DESIGN.md 4.19, tests/start_make_numpy.py is the independent numpy twin.  Included by pg_kernels.hip inside namespace pg.
//
// One lane per instance; nothing is shared between lanes, no lane waits on another.  Per instance: 7 Philox blocks (26 uniform draws, a pure function of seed, stream id
// and channel: no dependence on the batch), two binary searches over the instance's own tube, one sincos, and with steady = 1 the four-iteration steady_state of the cold
// node seeding.  The lookup is the controller's own (traj_at_s, traj_edges_at_s of pg_device.hpp) restated in DOUBLE on the channels as the library holds them, so the fp32
// library's starts are the double scheme on float-rounded channels, rounded once on store; no contraction, every operation rounded once as the numpy twin rounds it.
// steady_state itself runs in the library's element type: it is the function that seeds the cold nodes.

struct StartMakeArgs {
    int B, n_sets;
    const pg_start_set* sets;              // [n_sets] as the caller gave them
    const int* set_index;                  // [B], or nullptr: set 0
    const unsigned long long* stream;      // [B], or nullptr: stream[b] = b
    unsigned long long seed;
    real *state, *control, *other;         // [B][6], [B][3], [B][4]
    double *t0, *toff, *placed;            // [B], [B], [B][4] = s, e, dpsi, V(s)
};
enum { ST_S = 0, ST_E, ST_DPSI, ST_V, ST_UY, ST_DR, ST_DELTA, ST_FX, ST_DT0, ST_ODX, ST_ODY, ST_ODPSI, ST_OV, ST_CHANNELS, ST_BLOCK0 = 4 };

// count of knots < x (leq = false: Julia's searchsortedfirst - 1) or <= x (leq = true: searchsortedlast), x in double against the channel as stored
PG_DEV int start_count(const real* v, int n, double x, bool leq) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; const double k = (double)v[mid]; if (leq ? k <= x : k < x) lo = mid + 1; else hi = mid; }
    return lo;
}
struct StartLook { double V, A, t, psi, kappa, E, N, eL, eR; };
// traj[s] (trajectories.jl:55-68) with its t, and interp_by_s (:32-35) of psi, kappa, E, N and the edges: traj_at_s + traj_edges_at_s in double.
// The square root is the reference's (sqrt(2 A ds + V^2) - V) / A, not the rationalised 2 ds / (sqrt(..) + V) of traj_at_s: in double the two are one rounding apart,
// and only the reference's form makes the numpy twin equal spec_numpy.Trajectory.at_s bit for bit, which is what pins the twin (tests/test_start_make_host.py).  The
// cancellation costs at most 2^-52 V / |A| seconds in dt with |A| >= 1e-3: below 1.2e-12 s at 5 m/s, nothing to a start (traj_at_s is rationalised for float)
PG_DEV StartLook start_lookup(const TrajView& T, double sq) {
#pragma clang fp contract(off)
    StartLook o;
    const int i = clampi(start_count(T.s, T.L, sq, false), 1, T.L - 1) - 1;
    const double Vi = (double)T.V[i], ti = (double)T.t[i];
    const double Ai = ((double)T.V[i + 1] - Vi) / ((double)T.t[i + 1] - ti);
    const double ds = sq - (double)T.s[i];
    double dt;
    if (fabs(Ai) < 1e-3 || sq > (double)T.s[T.L - 1]) dt = ds / Vi;
    else dt = (sqrt(2.0 * Ai * ds + Vi * Vi) - Vi) / Ai;               // trajectories.jl:63 as written (see the note on start_lookup)
    o.V = Vi + Ai * dt; o.A = Ai; o.t = ti + dt;
    const int j = clampi(start_count(T.s, T.L, sq, true), 1, T.L - 1) - 1;
    const double sj = (double)T.s[j];
    const double w = (sq - sj) / ((double)T.s[j + 1] - sj);
    auto lin = [&](const real* c) -> double { const double a = (double)c[j]; return a + w * ((double)c[j + 1] - a); };
    o.psi = lin(T.psi); o.kappa = lin(T.kappa); o.E = lin(T.E); o.N = lin(T.N); o.eL = lin(T.edge_L); o.eR = lin(T.edge_R);
    return o;
}

__global__ __launch_bounds__(64) void k_make_starts(DevCfg C, StartMakeArgs P) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= P.B) return;
    const pg_start_set& S = P.sets[P.set_index ? P.set_index[b] : 0];
    const unsigned long long stream = P.stream ? P.stream[b] : (unsigned long long)b;
    // ---- draws: channel c takes word c % 4 of block ST_BLOCK0 + c / 4; value = lo + u (hi - lo), u = (x + 0.5) 2^-32 ----
    double val[ST_CHANNELS];
    {
        const uint32_t key[2] = {(uint32_t)P.seed, (uint32_t)(P.seed >> 32)};
        const double* range = &S.s_lo;                                 // the 13 (lo, hi) pairs lead the structure in the channel order
#pragma unroll
        for (int blk = 0; blk < (ST_CHANNELS + 3) / 4; blk++) {
            const uint32_t ctr[4] = {0u, (uint32_t)(ST_BLOCK0 + blk), (uint32_t)stream, (uint32_t)(stream >> 32)};
            uint32_t x[4];
            philox4x32_10(ctr, key, x);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = 4 * blk + k;
                if (c < ST_CHANNELS) {
                    const double lo = range[2 * c], hi = range[2 * c + 1];
                    const double u = ((double)x[k] + 0.5) * 0x1p-32;
                    val[c] = lo + u * (hi - lo);
                }
            }
        }
    }
    // ---- arclength, clamped to the instance's own tube ----
    const TrajView T = traj_of(C, b);
    const double s_first = (double)T.s[0], s_last = (double)T.s[T.L - 1];
    double s = S.s_mode ? s_first + val[ST_S] * (s_last - s_first) : s_first + val[ST_S];
    s = s < s_first ? s_first : (s > s_last ? s_last : s);
    const StartLook K = start_lookup(T, s);
    // ---- placement: psi from North, left normal (-cos psi, -sin psi) ----
    double e = val[ST_E];
    if (S.e_mode) { const double mid = 0.5 * (K.eL + K.eR), half = 0.5 * (K.eL - K.eR); e = mid + val[ST_E] * half; }
    double sp, cp; sincos(K.psi, &sp, &cp);
    const double E = K.E - e * cp, N = K.N - e * sp, psi = K.psi + val[ST_DPSI];
    // ---- body state and control ----
    const double vV = val[ST_V] * K.V;
    double Ux = vV, Uy = 0.0, r = K.kappa * vV, delta = 0.0, Fx = 0.0;
    if (S.steady) {
        const real Vr = (real)vV, kr = (real)K.kappa;
        const Steady est = steady_state(C.veh, Vr, (real)K.A, kr, 4, Vr * kr, real(0.0), real(0.0), real(1.0), real(0.0), real(0.0), real(1.0), real(0.0));
        Ux = (double)est.Ux; Uy = (double)est.Uy; r = (double)est.r; delta = (double)est.delta; Fx = (double)est.Fx;
    }
    Uy = Uy + val[ST_UY]; r = r + val[ST_DR]; delta = delta + val[ST_DELTA]; Fx = Fx + val[ST_FX];
    const double Fxf = Fx > 0.0 ? Fx * (double)C.veh.fwd_frac : Fx * (double)C.veh.fwb_frac;      // longitudinal_tire_forces (vehicle_dynamics.jl:279-283); no control limits
    const double Fxr = Fx > 0.0 ? Fx * (double)C.veh.rwd_frac : Fx * (double)C.veh.rwb_frac;
    // ---- the other car, in the frame of the MADE ego heading: forward (-sin psi, cos psi), left (-cos psi, -sin psi) ----
    double oE = 0.0, oN = 0.0, opsi = 0.0, oV = 0.0;
    if (S.other_mode) {
        double so, co; sincos(psi, &so, &co);
        const double dx = val[ST_ODX], dy = val[ST_ODY];
        oE = E + dx * (-so) + dy * (-co); oN = N + dx * co + dy * (-so); opsi = psi + val[ST_ODPSI]; oV = val[ST_OV];
    }
    // ---- store: state, control and other car rounded once to the library's element type; times and `placed` in double ----
    real* q = P.state + (size_t)b * 6;
    q[0] = (real)E; q[1] = (real)N; q[2] = (real)psi; q[3] = (real)Ux; q[4] = (real)Uy; q[5] = (real)r;
    real* u = P.control + (size_t)b * 3;
    u[0] = (real)delta; u[1] = (real)Fxf; u[2] = (real)Fxr;
    real* o = P.other + (size_t)b * 4;
    o[0] = (real)oE; o[1] = (real)oN; o[2] = (real)opsi; o[3] = (real)oV;
    P.t0[b] = K.t + val[ST_DT0];
    P.toff[b] = S.time_mode ? __builtin_nan("") : 0.0;
    double* pl = P.placed + (size_t)b * 4;
    pl[0] = s; pl[1] = e; pl[2] = val[ST_DPSI]; pl[3] = K.V;
}
