// pg_plan_speeds: friction-limited speed profiles of a library of paths under a library of plan sets, on the device.  The reference receives UxDes / AxDes from a planner
// outside its tree (ros_integration.jl:13-16), so the scheme is build-defined: stated in include/pigeon_mpc.h at pg_plan_speeds and in DESIGN.md,
// tests/speed_plan_numpy.py is the independent numpy twin.  Included by pg_kernels.hip inside namespace pg.
//
// The two passes are serial in the knot and independent across (path, set).  One wavefront takes spw <= 64 sets of ONE path, lane = set: s, kappa, i0 and the knot index are
// wave-uniform (scalar loads, no divergence, every lane at the same knot on a closed path too).  Three passes over the knots, each in the order the scheme visits them:
//   backward   W from the braking limit, into the V channel of the output (scratch until the forward pass has been there)
//   forward    reads that W back, takes the acceleration limit, writes V = sqrt(W) and A, counts the limiters, reduces usage_max
//   time       reads V, accumulates t in double from knot 0 (a closed path's passes start at i0, t does not), writes t, reduces v_min / v_max
// The output is [trajectory][channel][knot]: a lane that stores its own knot strides by 10 Lmax elements.  A variant that staged tiles of 32 knots x 64 lanes in LDS (padded
// rows) and stored them transposed, 32 contiguous knots per trajectory and instruction, was built and measured against this one: at 8 paths x 512 sets x 1000 knots it
// took 1.99 ms against 1.46 ms (fp64; EXPERIMENTS 27) -- the launch is 64 wavefronts on 256 CUs, bound by the latency of the serial sqrt / divide chain, the strided
// stores are fire-and-forget and each lane re-reads only what it wrote, while a lone wavefront per CU drains its LDS tile at a fraction of the LDS rate.  So the plain
// form stayed; what did help is more wavefronts: spw = 32 or 16 sets per wavefront while CUs are idle (speed_plan_spw in pg_api.hip; EXPERIMENTS 27).  No atomics: a lane owns its trajectory's stats.  No kernel waits on another.
// k_speed_plan_copy broadcasts the seven geometry channels of a path to its n_sets outputs and zeroes the tails, one element per thread (coalesced).

struct SpeedSet { real a_lim, ay, Wmax, Wfloor, Wstart, Wend, ax_max, nax_min, m, Fx_max, nFx_min, Px_max, Cd0, Cd1, Cd2, pad; };
// in [n_path][10][Lmax], out [n_path * n_sets][10][Lmax], L [n_path], i0 [n_path] (the start knot of a closed path's passes; -1: open), sets [n_sets]
struct SpeedPlanArgs { int n_path, n_sets, Lmax, spw;      /* spw: sets per wavefront (64, 32 or 16: fewer sets per wavefront = more wavefronts) */ const int* L; const int* i0; const real* in; const SpeedSet* sets; real* out; pg_speed_plan_stats* stats; };
enum { SP_T = 0, SP_S = 1, SP_V = 2, SP_A = 3, SP_KAPPA = 7, SP_CAP = 0, SP_ACCEL = 1, SP_BRAKE = 2 };

// cap_i = max(V_floor^2, min(V_max^2, ay / |kappa_i|)), V_max^2 where kappa_i = 0
PG_DEV real sp_cap(const SpeedSet& S, real kappa) {
    const real ak = fabs(kappa);
    real c = S.Wmax;
    if (ak > real(0.0)) c = fmin(S.Wmax, S.ay / ak);
    return fmax(S.Wfloor, c);
}
// No contraction in the limit functions: every product and sum is rounded once, as the numpy twin rounds it
PG_DEV void sp_along_drag(const SpeedSet& S, real W, real kappa, real& V, real& along, real& Fd) {
#pragma clang fp contract(off)
    V = sqrt(W);
    const real lat = W * kappa;
    const real a2 = S.a_lim * S.a_lim, l2 = lat * lat;
    along = sqrt(fmax(a2 - l2, real(0.0)));
    const real inner = S.Cd2 * V;
    const real mid = V * (S.Cd1 + inner);
    Fd = S.Cd0 + mid;
}
PG_DEV real sp_acc(const SpeedSet& S, real W, real kappa) {
#pragma clang fp contract(off)
    real V, along, Fd; sp_along_drag(S, W, kappa, V, along, Fd);
    const real F = fmin(fmin(S.m * along, S.Fx_max), S.Px_max / V);
    return fmin((F - Fd) / S.m, S.ax_max);
}
PG_DEV real sp_dec(const SpeedSet& S, real W, real kappa) {
#pragma clang fp contract(off)
    real V, along, Fd; sp_along_drag(S, W, kappa, V, along, Fd);
    const real F = fmin(S.m * along, S.nFx_min);
    return fmax(fmin((F + Fd) / S.m, S.nax_min), real(0.0));
}
PG_DEV real sp_step(real W, real ds, real a) {
#pragma clang fp contract(off)
    const real two_ds = real(2.0) * ds;
    const real d = two_ds * a;
    return W + d;
}
PG_DEV real sp_slope(real Wn, real W, real ds) {
#pragma clang fp contract(off)
    const real num = Wn - W, den = real(2.0) * ds;
    return num / den;
}
PG_DEV real sp_usage(const SpeedSet& S, real W, real A, real kappa) {
#pragma clang fp contract(off)
    const real lat = W * kappa;
    const real a2 = A * A, l2 = lat * lat;
    return sqrt(a2 + l2) / S.a_lim;
}
PG_DEV real sp_dt(real ds, real Va, real Vb) {
#pragma clang fp contract(off)
    const real num = real(2.0) * ds, den = Va + Vb;
    return num / den;
}

__global__ __launch_bounds__(64) void k_speed_plan(SpeedPlanArgs P) {
    const int lane = threadIdx.x, path = blockIdx.x, set0 = blockIdx.y * P.spw;
    // lanes that own a trajectory.  The others (past spw, or past n_sets in the last wavefront) follow the last live lane: they load from ITS trajectory (valid
    // addresses, which that lane is writing: whatever they read is discarded), repeat the arithmetic and store nothing -- the loops stay wave-uniform without a mask
    const int nv = min(P.spw, P.n_sets - set0);
    const int col = min(lane, nv - 1);
    const bool live = lane < nv;
    const SpeedSet S = P.sets[set0 + col];
    const int L = P.L[path], n = L - 1, i0 = P.i0[path];
    const bool closed = i0 >= 0;
    const size_t Lmax = (size_t)P.Lmax;
    const real* __restrict__ s = P.in + ((size_t)path * 10 + SP_S) * Lmax;
    const real* __restrict__ kap = P.in + ((size_t)path * 10 + SP_KAPPA) * Lmax;
    real* const o = P.out + ((size_t)path * P.n_sets + set0 + col) * 10 * Lmax;          // this lane's trajectory: every knot index below is < L <= Lmax
    auto put = [&](int ch, int knot, real v) { if (live) o[ch * Lmax + knot] = v; };
    auto get = [&](int ch, int knot) -> real { return o[ch * Lmax + knot]; };
    // W of a knot before the passes: its cap, the end knots of an open path lowered to the given end speeds
    auto init_of = [&](int k) -> real {
        real c = sp_cap(S, kap[k]);
        if (!closed && k == 0 && S.Wstart == S.Wstart) c = fmin(c, S.Wstart);
        if (!closed && k == n && S.Wend == S.Wend) c = fmin(c, S.Wend);
        return c;
    };

    // ---- backward pass: open from knot L-1 down to 0; closed from i0 once around (L-2 steps: i0 itself is not revisited) ----
    {
        int i = closed ? i0 : n;
        real W = init_of(i);
        put(SP_V, i, W);
        const int steps = closed ? n - 1 : n;
        for (int j = 0; j < steps; j++) {
            const int ip = (closed && i == 0) ? n - 1 : i - 1;      // the knot this step reaches; it comes from knot i (= ip + 1, modulo L-1 on a closed path)
            const real cand = sp_step(W, s[ip + 1] - s[ip], sp_dec(S, W, kap[i]));
            const real ini = init_of(ip);
            W = cand < ini ? cand : ini;
            put(SP_V, ip, W);
            i = ip;
        }
    }
    // ---- forward pass ----
    int n_cap = 0, n_accel = 0, n_brake = 0;
    auto count = [&](int lim) { n_cap += lim == SP_CAP; n_accel += lim == SP_ACCEL; n_brake += lim == SP_BRAKE; };
    real usage = real(0.0);
    {
        int i = closed ? i0 : 0;
        real W = get(SP_V, i);
        const real Whome = W;
        int lim = W < init_of(i) ? SP_BRAKE : SP_CAP, lim0 = lim;
        count(lim);
        real W0 = W, A0 = real(0.0);
        for (int j = 0; j < n; j++) {
            const int nx = (closed && i + 1 == n) ? 0 : i + 1;
            const real ds = s[i + 1] - s[i];
            real Wn;
            if (closed && nx == i0) Wn = Whome;                     // the step that arrives at i0 again leaves it alone
            else {
                const real Wb = get(SP_V, nx);
                lim = Wb < init_of(nx) ? SP_BRAKE : SP_CAP;
                const real cand = fmax(sp_step(W, ds, sp_acc(S, W, kap[i])), S.Wfloor);
                Wn = Wb;
                if (cand < Wb) { Wn = cand; lim = SP_ACCEL; }
                count(lim);
                if (nx == 0) lim0 = lim;
            }
            const real A = sp_slope(Wn, W, ds);
            put(SP_V, i, sqrt(W)); put(SP_A, i, A);
            usage = fmax(usage, sp_usage(S, W, A, kap[i]));
            if (i == 0) { W0 = W; A0 = A; }
            W = Wn; i = nx;
        }
        // knot L-1: open, the last knot with A = 0; closed, knot 0 again
        const real Wl = closed ? W0 : W, Al = closed ? A0 : real(0.0);
        put(SP_V, n, sqrt(Wl)); put(SP_A, n, Al);
        usage = fmax(usage, sp_usage(S, Wl, Al, kap[n]));
        if (closed) count(lim0);
    }
    // ---- time: t = invcumtrapz(V, s), accumulated in double from knot 0 and rounded on store ----
    {
        double t = 0.0;
        real Vp = get(SP_V, 0), vlo = Vp, vhi = Vp, tl = real(0.0);
        put(SP_T, 0, tl);
        for (int i = 1; i < L; i++) {
            const real Vi = get(SP_V, i);
            t += (double)sp_dt(s[i] - s[i - 1], Vp, Vi);
            tl = (real)t;
            put(SP_T, i, tl);
            vlo = fmin(vlo, Vi); vhi = fmax(vhi, Vi); Vp = Vi;
        }
        if (live) {
            pg_speed_plan_stats T;
            T.t_end = (double)tl; T.v_min = (double)vlo; T.v_max = (double)vhi; T.usage_max = (double)usage;
            T.n_cap = n_cap; T.n_accel = n_accel; T.n_brake = n_brake; T.reserved = 0;
            P.stats[(size_t)path * P.n_sets + set0 + lane] = T;
        }
    }
}

// the seven geometry channels of every valid knot, copied from the path to each of its n_sets outputs; every channel zeroed at and past L.  One element per thread
__global__ __launch_bounds__(256) void k_speed_plan_copy(SpeedPlanArgs P, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t Lmax = (size_t)P.Lmax;
    const size_t row = e / Lmax; const int knot = (int)(e - row * Lmax);
    const size_t k = row / 10; const int ch = (int)(row - k * 10);
    const int path = (int)(k / (size_t)P.n_sets);
    const bool valid = knot < P.L[path];
    if (valid && (ch == SP_T || ch == SP_V || ch == SP_A)) return;      // the plan kernel's
    P.out[e] = valid ? P.in[((size_t)path * 10 + ch) * Lmax + knot] : real(0.0);
}
