// pg_make_paths: a library of paths made on the device from line, arc and clothoid segments (curvature linear in the arc length within a segment).  The reference has one
// generator (straight_trajectory, trajectories.jl) and reads every other path from a file, so the scheme is build-defined: stated in include/pigeon_mpc.h at pg_make_paths
// and in DESIGN.md 4.16, tests/path_make_numpy.py is the independent numpy twin.  Included by pg_kernels.hip inside namespace pg.
//
// One workgroup of 256 threads per path.  s, psi, kappa, the edges and t of a knot are closed forms of its arc length: parallel in the knot.  E and N are the prefix sum
// of the interval increments (4-point Gauss-Legendre per piece of an interval): thread b owns block b, the c = ceil((n_knots - 1) / 256) consecutive intervals from b c on,
// adds their increments in order from zero and leaves every running sum in the call's scratch memory; the 256 block totals are scanned by doubling inside each wavefront
// (shuffles) and the four wavefront totals are added in order through LDS; a last pass, one knot per thread (coalesced), stores E0 + (P_b + running sum).  c depends on
// the path's own knot count only, so a path's bits do not depend on n_path, on its place in the library or on Lmax.  No atomics, no kernel waits on another, one launch
// (tails and the t, V, A fill included).  ALL arithmetic is double in both libraries and rounded to `real` on store: E and N of the recorded tracks sit 300 m from the
// origin, where a float carries 3e-5 m, and psi accumulates over laps -- a library is made once per sweep (tools/check_f32_purity.py lists k_path_make for this reason).

// one per (path, segment of the path): the segment's start in arc length and heading as the host summed them (pg_api.hip: path_bounds), then the caller's eight numbers
struct PathSeg { double b, psib, length, kappa0, kappa1, eL0, eL1, eR0, eR1, pad; };
struct PathSpec { double E0, N0, psi0, V_ref, total; int seg0, n_seg, n_knots, pad; };      // seg0: into the PathSeg table of the call
// out [n_path][10][Lmax]; scratch [n_path][Lmax][2] doubles (the running sums of E and N inside a block)
struct PathMakeArgs { int Lmax; const PathSpec* specs; const PathSeg* segs; real* out; double* scratch; pg_path_stats* stats; };
enum { PM_T = 0, PM_S = 1, PM_V = 2, PM_A = 3, PM_E = 4, PM_N = 5, PM_PSI = 6, PM_KAPPA = 7, PM_EL = 8, PM_ER = 9, PM_THREADS = 256 };

// No contraction in any of these: every product and sum is rounded once, as the numpy twin rounds it
PG_DEV double pm_lerp(double a0, double a1, double u, double length) {
#pragma clang fp contract(off)
    const double d = a1 - a0;
    const double du = d * u;
    const double q = du / length;
    return a0 + q;
}
PG_DEV double pm_psi(const PathSeg& S, double u) {
#pragma clang fp contract(off)
    const double d = S.kappa1 - S.kappa0;
    const double hd = 0.5 * d;
    const double hdu = hd * u;
    const double q = hdu / S.length;
    const double k = S.kappa0 + q;
    const double uk = u * k;
    return S.psib + uk;
}
PG_DEV double pm_knot_s(int i, int n_knots, double ds, double total) {
#pragma clang fp contract(off)
    return i == n_knots - 1 ? total : (double)i * ds;
}
// the piece [ua, ub] of segment S (local arc length): 4-point Gauss-Legendre of (-sin psi, cos psi), nodes in ascending order
PG_DEV void pm_piece(const PathSeg& S, double ua, double ub, double& dE, double& dN) {
#pragma clang fp contract(off)
    const double X[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
    const double Wt[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
    const double diff = ub - ua, sum = ua + ub;
    const double half = 0.5 * diff, mid = 0.5 * sum;
    double aS = 0.0, aC = 0.0;
    for (int k = 0; k < 4; k++) {
        const double hx = half * X[k];
        const double u = mid + hx;
        double sn, cs;
        sincos(pm_psi(S, u), &sn, &cs);
        const double ws = Wt[k] * sn, wc = Wt[k] * cs;
        aS = aS + ws; aC = aC + wc;
    }
    const double pe = half * aS;
    dE = -pe; dN = half * aC;
}
// the segment of arc length s: the largest j with b_j <= s (b is non-decreasing; j = 0 where none is)
PG_DEV int pm_find(const PathSeg* T, int n_seg, double s) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (T[m].b <= s) lo = m; else hi = m - 1; }
    return lo;
}

__global__ __launch_bounds__(PM_THREADS) void k_path_make(PathMakeArgs P) {
#pragma clang fp contract(off)
    __shared__ double sP[PM_THREADS][2];
    __shared__ double sW[PM_THREADS / 64][2];
    __shared__ double sK[PM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t path = blockIdx.x, Lmax = (size_t)P.Lmax;
    const PathSpec S = P.specs[path];
    const PathSeg* __restrict__ T = P.segs + S.seg0;
    const int n = S.n_knots, nint = n - 1, c = (nint + PM_THREADS - 1) / PM_THREADS;
    const double ds = S.total / (double)nint;
    real* const o = P.out + path * 10 * Lmax;                     // every knot index below is < n <= Lmax
    double* const run = P.scratch + path * 2 * Lmax;              // run[2 i], run[2 i + 1]: the running sums that reach knot i (1 <= i < n)
    auto knot = [&](int i, int j, double s, double u) -> double {     // the closed-form channels of knot i, which lies in segment j at local arc length u
        const PathSeg& G = T[j];
        const double kap = pm_lerp(G.kappa0, G.kappa1, u, G.length);
        o[PM_S * Lmax + i] = (real)s; o[PM_T * Lmax + i] = (real)(s / S.V_ref); o[PM_V * Lmax + i] = (real)S.V_ref; o[PM_A * Lmax + i] = real(0.0);
        o[PM_PSI * Lmax + i] = (real)pm_psi(G, u); o[PM_KAPPA * Lmax + i] = (real)kap;
        o[PM_EL * Lmax + i] = (real)pm_lerp(G.eL0, G.eL1, u, G.length); o[PM_ER * Lmax + i] = (real)pm_lerp(G.eR0, G.eR1, u, G.length);
        return fabs(kap);
    };

    // ---- block tid: intervals [i_lo, i_hi), their start knots, the running sums; the owner of the last interval also takes the last knot ----
    const int i_lo = min(tid * c, nint), i_hi = min(i_lo + c, nint);
    double aE = 0.0, aN = 0.0, kmax = 0.0;
    if (i_lo < i_hi) {
        int j = pm_find(T, S.n_seg, pm_knot_s(i_lo, n, ds, S.total));
        for (int i = i_lo; i < i_hi; i++) {
            const double s = pm_knot_s(i, n, ds, S.total), sn = pm_knot_s(i + 1, n, ds, S.total);
            while (j + 1 < S.n_seg && T[j + 1].b <= s) j++;
            double u = s - T[j].b;
            kmax = fmax(kmax, knot(i, j, s, u));
            // the interval [s, sn], cut at every segment bound strictly inside it; the pieces are added in order
            double dE = 0.0, dN = 0.0, pE, pN;
            while (j + 1 < S.n_seg && T[j + 1].b < sn) {
                pm_piece(T[j], u, T[j].length, pE, pN);
                dE = dE + pE; dN = dN + pN;
                j++; u = 0.0;
            }
            pm_piece(T[j], u, sn - T[j].b, pE, pN);
            dE = dE + pE; dN = dN + pN;
            aE = aE + dE; aN = aN + dN;
            run[2 * (size_t)(i + 1)] = aE; run[2 * (size_t)(i + 1) + 1] = aN;
        }
        if (i_hi == nint) { const int jl = S.n_seg - 1; kmax = fmax(kmax, knot(nint, jl, S.total, T[jl].length)); }
    }

    // ---- the block totals: inclusive scan by doubling inside each wavefront, the wavefront totals added in order ----
    double xE = aE, xN = aN;
    for (int d = 1; d < 64; d <<= 1) {
        const double yE = __shfl_up(xE, d, 64), yN = __shfl_up(xN, d, 64);
        if (lane >= d) { xE = xE + yE; xN = xN + yN; }
    }
    for (int d = 32; d >= 1; d >>= 1) kmax = fmax(kmax, __shfl_xor(kmax, d, 64));
    if (lane == 63) { sW[wave][0] = xE; sW[wave][1] = xN; }
    if (lane == 0) sK[wave] = kmax;
    double eE = __shfl_up(xE, 1, 64), eN = __shfl_up(xN, 1, 64);      // what lies before this block inside its wavefront
    if (lane == 0) { eE = 0.0; eN = 0.0; }
    __syncthreads();
    double gE = 0.0, gN = 0.0;
    for (int w = 0; w < wave; w++) { gE = gE + sW[w][0]; gN = gN + sW[w][1]; }
    sP[tid][0] = gE + eE; sP[tid][1] = gN + eN;
    __syncthreads();                                              // (also: every running sum of the workgroup is in memory)

    // ---- E and N, one knot per thread; knot i >= 1 is reached by interval i - 1 of block (i - 1) / c ----
    for (int i = tid; i < n; i += PM_THREADS) {
        double E = S.E0, N = S.N0;
        if (i > 0) {
            const int b = (i - 1) / c;
            const double qE = sP[b][0] + run[2 * (size_t)i], qN = sP[b][1] + run[2 * (size_t)i + 1];
            E = S.E0 + qE; N = S.N0 + qN;
        }
        o[PM_E * Lmax + i] = (real)E; o[PM_N * Lmax + i] = (real)N;
    }
    // ---- every channel is 0 at and past n_knots ----
    const size_t tail = Lmax - (size_t)n;
    for (size_t e = tid; e < 10 * tail; e += PM_THREADS) { const size_t ch = e / tail; o[ch * Lmax + (size_t)n + (e - ch * tail)] = real(0.0); }

    if (tid == 0) {
        const int b = (nint - 1) / c, jl = S.n_seg - 1;
        const double qE = sP[b][0] + run[2 * (size_t)nint], qN = sP[b][1] + run[2 * (size_t)nint + 1];
        const double E = S.E0 + qE, N = S.N0 + qN;
        pg_path_stats R;
        R.length = S.total; R.turn = pm_psi(T[jl], T[jl].length) - S.psi0;
        R.closure_pos = hypot(E - S.E0, N - S.N0);
        R.closure_psi = 0.0;                                      // the host reduces the turn (pg_api.hip)
        double km = sK[0]; for (int w = 1; w < PM_THREADS / 64; w++) km = fmax(km, sK[w]);
        R.kappa_abs_max = km; R.ds = ds;
        P.stats[path] = R;
    }
}
