// pg_fit_paths: a library of paths fitted on the device to waypoints (E, N, tube edges): an interpolating cubic spline over the chord-length parameter, natural on an open
// path and periodic on a closed one, resampled at knots equally spaced in arc length.  The reference reads every path from a file, so the scheme is build-defined: stated in
// include/pigeon_mpc.h at pg_fit_paths and in DESIGN.md 4.17, tests/path_fit_numpy.py is the independent numpy twin.  Included by pg_kernels.hip inside namespace pg.
//
// One workgroup of 256 threads per path, one launch; the phases are separated by workgroup barriers and hand their intermediates over in the call's scratch memory (LDS holds
// the scan totals and the reductions of the stats only).  Chords, right-hand sides, span coefficients and span lengths: one span per thread, strided.  The Thomas
// recurrences: lanes 0, 1 (and 2 on a closed path: the Sherman-Morrison correction vector) of wavefront 0, one right-hand side each, every lane with its own copy of the
// pivots -- the three recurrences run in lockstep at the price of one.  The prefix of the span lengths: the blocked order of k_path_make (thread b owns c = ceil(n_span /
// 256) consecutive spans).  Knots: one per thread, strided -- bisection for the span, three Newton steps, the channels, psi_raw to scratch --; the jumps of 2 pi are an
// integer prefix in blocks of ceil(n_knots / 256) knots, and a last strided pass stores psi and zeroes the tails.  No atomics, no kernel waits on another.  ALL arithmetic
// is double in both libraries, without contraction, and rounded to `real` on store (tools/check_f32_purity.py lists k_path_fit for this reason, as k_path_make).

struct FitSpec { double V_ref; long long soff; int wp0, n_wp, n_knots, closed; };      // soff: this path's first double in the span scratch, which holds PF_ARRAYS x (n_wp + 1)
// out [n_path][10][Lmax]; psi_raw, runk [n_path][Lmax]
struct PathFitArgs { int Lmax; const FitSpec* specs; const pg_waypoint* wps; real* out; double* span; double* psi_raw; int* runk; pg_fit_stats* stats; };
// the arrays of a path in the span scratch, each n_wp + 1 doubles: chord; slope of E, N (then c1); right-hand side of E, N, Z (then the solution); the pivots of the three
// lanes (those of E and N then hold M); the diagonal; c3 of E, N; span length; prefix S
enum { PF_H = 0, PF_SE, PF_SN, PF_GE, PF_GN, PF_GZ, PF_BE, PF_BN, PF_BZ, PF_BB, PF_C3E, PF_C3N, PF_L, PF_S, PF_ARRAYS, PF_THREADS = 256 };

struct FitCubic { double y0, c1, M0, c3; };      // y(u) = y0 + u (c1 + u (0.5 M0 + u c3))
PG_DEV double pf_pos(const FitCubic& C, double u) {
#pragma clang fp contract(off)
    const double a = u * C.c3;
    const double hm = 0.5 * C.M0;
    const double b = hm + a;
    const double c = u * b;
    const double d = C.c1 + c;
    const double e = u * d;
    return C.y0 + e;
}
PG_DEV double pf_d1(const FitCubic& C, double u) {
#pragma clang fp contract(off)
    const double k3 = 3.0 * C.c3;
    const double a = u * k3;
    const double b = C.M0 + a;
    const double c = u * b;
    return C.c1 + c;
}
PG_DEV double pf_d2(const FitCubic& C, double u) {
#pragma clang fp contract(off)
    const double k6 = 6.0 * C.c3;
    const double a = u * k6;
    return C.M0 + a;
}
PG_DEV double pf_speed(const FitCubic& A, const FitCubic& B, double u) {
#pragma clang fp contract(off)
    const double a = pf_d1(A, u), b = pf_d1(B, u);
    const double aa = a * a, bb = b * b;
    const double v2 = aa + bb;
    return sqrt(v2);
}
// the piece [ua, ub] of a span: 4-point Gauss-Legendre of the speed, nodes in ascending order (the rule of k_path_make)
PG_DEV double pf_piece(const FitCubic& A, const FitCubic& B, double ua, double ub) {
#pragma clang fp contract(off)
    const double X[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
    const double Wt[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
    const double diff = ub - ua, sum = ua + ub;
    const double half = 0.5 * diff, mid = 0.5 * sum;
    double acc = 0.0;
    for (int k = 0; k < 4; k++) {
        const double hx = half * X[k];
        const double u = mid + hx;
        const double wv = Wt[k] * pf_speed(A, B, u);
        acc = acc + wv;
    }
    return half * acc;
}
PG_DEV double pf_length(const FitCubic& A, const FitCubic& B, double u) {
#pragma clang fp contract(off)
    const double um = 0.5 * u;
    const double p0 = pf_piece(A, B, 0.0, um), p1 = pf_piece(A, B, um, u);
    return p0 + p1;
}
PG_DEV double pf_clamp(double u, double h) { return !(u >= 0.0) ? 0.0 : u > h ? h : u; }
PG_DEV double pf_lerp(double a0, double a1, double u, double length) {
#pragma clang fp contract(off)
    const double d = a1 - a0;
    const double du = d * u;
    const double q = du / length;
    return a0 + q;
}

__global__ __launch_bounds__(PF_THREADS) void k_path_fit(PathFitArgs P) {
#pragma clang fp contract(off)
    __shared__ double sW[PF_THREADS / 64];                        // the wavefront totals of the span-length scan
    __shared__ double sR[PF_THREADS / 64][4];                     // chord min / max, kappa max, s_err max of a wavefront
    __shared__ int sWk[PF_THREADS / 64];
    __shared__ int sPk[PF_THREADS];                               // the jumps before a block of knots
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t path = blockIdx.x, Lmax = (size_t)P.Lmax;
    const FitSpec S = P.specs[path];
    const pg_waypoint* __restrict__ W = P.wps + S.wp0;            // every waypoint index below is < n_wp
    const int nw = S.n_wp, nsp = S.closed ? nw : nw - 1, n = S.n_knots;
    const size_t stride = (size_t)nw + 1;                         // every span / waypoint index below is <= n_wp
    double* const A = P.span + (size_t)S.soff;
    double* const aH = A + PF_H * stride; double* const aSE = A + PF_SE * stride; double* const aSN = A + PF_SN * stride;
    double* const aGE = A + PF_GE * stride; double* const aGN = A + PF_GN * stride; double* const aGZ = A + PF_GZ * stride;
    double* const aBE = A + PF_BE * stride; double* const aBN = A + PF_BN * stride; double* const aBB = A + PF_BB * stride;
    double* const aC3E = A + PF_C3E * stride; double* const aC3N = A + PF_C3N * stride; double* const aL = A + PF_L * stride; double* const aS = A + PF_S * stride;
    real* const o = P.out + path * 10 * Lmax;                     // every knot index below is < n <= Lmax
    double* const praw = P.psi_raw + path * Lmax;
    int* const runk = P.runk + path * Lmax;
    auto next = [&](int j) -> int { return j + 1 == nw ? 0 : j + 1; };      // the waypoint a span ends on (0 again only on a closed path)

    // ---- chords and slopes, one span per thread ----
    double hmin = INFINITY, hmax = 0.0;
    for (int j = tid; j < nsp; j += PF_THREADS) {
        const pg_waypoint a = W[j], b = W[next(j)];
        const double dE = b.E - a.E, dN = b.N - a.N;
        const double ee = dE * dE, nn = dN * dN;
        const double h2 = ee + nn;
        const double h = sqrt(h2);
        aH[j] = h; aSE[j] = dE / h; aSN[j] = dN / h;
        hmin = fmin(hmin, h); hmax = fmax(hmax, h);
    }
    __syncthreads();
    // ---- diagonal and right-hand sides, one waypoint per thread.  Open: rows 1 .. n_wp - 2 (M = 0 at both ends); closed: rows 0 .. n_wp - 1 of the cyclic system ----
    const int lo = S.closed ? 0 : 1, hi = S.closed ? nw - 1 : nw - 2;
    for (int i = tid; i < nw; i += PF_THREADS) {
        double bb = 0.0, gE = 0.0, gN = 0.0, gZ = 0.0;
        if (i >= lo && i <= hi) {
            const int im = i > 0 ? i - 1 : nw - 1;
            const double hs = aH[im] + aH[i];
            bb = 2.0 * hs;
            const double dE = aSE[i] - aSE[im], dN = aSN[i] - aSN[im];
            gE = 6.0 * dE; gN = 6.0 * dN;
            if (S.closed) {
                const double hl = aH[nw - 1];
                const double h0 = hl + aH[0];
                const double b0 = 2.0 * h0;
                if (i == 0) { bb = 2.0 * b0; gZ = -b0; }
                if (i == nw - 1) { const double q = hl * hl; const double qb = q / b0; bb = bb + qb; gZ = hl; }
            }
        }
        aBB[i] = bb; aGE[i] = gE; aGN[i] = gN; aGZ[i] = gZ;
    }
    __syncthreads();
    // ---- the Thomas recurrences: lane r of wavefront 0 solves right-hand side r in place, with its own pivots ----
    if (tid < (S.closed ? 3 : 2) && hi >= lo) {
        double* const g = A + (PF_GE + tid) * stride; double* const be = A + (PF_BE + tid) * stride;
        double bp = aBB[lo], gp = g[lo];
        be[lo] = bp;
        for (int i = lo + 1; i <= hi; i++) {
            const double a = aH[i - 1];
            const double w = a / bp;
            const double wc = w * a, wg = w * gp;
            bp = aBB[i] - wc; gp = g[i] - wg;
            be[i] = bp; g[i] = gp;
        }
        double x = gp / bp;
        g[hi] = x;
        for (int i = hi - 1; i >= lo; i--) {
            const double cx = aH[i] * x;
            const double t = g[i] - cx;
            x = t / be[i];
            g[i] = x;
        }
    }
    __syncthreads();
    // ---- M at the waypoints (into the pivot arrays of E and N, which are done with): the Sherman-Morrison correction on a closed path ----
    {
        double fE = 0.0, fN = 0.0;
        if (S.closed) {
            const double hl = aH[nw - 1];
            const double h0 = hl + aH[0];
            const double b0 = 2.0 * h0;
            const double zq = hl * aGZ[nw - 1];
            const double zb = zq / b0;
            const double z1 = 1.0 + aGZ[0];
            const double den = z1 - zb;
            const double eq = hl * aGE[nw - 1], nq = hl * aGN[nw - 1];
            const double eb = eq / b0, nb = nq / b0;
            const double en = aGE[0] - eb, nn = aGN[0] - nb;
            fE = en / den; fN = nn / den;
        }
        for (int i = tid; i < nw; i += PF_THREADS) {
            double mE = aGE[i], mN = aGN[i];
            if (S.closed) { const double z = aGZ[i]; const double tE = fE * z, tN = fN * z; mE = mE - tE; mN = mN - tN; }
            aBE[i] = mE; aBN[i] = mN;
        }
    }
    __syncthreads();
    // ---- the cubic of a span as the knots read it (c1 over the slope, c3) and its length ----
    auto cubics = [&](int j, FitCubic& CE, FitCubic& CN) {
        CE.y0 = W[j].E; CE.c1 = aSE[j]; CE.M0 = aBE[j]; CE.c3 = aC3E[j];
        CN.y0 = W[j].N; CN.c1 = aSN[j]; CN.M0 = aBN[j]; CN.c3 = aC3N[j];
    };
    for (int j = tid; j < nsp; j += PF_THREADS) {
        const int jn = next(j);
        const double h = aH[j], h6 = 6.0 * h;
        auto coef = [&](double slope, double M0, double M1, double& c1, double& c3) {
#pragma clang fp contract(off)
            const double m2 = 2.0 * M0;
            const double ms = m2 + M1;
            const double hm = h * ms;
            const double q = hm / 6.0;
            c1 = slope - q;
            const double dm = M1 - M0;
            c3 = dm / h6;
        };
        double c1E, c3E, c1N, c3N;
        coef(aSE[j], aBE[j], aBE[jn], c1E, c3E); coef(aSN[j], aBN[j], aBN[jn], c1N, c3N);
        aSE[j] = c1E; aSN[j] = c1N; aC3E[j] = c3E; aC3N[j] = c3N;
        FitCubic CE, CN;
        CE.y0 = W[j].E; CE.c1 = c1E; CE.M0 = aBE[j]; CE.c3 = c3E;
        CN.y0 = W[j].N; CN.c1 = c1N; CN.M0 = aBN[j]; CN.c3 = c3N;
        aL[j] = pf_length(CE, CN, h);
    }
    __syncthreads();
    // ---- S: block tid holds the spans [j_lo, j_hi); the running sums, the scan of the block totals as in k_path_make, then S_{j+1} = P_b + r_{j+1} by the block's owner ----
    {
        const int c = (nsp + PF_THREADS - 1) / PF_THREADS;
        const int j_lo = min(tid * c, nsp), j_hi = min(j_lo + c, nsp);
        double a = 0.0;
        for (int j = j_lo; j < j_hi; j++) { a = a + aL[j]; aS[j + 1] = a; }
        double x = a;
        for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d, 64); if (lane >= d) x = x + y; }
        if (lane == 63) sW[wave] = x;
        double e = __shfl_up(x, 1, 64);
        if (lane == 0) e = 0.0;
        for (int d = 32; d >= 1; d >>= 1) { hmin = fmin(hmin, __shfl_xor(hmin, d, 64)); hmax = fmax(hmax, __shfl_xor(hmax, d, 64)); }
        if (lane == 0) { sR[wave][0] = hmin; sR[wave][1] = hmax; }
        __syncthreads();
        double g = 0.0;
        for (int w = 0; w < wave; w++) g = g + sW[w];
        const double Pb = g + e;
        for (int j = j_lo; j < j_hi; j++) aS[j + 1] = Pb + aS[j + 1];
        if (tid == 0) aS[0] = 0.0;
    }
    __syncthreads();
    // ---- the knots, one per thread: the span by bisection, three Newton steps, the channels; psi_raw goes to scratch ----
    const double total = aS[nsp];
    const double ds = total / (double)(n - 1);
    double kmax = 0.0, serr = 0.0;
    for (int i = tid; i < n; i += PF_THREADS) {
        const bool last = i == n - 1;
        const double s = last ? total : (double)i * ds;
        int j = nsp - 1;
        if (!last) {
            int l = 0, r = nsp - 1;
            while (l < r) { const int m = (l + r + 1) >> 1; if (aS[m] <= s) l = m; else r = m - 1; }
            j = l;
        }
        const int jn = next(j);
        FitCubic CE, CN;
        cubics(j, CE, CN);
        const double h = aH[j];
        const double target = s - aS[j];
        double u = h;
        if (!last) {
            const double th = target * h;
            u = pf_clamp(th / aL[j], h);
            for (int it = 0; it < 3; it++) {
                const double f = pf_length(CE, CN, u) - target;
                const double q = f / pf_speed(CE, CN, u);
                u = pf_clamp(u - q, h);
            }
        }
        serr = fmax(serr, fabs(pf_length(CE, CN, u) - target));
        const double d1E = pf_d1(CE, u), d1N = pf_d1(CN, u), d2E = pf_d2(CE, u), d2N = pf_d2(CN, u);
        const double ee = d1E * d1E, nn = d1N * d1N;
        const double v2 = ee + nn;
        const double v = sqrt(v2);
        const double v3 = v2 * v;
        const double c0 = d1E * d2N, c1 = d2E * d1N;
        const double cr = c0 - c1;
        const double kap = cr / v3;
        kmax = fmax(kmax, fabs(kap));
        const pg_waypoint wa = W[j], wb = W[jn];
        const double E = last ? wb.E : pf_pos(CE, u), N = last ? wb.N : pf_pos(CN, u);
        o[0 * Lmax + i] = (real)(s / S.V_ref); o[1 * Lmax + i] = (real)s; o[2 * Lmax + i] = (real)S.V_ref; o[3 * Lmax + i] = real(0.0);
        o[4 * Lmax + i] = (real)E; o[5 * Lmax + i] = (real)N; o[7 * Lmax + i] = (real)kap;
        o[8 * Lmax + i] = (real)pf_lerp(wa.edge_L, wb.edge_L, u, h); o[9 * Lmax + i] = (real)pf_lerp(wa.edge_R, wb.edge_R, u, h);
        praw[i] = atan2(-d1E, d1N);
    }
    for (int d = 32; d >= 1; d >>= 1) { kmax = fmax(kmax, __shfl_xor(kmax, d, 64)); serr = fmax(serr, __shfl_xor(serr, d, 64)); }
    if (lane == 0) { sR[wave][2] = kmax; sR[wave][3] = serr; }
    __syncthreads();
    // ---- the jumps: block tid holds the knots [i_lo, i_hi); an integer prefix, so its order cannot show ----
    const int ck = (n + PF_THREADS - 1) / PF_THREADS;
    {
        const double pi = 3.141592653589793;
        const int i_lo = min(tid * ck, n), i_hi = min(i_lo + ck, n);
        int a = 0;
        for (int i = i_lo; i < i_hi; i++) {
            if (i > 0) { const double d = praw[i] - praw[i - 1]; a += d > pi ? -1 : d < -pi ? 1 : 0; }
            runk[i] = a;
        }
        int x = a;
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
        if (lane == 63) sWk[wave] = x;
        int e = __shfl_up(x, 1, 64);
        if (lane == 0) e = 0;
        __syncthreads();
        int g = 0;
        for (int w = 0; w < wave; w++) g += sWk[w];
        sPk[tid] = g + e;
    }
    __syncthreads();
    // ---- psi, one knot per thread; every channel is 0 at and past n_knots ----
    auto psi_of = [&](int i) -> double {
#pragma clang fp contract(off)
        const int k = sPk[i / ck] + runk[i];
        const double off = (double)k * 6.283185307179586;
        return praw[i] + off;
    };
    for (int i = tid; i < n; i += PF_THREADS) o[6 * Lmax + i] = (real)psi_of(i);
    const size_t tail = Lmax - (size_t)n;
    for (size_t e = tid; e < 10 * tail; e += PF_THREADS) { const size_t ch = e / tail; o[ch * Lmax + (size_t)n + (e - ch * tail)] = real(0.0); }

    if (tid == 0) {
        pg_fit_stats R;
        R.length = total; R.turn = psi_of(n - 1) - psi_of(0);
        R.closure_psi = 0.0;                                      // the host reduces the turn (pg_api.hip)
        double v[4] = {sR[0][0], sR[0][1], sR[0][2], sR[0][3]};
        for (int w = 1; w < PF_THREADS / 64; w++) { v[0] = fmin(v[0], sR[w][0]); v[1] = fmax(v[1], sR[w][1]); v[2] = fmax(v[2], sR[w][2]); v[3] = fmax(v[3], sR[w][3]); }
        R.chord_min = v[0]; R.chord_max = v[1]; R.kappa_abs_max = v[2]; R.s_err_max = v[3]; R.ds = ds; R.reserved = 0.0;
        // the gap between the last knot (the end waypoint itself) and knot 0 (waypoint 0 itself: u = 0): 0 on a closed path
        const pg_waypoint w0 = W[0], w1 = W[S.closed ? 0 : nw - 1];
        const double gE = w1.E - w0.E, gN = w1.N - w0.N;
        const double ee = gE * gE, nn = gN * gN;
        const double g2 = ee + nn;
        R.closure_pos = sqrt(g2);
        P.stats[path] = R;
    }
}
