// pg_refine_paths: every (path, refine set) pair of a path library and a library of refine sets as a trajectory -- the same path with more knots where a manoeuvre or an
// obstacle needs them -- on the device.  The reference reads its paths from files (ros_integration.jl:13-16) or makes straight lines (trajectories.jl:46-58), so the scheme
// is build-defined: stated in include/pigeon_mpc.h at pg_refine_paths and in DESIGN.md 4.23, tests/path_refine_numpy.py is the independent numpy twin.  Included by
// pg_kernels.hip inside namespace pg.
//
// One workgroup of 256 threads per output trajectory (path * n_sets + set), one launch.  Source interval i is cut into m_i equal parts; every source knot stays a knot.
// Four phases, separated by workgroup barriers, which hand their intermediates over in the call's scratch memory (LDS holds the four wavefront totals of the scan and the
// reductions of the stats):  m_i of an interval and the integer exclusive prefix o_i, thread b owning block b of c = ceil((L - 1) / 256) consecutive intervals as in
// k_path_offset;  the whole-interval quadrature and its closure, one interval per thread, strided;  the output knots, strided -- a binary search of the offsets, then a
// copy (sub-knot 0) or an evaluation --, then the tails;  the stats.  The source is read as the doubles given, ALL arithmetic is double in both libraries, without
// contraction, and rounded to `real` on store (tools/check_f32_purity.py lists k_path_refine for this reason, as k_path_offset).  No atomics, no kernel waits on another.

enum { RF_M_MAX = 4096, RF_THREADS = 256 };

// m_i of the source interval [u_lo, u_hi] (arc length from the first knot) of length diff under the set S; RF_M_MAX + 1 stands for every count above RF_M_MAX.  ONE
// function for host and device: the host sizes every pair with it before the first allocation
__host__ __device__ inline int rf_parts(const pg_refine_set& S, double diff, double u_lo, double u_hi) {
#pragma clang fp contract(off)
    double w = S.ds;
    for (int j = 0; j < 4; j++)
        if (S.s_lo[j] < INFINITY && S.s_lo[j] < u_hi && S.s_hi[j] > u_lo) w = fmin(w, S.ds_w[j]);
    if (!(w < INFINITY) || diff <= w) return 1;
    const double q = diff / w;
    if (!(q <= (double)RF_M_MAX)) return RF_M_MAX + 1;
    return (int)ceil(q);
}

// psi_i + (v (a + (v b))): the heading v metres into an interval
struct RefineArc { double psi0, a, b; };
__host__ __device__ inline double rf_psi(const RefineArc& C, double v) {
#pragma clang fp contract(off)
    const double vb = v * C.b;
    const double in = C.a + vb;
    const double tp = v * in;
    return C.psi0 + tp;
}
// the 4-point Gauss-Legendre piece [va, vb] of (-sin psi, cos psi), as pg_make_paths states it
PG_DEV void rf_piece(const RefineArc& C, double va, double vb, double& pE, double& pN) {
#pragma clang fp contract(off)
    const double X[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
    const double Wt[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
    const double dv = vb - va, sv = va + vb;
    const double half = 0.5 * dv, mid = 0.5 * sv;
    double aS = 0.0, aC = 0.0;
    for (int q = 0; q < 4; q++) {
        const double hx = half * X[q];
        const double v = mid + hx;
        double sn, cs;
        sincos(rf_psi(C, v), &sn, &cs);
        const double ws = Wt[q] * sn, wc = Wt[q] * cs;
        aS = aS + ws; aC = aC + wc;
    }
    const double hs = half * aS;
    pE = -hs; pN = half * aC;
}
// the integral over [0, v] in two pieces, [0, 0.5 v] and [0.5 v, v]
PG_DEV void rf_integral(const RefineArc& C, double v, double& IE, double& IN) {
#pragma clang fp contract(off)
    const double hv = 0.5 * v;
    double e0, n0, e1, n1;
    rf_piece(C, 0.0, hv, e0, n0);
    rf_piece(C, hv, v, e1, n1);
    IE = e0 + e1; IN = n0 + n1;
}

// in [n_path][10][Lmax] doubles as the caller gave them; out [n_path * n_sets][10][Lmax_out]; len [n_path * n_sets]: L_out of a pair as the host computed it; off
// [n_path * n_sets][Lmax] ints (o_i); clos [n_path * n_sets][2][Lmax] doubles (the closure of an interval in E and in N); t_end [n_path * n_sets]: t of the last knot as
// stored; bad [n_path * n_sets]: s does not increase strictly as `real` holds it
struct PathRefineArgs { int n_sets, Lmax, Lmax_out; const int* L; const int* len; const double* in; const pg_refine_set* sets; real* out; int* off; double* clos; double* t_end; pg_refine_stats* stats; int* bad; };
enum { RF_T = 0, RF_S = 1, RF_V = 2, RF_A = 3, RF_E = 4, RF_N = 5, RF_PSI = 6, RF_KAPPA = 7, RF_EL = 8, RF_ER = 9 };

__global__ __launch_bounds__(RF_THREADS) void k_path_refine(PathRefineArgs P) {
#pragma clang fp contract(off)
    __shared__ int sW[RF_THREADS / 64];                           // the wavefront totals of the scan
    __shared__ double sR[RF_THREADS / 64][5];                     // ds min / max, closure_pos max, closure_psi max, |kappa| max of a wavefront
    __shared__ int sI[RF_THREADS / 64][2];                        // m max, bad
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t k = blockIdx.x, Lmax = (size_t)P.Lmax, Lout = (size_t)P.Lmax_out;
    const int path = (int)(k / (size_t)P.n_sets), set = (int)(k - (size_t)path * P.n_sets);
    const pg_refine_set S = P.sets[set];
    const int n = P.L[path], nint = n - 1, c = (nint + RF_THREADS - 1) / RF_THREADS;
    const int n_out = P.len[k];                                   // <= Lmax_out: the host refused every other pair
    const double* __restrict__ src = P.in + (size_t)path * 10 * Lmax;      // every source knot index below is < n <= Lmax
    const double* __restrict__ s = src + RF_S * Lmax; const double* __restrict__ psi = src + RF_PSI * Lmax; const double* __restrict__ kap = src + RF_KAPPA * Lmax;
    const double* __restrict__ E = src + RF_E * Lmax; const double* __restrict__ N = src + RF_N * Lmax;
    const double* __restrict__ V = src + RF_V * Lmax; const double* __restrict__ T = src + RF_T * Lmax;
    real* const o = P.out + k * 10 * Lout;
    int* const off = P.off + k * Lmax;
    double* const cE = P.clos + k * 2 * Lmax; double* const cN = cE + Lmax;
    const double s0 = s[0];
    const int i_lo = min(tid * c, nint), i_hi = min(i_lo + c, nint);      // block tid: the intervals [i_lo, i_hi)

    // ---- m_i of an interval, the running sums of a block; the scan of the 256 block totals (integers: the order cannot show); o_i ----
    {
        int a = 0;
        for (int i = i_lo; i < i_hi; i++) {
            const double sa = s[i], sb = s[i + 1];
            a += rf_parts(S, sb - sa, sa - s0, sb - s0);
            off[i + 1] = a;
        }
        int x = a;
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
        if (lane == 63) sW[wave] = x;
        int e = __shfl_up(x, 1, 64);
        if (lane == 0) e = 0;
        __syncthreads();
        for (int w = 0; w < wave; w++) e += sW[w];
        for (int i = i_lo; i < i_hi; i++) off[i + 1] += e;        // (this thread's own entries)
        if (tid == 0) off[0] = 0;
    }
    __syncthreads();
    // ---- the whole-interval quadrature and its closure, one interval per thread ----
    auto arc = [&](int i, double diff) -> RefineArc {
#pragma clang fp contract(off)
        const double dk = kap[i + 1] - kap[i], dp = psi[i + 1] - psi[i];
        const double hk = 0.5 * dk;
        RefineArc C;
        C.psi0 = psi[i];
        C.b = hk / diff;
        const double r = dp / diff, bd = C.b * diff;
        C.a = r - bd;
        return C;
    };
    double cpos = 0.0, cpsi = 0.0;
    int mmax = 0;
    for (int i = tid; i < nint; i += RF_THREADS) {
        const double diff = s[i + 1] - s[i];
        const RefineArc C = arc(i, diff);
        double FE, FN;
        rf_integral(C, diff, FE, FN);
        const double dE = E[i + 1] - E[i], dN = N[i + 1] - N[i];
        const double gE = dE - FE, gN = dN - FN;
        cE[i] = gE; cN[i] = gN;
        const double ee = gE * gE, nn = gN * gN;
        const double g2 = ee + nn;
        cpos = fmax(cpos, sqrt(g2));
        const double da = C.a - kap[i];
        const double ad = fabs(da) * diff;
        cpsi = fmax(cpsi, ad);
        mmax = max(mmax, off[i + 1] - off[i]);
    }
    __syncthreads();
    // ---- the output knots, strided: knot j belongs to the interval of the largest i with o_i <= j (o_{L-1} = L_out - 1: the last knot) ----
    double dsmin = INFINITY, dsmax = 0.0, kmax = 0.0;
    int bad = 0;
    for (int j = tid; j < n_out; j += RF_THREADS) {
        int lo = 0, hi = nint;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= j) lo = mid; else hi = mid - 1; }
        const int i = lo, sub = j - off[i];
        double sj, kj;
        if (sub == 0) {                                           // a source knot: its own values
            for (int ch = 0; ch < 10; ch++) o[ch * Lout + j] = (real)src[ch * Lmax + i];
            sj = s[i]; kj = kap[i];
            if (i == nint) P.t_end[k] = (double)(real)T[i];       // trajectory.t[end] as the library holds it
        } else {
            const int m = off[i + 1] - off[i];
            const double diff = s[i + 1] - s[i];
            const double kf = (double)sub, mf = (double)m;
            const double dkf = diff * kf;
            const double tau = dkf / mf;
            sj = s[i] + tau;
            auto lin = [&](const double* __restrict__ x) -> double {
#pragma clang fp contract(off)
                const double dx = x[i + 1] - x[i];
                const double xn = dx * tau;
                const double xq = xn / diff;
                return x[i] + xq;
            };
            kj = lin(kap);
            const RefineArc C = arc(i, diff);
            double IE, IN;
            rf_integral(C, tau, IE, IN);
            const double fr = tau / diff;
            const double fe = fr * cE[i], fn = fr * cN[i];
            const double pe = IE + fe, pn = IN + fn;
            const double wa = V[i] * V[i], wb = V[i + 1] * V[i + 1];
            const double dw = wb - wa;
            const double wn = dw * tau;
            const double wq = wn / diff;
            const double W = wa + wq;
            const double Vj = sqrt(W);
            const double dt = T[i + 1] - T[i];
            const double t2 = 2.0 * tau, va = V[i] + Vj;
            const double part = t2 / va;
            const double d2 = 2.0 * diff, vs = V[i] + V[i + 1];
            const double whole = d2 / vs;
            const double tn = dt * part;
            const double tq = tn / whole;
            o[RF_T * Lout + j] = (real)(T[i] + tq); o[RF_S * Lout + j] = (real)sj; o[RF_V * Lout + j] = (real)Vj; o[RF_A * Lout + j] = (real)src[RF_A * Lmax + i];
            o[RF_E * Lout + j] = (real)(E[i] + pe); o[RF_N * Lout + j] = (real)(N[i] + pn); o[RF_PSI * Lout + j] = (real)rf_psi(C, tau);
            o[RF_KAPPA * Lout + j] = (real)kj; o[RF_EL * Lout + j] = (real)lin(src + RF_EL * Lmax); o[RF_ER * Lout + j] = (real)lin(src + RF_ER * Lmax);
        }
        kmax = fmax(kmax, fabs(kj));
        if (j + 1 < n_out) {                                      // the spacing to the next output knot (i < nint here)
            const int m = off[i + 1] - off[i];
            double sn = s[i + 1];
            if (sub + 1 < m) {
                const double diff = s[i + 1] - s[i];
                const double dkf = diff * (double)(sub + 1);
                const double tau = dkf / (double)m;
                sn = s[i] + tau;
            }
            const double ds = sn - sj;
            dsmin = fmin(dsmin, ds); dsmax = fmax(dsmax, ds);
            bad |= !((real)sn > (real)sj);
        }
    }
    // ---- every channel is 0 at and past L_out ----
    const size_t tail = Lout - (size_t)n_out;
    for (size_t e = tid; e < 10 * tail; e += RF_THREADS) { const size_t ch = e / tail; o[ch * Lout + (size_t)n_out + (e - ch * tail)] = real(0.0); }

    for (int d = 32; d >= 1; d >>= 1) {
        dsmin = fmin(dsmin, __shfl_xor(dsmin, d, 64)); dsmax = fmax(dsmax, __shfl_xor(dsmax, d, 64)); kmax = fmax(kmax, __shfl_xor(kmax, d, 64));
        cpos = fmax(cpos, __shfl_xor(cpos, d, 64)); cpsi = fmax(cpsi, __shfl_xor(cpsi, d, 64));
        mmax = max(mmax, __shfl_xor(mmax, d, 64)); bad |= __shfl_xor(bad, d, 64);
    }
    if (lane == 0) { sR[wave][0] = dsmin; sR[wave][1] = dsmax; sR[wave][2] = cpos; sR[wave][3] = cpsi; sR[wave][4] = kmax; sI[wave][0] = mmax; sI[wave][1] = bad; }
    __syncthreads();
    if (tid == 0) {
        double v[5] = {sR[0][0], sR[0][1], sR[0][2], sR[0][3], sR[0][4]};
        int mm = sI[0][0], b = sI[0][1];
        for (int w = 1; w < RF_THREADS / 64; w++) {
            v[0] = fmin(v[0], sR[w][0]); v[1] = fmax(v[1], sR[w][1]); v[2] = fmax(v[2], sR[w][2]); v[3] = fmax(v[3], sR[w][3]); v[4] = fmax(v[4], sR[w][4]);
            mm = max(mm, sI[w][0]); b |= sI[w][1];
        }
        pg_refine_stats R;
        R.length = s[nint] - s[0]; R.ds_min = v[0]; R.ds_max = v[1]; R.closure_pos_max = v[2]; R.closure_psi_max = v[3]; R.kappa_abs_max = v[4];
        R.n_added = n_out - n; R.m_max = mm; R.reserved = 0.0;
        P.stats[k] = R;
        P.bad[k] = b;
    }
}
