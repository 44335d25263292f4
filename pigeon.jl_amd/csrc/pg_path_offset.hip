// pg_offset_paths: every (path, offset set) pair of a path library and a library of offset sets as a trajectory -- the same road d metres to the left, a lane change, a
// pass-by -- on the device.  The reference reads its paths from files (ros_integration.jl:13-16) or makes straight lines (trajectories.jl:46-58), so the scheme is
// build-defined: stated in include/pigeon_mpc.h at pg_offset_paths and in DESIGN.md 4.21, tests/path_offset_numpy.py is the independent numpy twin.  Included by
// pg_kernels.hip inside namespace pg.
//
// One workgroup of 256 threads per output trajectory (path * n_sets + set), one launch.  The scheme is knot-wise: output knot i belongs to source knot i.  Four phases,
// separated by workgroup barriers, which hand their intermediates over in the call's scratch memory (LDS holds the block offsets of the two scans and the reductions of the
// stats):  the extra arc length of an interval (4-point Gauss-Legendre of g - 1), thread b owning block b of c = ceil((L - 1) / 256) consecutive intervals as in
// k_path_make;  s' = s + X, one knot per thread, strided;  dt and A of an interval from the new s, the same blocked order;  the knots, strided -- offset, frame, curvature,
// edges, t --, then the tails.  The source is read as the doubles given, ALL arithmetic is double in both libraries, without contraction, and rounded to `real` on store
// (tools/check_f32_purity.py lists k_path_offset for this reason, as k_path_make and k_path_fit).  No atomics, no kernel waits on another.

struct OffsetEval { double d, d1, d2; };      // the offset and its first and second derivative in the source's arc length
// sigma(tau) = tau^3 (10 - 15 tau + 6 tau^2) over the window [a, b] at u, with its derivatives in u; a = +Inf: no window
__host__ __device__ inline void po_window(double u, double a, double b, double& f, double& f1, double& f2) {
#pragma clang fp contract(off)
    f = 0.0; f1 = 0.0; f2 = 0.0;
    if (!(a < INFINITY)) return;
    const double w = b - a;
    const double num = u - a;
    const double tau = num / w;
    if (!(tau > 0.0)) return;
    if (tau >= 1.0) { f = 1.0; return; }
    const double t6 = 6.0 * tau;
    const double p = t6 - 15.0;
    const double q = tau * p;
    const double r = 10.0 + q;
    const double t2 = tau * tau;
    const double t3 = t2 * tau;
    f = t3 * r;
    const double omt = 1.0 - tau;
    const double z = tau * omt;
    const double zz = z * z;
    const double n1 = 30.0 * zz;
    f1 = n1 / w;
    const double tt = 2.0 * tau;
    const double m = 1.0 - tt;
    const double z60 = 60.0 * z;
    const double n2 = z60 * m;
    const double ww = w * w;
    f2 = n2 / ww;
}
__host__ __device__ inline OffsetEval po_offset(const pg_offset_set& S, double u) {
#pragma clang fp contract(off)
    double r, r1, r2, f, f1, f2;
    po_window(u, S.s_a, S.s_b, r, r1, r2);
    po_window(u, S.s_c, S.s_d, f, f1, f2);
    const double dd = S.d1 - S.d0;
    const double e = r - f, e1 = r1 - f1, e2 = r2 - f2;
    const double de = dd * e;
    OffsetEval o;
    o.d = S.d0 + de; o.d1 = dd * e1; o.d2 = dd * e2;
    return o;
}

// in [n_path][10][Lmax] doubles as the caller gave them; out [n_path * n_sets][10][Lmax]; sp, run [n_path * n_sets][Lmax] doubles (s' of a knot; the running sum that
// reaches a knot inside its block); t_end [n_path * n_sets]: t of the last knot as stored; bad [n_path * n_sets]: s' does not increase strictly as `real` holds it
struct PathOffsetArgs { int n_sets, Lmax; const int* L; const int* closed; const double* in; const pg_offset_set* sets; real* out; double* sp; double* run; double* t_end; pg_offset_stats* stats; int* bad; };
enum { PO_T = 0, PO_S = 1, PO_V = 2, PO_A = 3, PO_E = 4, PO_N = 5, PO_PSI = 6, PO_KAPPA = 7, PO_EL = 8, PO_ER = 9, PO_THREADS = 256 };

// the scan of the 256 block totals as in k_path_make: by doubling inside each wavefront, the wavefront totals added in order; returns what lies before block tid
PG_DEV double po_block_offset(double total, double* sW, int lane, int wave) {
#pragma clang fp contract(off)
    double x = total;
    for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d, 64); if (lane >= d) x = x + y; }
    if (lane == 63) sW[wave] = x;
    double e = __shfl_up(x, 1, 64);
    if (lane == 0) e = 0.0;
    __syncthreads();
    double g = 0.0;
    for (int w = 0; w < wave; w++) g = g + sW[w];
    return g + e;
}

__global__ __launch_bounds__(PO_THREADS) void k_path_offset(PathOffsetArgs P) {
#pragma clang fp contract(off)
    __shared__ double sP[PO_THREADS];                             // what lies before a block, of the scan in hand
    __shared__ double sW[PO_THREADS / 64];
    __shared__ double sR[PO_THREADS / 64][5];                     // ds' min / max, |kappa'| max, x min, |d| max of a wavefront
    __shared__ int sI[PO_THREADS / 64][2];                        // n_outside, bad
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t k = blockIdx.x, Lmax = (size_t)P.Lmax;
    const int path = (int)(k / (size_t)P.n_sets), set = (int)(k - (size_t)path * P.n_sets);
    const pg_offset_set S = P.sets[set];
    const int n = P.L[path], nint = n - 1, c = (nint + PO_THREADS - 1) / PO_THREADS;
    const bool closed = P.closed[path] != 0;
    const double* __restrict__ src = P.in + (size_t)path * 10 * Lmax;      // every knot index below is < n <= Lmax
    const double* __restrict__ s = src + PO_S * Lmax; const double* __restrict__ V = src + PO_V * Lmax; const double* __restrict__ kap = src + PO_KAPPA * Lmax;
    real* const o = P.out + k * 10 * Lmax;
    double* const sp = P.sp + k * Lmax; double* const run = P.run + k * Lmax;
    const double s0 = s[0];
    const int i_lo = min(tid * c, nint), i_hi = min(i_lo + c, nint);      // block tid: the intervals [i_lo, i_hi)

    // ---- the extra arc length of an interval, the running sums of a block ----
    {
        const double X[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
        const double Wt[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
        double a = 0.0;
        for (int i = i_lo; i < i_hi; i++) {
            const double sa = s[i], sb = s[i + 1], ka = kap[i], kb = kap[i + 1];
            const double diff = sb - sa, sum = sa + sb;
            const double half = 0.5 * diff, mid = 0.5 * sum;
            const double dk = kb - ka;
            double acc = 0.0;
            for (int q = 0; q < 4; q++) {
                const double hx = half * X[q];
                const double u = mid + hx;
                const double du = u - sa;
                const double kn = dk * du;
                const double kq = kn / diff;
                const double kappa = ka + kq;
                const OffsetEval D = po_offset(S, u - s0);
                const double kd = kappa * D.d;
                const double x = 1.0 - kd;
                const double xx = x * x, yy = D.d1 * D.d1;
                const double g2 = xx + yy;
                const double g = sqrt(g2);
                const double gm = g - 1.0;
                const double wv = Wt[q] * gm;
                acc = acc + wv;
            }
            const double extra = half * acc;
            a = a + extra;
            run[i + 1] = a;
        }
        sP[tid] = po_block_offset(a, sW, lane, wave);
    }
    __syncthreads();
    // ---- s' = s + X, one knot per thread; knot i >= 1 is reached by interval i - 1 of block (i - 1) / c ----
    for (int i = tid; i < n; i += PO_THREADS) {
        double X = 0.0;
        if (i > 0) X = sP[(i - 1) / c] + run[i];
        sp[i] = s[i] + X;
    }
    __syncthreads();
    // ---- dt and A of an interval from the new s; the running sums of dt ----
    double dsmin = INFINITY, dsmax = 0.0;
    int bad = 0;
    {
        double a = 0.0;
        for (int i = i_lo; i < i_hi; i++) {
            const double pa = sp[i], pb = sp[i + 1], va = V[i], vb = V[i + 1];
            const double ds = pb - pa;
            const double ds2 = 2.0 * ds;
            const double vs = va + vb;
            const double dt = ds2 / vs;
            const double wa = va * va, wb = vb * vb;
            const double dw = wb - wa;
            o[PO_A * Lmax + i] = (real)(dw / ds2);
            a = a + dt;
            run[i + 1] = a;
            dsmin = fmin(dsmin, ds); dsmax = fmax(dsmax, ds);
            bad |= !((real)pb > (real)pa);
        }
        sP[tid] = po_block_offset(a, sW, lane, wave);             // (every thread has read sP of the first scan: the barrier after the s' pass)
    }
    __syncthreads();
    // ---- the knots, one per thread ----
    struct Placed { double d, x, E, N; };
    auto place = [&](int i, OffsetEval& D) -> Placed {
#pragma clang fp contract(off)
        D = po_offset(S, s[i] - s0);
        double sn, cs;
        sincos(src[PO_PSI * Lmax + i], &sn, &cs);
        const double kd = kap[i] * D.d;
        const double dc = D.d * cs, dsn = D.d * sn;
        Placed R;
        R.d = D.d; R.x = 1.0 - kd; R.E = src[PO_E * Lmax + i] - dc; R.N = src[PO_N * Lmax + i] - dsn;
        return R;
    };
    double kmax = 0.0, xmin = INFINITY, dmax = 0.0;
    int n_out = 0;
    for (int i = tid; i < n; i += PO_THREADS) {
        OffsetEval D;
        const Placed R = place(i, D);
        // kappa_s: central inside, one-sided at the ends of an open path, wrapped over the knots 0 .. L-2 on a closed one (knot L-1 is knot 0 again)
        double ks;
        if (closed && (i == 0 || i == nint)) {
            const double dk = kap[1] - kap[nint - 1];
            const double h0 = s[1] - s[0], h1 = s[nint] - s[nint - 1];
            const double hs = h0 + h1;
            ks = dk / hs;
        } else {
            const int ia = i > 0 ? i - 1 : 0, ib = i < nint ? i + 1 : nint;
            const double dk = kap[ib] - kap[ia];
            const double hs = s[ib] - s[ia];
            ks = dk / hs;
        }
        const double y = D.d1;
        const double xx = R.x * R.x, yy = y * y;
        const double g2 = xx + yy;
        const double g = sqrt(g2);
        const double a0 = ks * D.d, a1 = kap[i] * D.d1;
        const double as = a0 + a1;
        const double t0 = R.x * D.d2, t1 = y * as;
        const double num = t0 + t1;
        const double q = num / g2;
        const double kq = kap[i] + q;
        const double kp = kq / g;
        double eL = src[PO_EL * Lmax + i], eR = src[PO_ER * Lmax + i];
        if (S.edge_mode == 0) { eL = eL - D.d; eR = eR - D.d; }
        double t = src[PO_T * Lmax + 0];
        if (i > 0) { const double T = sP[(i - 1) / c] + run[i]; t = t + T; }
        if (i == nint) {                                          // A of the last knot: 0, or A_0 again on a closed path (the other knots: the interval's owner stored it)
            double A = 0.0;
            if (closed) {
                const double ds = sp[1] - sp[0];
                const double ds2 = 2.0 * ds;
                const double wa = V[0] * V[0], wb = V[1] * V[1];
                const double dw = wb - wa;
                A = dw / ds2;
            }
            o[PO_A * Lmax + i] = (real)A;
            P.t_end[k] = (double)(real)t;                         // trajectory.t[end] as the library holds it
        }
        o[PO_T * Lmax + i] = (real)t; o[PO_S * Lmax + i] = (real)sp[i]; o[PO_V * Lmax + i] = (real)V[i];
        o[PO_E * Lmax + i] = (real)R.E; o[PO_N * Lmax + i] = (real)R.N;
        o[PO_PSI * Lmax + i] = (real)(src[PO_PSI * Lmax + i] + atan2(y, R.x));
        o[PO_KAPPA * Lmax + i] = (real)kp; o[PO_EL * Lmax + i] = (real)eL; o[PO_ER * Lmax + i] = (real)eR;
        kmax = fmax(kmax, fabs(kp)); xmin = fmin(xmin, R.x); dmax = fmax(dmax, fabs(D.d));
        n_out += !(eR < 0.0 && 0.0 < eL);
    }
    // ---- every channel is 0 at and past L ----
    const size_t tail = Lmax - (size_t)n;
    for (size_t e = tid; e < 10 * tail; e += PO_THREADS) { const size_t ch = e / tail; o[ch * Lmax + (size_t)n + (e - ch * tail)] = real(0.0); }

    for (int d = 32; d >= 1; d >>= 1) {
        dsmin = fmin(dsmin, __shfl_xor(dsmin, d, 64)); dsmax = fmax(dsmax, __shfl_xor(dsmax, d, 64)); kmax = fmax(kmax, __shfl_xor(kmax, d, 64));
        xmin = fmin(xmin, __shfl_xor(xmin, d, 64)); dmax = fmax(dmax, __shfl_xor(dmax, d, 64));
        n_out += __shfl_xor(n_out, d, 64); bad |= __shfl_xor(bad, d, 64);
    }
    if (lane == 0) { sR[wave][0] = dsmin; sR[wave][1] = dsmax; sR[wave][2] = kmax; sR[wave][3] = xmin; sR[wave][4] = dmax; sI[wave][0] = n_out; sI[wave][1] = bad; }
    __syncthreads();
    if (tid == 0) {
        double v[5] = {sR[0][0], sR[0][1], sR[0][2], sR[0][3], sR[0][4]};
        int no = sI[0][0], b = sI[0][1];
        for (int w = 1; w < PO_THREADS / 64; w++) {
            v[0] = fmin(v[0], sR[w][0]); v[1] = fmax(v[1], sR[w][1]); v[2] = fmax(v[2], sR[w][2]); v[3] = fmin(v[3], sR[w][3]); v[4] = fmax(v[4], sR[w][4]);
            no += sI[w][0]; b |= sI[w][1];
        }
        OffsetEval D;
        const Placed a = place(0, D), z = place(nint, D);
        const double gE = z.E - a.E, gN = z.N - a.N;
        const double ee = gE * gE, nn = gN * gN;
        const double g2 = ee + nn;
        pg_offset_stats R;
        R.length = sp[nint] - sp[0]; R.ds_min = v[0]; R.ds_max = v[1]; R.kappa_abs_max = v[2]; R.x_min = v[3]; R.d_abs_max = v[4]; R.closure_pos = sqrt(g2);
        R.n_outside = no; R.reserved = 0;
        P.stats[k] = R;
        P.bad[k] = b;
    }
}
