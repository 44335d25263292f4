// pg_optimize_line: every (path, line set) pair of a library of waypoint lists and a library of line sets as waypoints moved along their normals, inside their own
// edge_R .. edge_L, to the least discrete bending energy -- a box-constrained pentadiagonal QP per pair, solved by ADMM on one band factorisation -- on the device.  The
// reference reads its paths from files (ros_integration.jl:13-16), so the scheme is build-defined: stated in include/pigeon_mpc.h at pg_optimize_line and in DESIGN.md
// 4.26, tests/line_opt_numpy.py is the independent twin.  Included by pg_kernels.hip inside namespace pg, after pg_waypoint_smooth.hip (SmoothSpec, ws_setup, ws_tree).
//
// One workgroup of 256 threads per pair (path * n_sets + set), one launch; the phases are separated by workgroup barriers and hand their intermediates over in the call's
// scratch memory.  Strided over the waypoints, thread t owning t, t + 256, .. in every such phase: chords, U (ws_setup of the smoother), normals, weights, the Hessian's
// band and g in closed form, the box; then per iteration the right-hand side, the clip, the dual update and the two residual maxima; then the output and the stats.  The
// serial part -- the band recurrence forward and back, and the border of a closed path -- runs in lane 0 of wavefront 0 (pg_line_opt.hpp: lo_solve; at the
// factorisation lane 1 carries the second border column).  Its state (l1, l2, d, the right-hand side, Za, Zb) lives in LDS where the path has at most LO_LDS_ROWS rows
// (dynamic LDS, sized by the host to the call's longest path) and in the call's scratch beyond; the arithmetic is the same, so the choice cannot show in the bits.  The
// loop's exit is decided from two maxima every thread reduces in the same order: uniform per workgroup.  ALL arithmetic is double, without contraction: both libraries
// return the same bits (tools/check_f32_purity.py lists k_line_opt).  No atomics, no kernel waits on another, plain vector stores.

#include "pg_line_opt.hpp"

// in [n_wp_total]; out [n_sets][n_wp_total], every block the input on entry; scratch [n_sets][n_used][LO_ARRAYS] doubles, a pair's arrays n_wp long each;
// lds_rows: the rows the launch's dynamic LDS holds (6 arrays of that many doubles): the call's longest path, at most LO_LDS_ROWS;
// bad [n_pair][3]: the first waypoint with a pivot that is not > 0, a non-finite output, a chord of the output that is not > 0 (-1: none)
struct LineOptArgs { int n_sets, n_wp_total, lds_rows; long long n_used; const SmoothSpec* specs; const pg_line_set* sets; const pg_waypoint* in; pg_waypoint* out; double* scratch; pg_line_stats* stats; int* bad; };
enum { LO_H = 0, LO_P, LO_U, LO_W, LO_SE, LO_SN, LO_NE, LO_NN, LO_FE, LO_FN, LO_G, LO_LO, LO_HI, LO_D, LO_E1, LO_E2, LO_Z, LO_UD, LO_REC, LO_ARRAYS = LO_REC + 6, LO_LDS_ROWS = 1024 };

__global__ __launch_bounds__(WS_THREADS) void k_line_opt(LineOptArgs P) {
#pragma clang fp contract(off)
    extern __shared__ double sRec[];                              // l1, l2, d, x, Za, Zb: 6 x lds_rows doubles
    __shared__ double sW[WS_THREADS / 64], sT[WS_THREADS / 64];
    __shared__ double sM[WS_THREADS / 64][2];                     // the residual maxima of the wavefronts
    __shared__ double sR[WS_THREADS / 64][5];                     // |alpha| max, its index, n_active, width min, chord min
    __shared__ int sB[WS_THREADS / 64][2];
    __shared__ double sPiv, sBa, sBb, sXa, sXb; __shared__ int sBadRow;
    const size_t k = blockIdx.x;
    const int path = (int)(k / (size_t)P.n_sets), set = (int)(k - (size_t)path * P.n_sets);
    const SmoothSpec S = P.specs[path];
    const pg_line_set T = P.sets[set];
    const pg_waypoint* __restrict__ W = P.in + S.wp0;
    pg_waypoint* const O = P.out + (size_t)set * (size_t)P.n_wp_total + (size_t)S.wp0;
    double* const A = P.scratch + ((size_t)set * (size_t)P.n_used + (size_t)S.soff) * LO_ARRAYS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n_wp, nsp = S.closed ? n : n - 1;             // every waypoint index below is < n_wp
    const bool closed = S.closed != 0;
    const size_t sn = (size_t)n;
    double* const aH = A + LO_H * sn; double* const aP = A + LO_P * sn; double* const aU = A + LO_U * sn; double* const aW = A + LO_W * sn;
    double* const aSE = A + LO_SE * sn; double* const aSN = A + LO_SN * sn; double* const aNE = A + LO_NE * sn; double* const aNN = A + LO_NN * sn;
    double* const aFE = A + LO_FE * sn; double* const aFN = A + LO_FN * sn; double* const aG = A + LO_G * sn; double* const aLo = A + LO_LO * sn; double* const aHi = A + LO_HI * sn;
    double* const aD = A + LO_D * sn; double* const aE1 = A + LO_E1 * sn; double* const aE2 = A + LO_E2 * sn; double* const aZ = A + LO_Z * sn; double* const aUd = A + LO_UD * sn;
    // the rows of the band system: all n of an open path, 0 .. n - 3 of a closed one (its last two unknowns are the border)
    const int m = closed ? n - 2 : n;
    const bool in_lds = m <= P.lds_rows;
    const size_t rs = in_lds ? (size_t)P.lds_rows : sn;          // m <= rs
    double* const rec = in_lds ? sRec : A + LO_REC * sn;
    double* const rL1 = rec; double* const rL2 = rec + rs; double* const rPv = rec + 2 * rs; double* const rX = rec + 3 * rs; double* const rZa = rec + 4 * rs; double* const rZb = rec + 5 * rs;
    auto prev = [&](int i) -> int { return i > 0 ? i - 1 : n - 1; };
    auto next = [&](int i) -> int { return i + 1 == n ? 0 : i + 1; };

    // ---- chords, 1 / h, slopes and U: the smoother's own phases (its winv, 1 under the identity set, lands in aW and is overwritten below) ----
    {
        pg_smooth_set I; I.lambda = 0.0; I.n_win = 0; I.pin_ends = 0; I.keep_walls = 0; I.reserved = 0;
        for (int j = 0; j < 4; j++) { I.u_lo[j] = 0.0; I.u_hi[j] = 0.0; I.factor[j] = 1.0; }
        ws_setup(S, I, W, aH, aP, aU, aW, aSE, aSN, sW);
    }
    // ---- normals, weights and f ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const int im = prev(i), ip = next(i);
        const int ia = !closed && i == 0 ? 0 : im, ib = !closed && i == n - 1 ? n - 1 : ip;
        double nE, nN;
        lo_normal(W[ia].E, W[ia].N, W[ib].E, W[ib].N, nE, nN);
        aNE[i] = nE; aNN[i] = nN;
        aFE[i] = aSE[i] - aSE[im]; aFN[i] = aSN[i] - aSN[im];
        aW[i] = closed || (i > 0 && i < n - 1) ? lo_weight(aH[im], aH[i]) : 0.0;      // (the place ws_setup filled for this same thread's waypoint)
    }
    __syncthreads();
    // ---- the band of K = H + rho I, g, the box, and the start z = clip(0), u = 0 ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const int im = prev(i), ip = next(i), ip2 = next(ip);
        const double nE = aNE[i], nN = aNN[i];
        const double c0 = lo_dot(nE, nN, nE, nN), c1 = lo_dot(nE, nN, aNE[ip], aNN[ip]), c2 = lo_dot(nE, nN, aNE[ip2], aNN[ip2]);
        const double pm = aP[im], p0 = aP[i];
        const double wm = aW[im], w0 = aW[i], w1 = aW[ip];
        double D, E1, E2;
        lo_hessian(T.mu, pm, p0, aP[ip], wm, w0, w1, c0, c1, c2, D, E1, E2);
        aD[i] = D + T.rho; aE1[i] = E1; aE2[i] = E2;
        const double npm = -pm;
        const double q = npm - p0;
        aG[i] = lo_grad(pm, q, p0, wm * aFE[im], w0 * aFE[i], w1 * aFE[ip], wm * aFN[im], w0 * aFN[i], w1 * aFN[ip], nE, nN);
        double lo, hi;
        lo_box(T.margin, T.alpha_max, T.n_win, T.u_lo, T.u_hi, T.win_margin, T.win_pin, aU[i], W[i].edge_L, W[i].edge_R, T.pin_ends && !closed && (i == 0 || i == n - 1), lo, hi);
        aLo[i] = lo; aHi[i] = hi;
        aZ[i] = lo_clip(0.0, lo, hi); aUd[i] = 0.0;
    }
    if (tid == 0) { sPiv = INFINITY; sBadRow = m; sBa = 0.0; sBb = 0.0; sXa = 0.0; sXb = 0.0; }
    __syncthreads();
    // ---- a closed path: the two border columns through the band, once; lane 0 stores the factor ----
    WsBorder B;
    for (int c = 0; c < 3; c++) { B.ra[c] = 0; B.rb[c] = 0; B.ca[c] = 0.0; B.cb[c] = 0.0; }
    B.S00 = 1.0; B.S01 = 0.0; B.S11 = 1.0; B.det = 1.0;
    if (closed) {
        for (int r = tid; r < m; r += WS_THREADS) {
            rZa[r] = r == 0 ? aE2[n - 2] : r == n - 4 ? aE2[n - 4] : r == n - 3 ? aE1[n - 3] : 0.0;
            rZb[r] = r == 0 ? aE1[n - 1] : r == 1 ? aE2[n - 1] : r == n - 3 ? aE2[n - 3] : 0.0;
        }
        __syncthreads();
        if (tid < 2) {
            double pm; int br;
            ws_forward(m, aD, aE1, aE2, tid == 0 ? rZa : rZb, tid == 0, rL1, rL2, rPv, pm, br);
            if (tid == 0) { sPiv = pm; sBadRow = br; }
        }
        __syncthreads();
        if (tid < 2) ws_backward(m, rL1, rL2, rPv, tid == 0 ? rZa : rZb);
        __syncthreads();
        B = ws_border(n, aD, aE1, aE2, rZa, rZb);
    }
    // ---- ADMM: the exit is uniform, every thread holds the same two maxima ----
    double r_prim = 0.0, r_dual = 0.0;
    int done = 0;
    for (int it = 1; it <= T.iters; it++) {
        for (int i = tid; i < n; i += WS_THREADS) {
            const double b = lo_rhs(T.rho, aZ[i], aUd[i], aG[i]);
            if (i < m) rX[i] = b;
            else if (i == n - 2) sBa = b;
            else sBb = b;
        }
        __syncthreads();
        if (tid == 0) {
            double xa, xb, pm; int br;
            const bool store = !closed && it == 1;                // (an open path's factor is stored on the first way forward)
            lo_solve(m, closed, aD, aE1, aE2, rL1, rL2, rPv, store, B, sBa, sBb, rX, xa, xb, pm, br);
            sXa = xa; sXb = xb;
            if (store) { sPiv = pm; sBadRow = br; }
        }
        __syncthreads();
        double rp = 0.0, dz = 0.0;
        {
            const double xa = sXa, xb = sXb;
            for (int i = tid; i < n; i += WS_THREADS) {
                const double x = i < m ? (closed ? lo_unborder(rX[i], rZa[i], rZb[i], xa, xb) : rX[i]) : i == n - 2 ? xa : xb;
                double z = aZ[i], u = aUd[i];
                lo_update(x, aLo[i], aHi[i], z, u, rp, dz);
                aZ[i] = z; aUd[i] = u;
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const double a = __shfl_xor(rp, d, 64), b = __shfl_xor(dz, d, 64);
            if (a > rp) rp = a;
            if (b > dz) dz = b;
        }
        if (lane == 0) { sM[wave][0] = rp; sM[wave][1] = dz; }
        __syncthreads();
        rp = sM[0][0]; dz = sM[0][1];
        for (int w = 1; w < WS_THREADS / 64; w++) { if (sM[w][0] > rp) rp = sM[w][0]; if (sM[w][1] > dz) dz = sM[w][1]; }
        r_prim = rp; r_dual = T.rho * dz; done = it;
        if (r_prim <= T.tol && r_dual <= T.tol) break;            // (sM is written again only after two more barriers)
    }
    __syncthreads();
    // ---- the result: alpha = z ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const double a = aZ[i];
        const pg_waypoint w = W[i];
        pg_waypoint o = w;
        if (a != 0.0) {
            const double dE = a * aNE[i], dN = a * aNN[i];
            o.E = w.E + dE; o.N = w.N + dN;
        }
        if (T.keep_walls) { o.edge_L = w.edge_L - a; o.edge_R = w.edge_R - a; }
        O[i] = o;
    }
    __syncthreads();
    // ---- the stats: the sums over blocks of consecutive waypoints, the rest exact in any order ----
    double amax = -1.0, imax = 0.0, nact = 0.0, wmin = INFINITY, cmin = INFINITY, bin = 0.0, bout = 0.0;
    int bad_fin = -1, bad_chord = -1;
    {
        const int c = (n + WS_THREADS - 1) / WS_THREADS;          // thread b owns block b of c consecutive waypoints
        const int i_lo = min(tid * c, n), i_hi = min(i_lo + c, n);
        for (int i = i_lo; i < i_hi; i++) {
            const int im = prev(i), ip = next(i);
            const double a = aZ[i], am = aZ[im], ap = aZ[ip];
            const double pm = aP[im], p0 = aP[i];
            const double npm = -pm;
            const double q = npm - p0;
            const double w = aW[i];
            bin = bin + lo_term(w, aFE[i], aFN[i]);
            bout = bout + lo_term(w, lo_resid(aFE[i], pm, q, p0, am, a, ap, aNE[im], aNE[i], aNE[ip]), lo_resid(aFN[i], pm, q, p0, am, a, ap, aNN[im], aNN[i], aNN[ip]));
            const double aa = fabs(a);
            if (aa > amax) { amax = aa; imax = (double)i; }
            if (a == aLo[i] || a == aHi[i]) nact = nact + 1.0;
            const pg_waypoint o = O[i];
            wmin = fmin(wmin, o.edge_L - o.edge_R);
            if (!(isfinite(o.E) && isfinite(o.N) && isfinite(o.edge_L) && isfinite(o.edge_R)) && bad_fin < 0) bad_fin = i;
            if (i < nsp) {
                const double gE = O[ip].E - o.E, gN = O[ip].N - o.N;
                const double ge = gE * gE, gn = gN * gN;
                const double g2 = ge + gn;
                const double ch = sqrt(g2);
                cmin = fmin(cmin, ch);
                if (!(ch > 0.0) && bad_chord < 0) bad_chord = i;
            }
        }
    }
    const double bin_tot = ws_tree(bin, sT, lane, wave);
    const double bout_tot = ws_tree(bout, sT, lane, wave);
    auto first = [](int a, int b) -> int { return a < 0 ? b : b < 0 ? a : min(a, b); };
    for (int d = 32; d >= 1; d >>= 1) {
        const double od = __shfl_xor(amax, d, 64), oi = __shfl_xor(imax, d, 64);
        if (od > amax || (od == amax && oi < imax)) { amax = od; imax = oi; }
        wmin = fmin(wmin, __shfl_xor(wmin, d, 64)); cmin = fmin(cmin, __shfl_xor(cmin, d, 64));
        nact = nact + __shfl_xor(nact, d, 64);                    // (a count: exact in any order)
        bad_fin = first(bad_fin, __shfl_xor(bad_fin, d, 64)); bad_chord = first(bad_chord, __shfl_xor(bad_chord, d, 64));
    }
    if (lane == 0) {
        sR[wave][0] = amax; sR[wave][1] = imax; sR[wave][2] = nact; sR[wave][3] = wmin; sR[wave][4] = cmin;
        sB[wave][0] = bad_fin; sB[wave][1] = bad_chord;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WS_THREADS / 64; w++) {
            if (sR[w][0] > amax || (sR[w][0] == amax && sR[w][1] < imax)) { amax = sR[w][0]; imax = sR[w][1]; }
            nact = nact + sR[w][2]; wmin = fmin(wmin, sR[w][3]); cmin = fmin(cmin, sR[w][4]);
            bad_fin = first(bad_fin, sB[w][0]); bad_chord = first(bad_chord, sB[w][1]);
        }
        double pivot_min = sPiv;
        int bad_piv = sBadRow < m ? sBadRow : -1;
        if (closed) {
            const double p2 = B.det / B.S00;
            if (bad_piv < 0 && !(B.S00 > 0.0)) bad_piv = n - 2;
            if (bad_piv < 0 && !(p2 > 0.0)) bad_piv = n - 1;
            pivot_min = fmin(pivot_min, fmin(B.S00, p2));
        }
        pg_line_stats R;
        R.bend_in = bin_tot; R.bend_out = bout_tot; R.alpha_abs_max = amax; R.i_alpha_max = imax; R.n_active = nact; R.r_prim = r_prim; R.r_dual = r_dual;
        R.iters_done = (double)done; R.pivot_min = pivot_min; R.chord_min = cmin; R.width_min = wmin; R.reserved = 0.0;
        P.stats[k] = R;
        P.bad[3 * k] = bad_piv; P.bad[3 * k + 1] = bad_fin; P.bad[3 * k + 2] = bad_chord;
    }
}
