// pg_smooth_waypoints: every (path, smoothing set) pair of a library of waypoint lists and a library of smoothing sets as smoothed waypoints -- a cubic smoothing spline
// (Reinsch) of E and of N over the chord-length parameter, natural on an open path and periodic on a closed one -- on the device.  The reference reads its paths from
// files (ros_integration.jl:13-16), so the scheme is build-defined: stated in include/pigeon_mpc.h at pg_smooth_waypoints and in DESIGN.md 4.24,
// tests/wp_smooth_numpy.py is the independent twin.  Included by pg_kernels.hip inside namespace pg.
//
// One workgroup of 256 threads per pair (path * n_sets + set), one launch; the phases are separated by workgroup barriers and hand their intermediates over in the call's
// scratch memory.  Strided over the waypoints: chords and slopes; U by the blocked prefix of k_path_make; winv; the band entries and the right-hand sides in closed form;
// gamma; g; the edge shift and the stats.  The serial part is the band LDL^T recurrence (pg_waypoint_smooth.hpp): lane r of wavefront 0 carries right-hand side r (E, N,
// and on a closed path the two border columns) and repeats the factor recurrence in its own registers, so the lanes run in lockstep at the price of one and exchange
// nothing; lane 0 stores the factor for the way back.  The recurrence's state (l1, l2, d and the four right-hand sides) lives in LDS where the path has at most
// WS_LDS_ROWS rows (dynamic LDS, sized by the host to the call's longest path) and in the call's scratch beyond; the arithmetic is the same, so the choice cannot show in the bits.  Waypoints are doubles in both libraries and ALL
// arithmetic is double, without contraction: both libraries return the same bits (tools/check_f32_purity.py lists k_wp_smooth).  No atomics, no kernel waits on another.

#include "pg_waypoint_smooth.hpp"

struct SmoothSpec { long long soff; int wp0, n_wp, closed, pad; };     // soff: the waypoints of the paths before this one
// in [n_wp_total]; out [n_sets][n_wp_total], every block the input on entry; scratch [n_sets][n_used][WS_ARRAYS] doubles, a pair's arrays n_wp long each;
// lds_rows: the rows the launch's dynamic LDS holds (7 arrays of that many doubles): the call's longest path, at most WS_LDS_ROWS;
// bad [n_pair][4]: the first waypoint with a pivot that is not > 0, a non-finite output, edge_L <= edge_R, a chord that is not > 0 (-1: none)
struct WpSmoothArgs { int n_sets, n_wp_total, lds_rows; long long n_used; const SmoothSpec* specs; const pg_smooth_set* sets; const pg_waypoint* in; pg_waypoint* out; double* scratch; pg_smooth_stats* stats; int* bad; };
enum { WS_H = 0, WS_P, WS_U, WS_WINV, WS_D, WS_E1, WS_E2, WS_FE, WS_FN, WS_GE, WS_GN, WS_L1, WS_L2, WS_PIV, WS_Z, WS_ARRAYS = WS_Z + 4, WS_THREADS = 256, WS_LDS_ROWS = 1024 };

// the sum of one value per thread: the tree of neighbouring pairs (xor 1, 2, .. 32 inside a wavefront, then (w0 + w1) + (w2 + w3)); every thread returns it
PG_DEV double ws_tree(double x, double* sT, int lane, int wave) {
#pragma clang fp contract(off)
    for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_xor(x, d, 64); x = x + y; }
    __syncthreads();
    if (lane == 0) sT[wave] = x;
    __syncthreads();
    const double a = sT[0] + sT[1], b = sT[2] + sT[3];
    return a + b;
}

// Result: g_i = y_i - (lambda (winv_i (((p_im gamma_im) + (q_i gamma_i)) + (p_i gamma_ip))))
PG_DEV double ws_moved(double y, double lambda, double w, double pm, double q, double p0, double gm, double g0, double gp) {
#pragma clang fp contract(off)
    const double a = pm * gm, b = q * g0, c = p0 * gp;
    const double ab = a + b;
    const double qg = ab + c;
    const double wq = w * qg;
    const double lw = lambda * wq;
    return y - lw;
}

// The phases that do not depend on lambda, strided over the waypoints by the workgroup: chords h, p = 1 / h and the slopes (into sE, sN), U, winv; ends on a barrier.
// sW: one double per wavefront
PG_DEV void ws_setup(const SmoothSpec S, const pg_smooth_set& T, const pg_waypoint* __restrict__ W, double* const aH, double* const aP, double* const aU, double* const aWi,
                     double* const aGE, double* const aGN, double* const sW) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n_wp, nsp = S.closed ? n : n - 1;
    const bool closed = S.closed != 0;
    auto next = [&](int i) -> int { return i + 1 == n ? 0 : i + 1; };
    // ---- chords, 1 / h and slopes (into the arrays gamma takes later), one span per thread; place n - 1 of an open path holds 0 ----
    for (int j = tid; j < n; j += WS_THREADS) {
        double h = 0.0, p = 0.0, sE = 0.0, sN = 0.0;
        if (j < nsp) {
            const pg_waypoint a = W[j], b = W[next(j)];
            const double dE = b.E - a.E, dN = b.N - a.N;
            const double ee = dE * dE, nn = dN * dN;
            const double h2 = ee + nn;
            h = sqrt(h2); p = 1.0 / h; sE = dE / h; sN = dN / h;
        }
        aH[j] = h; aP[j] = p; aGE[j] = sE; aGN[j] = sN;
    }
    __syncthreads();
    // ---- U: the blocked prefix of k_path_make over the n - 1 chords between waypoint 0 and waypoint n - 1 ----
    {
        const int nu = n - 1, c = (nu + WS_THREADS - 1) / WS_THREADS;
        const int j_lo = min(tid * c, nu), j_hi = min(j_lo + c, nu);
        double a = 0.0;
        for (int j = j_lo; j < j_hi; j++) { a = a + aH[j]; aU[j + 1] = a; }
        double x = a;
        for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d, 64); if (lane >= d) x = x + y; }
        if (lane == 63) sW[wave] = x;
        double e = __shfl_up(x, 1, 64);
        if (lane == 0) e = 0.0;
        __syncthreads();
        double g = 0.0;
        for (int w = 0; w < wave; w++) g = g + sW[w];
        const double Pb = g + e;
        for (int j = j_lo; j < j_hi; j++) aU[j + 1] = Pb + aU[j + 1];
        if (tid == 0) aU[0] = 0.0;
    }
    __syncthreads();
    // ---- winv: the factor of the last listed window that holds U_i, else 1; pinned ends of an open path ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const double u = aU[i];
        double w = 1.0;
        for (int q = 0; q < 4; q++) if (q < T.n_win && T.u_lo[q] <= u && u <= T.u_hi[q]) w = T.factor[q];
        if (T.pin_ends && !closed && (i == 0 || i == n - 1)) w = 0.0;
        aWi[i] = w;
    }
    __syncthreads();
}

// One pair: the whole scheme for the path S (its waypoints W, its output O) under the set T with the weight `lambda`, by the 256 threads of a workgroup.  A: the pair's
// WS_ARRAYS arrays of n_wp doubles in scratch; sRec: dynamic LDS of 7 x lds_rows doubles; stat, bad [4]: the pair's records.  k_wp_smooth calls it with T.lambda,
// k_wp_tune (pg_waypoint_tune.hip) with the weight it has chosen: one text, so the two return the same bits
PG_DEV void ws_pair(const SmoothSpec S, const pg_smooth_set& T, const double lambda, const int lds_rows, const pg_waypoint* __restrict__ W, pg_waypoint* const O, double* const A,
                    double* const sRec, pg_smooth_stats* const stat, int* const bad) {
#pragma clang fp contract(off)
    __shared__ double sW[WS_THREADS / 64], sT[WS_THREADS / 64];
    __shared__ double sR[WS_THREADS / 64][6];                     // dev max, its index, width min, chord min, n_outside, -
    __shared__ int sB[WS_THREADS / 64][4];
    __shared__ double sPiv; __shared__ int sBadRow;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n_wp, nsp = S.closed ? n : n - 1;             // every waypoint index below is < n_wp
    const bool closed = S.closed != 0;
    const size_t sn = (size_t)n;
    double* const aH = A + WS_H * sn; double* const aP = A + WS_P * sn; double* const aU = A + WS_U * sn; double* const aWi = A + WS_WINV * sn;
    double* const aD = A + WS_D * sn; double* const aE1 = A + WS_E1 * sn; double* const aE2 = A + WS_E2 * sn; double* const aFE = A + WS_FE * sn; double* const aFN = A + WS_FN * sn;
    double* const aGE = A + WS_GE * sn; double* const aGN = A + WS_GN * sn;
    // the rows of the band system: 1 .. n - 2 of an open path, 0 .. n - 3 of a closed one (its last two unknowns are the border)
    const int m = n - 2, base = closed ? 0 : 1, nrhs = closed ? 4 : 2;
    const bool in_lds = m <= lds_rows;
    const size_t rs = in_lds ? (size_t)lds_rows : sn;           // m <= rs
    double* const rec = in_lds ? sRec : A + WS_L1 * sn;
    double* const rL1 = rec; double* const rL2 = rec + rs; double* const rPv = rec + 2 * rs; double* const rZ = rec + 3 * rs;
    auto prev = [&](int i) -> int { return i > 0 ? i - 1 : n - 1; };
    auto next = [&](int i) -> int { return i + 1 == n ? 0 : i + 1; };

    ws_setup(S, T, W, aH, aP, aU, aWi, aGE, aGN, sW);
    // ---- the band entries of every row and the right-hand sides, in closed form ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const int im = prev(i), ip = next(i);
        double dd, e1, e2;
        ws_band(lambda, aH[im], aH[i], aP[im], aP[i], aP[ip], aWi[im], aWi[i], aWi[ip], dd, e1, e2);
        aD[i] = dd; aE1[i] = e1; aE2[i] = e2;
        aFE[i] = aGE[i] - aGE[im]; aFN[i] = aGN[i] - aGN[im];
    }
    __syncthreads();
    // ---- the right-hand sides of the recurrence: E, N, and on a closed path the two border columns ----
    for (int r = tid; r < m; r += WS_THREADS) {
        rZ[r] = aFE[base + r]; rZ[rs + r] = aFN[base + r];
        if (closed) {
            rZ[2 * rs + r] = r == 0 ? aE2[n - 2] : r == n - 4 ? aE2[n - 4] : r == n - 3 ? aE1[n - 3] : 0.0;
            rZ[3 * rs + r] = r == 0 ? aE1[n - 1] : r == 1 ? aE2[n - 1] : r == n - 3 ? aE2[n - 3] : 0.0;
        }
    }
    if (tid == 0) { sPiv = INFINITY; sBadRow = m; }
    __syncthreads();
    // ---- the recurrence, forward: lane r carries right-hand side r and its own copy of the pivots ----
    if (tid < nrhs && m > 0) {
        double pm; int br;
        ws_forward(m, aD + base, aE1 + base, aE2 + base, rZ + (size_t)tid * rs, tid == 0, rL1, rL2, rPv, pm, br);
        if (tid == 0) { sPiv = pm; sBadRow = br; }
    }
    __syncthreads();
    if (tid < nrhs && m > 0) ws_backward(m, rL1, rL2, rPv, rZ + (size_t)tid * rs);
    __syncthreads();
    // ---- gamma at the waypoints: 0 at the natural ends; on a closed path the border's two unknowns and x1 = x0 - Z x2 ----
    double pivot_min = sPiv;
    int bad_piv = sBadRow < m ? base + sBadRow : -1;
    {
        WsBorder B; double xaE = 0.0, xbE = 0.0, xaN = 0.0, xbN = 0.0;
        if (closed) {
            B = ws_border(n, aD, aE1, aE2, rZ + 2 * rs, rZ + 3 * rs);
            ws_border_solve(B, aFE[n - 2], aFE[n - 1], rZ, xaE, xbE);
            ws_border_solve(B, aFN[n - 2], aFN[n - 1], rZ + rs, xaN, xbN);
            const double p2 = B.det / B.S00;
            if (bad_piv < 0 && !(B.S00 > 0.0)) bad_piv = n - 2;
            if (bad_piv < 0 && !(p2 > 0.0)) bad_piv = n - 1;
            pivot_min = fmin(pivot_min, fmin(B.S00, p2));
        }
        for (int i = tid; i < n; i += WS_THREADS) {
            double gE = 0.0, gN = 0.0;
            const int r = i - base;
            if (r >= 0 && r < m) {
                gE = rZ[r]; gN = rZ[rs + r];
                if (closed) {
                    const double za = rZ[2 * rs + r], zb = rZ[3 * rs + r];
                    const double aE = za * xaE, bE = zb * xbE, aN = za * xaN, bN = zb * xbN;
                    const double uE = gE - aE, uN = gN - aN;
                    gE = uE - bE; gN = uN - bN;
                }
            } else if (closed) { gE = i == n - 2 ? xaE : xbE; gN = i == n - 2 ? xaN : xbN; }
            aGE[i] = gE; aGN[i] = gN;
        }
    }
    __syncthreads();
    // ---- g = y - (lambda (winv (Q gamma))) ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const int im = prev(i), ip = next(i);
        const double pm = aP[im], p0 = aP[i];
        const double npm = -pm;
        const double q = npm - p0;
        const double w = aWi[i];
        O[i].E = ws_moved(W[i].E, lambda, w, pm, q, p0, aGE[im], aGE[i], aGE[ip]); O[i].N = ws_moved(W[i].N, lambda, w, pm, q, p0, aGN[im], aGN[i], aGN[ip]);
    }
    __syncthreads();
    // ---- the edges, the displacement, the bend and the chords of the result ----
    double dmax = -1.0, imax = 0.0, wmin = INFINITY, cmin = INFINITY, nout = 0.0, d2sum = 0.0, bsum = 0.0;
    int bad_fin = -1, bad_wall = -1, bad_chord = -1;
    {
        const int c = (n + WS_THREADS - 1) / WS_THREADS;          // the sums: thread b owns block b of c consecutive waypoints
        const int i_lo = min(tid * c, n), i_hi = min(i_lo + c, n);
        for (int i = i_lo; i < i_hi; i++) {
            const int im = prev(i), ip = next(i);
            const pg_waypoint w = W[i];
            const double oE = O[i].E, oN = O[i].N;
            const bool fwd = closed || i < n - 1;                 // the tangent: the smoothed spline's first derivative at the waypoint, from the span that starts
            const int ja = fwd ? i : im, jb = fwd ? ip : i;       // on it (the last waypoint of an open path: from the end of the span that ends on it)
            const double h = aH[ja];
            auto tangent = [&](double ya, double yb, const double* g) -> double {
#pragma clang fp contract(off)
                const double dy = yb - ya;
                const double sl = dy / h;
                const double g2 = 2.0 * g[i];
                const double gs = g2 + g[fwd ? ip : im];
                const double hg = h * gs;
                const double t6 = hg / 6.0;
                return fwd ? sl - t6 : sl + t6;
            };
            const double tE = tangent(O[ja].E, O[jb].E, aGE), tN = tangent(O[ja].N, O[jb].N, aGN);
            const double te = tE * tE, tn = tN * tN;
            const double v2 = te + tn;
            const double v = sqrt(v2);
            const double ntN = -tN;
            const double nE = ntN / v, nN = tE / v;               // the left normal: dE/ds = -sin psi, dN/ds = cos psi, e positive to the left
            const double dE = oE - w.E, dN = oN - w.N;
            const double ce = dE * nE, cn = dN * nN;
            const double cc = ce + cn;
            const double de = dE * dE, dn = dN * dN;
            const double d2 = de + dn;
            const double dev = sqrt(d2);
            d2sum = d2sum + d2;
            if (dev > dmax) { dmax = dev; imax = (double)i; }
            if (cc > w.edge_L || cc < w.edge_R) nout = nout + 1.0;
            const double eL = T.keep_walls ? w.edge_L - cc : w.edge_L, eR = T.keep_walls ? w.edge_R - cc : w.edge_R;
            O[i].edge_L = eL; O[i].edge_R = eR;
            wmin = fmin(wmin, eL - eR);
            if (!(isfinite(oE) && isfinite(oN) && isfinite(eL) && isfinite(eR)) && bad_fin < 0) bad_fin = i;
            if (!(eL > eR) && bad_wall < 0) bad_wall = i;
            const double hm = aH[im], h0 = aH[i];
            const double hs = hm + h0;
            const double r0 = hs / 3.0, rm = hm / 6.0, rp = h0 / 6.0;
            auto bend = [&](const double* g) -> double {
#pragma clang fp contract(off)
                const double a = rm * g[im], b = r0 * g[i], c2 = rp * g[ip];
                const double ab = a + b;
                const double in = ab + c2;
                return g[i] * in;
            };
            const double bE = bend(aGE), bN = bend(aGN);
            const double b0 = 0.0 + bE;
            const double bb = b0 + bN;
            bsum = bsum + bb;
            if (i < nsp) {
                const double gE = O[ip].E - oE, gN = O[ip].N - oN;
                const double ge = gE * gE, gn = gN * gN;
                const double g2 = ge + gn;
                const double ch = sqrt(g2);
                cmin = fmin(cmin, ch);
                if (!(ch > 0.0) && bad_chord < 0) bad_chord = i;
            }
        }
    }
    const double d2tot = ws_tree(d2sum, sT, lane, wave);
    const double btot = ws_tree(bsum, sT, lane, wave);
    // ---- the exact reductions: the largest displacement with its smallest index, the minima, the count, the first bad waypoint of every kind ----
    auto first = [](int a, int b) -> int { return a < 0 ? b : b < 0 ? a : min(a, b); };
    for (int d = 32; d >= 1; d >>= 1) {
        const double od = __shfl_xor(dmax, d, 64), oi = __shfl_xor(imax, d, 64);
        if (od > dmax || (od == dmax && oi < imax)) { dmax = od; imax = oi; }
        wmin = fmin(wmin, __shfl_xor(wmin, d, 64)); cmin = fmin(cmin, __shfl_xor(cmin, d, 64));
        nout = nout + __shfl_xor(nout, d, 64);                    // (a count: exact in any order)
        bad_fin = first(bad_fin, __shfl_xor(bad_fin, d, 64)); bad_wall = first(bad_wall, __shfl_xor(bad_wall, d, 64)); bad_chord = first(bad_chord, __shfl_xor(bad_chord, d, 64));
    }
    if (lane == 0) {
        sR[wave][0] = dmax; sR[wave][1] = imax; sR[wave][2] = wmin; sR[wave][3] = cmin; sR[wave][4] = nout;
        sB[wave][0] = bad_fin; sB[wave][1] = bad_wall; sB[wave][2] = bad_chord;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WS_THREADS / 64; w++) {
            if (sR[w][0] > dmax || (sR[w][0] == dmax && sR[w][1] < imax)) { dmax = sR[w][0]; imax = sR[w][1]; }
            wmin = fmin(wmin, sR[w][2]); cmin = fmin(cmin, sR[w][3]); nout = nout + sR[w][4];
            bad_fin = first(bad_fin, sB[w][0]); bad_wall = first(bad_wall, sB[w][1]); bad_chord = first(bad_chord, sB[w][2]);
        }
        pg_smooth_stats R;
        const double ms = d2tot / (double)n;
        R.dev_max = dmax; R.dev_rms = sqrt(ms); R.i_dev_max = imax; R.bend = btot; R.n_outside = nout; R.width_min = wmin; R.pivot_min = pivot_min; R.chord_min = cmin;
        R.reserved = 0.0;
        *stat = R;
        bad[0] = bad_piv; bad[1] = bad_fin; bad[2] = bad_wall; bad[3] = bad_chord;
    }
}

__global__ __launch_bounds__(WS_THREADS) void k_wp_smooth(WpSmoothArgs P) {
    extern __shared__ double sRec[];                              // l1, l2, d, z of four right-hand sides: 7 x lds_rows doubles
    const size_t k = blockIdx.x;
    const int path = (int)(k / (size_t)P.n_sets), set = (int)(k - (size_t)path * P.n_sets);
    const SmoothSpec S = P.specs[path];
    const pg_smooth_set T = P.sets[set];
    ws_pair(S, T, T.lambda, P.lds_rows, P.in + S.wp0, P.out + (size_t)set * (size_t)P.n_wp_total + (size_t)S.wp0,
            P.scratch + ((size_t)set * (size_t)P.n_used + (size_t)S.soff) * WS_ARRAYS, sRec, P.stats + k, P.bad + 4 * k);
}
