// pg_tune_smoothing: the smoothing weight of every (path, tune set) pair chosen on the device -- the largest lambda of a geometric ladder whose dev_rms does not exceed
// the set's target -- and the pair smoothed under it.  The scheme is stated in include/pigeon_mpc.h at pg_tune_smoothing and in DESIGN.md 4.25;
// tests/wp_tune_numpy.py is the independent twin.  Included by pg_kernels.hip inside namespace pg, after pg_waypoint_smooth.hip.
//
// One workgroup of 256 threads per pair, one launch.  The phases that do not depend on lambda run once (ws_setup of the smoother, then the five parts of the band and the
// right-hand sides).  A round evaluates F = dev_rms at the WT_CAND = 17 candidates of the bracket's ladder: lane c of wavefront 0 carries candidate c -- its own
// factorisation and its 2 (open path) or 4 (closed path) right-hand sides, forward, back and the border -- so the 17 lanes run in lockstep at the price of one
// (the other mapping, a lane per (candidate, right-hand side) over two wavefronts, was compiled and not kept; DESIGN 4.25 has the registers of both).  The recurrence's
// state is [array][row][candidate], so the lanes of a row store side by side; it lives in LDS where the path has at most WT_LDS_ROWS rows and in the call's scratch
// beyond, the arithmetic being the same.  g and the Sum of dev_rms are strided over waypoints x candidates by all threads, each candidate in the block-and-tree order of
// the smoother.  Thread 0 narrows the bracket.  The final solve is ws_pair, the text k_wp_smooth runs.  Doubles in both libraries, no contraction, no atomics, no kernel
// waits on another (tools/check_f32_purity.py lists k_wp_tune).

#include "pg_waypoint_tune.hpp"

// the search's arrays of a pair in scratch, n_wp doubles each; the recurrence's state follows them where it is not in LDS.  The final solve takes the same memory over
enum { WT_H = 0, WT_P, WT_U, WT_WINV, WT_SE, WT_SN, WT_A0, WT_A1, WT_A2, WT_R0, WT_R1, WT_FE, WT_FN, WT_ARRAYS, WT_LDS_ROWS = 64,
       WT_ARRAYS_LDS = WS_ARRAYS > WT_ARRAYS ? WS_ARRAYS : WT_ARRAYS, WT_ARRAYS_SCRATCH = WT_ARRAYS + WT_STATE * WT_CAND };
// in, out, stats, bad: as WpSmoothArgs.  scratch [n_sets][n_used][n_arr]: n_arr = WT_ARRAYS_LDS where every path's rows fit tune_rows, else WT_ARRAYS_SCRATCH;
// tune_rows: the rows of state the dynamic LDS holds for the search (WT_STATE x WT_CAND doubles each), lds_rows: for the final solve (7 doubles each);
// bad_tune [n_pair][2]: the first round with a candidate whose pivot is not > 0 or whose F is not finite (-1: none), and which of the two (0, 1)
struct WpTuneArgs { int n_sets, n_wp_total, lds_rows, tune_rows, n_arr; long long n_used; const SmoothSpec* specs; const pg_tune_set* sets; const pg_waypoint* in; pg_waypoint* out;
                    double* scratch; pg_smooth_stats* stats; pg_tune_stats* tune; int* bad; int* bad_tune; };

__global__ __launch_bounds__(WS_THREADS) void k_wp_tune(WpTuneArgs P) {
#pragma clang fp contract(off)
    extern __shared__ double sDyn[];                              // the search's state, then the final solve's
    __shared__ double sC[WT_CAND], sF[WT_CAND], sX[WT_CAND][4], sSum[WS_THREADS / 64][WT_CAND], sWv[WS_THREADS / 64];
    __shared__ int sBadC[WT_CAND];
    __shared__ double sLambda; __shared__ int sGo, sOn;      // sGo: this round evaluates; sOn: another round follows (two flags: thread 0 is a phase ahead)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t k = blockIdx.x;
    const int path = (int)(k / (size_t)P.n_sets), set = (int)(k - (size_t)path * P.n_sets);
    const SmoothSpec S = P.specs[path];
    const pg_tune_set T = P.sets[set];
    const int n = S.n_wp;
    const bool closed = S.closed != 0;
    const pg_waypoint* __restrict__ W = P.in + S.wp0;             // every waypoint index below is < n_wp
    double* const A = P.scratch + ((size_t)set * (size_t)P.n_used + (size_t)S.soff) * (size_t)P.n_arr;
    const size_t sn = (size_t)n;
    double* const aH = A + WT_H * sn; double* const aP = A + WT_P * sn; double* const aWi = A + WT_WINV * sn; double* const aSE = A + WT_SE * sn; double* const aSN = A + WT_SN * sn;
    double* const aA0 = A + WT_A0 * sn; double* const aA1 = A + WT_A1 * sn; double* const aA2 = A + WT_A2 * sn; double* const aR0 = A + WT_R0 * sn; double* const aR1 = A + WT_R1 * sn;
    double* const aFE = A + WT_FE * sn; double* const aFN = A + WT_FN * sn;
    const int m = n - 2;
    const bool in_lds = m <= P.tune_rows;
    const size_t rows = in_lds ? (size_t)P.tune_rows : sn;        // m <= rows
    double* const state = in_lds ? sDyn : A + WT_ARRAYS * sn;     // (in scratch only where n_arr = WT_ARRAYS_SCRATCH: the host sizes both from the same rows)
    auto prev = [&](int i) -> int { return i > 0 ? i - 1 : n - 1; };
    auto next = [&](int i) -> int { return i + 1 == n ? 0 : i + 1; };
    WtParts Q; Q.a0 = aA0; Q.a1 = aA1; Q.a2 = aA2; Q.r0 = aR0; Q.r1 = aR1;

    ws_setup(S, T.base, W, aH, aP, A + WT_U * sn, aWi, aSE, aSN, sWv);
    // ---- the parts of the band of every row and the right-hand sides ----
    for (int i = tid; i < n; i += WS_THREADS) {
        const int im = prev(i), ip = next(i);
        double a0, a1, a2, r0, r1;
        wt_band_parts(aH[im], aH[i], aP[im], aP[i], aP[ip], aWi[im], aWi[i], aWi[ip], a0, a1, a2, r0, r1);
        aA0[i] = a0; aA1[i] = a1; aA2[i] = a2; aR0[i] = r0; aR1[i] = r1;
        aFE[i] = aSE[i] - aSE[im]; aFN[i] = aSN[i] - aSN[im];
    }
    // thread 0 alone reads these
    double lo = T.lambda_lo, hi = T.lambda_hi, rms_lo = 0.0, rms_hi = 0.0, verdict = 0.0, rounds_done = 0.0, monotone = 1.0;
    int bad_round = -1, bad_kind = 0;
    __syncthreads();

    for (int t = 0; t < T.rounds; t++) {
        if (tid == 0) { wt_ladder(lo, hi, sC); sGo = !(t >= 1 && wt_repeats(sC)); }
        __syncthreads();
        if (!sGo) break;
        // ---- the recurrence, the way back and the border: candidates across lanes ----
        if (tid < WT_CAND) {
            const int cand = tid;
            int bad = 0;
            if (m > 0) {
                double pm; int br;
                if (closed) { wt_forward<4>(n, true, sC[cand], Q, aFE, aFN, 0, true, state + cand, rows, pm, br); wt_backward<4>(m, 0, state + cand, rows); }
                else { wt_forward<2>(n, false, sC[cand], Q, aFE, aFN, 0, true, state + cand, rows, pm, br); wt_backward<2>(m, 0, state + cand, rows); }
                bad = br < m;
            }
            double x[4] = {0.0, 0.0, 0.0, 0.0};
            if (closed) {
                double S00, p2;
                wt_border(n, sC[cand], Q, aFE, aFN, state + cand, rows, x, S00, p2);
                if (!(S00 > 0.0) || !(p2 > 0.0)) bad = 1;
            }
            sX[cand][0] = x[0]; sX[cand][1] = x[1]; sX[cand][2] = x[2]; sX[cand][3] = x[3];
            sBadC[cand] = bad;
        }
        __syncthreads();
        // ---- g and Sum((dE dE) + (dN dN)) of every candidate: thread b owns block b of c consecutive waypoints ----
        {
            const int c = (n + WS_THREADS - 1) / WS_THREADS;
            const int i_lo = min(tid * c, n), i_hi = min(i_lo + c, n);
            for (int cand = 0; cand < WT_CAND; cand++) {
                const double lambda = sC[cand];
                const double* const st = state + cand;
                const double* const x = sX[cand];
                double d2sum = 0.0;
                if (i_lo < i_hi) {
                    double gmE = wt_gamma(prev(i_lo), 0, n, closed, st, rows, x), gmN = wt_gamma(prev(i_lo), 1, n, closed, st, rows, x);
                    double g0E = wt_gamma(i_lo, 0, n, closed, st, rows, x), g0N = wt_gamma(i_lo, 1, n, closed, st, rows, x);
                    for (int i = i_lo; i < i_hi; i++) {
                        const int im = prev(i), ip = next(i);
                        const double gpE = wt_gamma(ip, 0, n, closed, st, rows, x), gpN = wt_gamma(ip, 1, n, closed, st, rows, x);
                        const double pm = aP[im], p0 = aP[i];
                        const double npm = -pm;
                        const double q = npm - p0;
                        const double w = aWi[i];
                        const pg_waypoint y = W[i];
                        const double oE = ws_moved(y.E, lambda, w, pm, q, p0, gmE, g0E, gpE), oN = ws_moved(y.N, lambda, w, pm, q, p0, gmN, g0N, gpN);
                        const double dE = oE - y.E, dN = oN - y.N;
                        const double de = dE * dE, dn = dN * dN;
                        const double d2 = de + dn;
                        d2sum = d2sum + d2;
                        gmE = g0E; gmN = g0N; g0E = gpE; g0N = gpN;
                    }
                }
                for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_xor(d2sum, d, 64); d2sum = d2sum + y; }
                if (lane == 0) sSum[wave][cand] = d2sum;
            }
        }
        __syncthreads();
        // ---- F, the verdict of round 0 and the narrowing ----
        if (tid == 0) {
            bool piv = false, fin = true;
            for (int c = 0; c < WT_CAND; c++) {
                const double a = sSum[0][c] + sSum[1][c], b = sSum[2][c] + sSum[3][c];
                const double tot = a + b;
                const double ms = tot / (double)n;
                sF[c] = sqrt(ms);
                piv = piv || sBadC[c] != 0; fin = fin && isfinite(sF[c]);
            }
            rounds_done = rounds_done + 1.0;
            if (!wt_monotone(sF)) monotone = 0.0;
            int go = 1;
            if (piv || !fin) { bad_round = t; bad_kind = piv ? 0 : 1; go = 0; }
            else if (t == 0 && sF[0] > T.target) { verdict = -1.0; hi = lo; rms_lo = sF[0]; rms_hi = sF[0]; go = 0; }
            else if (t == 0 && sF[WT_CAND - 1] <= T.target) { verdict = 1.0; lo = hi; rms_lo = sF[WT_CAND - 1]; rms_hi = sF[WT_CAND - 1]; go = 0; }
            else {
                const int j = min(wt_first_above(sF, T.target), WT_CAND - 1);      // (a j exists: F_0 <= target < F_16 holds from round 0 on)
                lo = sC[j - 1]; hi = sC[j]; rms_lo = sF[j - 1]; rms_hi = sF[j];
            }
            sOn = go;
        }
        __syncthreads();
        if (!sOn) break;
    }
    if (tid == 0) {
        pg_tune_stats R;
        R.lambda = lo; R.lo = lo; R.hi = hi; R.rms_lo = rms_lo; R.rms_hi = rms_hi; R.verdict = verdict; R.rounds_done = rounds_done; R.monotone = monotone; R.reserved = 0.0;
        P.tune[k] = R;
        P.bad_tune[2 * k] = bad_round; P.bad_tune[2 * k + 1] = bad_kind;
        sLambda = lo;
    }
    __syncthreads();                                              // (the search's arrays and LDS are free from here on)
    // ---- the final solve: pg_smooth_waypoints' own text under base with the chosen weight ----
    ws_pair(S, T.base, sLambda, P.lds_rows, W, P.out + (size_t)set * (size_t)P.n_wp_total + (size_t)S.wp0, A, sDyn, P.stats + k, P.bad + 4 * k);
}
