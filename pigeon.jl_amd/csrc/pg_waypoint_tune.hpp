// The search of pg_tune_smoothing as functions for host and device alike: k_wp_tune (pg_waypoint_tune.hip) calls them with one candidate weight per lane,
// tests/wp_tune_host_main.cpp calls them in a stand-alone host program (the unit a host sanitizer build can run).  The scheme is stated in include/pigeon_mpc.h at
// pg_tune_smoothing; F is the scheme of pg_smooth_waypoints unchanged, so every operation here is the one pg_waypoint_smooth.hpp does, rounded on its own, without
// contraction -- only the layout differs: WT_CAND candidates share a row, so a candidate's recurrence state is WT_CAND doubles apart.
#pragma once
#include <stddef.h>
#include "pg_waypoint_smooth.hpp"

enum { WT_CAND = 17, WT_STATE = 7 };      // the candidates of a ladder; the state arrays of the recurrence: l1, l2, d and z of the four right-hand sides

// Ladder: c_0 = lo, c_16 = hi, then four levels of midpoints, each sqrt(left right) of its two neighbours on the level above
__host__ __device__ inline void wt_ladder(double lo, double hi, double* c) {
#pragma clang fp contract(off)
    c[0] = lo; c[WT_CAND - 1] = hi;
    for (int half = (WT_CAND - 1) / 2; half >= 1; half >>= 1)
        for (int j = half; j < WT_CAND - 1; j += 2 * half) { const double pr = c[j - half] * c[j + half]; c[j] = sqrt(pr); }
}
// Stop: two equal neighbouring candidates
__host__ __device__ inline bool wt_repeats(const double* c) {
    for (int j = 0; j + 1 < WT_CAND; j++) if (c[j] == c[j + 1]) return true;
    return false;
}
// Narrowing: the smallest j in 1 .. 16 with F_j > target (WT_CAND: none)
__host__ __device__ inline int wt_first_above(const double* F, double target) {
    for (int j = 1; j < WT_CAND; j++) if (F[j] > target) return j;
    return WT_CAND;
}
__host__ __device__ inline bool wt_monotone(const double* F) {
    for (int j = 0; j + 1 < WT_CAND; j++) if (!(F[j] <= F[j + 1])) return false;
    return true;
}

// The parts of the band of row i that do not depend on lambda, in the operations of ws_band: D = r0 + (lambda a0), E1 = r1 + (lambda a1), E2 = lambda a2
__host__ __device__ inline void wt_band_parts(double hm, double h0, double pm, double p0, double p1, double wm, double w0, double w1, double& a0, double& a1, double& a2,
                                              double& r0, double& r1) {
#pragma clang fp contract(off)
    const double npm = -pm, np0 = -p0;
    const double q0 = npm - p0, q1 = np0 - p1;
    const double pm2 = pm * pm, q02 = q0 * q0, p02 = p0 * p0;
    const double ta = wm * pm2, tb = w0 * q02, tc = w1 * p02;
    const double tab = ta + tb;
    a0 = tab + tc;
    const double ua = w0 * q0, ub = w1 * q1;
    const double us = ua + ub;
    a1 = p0 * us;
    const double pp = p0 * p1;
    a2 = w1 * pp;
    const double hs = hm + h0;
    r0 = hs / 3.0; r1 = h0 / 6.0;
}
// the five arrays of parts of a path, one entry per waypoint
struct WtParts { const double *a0, *a1, *a2, *r0, *r1; };
__host__ __device__ inline double wt_D(const WtParts& P, double lambda, int i) {
#pragma clang fp contract(off)
    const double l0 = lambda * P.a0[i];
    return P.r0[i] + l0;
}
__host__ __device__ inline double wt_E1(const WtParts& P, double lambda, int i) {
#pragma clang fp contract(off)
    const double l1 = lambda * P.a1[i];
    return P.r1[i] + l1;
}
__host__ __device__ inline double wt_E2(const WtParts& P, double lambda, int i) {
#pragma clang fp contract(off)
    return lambda * P.a2[i];
}

// A candidate's recurrence state: array a (0: l1, 1: l2, 2: d, 3 + q: z of right-hand side q), row r, in a block of `rows` rows; st points at the candidate's own column
__host__ __device__ inline size_t wt_at(int a, size_t rows, int r) { return ((size_t)a * rows + (size_t)r) * WT_CAND; }

// ws_forward for one candidate weight and the NR right-hand sides q0 .. q0 + NR - 1 (0: E, 1: N, 2 and 3: the border columns a and b of a closed path), the band taken
// from the parts as it goes.  n: the waypoints; the rows are base .. base + m - 1.  `store`: this caller writes l1, l2, d
template <int NR>
__host__ __device__ inline void wt_forward(int n, bool closed, double lambda, const WtParts& P, const double* FE, const double* FN, int q0, bool store, double* st, size_t rows,
                                           double& pivot_min, int& bad_row) {
#pragma clang fp contract(off)
    const int m = n - 2, base = closed ? 0 : 1;
    double ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0};
    if (closed && q0 + NR > 2) {
        ca[0] = wt_E2(P, lambda, n - 2); ca[1] = wt_E2(P, lambda, n - 4); ca[2] = wt_E1(P, lambda, n - 3);
        cb[0] = wt_E1(P, lambda, n - 1); cb[1] = wt_E2(P, lambda, n - 1); cb[2] = wt_E2(P, lambda, n - 3);
    }
    double d1 = 1.0, d2 = 1.0, lp = 0.0, e1 = 0.0, e2 = 0.0, e2n = 0.0;      // e1 = E1 of the row before, e2 = E2 of the row before that, e2n = E2 of the row before
    double z1[NR], z2[NR];
    for (int k = 0; k < NR; k++) { z1[k] = 0.0; z2[k] = 0.0; }
    pivot_min = INFINITY; bad_row = m;
    for (int r = 0; r < m; r++) {
        const int i = base + r;
        const double Dr = wt_D(P, lambda, i), E1r = wt_E1(P, lambda, i), E2r = wt_E2(P, lambda, i);
        const double b2 = e2 / d2;
        const double el = e2 * lp;
        const double c1 = e1 - el;
        const double b1 = c1 / d1;
        const double s2 = e2 * b2, s1 = c1 * b1;
        const double t = Dr - s2;
        const double dr = t - s1;
        for (int k = 0; k < NR; k++) {
            const int q = q0 + k;
            const double f = q == 0 ? FE[i] : q == 1 ? FN[i] : q == 2 ? (r == 0 ? ca[0] : r == n - 4 ? ca[1] : r == n - 3 ? ca[2] : 0.0)
                                                                      : (r == 0 ? cb[0] : r == 1 ? cb[1] : r == n - 3 ? cb[2] : 0.0);
            const double f1 = b1 * z1[k], f2 = b2 * z2[k];
            const double u = f - f1;
            const double zr = u - f2;
            st[wt_at(3 + q, rows, r)] = zr;
            z2[k] = z1[k]; z1[k] = zr;
        }
        if (store) { st[wt_at(0, rows, r)] = b1; st[wt_at(1, rows, r)] = b2; st[wt_at(2, rows, r)] = dr; }
        if (!(dr > 0.0) && bad_row == m) bad_row = r;
        pivot_min = fmin(pivot_min, dr);
        d2 = d1; d1 = dr; lp = b1; e2 = e2n; e2n = E2r; e1 = E1r;
    }
}
// ws_backward for the same right-hand sides, in place
template <int NR>
__host__ __device__ inline void wt_backward(int m, int q0, double* st, size_t rows) {
#pragma clang fp contract(off)
    double x1[NR], x2[NR];
    for (int k = 0; k < NR; k++) { x1[k] = 0.0; x2[k] = 0.0; }
    for (int r = m - 1; r >= 0; r--) {
        const double l1n = r + 1 < m ? st[wt_at(0, rows, r + 1)] : 0.0, l2n = r + 2 < m ? st[wt_at(1, rows, r + 2)] : 0.0, dr = st[wt_at(2, rows, r)];
        for (int k = 0; k < NR; k++) {
            const double a = r + 1 < m ? l1n * x1[k] : 0.0, b = r + 2 < m ? l2n * x2[k] : 0.0;
            const double q = st[wt_at(3 + q0 + k, rows, r)] / dr;
            const double u = q - a;
            const double x = u - b;
            st[wt_at(3 + q0 + k, rows, r)] = x;
            x2[k] = x1[k]; x1[k] = x;
        }
    }
}

// The border of a closed path for one candidate after the way back: the four rows a product C^T x reads (0, 1, n - 4, n - 3) gathered into places 0 .. 3, then ws_dot3
// and ws_border_solve as pg_smooth_waypoints runs them.  x [4]: gamma_a and gamma_b of E, then of N; S00 and p2 = det / S00 are the border's two pivots
__host__ __device__ inline void wt_border(int n, double lambda, const WtParts& P, const double* FE, const double* FN, const double* st, size_t rows, double* x, double& S00,
                                          double& p2) {
#pragma clang fp contract(off)
    const int row[4] = {0, 1, n - 4, n - 3};
    double g[4][4];                                             // [right-hand side][place]
    for (int q = 0; q < 4; q++) for (int j = 0; j < 4; j++) g[q][j] = st[wt_at(3 + q, rows, row[j])];
    WsBorder B;
    B.ra[0] = 0; B.ra[1] = 2; B.ra[2] = 3; B.ca[0] = wt_E2(P, lambda, n - 2); B.ca[1] = wt_E2(P, lambda, n - 4); B.ca[2] = wt_E1(P, lambda, n - 3);
    B.rb[0] = 0; B.rb[1] = 1; B.rb[2] = 3; B.cb[0] = wt_E1(P, lambda, n - 1); B.cb[1] = wt_E2(P, lambda, n - 1); B.cb[2] = wt_E2(P, lambda, n - 3);
    B.S00 = wt_D(P, lambda, n - 2) - ws_dot3(B.ra, B.ca, g[2]);
    B.S01 = wt_E1(P, lambda, n - 2) - ws_dot3(B.ra, B.ca, g[3]);
    B.S11 = wt_D(P, lambda, n - 1) - ws_dot3(B.rb, B.cb, g[3]);
    const double a = B.S00 * B.S11, b = B.S01 * B.S01;
    B.det = a - b;
    ws_border_solve(B, FE[n - 2], FE[n - 1], g[0], x[0], x[1]);
    ws_border_solve(B, FN[n - 2], FN[n - 1], g[1], x[2], x[3]);
    S00 = B.S00; p2 = B.det / B.S00;
}
// gamma of coordinate q (0: E, 1: N) at waypoint i for one candidate: 0 at the natural ends, the border's unknowns and x0 - Za gamma_a - Zb gamma_b on a closed path
__host__ __device__ inline double wt_gamma(int i, int q, int n, bool closed, const double* st, size_t rows, const double* x) {
#pragma clang fp contract(off)
    const int m = n - 2, r = i - (closed ? 0 : 1);
    if (r >= 0 && r < m) {
        const double g = st[wt_at(3 + q, rows, r)];
        if (!closed) return g;
        const double a = st[wt_at(5, rows, r)] * x[2 * q], b = st[wt_at(6, rows, r)] * x[2 * q + 1];
        const double u = g - a;
        return u - b;
    }
    return closed ? (i == n - 2 ? x[2 * q] : x[2 * q + 1]) : 0.0;
}
