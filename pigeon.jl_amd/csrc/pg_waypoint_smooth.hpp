// The serial part of pg_smooth_waypoints and the closed forms around it, as functions for host and device alike: k_wp_smooth (pg_waypoint_smooth.hip) calls them in the
// lanes of one wavefront, tests/wp_smooth_host_main.cpp calls them in a stand-alone host program (the unit a host sanitizer build can run).  The scheme is stated in
// include/pigeon_mpc.h at pg_smooth_waypoints; every operation is one rounded double operation, without contraction.
#pragma once
#include <math.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

// The band entries of row i in closed form from the chords and the inverse weights around it: dd = A(i, i), e1 = A(i, i + 1), e2 = A(i, i + 2).  hm, pm: h and 1 / h of
// the span that ends on waypoint i; h0, p0: of the span that starts on it; p1: of the span after that; wm, w0, w1: winv of waypoints i - 1, i, i + 1
__host__ __device__ inline void ws_band(double lambda, double hm, double h0, double pm, double p0, double p1, double wm, double w0, double w1, double& dd, double& e1, double& e2) {
#pragma clang fp contract(off)
    const double npm = -pm, np0 = -p0;
    const double q0 = npm - p0, q1 = np0 - p1;
    const double pm2 = pm * pm, q02 = q0 * q0, p02 = p0 * p0;
    const double ta = wm * pm2, tb = w0 * q02, tc = w1 * p02;
    const double tab = ta + tb;
    const double a0 = tab + tc;
    const double ua = w0 * q0, ub = w1 * q1;
    const double us = ua + ub;
    const double a1 = p0 * us;
    const double pp = p0 * p1;
    const double a2 = w1 * pp;
    const double hs = hm + h0;
    const double r0 = hs / 3.0, r1 = h0 / 6.0;
    const double l0 = lambda * a0, l1 = lambda * a1;
    dd = r0 + l0; e1 = r1 + l1; e2 = lambda * a2;
}

// The band LDL^T recurrence without pivoting over the rows 0 .. m - 1 (D[r] = A(r, r), E1[r] = A(r, r + 1), E2[r] = A(r, r + 2)) and the forward substitution of one
// right-hand side, z in place.  Every caller repeats the factor recurrence in its own registers; `store` says whether this one writes l1, l2, d for the way back.
// pivot_min: the smallest pivot; bad_row: the first row whose pivot is not > 0 (m: none)
__host__ __device__ inline void ws_forward(int m, const double* D, const double* E1, const double* E2, double* z, bool store, double* l1, double* l2, double* d,
                                           double& pivot_min, int& bad_row) {
#pragma clang fp contract(off)
    double d1 = 1.0, d2 = 1.0, lp = 0.0, z1 = 0.0, z2 = 0.0;   // the pivots of the two rows before, l1 of the row before, z of the two rows before
    pivot_min = INFINITY; bad_row = m;
    for (int r = 0; r < m; r++) {
        const double e1 = r >= 1 ? E1[r - 1] : 0.0, e2 = r >= 2 ? E2[r - 2] : 0.0;
        const double b2 = e2 / d2;
        const double el = e2 * lp;
        const double c1 = e1 - el;
        const double b1 = c1 / d1;
        const double s2 = e2 * b2, s1 = c1 * b1;
        const double t = D[r] - s2;
        const double dr = t - s1;
        const double f1 = b1 * z1, f2 = b2 * z2;
        const double u = z[r] - f1;
        const double zr = u - f2;
        z[r] = zr;
        if (store) { l1[r] = b1; l2[r] = b2; d[r] = dr; }
        if (!(dr > 0.0) && bad_row == m) bad_row = r;
        pivot_min = fmin(pivot_min, dr);
        d2 = d1; d1 = dr; lp = b1; z2 = z1; z1 = zr;
    }
}
// the way back: x_r = ((z_r / d_r) - (l1_{r+1} x_{r+1})) - (l2_{r+2} x_{r+2}), in place
__host__ __device__ inline void ws_backward(int m, const double* l1, const double* l2, const double* d, double* z) {
#pragma clang fp contract(off)
    double x1 = 0.0, x2 = 0.0;
    for (int r = m - 1; r >= 0; r--) {
        const double a = r + 1 < m ? l1[r + 1] * x1 : 0.0, b = r + 2 < m ? l2[r + 2] * x2 : 0.0;
        const double q = z[r] / d[r];
        const double u = q - a;
        const double x = u - b;
        z[r] = x;
        x2 = x1; x1 = x;
    }
}

// The border of a closed path of n waypoints: the last two unknowns.  Column a (node n - 2) of C has the rows 0, n - 4, n - 3; column b (node n - 1) the rows 0, 1, n - 3
struct WsBorder { int ra[3], rb[3]; double ca[3], cb[3]; double S00, S01, S11, det; };
__host__ __device__ inline double ws_dot3(const int* rows, const double* col, const double* x) {
#pragma clang fp contract(off)
    const double t0 = col[0] * x[rows[0]], t1 = col[1] * x[rows[1]], t2 = col[2] * x[rows[2]];
    const double s = t0 + t1;
    return s + t2;
}
// D, E1, E2: the band of all n rows; Za, Zb: the solutions of B Z = C
__host__ __device__ inline WsBorder ws_border(int n, const double* D, const double* E1, const double* E2, const double* Za, const double* Zb) {
#pragma clang fp contract(off)
    WsBorder B;
    B.ra[0] = 0; B.ra[1] = n - 4; B.ra[2] = n - 3; B.ca[0] = E2[n - 2]; B.ca[1] = E2[n - 4]; B.ca[2] = E1[n - 3];
    B.rb[0] = 0; B.rb[1] = 1; B.rb[2] = n - 3; B.cb[0] = E1[n - 1]; B.cb[1] = E2[n - 1]; B.cb[2] = E2[n - 3];
    B.S00 = D[n - 2] - ws_dot3(B.ra, B.ca, Za);
    B.S01 = E1[n - 2] - ws_dot3(B.ra, B.ca, Zb);
    B.S11 = D[n - 1] - ws_dot3(B.rb, B.cb, Zb);
    const double a = B.S00 * B.S11, b = B.S01 * B.S01;
    B.det = a - b;
    return B;
}
// x2 = S^-1 (f2 - C^T x0) by the closed form of the 2 x 2 inverse: fa, fb are the right-hand side's last two entries, x0 the band solution
__host__ __device__ inline void ws_border_solve(const WsBorder& B, double fa, double fb, const double* x0, double& xa, double& xb) {
#pragma clang fp contract(off)
    const double ra = fa - ws_dot3(B.ra, B.ca, x0), rb = fb - ws_dot3(B.rb, B.cb, x0);
    const double a0 = B.S11 * ra, a1 = B.S01 * rb, b0 = B.S00 * rb, b1 = B.S01 * ra;
    const double na = a0 - a1, nb = b0 - b1;
    xa = na / B.det; xb = nb / B.det;
}
