// The closed forms and the serial solve of pg_optimize_line as functions for host and device alike: k_line_opt (pg_line_opt.hip) calls them, the serial ones in lane 0 of
// wavefront 0; tests/line_opt_host_main.cpp calls them in a stand-alone host program (the unit a host sanitizer build can run).  The scheme is stated in
// include/pigeon_mpc.h at pg_optimize_line; every operation is one rounded double operation, without contraction.  The band recurrence, the way back and the border are
// the smoother's (pg_waypoint_smooth.hpp), called, not restated.
#pragma once
#include "pg_waypoint_smooth.hpp"

// Normal: the left normal of the chord from (Ea, Na) to (Eb, Nb)
__host__ __device__ inline void lo_normal(double Ea, double Na, double Eb, double Nb, double& nE, double& nN) {
#pragma clang fp contract(off)
    const double tE = Eb - Ea, tN = Nb - Na;
    const double te = tE * tE, tn = tN * tN;
    const double v2 = te + tn;
    const double v = sqrt(v2);
    const double ntN = -tN;
    nE = ntN / v; nN = tE / v;
}
__host__ __device__ inline double lo_dot(double aE, double aN, double bE, double bN) {
#pragma clang fp contract(off)
    const double e = aE * bE, n = aN * bN;
    return e + n;
}
// Bend rows: w_j = 2 / (h_jm + h_j)
__host__ __device__ inline double lo_weight(double hm, double h0) {
#pragma clang fp contract(off)
    const double hs = hm + h0;
    return 2.0 / hs;
}
// Hessian: the band of row i of H, D = (c0 a0) + mu, E1 = c1 a1, E2 = c2 a2, with a0, a1, a2 from the smoother's ws_band (lambda = 1, no R terms)
__host__ __device__ inline void lo_hessian(double mu, double pm, double p0, double p1, double wm, double w0, double w1, double c0, double c1, double c2, double& D, double& E1, double& E2) {
#pragma clang fp contract(off)
    double a0, a1, a2;
    ws_band(1.0, 0.0, 0.0, pm, p0, p1, wm, w0, w1, a0, a1, a2);
    const double ca = c0 * a0;
    D = ca + mu; E1 = c1 * a1; E2 = c2 * a2;
}
// g_i = (nE s_E) + (nN s_N), s_y = ((p_im k_y,im) + (q_i k_y,i)) + (p_i k_y,ip), k = w f
__host__ __device__ inline double lo_grad(double pm, double q, double p0, double kEm, double kE0, double kEp, double kNm, double kN0, double kNp, double nE, double nN) {
#pragma clang fp contract(off)
    const double ea = pm * kEm, eb = q * kE0, ec = p0 * kEp;
    const double eab = ea + eb;
    const double sE = eab + ec;
    const double na = pm * kNm, nb = q * kN0, nc = p0 * kNp;
    const double nab = na + nb;
    const double sN = nab + nc;
    return lo_dot(nE, nN, sE, sN);
}
__host__ __device__ inline double lo_clip(double x, double lo, double hi) {
    const double c = x > lo ? x : lo;
    return c > hi ? hi : c;
}
// Box: the margin and the pin of the last listed window that holds U, then lo and hi; `pinned`: the waypoint is an end that pin_ends pins
__host__ __device__ inline void lo_box(double margin, double alpha_max, int n_win, const double* u_lo, const double* u_hi, const double* win_margin, const int* win_pin,
                                       double U, double edge_L, double edge_R, bool pinned, double& lo, double& hi) {
#pragma clang fp contract(off)
    double mg = margin;
    bool pin = false;
    for (int k = 0; k < 4; k++) if (k < n_win && u_lo[k] <= U && U <= u_hi[k]) { mg = win_margin[k]; pin = win_pin[k] != 0; }
    const double a = edge_R + mg, b = edge_L - mg;
    const double na = -alpha_max;
    lo = a > na ? a : na; hi = b < alpha_max ? b : alpha_max;
    if (pin || pinned) { lo = 0.0; hi = 0.0; }
}
// b_i = (rho (z_i - u_i)) - g_i
__host__ __device__ inline double lo_rhs(double rho, double z, double u, double g) {
#pragma clang fp contract(off)
    const double d = z - u;
    const double r = rho * d;
    return r - g;
}
// z' = clip(x + u); u = u + (x - z'); the two maxima take |x - z'| and |z' - z|; z = z'
__host__ __device__ inline void lo_update(double x, double lo, double hi, double& z, double& u, double& rp, double& dz) {
#pragma clang fp contract(off)
    const double s = x + u;
    const double zn = lo_clip(s, lo, hi);
    const double e = x - zn;
    u = u + e;
    const double a = fabs(e), b = fabs(zn - z);
    if (a > rp) rp = a;
    if (b > dz) dz = b;
    z = zn;
}
// term_i = w_i ((rE rE) + (rN rN)), r_y = ((f_y + (p_im (alpha_im n_y,im))) + (q_i (alpha_i n_y,i))) + (p_i (alpha_ip n_y,ip))
__host__ __device__ inline double lo_resid(double f, double pm, double q, double p0, double am, double a0, double ap, double nm, double n0, double np) {
#pragma clang fp contract(off)
    const double ma = am * nm, mb = a0 * n0, mc = ap * np;
    const double ta = pm * ma, tb = q * mb, tc = p0 * mc;
    const double s0 = f + ta;
    const double s1 = s0 + tb;
    return s1 + tc;
}
__host__ __device__ inline double lo_term(double w, double rE, double rN) {
#pragma clang fp contract(off)
    const double e = rE * rE, n = rN * rN;
    const double s = e + n;
    return w * s;
}

// One right-hand side through K = H + rho I: b [m] in place becomes the band solution x0.  D, E1, E2: the band of K over all n rows; m = n on an open path, n - 2 on a
// closed one, whose last two unknowns (xa, xb) come from the border B with the right-hand side's last two entries ba, bb.  store: write l1, l2, d (the factor) on the
// way forward; otherwise they are read as stored
__host__ __device__ inline void lo_solve(int m, bool closed, const double* D, const double* E1, const double* E2, double* l1, double* l2, double* d, bool store,
                                         const WsBorder& B, double ba, double bb, double* b, double& xa, double& xb, double& pivot_min, int& bad_row) {
    ws_forward(m, D, E1, E2, b, store, l1, l2, d, pivot_min, bad_row);
    ws_backward(m, l1, l2, d, b);
    xa = 0.0; xb = 0.0;
    if (closed) ws_border_solve(B, ba, bb, b, xa, xb);
}
// x_i of a closed path for i <= n - 3: (x0_i - (Za_i xa)) - (Zb_i xb)
__host__ __device__ inline double lo_unborder(double x0, double za, double zb, double xa, double xb) {
#pragma clang fp contract(off)
    const double a = za * xa, b = zb * xb;
    const double u = x0 - a;
    return u - b;
}

// U on the host, for the box before the first allocation: U_0 = 0 and U_{j+1} = P_{j / c} + r_{j+1}, the blocked prefix the kernels compute with 256 threads (Prefix of
// pg_make_paths) over the nu = n - 1 chords h: r the running sum inside block j / c, c = ceil(nu / 256); the block totals scanned inside each group of 64 by doubling
// steps (I_b = I_b + I_{b-d}, d = 1, 2, .. 32, for b mod 64 >= d), the group totals summed from 0 in order
inline void lo_prefix_host(int nu, const double* h, double* U) {
#pragma clang fp contract(off)
    const int T = 256, c = (nu + T - 1) / T;
    double I[256], J[256], G[4];
    for (int b = 0; b < T; b++) {
        const int j_lo = b * c < nu ? b * c : nu, j_hi = j_lo + c < nu ? j_lo + c : nu;
        double a = 0.0;
        for (int j = j_lo; j < j_hi; j++) { a = a + h[j]; U[j + 1] = a; }
        I[b] = a;
    }
    for (int s = 1; s < 64; s <<= 1) {
        for (int b = 0; b < T; b++) J[b] = (b & 63) >= s ? I[b] + I[b - s] : I[b];
        for (int b = 0; b < T; b++) I[b] = J[b];
    }
    G[0] = 0.0;
    for (int g = 1; g < 4; g++) G[g] = G[g - 1] + I[64 * (g - 1) + 63];
    for (int b = 0; b < T; b++) {
        const int j_lo = b * c < nu ? b * c : nu, j_hi = j_lo + c < nu ? j_lo + c : nu;
        const double e = (b & 63) > 0 ? I[b - 1] : 0.0;
        const double Pb = G[b >> 6] + e;
        for (int j = j_lo; j < j_hi; j++) U[j + 1] = Pb + U[j + 1];
    }
    U[0] = 0.0;
}
