// The helpers of pg_optimize_line on the host (pigeon.jl_amd/csrc/pg_line_opt.hpp: lo_normal, lo_weight, lo_hessian, lo_grad, lo_box, lo_rhs, lo_solve, lo_unborder,
// lo_update, lo_prefix_host, and through them the smoother's ws_band, ws_forward, ws_backward, ws_border, ws_border_solve), as the kernel calls them:
// tests/test_line_opt_host.py builds this stand-alone program (its own main; with -fsanitize=address,undefined) and compares what it prints with the twin bit for bit.
// Two paths of tests/line_opt_cases.py under its plain set with 40 iterations: the closed one of 5 waypoints (three band rows, the two border unknowns) and the open one
// of 5 (five rows).  Output: one line per waypoint, "name i alpha lo hi U" in hexadecimal floating point, then r_prim, r_dual, iters_done and the smallest pivot.
#include <stdio.h>
#include <vector>
#include "pg_line_opt.hpp"

static void run(const char* name, const std::vector<double>& E, const std::vector<double>& N, const std::vector<double>& eL, const std::vector<double>& eR, bool closed,
                double mu, double rho, double margin, double alpha_max, int iters) {
    const int n = (int)E.size(), nsp = closed ? n : n - 1, m = closed ? n - 2 : n;
    auto prev = [&](int i) { return i > 0 ? i - 1 : n - 1; };
    auto next = [&](int i) { return i + 1 == n ? 0 : i + 1; };
    std::vector<double> h(n, 0.0), p(n, 0.0), sE(n, 0.0), sN(n, 0.0), U(n), nE(n), nN(n), w(n), fE(n), fN(n), D(n), E1(n), E2(n), g(n), lo(n), hi(n), z(n), u(n, 0.0);
    for (int j = 0; j < nsp; j++) {
        const double dE = E[next(j)] - E[j], dN = N[next(j)] - N[j];
        const double ee = dE * dE, nn = dN * dN;
        h[j] = sqrt(ee + nn); p[j] = 1.0 / h[j]; sE[j] = dE / h[j]; sN[j] = dN / h[j];
    }
    lo_prefix_host(n - 1, h.data(), U.data());
    for (int i = 0; i < n; i++) {
        const int ia = !closed && i == 0 ? 0 : prev(i), ib = !closed && i == n - 1 ? n - 1 : next(i);
        lo_normal(E[ia], N[ia], E[ib], N[ib], nE[i], nN[i]);
        fE[i] = sE[i] - sE[prev(i)]; fN[i] = sN[i] - sN[prev(i)];
        w[i] = closed || (i > 0 && i < n - 1) ? lo_weight(h[prev(i)], h[i]) : 0.0;
    }
    const double none[4] = {0.0, 0.0, 0.0, 0.0}; const int nopin[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        const int im = prev(i), ip = next(i), ip2 = next(ip);
        double d;
        lo_hessian(mu, p[im], p[i], p[ip], w[im], w[i], w[ip], lo_dot(nE[i], nN[i], nE[i], nN[i]), lo_dot(nE[i], nN[i], nE[ip], nN[ip]), lo_dot(nE[i], nN[i], nE[ip2], nN[ip2]),
                   d, E1[i], E2[i]);
        D[i] = d + rho;
        const double q = -p[im] - p[i];
        g[i] = lo_grad(p[im], q, p[i], w[im] * fE[im], w[i] * fE[i], w[ip] * fE[ip], w[im] * fN[im], w[i] * fN[i], w[ip] * fN[ip], nE[i], nN[i]);
        lo_box(margin, alpha_max, 0, none, none, none, nopin, U[i], eL[i], eR[i], false, lo[i], hi[i]);
        z[i] = lo_clip(0.0, lo[i], hi[i]);
    }
    // exactly m entries each: an index past a row is an error a sanitizer sees
    std::vector<double> l1(m), l2(m), piv(m), x(m), Za(m, 0.0), Zb(m, 0.0);
    WsBorder B = {};
    double pivot_min = INFINITY; int bad = m;
    if (closed) {
        for (int r = 0; r < m; r++) {
            Za[r] = r == 0 ? E2[n - 2] : r == n - 4 ? E2[n - 4] : r == n - 3 ? E1[n - 3] : 0.0;
            Zb[r] = r == 0 ? E1[n - 1] : r == 1 ? E2[n - 1] : r == n - 3 ? E2[n - 3] : 0.0;
        }
        double pm; int br;
        ws_forward(m, D.data(), E1.data(), E2.data(), Za.data(), true, l1.data(), l2.data(), piv.data(), pivot_min, bad);
        ws_forward(m, D.data(), E1.data(), E2.data(), Zb.data(), false, l1.data(), l2.data(), piv.data(), pm, br);
        ws_backward(m, l1.data(), l2.data(), piv.data(), Za.data());
        ws_backward(m, l1.data(), l2.data(), piv.data(), Zb.data());
        B = ws_border(n, D.data(), E1.data(), E2.data(), Za.data(), Zb.data());
        pivot_min = fmin(pivot_min, fmin(B.S00, B.det / B.S00));
    }
    double r_prim = 0.0, r_dual = 0.0;
    int done = 0;
    for (int it = 1; it <= iters; it++) {
        double ba = 0.0, bb = 0.0;
        for (int i = 0; i < n; i++) {
            const double b = lo_rhs(rho, z[i], u[i], g[i]);
            if (i < m) x[i] = b; else if (i == n - 2) ba = b; else bb = b;
        }
        double xa, xb, pm; int br;
        const bool store = !closed && it == 1;
        lo_solve(m, closed, D.data(), E1.data(), E2.data(), l1.data(), l2.data(), piv.data(), store, B, ba, bb, x.data(), xa, xb, pm, br);
        if (store) { pivot_min = pm; bad = br; }
        double rp = 0.0, dz = 0.0;
        for (int i = 0; i < n; i++) {
            const double xi = i < m ? (closed ? lo_unborder(x[i], Za[i], Zb[i], xa, xb) : x[i]) : i == n - 2 ? xa : xb;
            lo_update(xi, lo[i], hi[i], z[i], u[i], rp, dz);
        }
        r_prim = rp; r_dual = rho * dz; done = it;
        if (r_prim <= 0.0 && r_dual <= 0.0) break;                 // (tol = 0)
    }
    for (int i = 0; i < n; i++) printf("%s %d %a %a %a %a\n", name, i, z[i], lo[i], hi[i], U[i]);
    printf("%s stats %a %a %d %a bad_row %d of %d\n", name, r_prim, r_dual, done, pivot_min, bad, m);
}

int main() {
    const double scale = 1.0 / (3.74 * 3.74 * 3.74);
    run("closed5", {0.0, 4.0, 8.5, 9.0, 5.0}, {0.0, -1.0, 1.5, 6.0, 9.5}, {4.0, 4.0, 4.0, 4.0, 4.0}, {-4.0, -4.0, -4.0, -4.0, -4.0}, true, 1e-6 * scale, 0.1 * scale, 0.5, 2.0, 40);
    run("open5", {0.0, 3.0, 5.0, 9.5, 12.0}, {0.0, 0.5, 2.5, 3.0, 7.0}, {3.0, 3.25, 3.5, 3.75, 4.0}, {-2.0, -2.5, -3.0, -3.5, -4.0}, false, 1e-6 * scale, 0.1 * scale, 0.5, 2.0, 40);
    return 0;
}
