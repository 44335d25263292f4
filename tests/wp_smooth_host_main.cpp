// The recurrence helpers of pg_smooth_waypoints on the host (pigeon.jl_amd/csrc/pg_waypoint_smooth.hpp: ws_band, ws_forward, ws_backward, ws_border, ws_border_solve), as
// the kernel calls them: tests/test_wp_smooth_host.py builds this stand-alone program (its own main; also with -fsanitize=address,undefined) and compares what it prints
// with the twin bit for bit.  Two paths of tests/wp_smooth_cases.py at lambda = 0.1 and winv = 1: the closed one of 5 waypoints (three band rows, the two border
// unknowns) and the open one of 3 (one row).  Output: one line per waypoint, "name i gamma_E gamma_N" in hexadecimal floating point, then the smallest pivot.
#include <stdio.h>
#include <vector>
#include "pg_waypoint_smooth.hpp"

static void run(const char* name, const std::vector<double>& E, const std::vector<double>& N, bool closed, double lambda) {
    const int n = (int)E.size(), nsp = closed ? n : n - 1, m = n - 2, base = closed ? 0 : 1;
    std::vector<double> h(n, 0.0), p(n, 0.0), sE(n, 0.0), sN(n, 0.0), w(n, 1.0), D(n), E1(n), E2(n), fE(n), fN(n);
    for (int j = 0; j < nsp; j++) {
        const int jn = j + 1 == n ? 0 : j + 1;
        const double dE = E[jn] - E[j], dN = N[jn] - N[j];
        const double ee = dE * dE, nn = dN * dN;
        h[j] = sqrt(ee + nn); p[j] = 1.0 / h[j]; sE[j] = dE / h[j]; sN[j] = dN / h[j];
    }
    for (int i = 0; i < n; i++) {
        const int im = i > 0 ? i - 1 : n - 1, ip = i + 1 == n ? 0 : i + 1;
        ws_band(lambda, h[im], h[i], p[im], p[i], p[ip], w[im], w[i], w[ip], D[i], E1[i], E2[i]);
        fE[i] = sE[i] - sE[im]; fN[i] = sN[i] - sN[im];
    }
    // exactly m entries each: an index past a row is an error a sanitizer sees
    std::vector<double> l1(m), l2(m), d(m), z[4];
    const int nrhs = closed ? 4 : 2;
    for (int r = 0; r < 4; r++) z[r].assign(m, 0.0);
    for (int r = 0; r < m; r++) { z[0][r] = fE[base + r]; z[1][r] = fN[base + r]; }
    if (closed) {
        z[2][0] = E2[n - 2]; z[2][n - 4] = E2[n - 4]; z[2][n - 3] = E1[n - 3];
        z[3][0] = E1[n - 1]; z[3][1] = E2[n - 1]; z[3][n - 3] = E2[n - 3];
    }
    double pivot_min = INFINITY; int bad = m;
    for (int r = 0; r < nrhs; r++) {
        double pm; int br;
        ws_forward(m, D.data() + base, E1.data() + base, E2.data() + base, z[r].data(), r == 0, l1.data(), l2.data(), d.data(), pm, br);
        if (r == 0) { pivot_min = pm; bad = br; }
    }
    for (int r = 0; r < nrhs; r++) ws_backward(m, l1.data(), l2.data(), d.data(), z[r].data());
    std::vector<double> gE(n, 0.0), gN(n, 0.0);
    for (int r = 0; r < m; r++) { gE[base + r] = z[0][r]; gN[base + r] = z[1][r]; }
    if (closed) {
        const WsBorder B = ws_border(n, D.data(), E1.data(), E2.data(), z[2].data(), z[3].data());
        double xaE, xbE, xaN, xbN;
        ws_border_solve(B, fE[n - 2], fE[n - 1], z[0].data(), xaE, xbE);
        ws_border_solve(B, fN[n - 2], fN[n - 1], z[1].data(), xaN, xbN);
        for (int r = 0; r < m; r++) {
            const double aE = z[2][r] * xaE, bE = z[3][r] * xbE, aN = z[2][r] * xaN, bN = z[3][r] * xbN;
            const double uE = z[0][r] - aE, uN = z[1][r] - aN;
            gE[r] = uE - bE; gN[r] = uN - bN;
        }
        gE[n - 2] = xaE; gE[n - 1] = xbE; gN[n - 2] = xaN; gN[n - 1] = xbN;
        pivot_min = fmin(pivot_min, fmin(B.S00, B.det / B.S00));
    }
    for (int i = 0; i < n; i++) printf("%s %d %a %a\n", name, i, gE[i], gN[i]);
    printf("%s pivot_min %a bad_row %d of %d\n", name, pivot_min, bad, m);
}

int main() {
    run("closed5", {0.0, 4.0, 8.5, 9.0, 5.0}, {0.0, -1.0, 1.5, 6.0, 9.5}, true, 0.1);
    run("open3", {0.0, 3.0, 5.0}, {0.0, 0.5, 2.5}, false, 0.1);
    return 0;
}
