// The search helpers of pg_tune_smoothing on the host (pigeon.jl_amd/csrc/pg_waypoint_tune.hpp: wt_ladder, wt_band_parts, wt_forward, wt_backward, wt_border, wt_gamma,
// wt_first_above, wt_monotone, wt_repeats), as the kernel calls them with one candidate per lane: tests/test_wp_tune_host.py builds this stand-alone program (its own
// main; with -fsanitize=address,undefined) and compares what it prints with the twin bit for bit.  Two paths of tests/wp_tune_cases.py with winv = 1: the closed one of
// 5 waypoints (three band rows, the two border unknowns) and the open one of 3 (one row), round 0 of the bracket [1e-4, 1e2] against the target 2e-3.
// Output: one line per candidate, "name j c_j F_j" in hexadecimal floating point, then "name narrow j* monotone repeats".
#include <stdio.h>
#include <vector>
#include "pg_waypoint_tune.hpp"

static void run(const char* name, const std::vector<double>& E, const std::vector<double>& N, bool closed, double lo, double hi, double target) {
    const int n = (int)E.size(), nsp = closed ? n : n - 1, m = n - 2;
    std::vector<double> h(n, 0.0), p(n, 0.0), sE(n, 0.0), sN(n, 0.0), w(n, 1.0), a0(n), a1(n), a2(n), r0(n), r1(n), fE(n), fN(n);
    for (int j = 0; j < nsp; j++) {
        const int jn = j + 1 == n ? 0 : j + 1;
        const double dE = E[jn] - E[j], dN = N[jn] - N[j];
        const double ee = dE * dE, nn = dN * dN;
        h[j] = sqrt(ee + nn); p[j] = 1.0 / h[j]; sE[j] = dE / h[j]; sN[j] = dN / h[j];
    }
    for (int i = 0; i < n; i++) {
        const int im = i > 0 ? i - 1 : n - 1, ip = i + 1 == n ? 0 : i + 1;
        wt_band_parts(h[im], h[i], p[im], p[i], p[ip], w[im], w[i], w[ip], a0[i], a1[i], a2[i], r0[i], r1[i]);
        fE[i] = sE[i] - sE[im]; fN[i] = sN[i] - sN[im];
    }
    WtParts Q; Q.a0 = a0.data(); Q.a1 = a1.data(); Q.a2 = a2.data(); Q.r0 = r0.data(); Q.r1 = r1.data();
    double c[WT_CAND], F[WT_CAND];
    wt_ladder(lo, hi, c);
    // exactly WT_STATE x m x WT_CAND entries: an index past a row or a candidate is an error a sanitizer sees
    const size_t rows = (size_t)m;
    std::vector<double> state((size_t)WT_STATE * rows * WT_CAND, 0.0);
    for (int k = 0; k < WT_CAND; k++) {
        double* const st = state.data() + k;
        double pm; int br;
        if (closed) { wt_forward<4>(n, true, c[k], Q, fE.data(), fN.data(), 0, true, st, rows, pm, br); wt_backward<4>(m, 0, st, rows); }
        else { wt_forward<2>(n, false, c[k], Q, fE.data(), fN.data(), 0, true, st, rows, pm, br); wt_backward<2>(m, 0, st, rows); }
        double x[4] = {0.0, 0.0, 0.0, 0.0}, S00 = 1.0, p2 = 1.0;
        if (closed) wt_border(n, c[k], Q, fE.data(), fN.data(), st, rows, x, S00, p2);
        if (br < m || !(S00 > 0.0) || !(p2 > 0.0)) { printf("%s bad pivot at candidate %d\n", name, k); return; }
        // Sum: n <= 256, so a block is one waypoint (0 + d2) and the rest are 0; then the tree of neighbouring pairs
        std::vector<double> T(256, 0.0);
        for (int i = 0; i < n; i++) {
            const int im = i > 0 ? i - 1 : n - 1, ip = i + 1 == n ? 0 : i + 1;
            const double npm = -p[im];
            const double q = npm - p[i];
            double d2 = 0.0;
            for (int co = 0; co < 2; co++) {
                const double gm = wt_gamma(im, co, n, closed, st, rows, x), g0 = wt_gamma(i, co, n, closed, st, rows, x), gp = wt_gamma(ip, co, n, closed, st, rows, x);
                const double a = p[im] * gm, b = q * g0, cc = p[i] * gp;
                const double ab = a + b;
                const double qg = ab + cc;
                const double wq = w[i] * qg;
                const double lw = c[k] * wq;
                const double y = co == 0 ? E[i] : N[i];
                const double o = y - lw;
                const double d = o - y;
                const double dd = d * d;
                d2 = co == 0 ? dd : d2 + dd;
            }
            T[i] = 0.0 + d2;
        }
        for (int len = 256; len > 1; len /= 2) for (int j = 0; j < len / 2; j++) T[j] = T[2 * j] + T[2 * j + 1];
        const double ms = T[0] / (double)n;
        F[k] = sqrt(ms);
        printf("%s %d %a %a\n", name, k, c[k], F[k]);
    }
    printf("%s narrow %d monotone %d repeats %d\n", name, wt_first_above(F, target), (int)wt_monotone(F), (int)wt_repeats(c));
}

int main() {
    run("closed5", {0.0, 4.0, 8.5, 9.0, 5.0}, {0.0, -1.0, 1.5, 6.0, 9.5}, true, 1e-4, 1e2, 2e-3);
    run("open3", {0.0, 3.0, 5.0}, {0.0, 0.5, 2.5}, false, 1e-4, 1e2, 2e-3);
    double c[WT_CAND];
    wt_ladder(1.0, 1.0 + 0x1p-50, c);                              // a bracket four doubles wide: the ladder must repeat
    printf("narrowest repeats %d\n", (int)wt_repeats(c));
    return 0;
}
