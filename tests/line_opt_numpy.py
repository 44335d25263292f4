"""Float64 twin of pg_optimize_line, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, set) pair at a time, every operation rounded
on its own, in the order the header gives -- the chords and the blocked prefix of the smoother, the normals, the bend rows, the pentadiagonal Hessian in closed form, the
box, ADMM on one band factorisation (bordered on a closed path), the tree sums of the stats.  The band recurrence, the way back and the border are the smoother's text and
are taken from its twin (tests/wp_smooth_numpy.py).  The scheme has only + - * / sqrt and exact comparisons, so the library's output is this one's bit for bit.
dense() restates the same problem with dense matrices built from A and W and numpy.linalg.solve."""
import math

import numpy as np

from wp_smooth_numpy import band_backward, band_forward, blocked_prefix, dot3, tree_sum

SET_DEFAULTS = dict(mu=1e-6, rho=0.1, margin=0.5, alpha_max=2.0, tol=0.0, iters=1000, pin_ends=False, keep_walls=False, windows=())
STATS = ("bend_in", "bend_out", "alpha_abs_max", "i_alpha_max", "n_active", "r_prim", "r_dual", "iters_done", "pivot_min", "chord_min", "width_min", "reserved")


def line_set(**kw):
    """windows: (u_lo, u_hi, margin, pin) entries"""
    s = dict(SET_DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


def clip(x, lo, hi):
    c = x if x > lo else lo
    return hi if c > hi else c


def system(E, N, eL, eR, closed, s):
    """what the scheme computes before the solve: h, p, q, U, the normals, w, f, the band D, E1, E2 of H [n], g, lo, hi"""
    n = len(E)
    nsp = n if closed else n - 1
    h = [0.0] * n; p = [0.0] * n; sE = [0.0] * n; sN = [0.0] * n
    for j in range(nsp):
        jn = (j + 1) % n
        a = E[jn] - E[j]; b = N[jn] - N[j]
        h[j] = math.sqrt((a * a) + (b * b))
        p[j] = 1.0 / h[j]; sE[j] = a / h[j]; sN[j] = b / h[j]
    U = blocked_prefix(h[:n - 1])
    prev = lambda i: i - 1 if i > 0 else n - 1
    q = [(-p[prev(i)]) - p[i] for i in range(n)]
    nE = [0.0] * n; nN = [0.0] * n
    for i in range(n):
        ia, ib = prev(i), (i + 1) % n
        if not closed and i == 0:
            ia = 0
        if not closed and i == n - 1:
            ib = n - 1
        tE = E[ib] - E[ia]; tN = N[ib] - N[ia]
        v = math.sqrt((tE * tE) + (tN * tN))
        nE[i] = (-tN) / v; nN[i] = tE / v
    w = [0.0] * n; fE = [0.0] * n; fN = [0.0] * n
    for j in range(n):
        jm = prev(j)
        fE[j] = sE[j] - sE[jm]; fN[j] = sN[j] - sN[jm]
        if closed or 0 < j < n - 1:
            w[j] = 2.0 / (h[jm] + h[j])
    mu = float(s["mu"])
    D = [0.0] * n; E1 = [0.0] * n; E2 = [0.0] * n; g = [0.0] * n
    for i in range(n):
        im = prev(i); ip = (i + 1) % n; ip2 = (i + 2) % n
        a0 = ((w[im] * (p[im] * p[im])) + (w[i] * (q[i] * q[i]))) + (w[ip] * (p[i] * p[i]))
        a1 = p[i] * ((w[i] * q[i]) + (w[ip] * q[ip]))
        a2 = w[ip] * (p[i] * p[ip])
        a0 = 0.0 + (1.0 * a0); a1 = 0.0 + (1.0 * a1); a2 = 1.0 * a2
        c0 = (nE[i] * nE[i]) + (nN[i] * nN[i])
        c1 = (nE[i] * nE[ip]) + (nN[i] * nN[ip])
        c2 = (nE[i] * nE[ip2]) + (nN[i] * nN[ip2])
        D[i] = (c0 * a0) + mu; E1[i] = c1 * a1; E2[i] = c2 * a2
        kE = (w[im] * fE[im], w[i] * fE[i], w[ip] * fE[ip]); kN = (w[im] * fN[im], w[i] * fN[i], w[ip] * fN[ip])
        s_E = ((p[im] * kE[0]) + (q[i] * kE[1])) + (p[i] * kE[2])
        s_N = ((p[im] * kN[0]) + (q[i] * kN[1])) + (p[i] * kN[2])
        g[i] = (nE[i] * s_E) + (nN[i] * s_N)
    amax = float(s["alpha_max"])
    lo = [0.0] * n; hi = [0.0] * n
    for i in range(n):
        margin = float(s["margin"]); pinned = False
        for (u_lo, u_hi, wm, pin) in s["windows"]:
            if u_lo <= U[i] <= u_hi:
                margin = float(wm); pinned = bool(pin)
        if s["pin_ends"] and not closed and (i == 0 or i == n - 1):
            pinned = True
        a = eR[i] + margin; b = eL[i] - margin
        lo[i] = a if a > -amax else -amax
        hi[i] = b if b < amax else amax
        if pinned:
            lo[i] = 0.0; hi[i] = 0.0
    return dict(h=h, p=p, q=q, U=U, nE=nE, nN=nN, w=w, fE=fE, fN=fN, D=D, E1=E1, E2=E2, g=g, lo=lo, hi=hi)


def bend_terms(S, alpha):
    n = len(alpha)
    h, p, q, w, nE, nN = S["h"], S["p"], S["q"], S["w"], S["nE"], S["nN"]
    out = []
    for i in range(n):
        im = i - 1 if i > 0 else n - 1
        ip = (i + 1) % n
        r = []
        for f, nn in ((S["fE"], nE), (S["fN"], nN)):
            r.append(((f[i] + (p[im] * (alpha[im] * nn[im]))) + (q[i] * (alpha[i] * nn[i]))) + (p[i] * (alpha[ip] * nn[ip])))
        out.append(w[i] * ((r[0] * r[0]) + (r[1] * r[1])))
    return out


class Factor:
    """K = H + rho I factored once: the band of all n rows on an open path; the band of the rows 0 .. n - 3 with the border n - 2, n - 1 on a closed one"""

    def __init__(self, S, rho, closed):
        n = len(S["D"])
        self.n, self.closed = n, closed
        self.D = [d + rho for d in S["D"]]; self.E1 = S["E1"]; self.E2 = S["E2"]
        D, E1, E2 = self.D, self.E1, self.E2
        if not closed:
            self.m = n
            _, _, d, _ = band_forward(D, E1, E2, [0.0] * n)
            self.pivots = list(d)
            return
        m = self.m = n - 2
        self.rows_a = (0, n - 4, n - 3); self.col_a = (E2[n - 2], E2[n - 4], E1[n - 3])
        self.rows_b = (0, 1, n - 3); self.col_b = (E1[n - 1], E2[n - 1], E2[n - 3])
        Ca = [0.0] * m; Cb = [0.0] * m
        for r in range(m):
            Ca[r] = E2[n - 2] if r == 0 else E2[n - 4] if r == n - 4 else E1[n - 3] if r == n - 3 else 0.0
            Cb[r] = E1[n - 1] if r == 0 else E2[n - 1] if r == 1 else E2[n - 3] if r == n - 3 else 0.0
        l1, l2, d, za = band_forward(D[:m], E1[:m], E2[:m], Ca)
        self.Za = band_backward(l1, l2, d, za)
        _, _, _, zb = band_forward(D[:m], E1[:m], E2[:m], Cb)
        self.Zb = band_backward(l1, l2, d, zb)
        self.S00 = D[n - 2] - dot3(self.rows_a, self.col_a, self.Za)
        self.S01 = E1[n - 2] - dot3(self.rows_a, self.col_a, self.Zb)
        self.S11 = D[n - 1] - dot3(self.rows_b, self.col_b, self.Zb)
        self.det = (self.S00 * self.S11) - (self.S01 * self.S01)
        self.pivots = list(d) + [self.S00, self.det / self.S00]

    def solve(self, b):
        m, n = self.m, self.n
        l1, l2, d, z = band_forward(self.D[:m], self.E1[:m], self.E2[:m], b[:m])
        x0 = band_backward(l1, l2, d, z)
        if not self.closed:
            return x0
        ra = b[n - 2] - dot3(self.rows_a, self.col_a, x0)
        rb = b[n - 1] - dot3(self.rows_b, self.col_b, x0)
        xa = ((self.S11 * ra) - (self.S01 * rb)) / self.det
        xb = ((self.S00 * rb) - (self.S01 * ra)) / self.det
        return [(x0[i] - (self.Za[i] * xa)) - (self.Zb[i] * xb) for i in range(m)] + [xa, xb]


def admm(S, s, solve):
    """the iteration of the header with any x = K^-1 b -> (alpha, r_prim, r_dual, iters_done, the largest |x| met)"""
    n = len(S["g"])
    rho, tol = float(s["rho"]), float(s["tol"])
    lo, hi, g = S["lo"], S["hi"], S["g"]
    z = [clip(0.0, lo[i], hi[i]) for i in range(n)]
    u = [0.0] * n
    rp = rd = 0.0
    done = 0
    xmax = 0.0
    for k in range(1, int(s["iters"]) + 1):
        b = [(rho * (z[i] - u[i])) - g[i] for i in range(n)]
        x = solve(b)
        rp = 0.0; dz = 0.0
        for i in range(n):
            zn = clip(x[i] + u[i], lo[i], hi[i])
            u[i] = u[i] + (x[i] - zn)
            a = abs(x[i] - zn)
            if a > rp:
                rp = a
            a = abs(zn - z[i])
            if a > dz:
                dz = a
            z[i] = zn
            xmax = max(xmax, abs(x[i])) if x[i] == x[i] else xmax
        rd = rho * dz
        done = k
        if rp <= tol and rd <= tol:
            break
    return z, rp, rd, done, xmax


def optimize(waypoints, closed=False, s=None):
    """waypoints: dicts of E, N, edge_L, edge_R; s: line_set(...) -> dict(E, N, edge_L, edge_R: float64 [n_wp]; alpha, lo, hi, nE, nN, U, pivots; stats: the fields of
    pg_line_stats)"""
    s = line_set() if s is None else s
    closed = bool(closed)
    E = [float(w["E"]) for w in waypoints]; N = [float(w["N"]) for w in waypoints]
    eL = [float(w["edge_L"]) for w in waypoints]; eR = [float(w["edge_R"]) for w in waypoints]
    n = len(E)
    S = system(E, N, eL, eR, closed, s)
    F = Factor(S, float(s["rho"]), closed)
    alpha, rp, rd, done, _ = admm(S, s, F.solve)
    oE = [E[i] + (alpha[i] * S["nE"][i]) if alpha[i] != 0.0 else E[i] for i in range(n)]
    oN = [N[i] + (alpha[i] * S["nN"][i]) if alpha[i] != 0.0 else N[i] for i in range(n)]
    oL = [eL[i] - alpha[i] if s["keep_walls"] else eL[i] for i in range(n)]
    oR = [eR[i] - alpha[i] if s["keep_walls"] else eR[i] for i in range(n)]
    nsp = n if closed else n - 1
    ch = []
    for j in range(nsp):
        jn = (j + 1) % n
        a = oE[jn] - oE[j]; b = oN[jn] - oN[j]
        ch.append(math.sqrt((a * a) + (b * b)))
    aa = [abs(a) for a in alpha]
    amax = max(aa)
    stats = dict(bend_in=tree_sum([S["w"][i] * ((S["fE"][i] * S["fE"][i]) + (S["fN"][i] * S["fN"][i])) for i in range(n)]), bend_out=tree_sum(bend_terms(S, alpha)),
                 alpha_abs_max=amax, i_alpha_max=float(aa.index(amax)), n_active=float(sum(1 for i in range(n) if alpha[i] == S["lo"][i] or alpha[i] == S["hi"][i])),
                 r_prim=rp, r_dual=rd, iters_done=float(done), pivot_min=min(F.pivots), chord_min=min(ch), width_min=min(a - b for a, b in zip(oL, oR)), reserved=0.0)
    return dict(E=np.array(oE), N=np.array(oN), edge_L=np.array(oL), edge_R=np.array(oR), alpha=np.array(alpha), lo=np.array(S["lo"]), hi=np.array(S["hi"]),
                nE=np.array(S["nE"]), nN=np.array(S["nN"]), U=np.array(S["U"]), pivots=np.array(F.pivots), h=np.array(S["h"][:nsp]), stats=stats)


def dense(waypoints, closed, s):
    """The same problem with dense matrices: A (two rows per bend row, one column per waypoint) and W built from the issue's statement, H = A^T W A + mu I, g = A^T W f,
    the same ADMM with numpy.linalg.solve -> dict(alpha, H, g, cond: the 2-norm condition number of H + rho I, iters_done, xmax)"""
    E = [float(w["E"]) for w in waypoints]; N = [float(w["N"]) for w in waypoints]
    eL = [float(w["edge_L"]) for w in waypoints]; eR = [float(w["edge_R"]) for w in waypoints]
    n = len(E)
    S = system(E, N, eL, eR, bool(closed), s)                       # (h, the normals, f and the box are taken from the twin; H and g are rebuilt here)
    h, nE, nN = S["h"], S["nE"], S["nN"]
    rows = list(range(n)) if closed else list(range(1, n - 1))
    A = np.zeros((2 * len(rows), n)); f = np.zeros(2 * len(rows)); W = np.zeros(2 * len(rows))
    for k, j in enumerate(rows):
        jm = (j - 1) % n; jp = (j + 1) % n
        for c, nn, ff in ((0, nE, S["fE"]), (1, nN, S["fN"])):
            A[2 * k + c, jm] += nn[jm] / h[jm]
            A[2 * k + c, j] += -(1.0 / h[jm] + 1.0 / h[j]) * nn[j]
            A[2 * k + c, jp] += nn[jp] / h[j]
            f[2 * k + c] = ff[j]
            W[2 * k + c] = 2.0 / (h[jm] + h[j])
    H = A.T @ (W[:, None] * A) + float(s["mu"]) * np.eye(n)
    g = A.T @ (W * f)
    K = H + float(s["rho"]) * np.eye(n)
    Sd = dict(S, g=list(g))
    alpha, rp, rd, done, xmax = admm(Sd, s, lambda b: list(np.linalg.solve(K, np.array(b))))
    return dict(alpha=np.array(alpha), H=H, g=g, cond=float(np.linalg.cond(K)), iters_done=done, xmax=xmax, r_prim=rp, r_dual=rd,
                bend_in=float(np.sum(W * f * f)), bend_out=float(np.sum(W * (f + A @ np.array(alpha)) ** 2)))
