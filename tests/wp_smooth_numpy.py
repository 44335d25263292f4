"""Float64 twin of pg_smooth_waypoints, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, set) pair at a time, every operation rounded
on its own, in the order the header gives -- the blocked prefix of the chords, the band entries in closed form, the band LDL^T recurrence without pivoting, the bordering of
a closed path with its 2 x 2 Schur complement, the tree sums of the stats.  The scheme has only + - * / sqrt, so the library's output is this one's bit for bit."""
import math

import numpy as np

THREADS = 256
SET_DEFAULTS = dict(lam=0.0, pin_ends=False, keep_walls=False, windows=())
STATS = ("dev_max", "dev_rms", "i_dev_max", "bend", "n_outside", "width_min", "pivot_min", "chord_min", "reserved")


def smooth_set(**kw):
    s = dict(SET_DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


def blocked_prefix(l):
    """[0, S_1, .., S_n]: S_{j+1} = P_{j / c} + r_{j+1}, the blocked order of pg_make_paths (Prefix), c = ceil(n / 256)"""
    n = len(l)
    c = max(1, (n + THREADS - 1) // THREADS)
    r = [0.0] * (n + 1); T = [0.0] * THREADS
    for b in range(THREADS):
        a = 0.0
        for j in range(min(b * c, n), min(b * c + c, n)):
            a = a + l[j]
            r[j + 1] = a
        T[b] = a
    I = list(T)
    d = 1
    while d < 64:
        I = [I[b] + I[b - d] if b % 64 >= d else I[b] for b in range(THREADS)]
        d *= 2
    G = [0.0]
    for g in range(THREADS // 64 - 1):
        G.append(G[-1] + I[64 * g + 63])
    P = [G[b // 64] + (I[b - 1] if b % 64 > 0 else 0.0) for b in range(THREADS)]
    return [0.0] + [P[j // c] + r[j + 1] for j in range(n)]


def tree_sum(v):
    """Sum: block b of c = ceil(n / 256) consecutive terms summed from 0 in order, then the 256 block totals by the tree of neighbouring pairs"""
    n = len(v)
    c = max(1, (n + THREADS - 1) // THREADS)
    T = []
    for b in range(THREADS):
        a = 0.0
        for j in range(min(b * c, n), min(b * c + c, n)):
            a = a + v[j]
        T.append(a)
    while len(T) > 1:
        T = [T[k] + T[k + 1] for k in range(0, len(T), 2)]
    return T[0]


def band_forward(D, E1, E2, f):
    """Rows 0 .. m - 1 of the band system: the LDL^T recurrence and the forward substitution -> (l1, l2, d, z)"""
    m = len(f)
    l1 = [0.0] * m; l2 = [0.0] * m; d = [0.0] * m; z = [0.0] * m
    for r in range(m):
        e1 = E1[r - 1] if r >= 1 else 0.0
        e2 = E2[r - 2] if r >= 2 else 0.0
        d1 = d[r - 1] if r >= 1 else 1.0
        d2 = d[r - 2] if r >= 2 else 1.0
        lp = l1[r - 1] if r >= 1 else 0.0
        z1 = z[r - 1] if r >= 1 else 0.0
        z2 = z[r - 2] if r >= 2 else 0.0
        l2[r] = e2 / d2
        c1 = e1 - (e2 * lp)
        l1[r] = c1 / d1
        d[r] = (D[r] - (e2 * l2[r])) - (c1 * l1[r])
        z[r] = (f[r] - (l1[r] * z1)) - (l2[r] * z2)
    return l1, l2, d, z


def band_backward(l1, l2, d, z):
    m = len(z)
    x = [0.0] * m
    for r in range(m - 1, -1, -1):
        a = l1[r + 1] * x[r + 1] if r + 1 < m else 0.0
        b = l2[r + 2] * x[r + 2] if r + 2 < m else 0.0
        x[r] = ((z[r] / d[r]) - a) - b
    return x


def band_solve(D, E1, E2, f):
    l1, l2, d, z = band_forward(D, E1, E2, f)
    return band_backward(l1, l2, d, z), d


def system(E, N, closed, s):
    """what the scheme computes before the solve: h, p (0 in place n - 1 of an open path), U, winv, the band D, E1, E2 [n] and the right-hand sides fE, fN [n]"""
    n = len(E)
    lam = float(s["lam"])
    nsp = n if closed else n - 1
    h = [0.0] * n; p = [0.0] * n; dE = [0.0] * n; dN = [0.0] * n
    for j in range(nsp):
        jn = (j + 1) % n
        a = E[jn] - E[j]; b = N[jn] - N[j]
        h[j] = math.sqrt(a * a + b * b)
        p[j] = 1.0 / h[j]; dE[j] = a / h[j]; dN[j] = b / h[j]
    U = blocked_prefix(h[:n - 1])
    winv = [1.0] * n
    for i in range(n):
        for (u_lo, u_hi, factor) in s["windows"]:
            if u_lo <= U[i] <= u_hi:
                winv[i] = float(factor)
    if s["pin_ends"] and not closed:
        winv[0] = 0.0; winv[n - 1] = 0.0
    q = [(-p[i - 1 if i > 0 else n - 1]) - p[i] for i in range(n)]
    D = [0.0] * n; E1 = [0.0] * n; E2 = [0.0] * n; fE = [0.0] * n; fN = [0.0] * n
    for i in range(n):
        im = i - 1 if i > 0 else n - 1
        ip = (i + 1) % n; ip2 = (i + 2) % n
        a0 = ((winv[im] * (p[im] * p[im])) + (winv[i] * (q[i] * q[i]))) + (winv[ip] * (p[i] * p[i]))
        a1 = p[i] * ((winv[i] * q[i]) + (winv[ip] * q[ip]))
        a2 = winv[ip] * (p[i] * p[ip])
        D[i] = ((h[im] + h[i]) / 3.0) + (lam * a0)
        E1[i] = (h[i] / 6.0) + (lam * a1)
        E2[i] = lam * a2
        fE[i] = dE[i] - dE[im]; fN[i] = dN[i] - dN[im]
    return dict(h=h, p=p, q=q, U=U, winv=winv, D=D, E1=E1, E2=E2, fE=fE, fN=fN)


def dot3(rows, col, x):
    a = col[0] * x[rows[0]]
    a = a + col[1] * x[rows[1]]
    return a + col[2] * x[rows[2]]


def gammas(S, n, closed):
    """gamma_E, gamma_N [n] (0 outside the rows) and the smallest pivot"""
    D, E1, E2 = S["D"], S["E1"], S["E2"]
    if not closed:
        gE = [0.0] * n; gN = [0.0] * n
        if n < 3:
            return gE, gN, math.inf, []
        xE, d = band_solve(D[1:n - 1], E1[1:n - 1], E2[1:n - 1], S["fE"][1:n - 1])
        xN, _ = band_solve(D[1:n - 1], E1[1:n - 1], E2[1:n - 1], S["fN"][1:n - 1])
        gE[1:n - 1] = xE; gN[1:n - 1] = xN
        return gE, gN, min(d), d
    m = n - 2
    rows_a = (0, n - 4, n - 3); col_a = (E2[n - 2], E2[n - 4], E1[n - 3])
    rows_b = (0, 1, n - 3); col_b = (E1[n - 1], E2[n - 1], E2[n - 3])
    Ca = [0.0] * m; Cb = [0.0] * m
    for r, v in zip(rows_a, col_a):
        Ca[r] = v
    for r, v in zip(rows_b, col_b):
        Cb[r] = v
    Za, d = band_solve(D[:m], E1[:m], E2[:m], Ca)
    Zb, _ = band_solve(D[:m], E1[:m], E2[:m], Cb)
    S00 = D[n - 2] - dot3(rows_a, col_a, Za)
    S01 = E1[n - 2] - dot3(rows_a, col_a, Zb)
    S11 = D[n - 1] - dot3(rows_b, col_b, Zb)
    det = (S00 * S11) - (S01 * S01)
    out = []
    for f in (S["fE"], S["fN"]):
        x0, _ = band_solve(D[:m], E1[:m], E2[:m], f[:m])
        ra = f[n - 2] - dot3(rows_a, col_a, x0)
        rb = f[n - 1] - dot3(rows_b, col_b, x0)
        xa = ((S11 * ra) - (S01 * rb)) / det
        xb = ((S00 * rb) - (S01 * ra)) / det
        out.append([(x0[i] - (Za[i] * xa)) - (Zb[i] * xb) for i in range(m)] + [xa, xb])
    return out[0], out[1], min(min(d), S00, det / S00), d + [S00, det / S00]


def smooth(waypoints, closed=False, s=None):
    """waypoints: dicts of E, N, edge_L, edge_R; s: smooth_set(...) -> dict(E, N, edge_L, edge_R: float64 [n_wp]; gamma_E, gamma_N, U, winv, pivots; stats: the fields of
    pg_smooth_stats)"""
    s = smooth_set() if s is None else s
    closed = bool(closed)
    E = [float(w["E"]) for w in waypoints]; N = [float(w["N"]) for w in waypoints]
    eL = [float(w["edge_L"]) for w in waypoints]; eR = [float(w["edge_R"]) for w in waypoints]
    n = len(E)
    lam = float(s["lam"])
    S = system(E, N, closed, s)
    h, p, q, winv = S["h"], S["p"], S["q"], S["winv"]
    gE, gN, pivot_min, pivots = gammas(S, n, closed)
    oE = [0.0] * n; oN = [0.0] * n
    for i in range(n):
        im = i - 1 if i > 0 else n - 1
        ip = (i + 1) % n
        for y, g, o in ((E, gE, oE), (N, gN, oN)):
            qg = ((p[im] * g[im]) + (q[i] * g[i])) + (p[i] * g[ip])
            o[i] = y[i] - (lam * (winv[i] * qg))
    oL = [0.0] * n; oR = [0.0] * n; dev2 = [0.0] * n; bend = [0.0] * n
    n_out = 0
    for i in range(n):
        im = i - 1 if i > 0 else n - 1
        ip = (i + 1) % n
        t = []
        for o, g in ((oE, gE), (oN, gN)):
            if closed or i < n - 1:
                sl = (o[ip] - o[i]) / h[i]
                t.append(sl - ((h[i] * ((2.0 * g[i]) + g[ip])) / 6.0))
            else:
                sl = (o[i] - o[im]) / h[im]
                t.append(sl + ((h[im] * ((2.0 * g[i]) + g[im])) / 6.0))
        v = math.sqrt((t[0] * t[0]) + (t[1] * t[1]))
        nE = (-t[1]) / v; nN = t[0] / v
        dE = oE[i] - E[i]; dN = oN[i] - N[i]
        c = (dE * nE) + (dN * nN)
        dev2[i] = (dE * dE) + (dN * dN)
        if c > eL[i] or c < eR[i]:
            n_out += 1
        oL[i] = eL[i] - c if s["keep_walls"] else eL[i]
        oR[i] = eR[i] - c if s["keep_walls"] else eR[i]
        b = 0.0
        for g in (gE, gN):
            r0 = (h[im] + h[i]) / 3.0
            inner = (((h[im] / 6.0) * g[im]) + (r0 * g[i])) + ((h[i] / 6.0) * g[ip])
            b = b + (g[i] * inner)
        bend[i] = b
    dev = [math.sqrt(v) for v in dev2]
    nsp = n if closed else n - 1
    ch = []
    for j in range(nsp):
        jn = (j + 1) % n
        a = oE[jn] - oE[j]; b = oN[jn] - oN[j]
        ch.append(math.sqrt((a * a) + (b * b)))
    dev_max = max(dev)
    stats = dict(dev_max=dev_max, dev_rms=math.sqrt(tree_sum(dev2) / float(n)), i_dev_max=float(dev.index(dev_max)), bend=tree_sum(bend), n_outside=float(n_out),
                 width_min=min(a - b for a, b in zip(oL, oR)), pivot_min=pivot_min, chord_min=min(ch), reserved=0.0)
    return dict(E=np.array(oE), N=np.array(oN), edge_L=np.array(oL), edge_R=np.array(oR), gamma_E=np.array(gE), gamma_N=np.array(gN), U=np.array(S["U"]),
                winv=np.array(winv), pivots=np.array(pivots), h=np.array(h[:nsp]), stats=stats)


def dense(waypoints, closed, s):
    """The same system assembled as dense matrices from Q, R and Winv as the issue states them and solved by numpy.linalg.solve -> (gamma [rows][2], g [n][2]); the rows are
    1 .. n - 2 on an open path and all n on a closed one"""
    y = np.array([[float(w["E"]), float(w["N"])] for w in waypoints])
    n = len(y)
    S = system(list(y[:, 0]), list(y[:, 1]), bool(closed), s)
    h = S["h"]
    rows = list(range(n)) if closed else list(range(1, n - 1))
    Q = np.zeros((n, len(rows))); R = np.zeros((len(rows), len(rows)))
    for k, i in enumerate(rows):
        im = (i - 1) % n; ip = (i + 1) % n
        Q[im, k] += 1.0 / h[im]; Q[i, k] += -(1.0 / h[im]) - (1.0 / h[i]); Q[ip, k] += 1.0 / h[i]
        R[k, k] = (h[im] + h[i]) / 3.0
        if closed or i + 1 <= n - 2:
            kp = rows.index(ip)
            R[k, kp] += h[i] / 6.0; R[kp, k] += h[i] / 6.0
    W = np.diag(S["winv"])
    lam = float(s["lam"])
    if not rows:
        return np.zeros((0, 2)), y.copy()
    gamma = np.linalg.solve(R + lam * Q.T @ W @ Q, Q.T @ y)
    return gamma, y - lam * W @ Q @ gamma
