"""Float64 numpy twin of pg_fit_paths, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one path at a time, every operation rounded on its own,
in the order the header gives -- the Thomas recurrences, the Sherman-Morrison correction of a closed path, the two 4-point Gauss-Legendre pieces of a span length, the blocked
prefix of the span lengths and the three fixed Newton steps included.  Everything but atan2 is therefore the library's bit for bit; psi, turn and closure_psi are within
8 * 2^-52 * max(pi, |psi|) (two ulp of the device's atan2, one of libm's, the rounding of the offset add)."""
import math

import numpy as np

WAYPOINT_DEFAULTS = dict(E=0.0, N=0.0, edge_L=4.0, edge_R=-4.0)
GL_X = (-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526)
GL_W = (0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538)
TWO_PI = 6.283185307179586
THREADS = 256


def waypoint(**kw):
    w = dict(WAYPOINT_DEFAULTS)
    for k, v in kw.items():
        if k not in w:
            raise KeyError(k)
        w[k] = float(v)
    return w


def chords(E, N, closed):
    """h [n_span], and the slopes dE / h, dN / h of the spans; span j runs from waypoint j to waypoint (j + 1) mod n_wp"""
    n = len(E)
    n_span = n if closed else n - 1
    h, sE, sN = [], [], []
    for j in range(n_span):
        jn = (j + 1) % n
        dE = E[jn] - E[j]; dN = N[jn] - N[j]
        hj = math.sqrt(dE * dE + dN * dN)
        h.append(hj); sE.append(dE / hj); sN.append(dN / hj)
    return h, sE, sN


def thomas(h, bb, g, lo, hi):
    """the rows lo .. hi of a tridiagonal system with the sub-diagonal a_i = h_{i-1}, the diagonal bb_i and the super-diagonal c_i = h_i; g is overwritten by the solution"""
    if hi < lo:
        return
    beta = [0.0] * len(g)
    beta[lo] = bb[lo]
    for i in range(lo + 1, hi + 1):
        w = h[i - 1] / beta[i - 1]
        beta[i] = bb[i] - w * h[i - 1]
        g[i] = g[i] - w * g[i - 1]
    g[hi] = g[hi] / beta[hi]
    for i in range(hi - 1, lo - 1, -1):
        g[i] = (g[i] - h[i] * g[i + 1]) / beta[i]


def second_derivatives(h, sE, sN, n, closed):
    """M_E, M_N at the n waypoints"""
    gE = [0.0] * n; gN = [0.0] * n; gZ = [0.0] * n; bb = [0.0] * n
    if not closed:
        for i in range(1, n - 1):
            bb[i] = 2.0 * (h[i - 1] + h[i])
            gE[i] = 6.0 * (sE[i] - sE[i - 1]); gN[i] = 6.0 * (sN[i] - sN[i - 1])
        thomas(h, bb, gE, 1, n - 2); thomas(h, bb, gN, 1, n - 2)
        return gE, gN
    hl = h[n - 1]
    b0 = 2.0 * (hl + h[0])
    for i in range(n):
        im = i - 1 if i > 0 else n - 1
        bb[i] = 2.0 * (h[im] + h[i])
        gE[i] = 6.0 * (sE[i] - sE[im]); gN[i] = 6.0 * (sN[i] - sN[im])
    bb[0] = 2.0 * b0
    bb[n - 1] = bb[n - 1] + (hl * hl) / b0
    gZ[0] = -b0; gZ[n - 1] = hl
    for g in (gE, gN, gZ):
        thomas(h, bb, g, 0, n - 1)
    den = (1.0 + gZ[0]) - (hl * gZ[n - 1]) / b0
    out = []
    for g in (gE, gN):
        fact = (g[0] - (hl * g[n - 1]) / b0) / den
        out.append([g[i] - fact * gZ[i] for i in range(n)])
    return out[0], out[1]


class Span:
    """the cubic of one span in u in [0, h]: y(u) = y0 + u (c1 + u (0.5 M0 + u c3))"""
    def __init__(self, h, y0, slope, M0, M1):
        self.h = h; self.y0 = y0; self.M0 = M0
        self.c1 = slope - (h * (2.0 * M0 + M1)) / 6.0
        self.c3 = (M1 - M0) / (6.0 * h)

    def pos(self, u):
        return self.y0 + u * (self.c1 + u * (0.5 * self.M0 + u * self.c3))

    def d1(self, u):
        return self.c1 + u * (self.M0 + u * (3.0 * self.c3))

    def d2(self, u):
        return self.M0 + u * (6.0 * self.c3)


def speed(sE, sN, u):
    a = sE.d1(u); b = sN.d1(u)
    return math.sqrt(a * a + b * b)


def piece(sE, sN, ua, ub):
    half = 0.5 * (ub - ua); mid = 0.5 * (ua + ub)
    acc = 0.0
    for x, w in zip(GL_X, GL_W):
        acc = acc + w * speed(sE, sN, mid + half * x)
    return half * acc


def length(sE, sN, u):
    um = 0.5 * u
    return piece(sE, sN, 0.0, um) + piece(sE, sN, um, u)


def blocked_prefix(l):
    """S [n_span + 1]: S_0 = 0, S_{j+1} = P_{j / c} + r_{j+1}, the blocked order of pg_make_paths (include/pigeon_mpc.h, Prefix) over the span lengths"""
    n = len(l)
    c = (n + THREADS - 1) // THREADS
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


def clamp(u, h):
    if not u >= 0.0:
        return 0.0
    return h if u > h else u


def fit(waypoints, n_knots, V_ref=6.0, closed=False):
    """waypoints: dicts of E, N, edge_L, edge_R -> dict(t, s, V, A, E, N, psi, kappa, edge_L, edge_R: float64 [n_knots]; psi_raw; M_E, M_N at the waypoints; h, l, S of
    the spans; stats: the fields of pg_fit_stats)"""
    E = [float(w["E"]) for w in waypoints]; N = [float(w["N"]) for w in waypoints]
    eL = [float(w["edge_L"]) for w in waypoints]; eR = [float(w["edge_R"]) for w in waypoints]
    n = len(E)
    h, slE, slN = chords(E, N, closed)
    n_span = len(h)
    ME, MN = second_derivatives(h, slE, slN, n, closed)
    spans = [(Span(h[j], E[j], slE[j], ME[j], ME[(j + 1) % n]), Span(h[j], N[j], slN[j], MN[j], MN[(j + 1) % n])) for j in range(n_span)]
    l = [length(a, b, h[j]) for j, (a, b) in enumerate(spans)]
    S = blocked_prefix(l)
    total = S[n_span]
    ds = total / (n_knots - 1)
    out = {k: np.zeros(n_knots) for k in ("s", "E", "N", "psi_raw", "kappa", "edge_L", "edge_R")}
    s_err = 0.0
    for i in range(n_knots):
        last = i == n_knots - 1
        s = total if last else i * ds
        if last:
            j = n_span - 1
        else:
            lo, hi = 0, n_span - 1
            while lo < hi:
                m = (lo + hi + 1) >> 1
                if S[m] <= s:
                    lo = m
                else:
                    hi = m - 1
            j = lo
        a, b = spans[j]
        target = s - S[j]
        if last:
            u = h[j]
        else:
            u = clamp((target * h[j]) / l[j], h[j])
            for _ in range(3):
                u = clamp(u - (length(a, b, u) - target) / speed(a, b, u), h[j])
        s_err = max(s_err, abs(length(a, b, u) - target))
        jn = (j + 1) % n
        d1E = a.d1(u); d1N = b.d1(u); d2E = a.d2(u); d2N = b.d2(u)
        v2 = d1E * d1E + d1N * d1N
        out["s"][i] = s
        out["E"][i] = E[jn] if last else a.pos(u)
        out["N"][i] = N[jn] if last else b.pos(u)
        out["kappa"][i] = (d1E * d2N - d2E * d1N) / (v2 * math.sqrt(v2))
        out["psi_raw"][i] = math.atan2(-d1E, d1N)
        out["edge_L"][i] = eL[j] + ((eL[jn] - eL[j]) * u) / h[j]
        out["edge_R"][i] = eR[j] + ((eR[jn] - eR[j]) * u) / h[j]
    k = 0
    psi = np.zeros(n_knots)
    for i in range(n_knots):
        if i > 0:
            d = out["psi_raw"][i] - out["psi_raw"][i - 1]
            k += -1 if d > math.pi else 1 if d < -math.pi else 0
        psi[i] = out["psi_raw"][i] + k * TWO_PI
    turn = float(psi[-1] - psi[0])
    r = math.remainder(turn, TWO_PI)
    if r <= -math.pi:
        r = r + TWO_PI
    gE = out["E"][-1] - out["E"][0]; gN = out["N"][-1] - out["N"][0]
    stats = dict(length=total, turn=turn, closure_pos=math.sqrt(gE * gE + gN * gN), closure_psi=r, kappa_abs_max=float(np.max(np.abs(out["kappa"]))), ds=ds,
                 chord_min=min(h), chord_max=max(h), s_err_max=s_err, reserved=0.0)
    out.update(t=out["s"] / V_ref, V=np.full(n_knots, float(V_ref)), A=np.zeros(n_knots), psi=psi, M_E=np.array(ME), M_N=np.array(MN), h=np.array(h), l=np.array(l),
               S=np.array(S), stats=stats)
    return out


CHANNELS = ("t", "s", "V", "A", "E", "N", "psi", "kappa", "edge_L", "edge_R")


def channels(r, Lmax):
    """[10][Lmax] in the order of pg_set_trajectories, 0 at and past n_knots"""
    out = np.zeros((10, Lmax))
    for c, name in enumerate(CHANNELS):
        out[c, :len(r[name])] = r[name]
    return out
