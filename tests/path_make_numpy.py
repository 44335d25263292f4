"""Float64 numpy twin of pg_make_paths, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one path at a time, every operation rounded on its own,
in the order the header gives.  s, psi, kappa, the edges, t, V and A are the library's bit for bit.  E and N are the serial sum (np.cumsum) of the interval increments, not the
blocked sum of the library: the two agree within 4 (n_knots + 64) 2^-53 total (the bound of DESIGN.md 4.16, which the GPU test asserts)."""
import math

import numpy as np

SEGMENT_DEFAULTS = dict(length=1.0, kappa0=0.0, kappa1=0.0, edge_L0=4.0, edge_L1=4.0, edge_R0=-4.0, edge_R1=-4.0, reserved=0.0)
GL_X = (-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526)
GL_W = (0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538)
TWO_PI = 6.283185307179586


def segment(**kw):
    s = dict(SEGMENT_DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = float(v)
    return s


def bounds(segs, psi0):
    """b [n_seg + 1], psib [n_seg + 1]"""
    b, psib = [0.0], [float(psi0)]
    for g in segs:
        b.append(b[-1] + g["length"])
        psib.append(psib[-1] + (0.5 * (g["kappa0"] + g["kappa1"])) * g["length"])
    return b, psib


def lerp(a0, a1, u, length):
    return a0 + ((a1 - a0) * u) / length


def psi_of(g, psib, u):
    return psib + u * (g["kappa0"] + ((0.5 * (g["kappa1"] - g["kappa0"])) * u) / g["length"])


def piece(g, psib, ua, ub):
    half = 0.5 * (ub - ua); mid = 0.5 * (ua + ub)
    aS = 0.0; aC = 0.0
    for x, w in zip(GL_X, GL_W):
        p = psi_of(g, psib, mid + half * x)
        aS = aS + w * math.sin(p); aC = aC + w * math.cos(p)
    return -(half * aS), half * aC


def segment_of(b, n_seg, s):
    """the largest j with b_j <= s, among the segments"""
    j = 0
    while j + 1 < n_seg and b[j + 1] <= s:
        j += 1
    return j


def make(segs, n_knots, pose=(0.0, 0.0, 0.0), V_ref=6.0):
    """-> dict(t, s, V, A, E, N, psi, kappa, edge_L, edge_R: float64 [n_knots]; dE, dN: the interval increments; stats: the fields of pg_path_stats)"""
    E0, N0, psi0 = (float(x) for x in pose)
    n_seg = len(segs)
    b, psib = bounds(segs, psi0)
    total = b[-1]
    ds = total / (n_knots - 1)
    s = np.array([i * ds for i in range(n_knots - 1)] + [total])
    where = [segment_of(b, n_seg, s[i]) for i in range(n_knots - 1)] + [n_seg - 1]
    psi = np.zeros(n_knots); kappa = np.zeros(n_knots); eL = np.zeros(n_knots); eR = np.zeros(n_knots)
    for i in range(n_knots):
        j = where[i]; g = segs[j]
        u = s[i] - b[j] if i < n_knots - 1 else g["length"]
        kappa[i] = lerp(g["kappa0"], g["kappa1"], u, g["length"])
        psi[i] = psi_of(g, psib[j], u)
        eL[i] = lerp(g["edge_L0"], g["edge_L1"], u, g["length"]); eR[i] = lerp(g["edge_R0"], g["edge_R1"], u, g["length"])
    dE = np.zeros(n_knots - 1); dN = np.zeros(n_knots - 1)
    for i in range(n_knots - 1):
        j = where[i]; u = s[i] - b[j]; sn = s[i + 1]
        aE = 0.0; aN = 0.0
        while j + 1 < n_seg and b[j + 1] < sn:
            pE, pN = piece(segs[j], psib[j], u, segs[j]["length"])
            aE = aE + pE; aN = aN + pN
            j += 1; u = 0.0
        pE, pN = piece(segs[j], psib[j], u, sn - b[j])
        dE[i] = aE + pE; dN[i] = aN + pN
    E = E0 + np.concatenate([[0.0], np.cumsum(dE)]); N = N0 + np.concatenate([[0.0], np.cumsum(dN)])
    turn = psi[-1] - psi0
    r = math.remainder(turn, TWO_PI)
    if r <= -math.pi:
        r = r + TWO_PI
    stats = dict(length=total, turn=turn, closure_pos=math.hypot(E[-1] - E0, N[-1] - N0), closure_psi=r, kappa_abs_max=float(np.max(np.abs(kappa))), ds=ds)
    return dict(t=s / V_ref, s=s, V=np.full(n_knots, float(V_ref)), A=np.zeros(n_knots), E=E, N=N, psi=psi, kappa=kappa, edge_L=eL, edge_R=eR, dE=dE, dN=dN, stats=stats)


CHANNELS = ("t", "s", "V", "A", "E", "N", "psi", "kappa", "edge_L", "edge_R")


def channels(r, Lmax):
    """[10][Lmax] in the order of pg_set_trajectories, 0 at and past n_knots"""
    out = np.zeros((10, Lmax))
    for c, name in enumerate(CHANNELS):
        out[c, :len(r[name])] = r[name]
    return out
