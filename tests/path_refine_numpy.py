"""Float64 twin of pg_refine_paths, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, refine set) pair at a time, every operation
rounded on its own, in the order the header gives (a parenthesis of the header is one Python operation here).  L_out, t, s, V, A, psi, kappa, both edges and every stat
but closure_pos_max are the library's bit for bit; E, N and closure_pos_max carry sin and cos.  The offsets are a prefix over integers: a plain running sum."""
import math

import numpy as np

from path_make_numpy import GL_W, GL_X

INF = math.inf
M_MAX = 4096
CHANNELS = ("t", "s", "V", "A", "E", "N", "psi", "kappa", "edge_L", "edge_R")


def refine_set(ds=INF, windows=()):
    """ds and up to four (s_lo, s_hi, ds_w); the unused slots are (+Inf, +Inf, +Inf)"""
    w = [tuple(float(x) for x in win) for win in windows]
    assert len(w) <= 4
    return dict(ds=float(ds), windows=w + [(INF, INF, INF)] * (4 - len(w)), reserved=(0.0, 0.0, 0.0))


def parts(S, diff, u_lo, u_hi):
    """Parts of the header: m_i; raises ValueError where the library refuses"""
    w = S["ds"]
    for s_lo, s_hi, ds_w in S["windows"]:
        if s_lo < INF and s_lo < u_hi and s_hi > u_lo:
            w = min(w, ds_w)
    if w == INF or diff <= w:
        return 1
    q = diff / w
    if not q <= 4096.0:
        raise ValueError("more than 4096 parts")
    return int(math.ceil(q))


def lengths(s, S):
    """(m [L - 1], o [L], L_out) of one pair"""
    s = [float(v) for v in s]
    m = [parts(S, s[i + 1] - s[i], s[i] - s[0], s[i + 1] - s[0]) for i in range(len(s) - 1)]
    o = [0]
    for mi in m:
        o.append(o[-1] + mi)
    return m, o, o[-1] + 1


def _psi(psi0, a, b, v):
    return psi0 + (v * (a + (v * b)))


def _piece(psi0, a, b, va, vb):
    half = 0.5 * (vb - va); mid = 0.5 * (va + vb)
    aS = 0.0; aC = 0.0
    for x, w in zip(GL_X, GL_W):
        p = _psi(psi0, a, b, mid + (half * x))
        aS = aS + (w * math.sin(p)); aC = aC + (w * math.cos(p))
    return -(half * aS), half * aC


def _integral(psi0, a, b, v):
    hv = 0.5 * v
    e0, n0 = _piece(psi0, a, b, 0.0, hv)
    e1, n1 = _piece(psi0, a, b, hv, v)
    return e0 + e1, n0 + n1


def refine(ch, S):
    """ch: the source's channels [10][L] float64; S: refine_set(...) -> dict(the ten channels [L_out]; m, o: parts and offsets; stats: the fields of pg_refine_stats)"""
    ch = np.asarray(ch, dtype=np.float64)
    T, s, V, A, E, N, psi, kap, eL, eR = ([float(v) for v in ch[c]] for c in range(10))
    L = len(s); nint = L - 1
    m, o, L_out = lengths(s, S)
    out = {name: np.zeros(L_out) for name in CHANNELS}
    cpos = 0.0; cpsi = 0.0
    for i in range(nint):
        diff = s[i + 1] - s[i]
        b = (0.5 * (kap[i + 1] - kap[i])) / diff
        a = ((psi[i + 1] - psi[i]) / diff) - (b * diff)
        FE, FN = _integral(psi[i], a, b, diff)
        cE = (E[i + 1] - E[i]) - FE; cN = (N[i + 1] - N[i]) - FN
        cpos = max(cpos, math.sqrt((cE * cE) + (cN * cN)))
        cpsi = max(cpsi, abs(a - kap[i]) * diff)
        for c, name in enumerate(CHANNELS):
            out[name][o[i]] = ch[c, i]
        for k in range(1, m[i]):
            j = o[i] + k
            tau = (diff * float(k)) / float(m[i])
            lin = lambda x: x[i] + (((x[i + 1] - x[i]) * tau) / diff)
            out["s"][j] = s[i] + tau
            out["kappa"][j] = lin(kap); out["edge_L"][j] = lin(eL); out["edge_R"][j] = lin(eR)
            out["psi"][j] = _psi(psi[i], a, b, tau)
            IE, IN = _integral(psi[i], a, b, tau)
            fr = tau / diff
            out["E"][j] = E[i] + (IE + (fr * cE)); out["N"][j] = N[i] + (IN + (fr * cN))
            Wa = V[i] * V[i]
            W = Wa + ((((V[i + 1] * V[i + 1]) - Wa) * tau) / diff)
            Vj = math.sqrt(W)
            out["V"][j] = Vj; out["A"][j] = A[i]
            out["t"][j] = T[i] + (((T[i + 1] - T[i]) * ((2.0 * tau) / (V[i] + Vj))) / ((2.0 * diff) / (V[i] + V[i + 1])))
    for c, name in enumerate(CHANNELS):
        out[name][L_out - 1] = ch[c, nint]
    ds = [float(out["s"][j + 1]) - float(out["s"][j]) for j in range(L_out - 1)]
    out.update(m=m, o=o, stats=dict(length=s[nint] - s[0], ds_min=min(ds), ds_max=max(ds), closure_pos_max=cpos, closure_psi_max=cpsi,
                                    kappa_abs_max=float(np.max(np.abs(out["kappa"]))), n_added=L_out - L, m_max=max(m), reserved=0.0))
    return out


def channels(r, Lmax):
    """[10][Lmax] in the order of pg_set_trajectories, 0 at and past L_out"""
    out = np.zeros((10, Lmax))
    for c, name in enumerate(CHANNELS):
        out[c, :len(r[name])] = r[name]
    return out
