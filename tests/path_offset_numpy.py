"""Float64 twin of pg_offset_paths, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, offset set) pair at a time, every operation
rounded on its own, in the order the header gives (a parenthesis of the header is one Python operation here).  t, s, V, A, kappa, both edges and every stat but closure_pos
are the library's bit for bit; psi carries atan2, E and N carry sin and cos.  The blocked prefix is pg_make_paths' (Prefix) as
path_fit_numpy.blocked_prefix states it from the header: path_make_numpy itself has no such function (its E and N are a serial np.cumsum, compared with the library
within a bound), so there is nothing of the kind to import from it."""
import math

import numpy as np

from path_fit_numpy import blocked_prefix
from path_make_numpy import GL_W, GL_X

INF = math.inf
SET_DEFAULTS = dict(d0=0.0, d1=0.0, s_a=INF, s_b=INF, s_c=INF, s_d=INF, x_min=0.1, edge_mode=0, reserved=0)


def offset_set(**kw):
    s = dict(SET_DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = int(v) if k in ("edge_mode", "reserved") else float(v)
    return s


def window(u, a, b):
    """(f, f', f'') of sigma over [a, b] at u"""
    if a == INF:
        return 0.0, 0.0, 0.0
    w = b - a
    tau = (u - a) / w
    if not tau > 0.0:
        return 0.0, 0.0, 0.0
    if tau >= 1.0:
        return 1.0, 0.0, 0.0
    z = tau * (1.0 - tau)
    f = ((tau * tau) * tau) * (10.0 + (tau * ((6.0 * tau) - 15.0)))
    f1 = (30.0 * (z * z)) / w
    f2 = ((60.0 * z) * (1.0 - (2.0 * tau))) / (w * w)
    return f, f1, f2


def offset_at(S, u):
    """(d, d', d'') at u = s - s_first"""
    r, r1, r2 = window(u, S["s_a"], S["s_b"])
    f, f1, f2 = window(u, S["s_c"], S["s_d"])
    dd = S["d1"] - S["d0"]
    return S["d0"] + (dd * (r - f)), dd * (r1 - f1), dd * (r2 - f2)


def offset(ch, S, closed=False):
    """ch: the source's channels [10][L] (t, s, V, A, E, N, psi, kappa, edge_L, edge_R), float64 -> dict(t, s, V, A, E, N, psi, kappa, edge_L, edge_R: float64 [L]; d, x:
    the offset and 1 - kappa d of the knots; stats: the fields of pg_offset_stats)"""
    ch = np.asarray(ch, dtype=np.float64)
    t_in, s, V, _, E, N, psi, kap, eL, eR = (ch[c] for c in range(10))
    L = len(s); nint = L - 1
    s0 = float(s[0])
    # Arclength
    extra = []
    for i in range(nint):
        sa = float(s[i]); sb = float(s[i + 1]); ka = float(kap[i]); kb = float(kap[i + 1])
        diff = sb - sa
        half = 0.5 * diff; mid = 0.5 * (sa + sb)
        acc = 0.0
        for xk, wk in zip(GL_X, GL_W):
            u = mid + (half * xk)
            kappa = ka + (((kb - ka) * (u - sa)) / diff)
            d, d1, _ = offset_at(S, u - s0)
            x = 1.0 - (kappa * d)
            g = math.sqrt((x * x) + (d1 * d1))
            acc = acc + (wk * (g - 1.0))
        extra.append(half * acc)
    X = blocked_prefix(extra)
    sp = [float(s[i]) + X[i] for i in range(L)]
    # Speed
    A = [0.0] * L; dt = []
    for i in range(nint):
        ds2 = 2.0 * (sp[i + 1] - sp[i])
        va = float(V[i]); vb = float(V[i + 1])
        A[i] = ((vb * vb) - (va * va)) / ds2
        dt.append(ds2 / (va + vb))
    A[nint] = A[0] if closed else 0.0
    T = blocked_prefix(dt)
    t0 = float(t_in[0])
    t = [t0] + [t0 + T[i] for i in range(1, L)]
    # Frame, edges
    out = {k: np.zeros(L) for k in ("E", "N", "psi", "kappa", "edge_L", "edge_R", "d", "x")}
    for i in range(L):
        d, d1, d2 = offset_at(S, float(s[i]) - s0)
        k = float(kap[i])
        if closed and i in (0, nint):
            ks = (float(kap[1]) - float(kap[nint - 1])) / ((float(s[1]) - float(s[0])) + (float(s[nint]) - float(s[nint - 1])))
        else:
            ia = max(i - 1, 0); ib = min(i + 1, nint)
            ks = (float(kap[ib]) - float(kap[ia])) / (float(s[ib]) - float(s[ia]))
        x = 1.0 - (k * d); y = d1
        g2 = (x * x) + (y * y)
        g = math.sqrt(g2)
        p = float(psi[i])
        out["E"][i] = float(E[i]) - (d * math.cos(p)); out["N"][i] = float(N[i]) - (d * math.sin(p))
        out["psi"][i] = p + math.atan2(y, x)
        out["kappa"][i] = (k + (((x * d2) + (y * ((ks * d) + (k * d1)))) / g2)) / g
        if S["edge_mode"] == 0:
            out["edge_L"][i] = float(eL[i]) - d; out["edge_R"][i] = float(eR[i]) - d
        else:
            out["edge_L"][i] = float(eL[i]); out["edge_R"][i] = float(eR[i])
        out["d"][i] = d; out["x"][i] = x
    out.update(t=np.array(t), s=np.array(sp), V=np.array(V, dtype=np.float64), A=np.array(A))
    ds = [sp[i + 1] - sp[i] for i in range(nint)]
    dE = out["E"][-1] - out["E"][0]; dN = out["N"][-1] - out["N"][0]
    out["stats"] = dict(length=sp[nint] - sp[0], ds_min=min(ds), ds_max=max(ds), kappa_abs_max=float(np.max(np.abs(out["kappa"]))), x_min=float(np.min(out["x"])),
                        d_abs_max=float(np.max(np.abs(out["d"]))), closure_pos=math.sqrt((dE * dE) + (dN * dN)),
                        n_outside=int(np.count_nonzero(~((out["edge_R"] < 0.0) & (0.0 < out["edge_L"])))), reserved=0)
    return out


CHANNELS = ("t", "s", "V", "A", "E", "N", "psi", "kappa", "edge_L", "edge_R")


def channels(r, Lmax):
    """[10][Lmax] in the order of pg_set_trajectories, 0 at and past L"""
    out = np.zeros((10, Lmax))
    for c, name in enumerate(CHANNELS):
        out[c, :len(r[name])] = r[name]
    return out
