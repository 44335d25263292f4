"""Float64 twin of pg_clip_tubes, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, obstacle set) pair at a time, every operation
rounded on its own, in the order the header gives (a parenthesis of the header is one numpy operation here; numpy rounds every elementwise operation once and contracts
nothing).  The copied channels, every integer and every edge no obstacle touches are the library's bit for bit; a touched edge and the report's doubles carry sin and cos
of psi and are compared within `bar`, the bound the header states, evaluated here with this twin's own b and h.  The twin also returns how far every decision it took is
from a floating-point tie (`margin`), which tests/tube_clip_cases.py bounds from below."""
import math

import numpy as np

INF = math.inf
EPS8 = 8.0 * 2.0 ** -52
CENTRE, WIDER, LEFT, RIGHT = 0, 1, 2, 3
SET_DEFAULTS = dict(first=0, count=0, margin=0.0, taper=INF, min_width=0.0, policy=CENTRE, reserved=0)
REPORT_FIELDS = ("u_at", "a_at", "h_at", "dist_at", "free_left", "free_right", "k_at", "k_first", "k_last", "side")
STATS_INTS = ("n_clip_L", "n_clip_R", "n_blocked", "n_centre_out", "n_seen", "n_ignored")
CHANNELS = ("t", "s", "V", "A", "E", "N", "psi", "kappa", "edge_L", "edge_R")


def obstacle_set(**kw):
    s = dict(SET_DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = int(v) if k in ("first", "count", "policy", "reserved") else float(v)
    return s


def sight(E, N, psi, eL, eR, oE, oN, R):
    """Sight of the header over the knots given (arrays): a, b, q, h (0 where |b| >= R), sees"""
    cs = np.cos(psi); sn = np.sin(psi)
    wE = oE - E; wN = oN - N
    a = (wE * (-cs)) + (wN * (-sn))
    b = (wE * (-sn)) + (wN * cs)
    q = (wE * wE) + (wN * wN)
    inside = np.abs(b) < R
    h = np.zeros_like(a)
    h[inside] = np.sqrt((R * R) - (b[inside] * b[inside]))
    sees = inside & ((a - h) < eL) & ((a + h) > eR)
    return a, b, q, h, sees, wE, wN


def side_of(policy, a_at, free_left, free_right):
    centre = 1 if a_at > 0.0 else -1
    if policy == LEFT:
        return -1
    if policy == RIGHT:
        return 1
    if policy == WIDER:
        if free_right > free_left:
            return 1
        if free_left > free_right:
            return -1
    return centre


def clip(ch, S, obstacles, closed=False):
    """ch: the source's channels [10][L] float64; S: obstacle_set(...) whose first / count point into `obstacles`, a sequence of (E, N, radius).
    -> dict(the ten channels [L]; stats; report: one dict per obstacle of the set; bar_L, bar_R [L]: the header's bound on |edge' - twin| of a touched edge, 0 elsewhere;
    report_bar: the same bound per obstacle at k_at; margin: the smallest distance of a decision from a tie)"""
    ch = np.asarray(ch, dtype=np.float64)
    L = ch.shape[1]
    nk = L - 1 if closed else L
    s, E, N, psi, eL, eR = (np.array(ch[c, :nk]) for c in (1, 4, 5, 6, 8, 9))
    s0 = float(ch[1, 0])
    cL = eL.copy(); cR = eR.copy()
    kbarL = np.zeros(nk); kbarR = np.zeros(nk)                      # the bound of the clip that holds a knot's hard edge
    report, report_bar = [], []
    margin = INF
    for j in range(S["first"], S["first"] + S["count"]):
        oE, oN, rad = (float(v) for v in obstacles[j])
        R = rad + S["margin"]
        a, b, q, h, sees, wE, wN = sight(E, N, psi, eL, eR, oE, oN, R)
        order = np.argsort(q, kind="stable")
        k = int(order[0])                                           # (stable: the lowest index on ties)
        if nk > 1:
            margin = min(margin, float(q[order[1]] - q[k]))
        inside = np.abs(b) < R
        margin = min(margin, float(np.min(np.abs(np.abs(b) - R))))
        if inside.any():
            margin = min(margin, float(np.min(np.abs((a - h)[inside] - eL[inside]))), float(np.min(np.abs((a + h)[inside] - eR[inside]))))
        hb = np.where(inside, h, R)
        bar = EPS8 * (np.abs(wE) + np.abs(wN) + R) * (1.0 + np.abs(b) / hb)
        a_at = float(a[k]); h_at = float(h[k])
        free_right = (a_at - h_at) - float(eR[k]); free_left = float(eL[k]) - (a_at + h_at)
        seen = bool(sees.any())
        side = side_of(S["policy"], a_at, free_left, free_right) if seen else 0
        if seen and S["policy"] in (CENTRE, WIDER):
            margin = min(margin, abs(a_at) if S["policy"] == CENTRE else abs(free_right - free_left))
        idx = np.flatnonzero(sees)
        report.append(dict(u_at=float(s[k]) - s0, a_at=a_at, h_at=h_at, dist_at=math.sqrt(float(q[k])), free_left=free_left, free_right=free_right, k_at=k,
                           k_first=int(idx[0]) if seen else -1, k_last=int(idx[-1]) if seen else -1, side=side))
        report_bar.append(float(bar[k]))
        if side > 0:
            lo = a - h
            take = sees & (lo < cL)
            cL[take] = lo[take]; kbarL[take] = bar[take]
        elif side < 0:
            hi = a + h
            take = sees & (hi > cR)
            cR[take] = hi[take]; kbarR[take] = bar[take]
    outL = cL.copy(); outR = cR.copy()
    barL = np.where(cL < eL, kbarL, 0.0); barR = np.where(cR > eR, kbarR, 0.0)
    m = S["taper"]
    if m < INF:
        per = float(ch[1, L - 1]) - s0
        for k in np.flatnonzero(cL < eL):
            d = np.abs(s - s[k])
            if closed:
                d = np.minimum(d, per - d)
            outL = np.minimum(outL, cL[k] + (m * d))
        for k in np.flatnonzero(cR > eR):
            d = np.abs(s - s[k])
            if closed:
                d = np.minimum(d, per - d)
            outR = np.maximum(outR, cR[k] - (m * d))
        # |min_k x_k - min_k y_k| <= max_k |x_k - y_k|: a tapered edge carries the largest bound of the clips of its side
        if (cL < eL).any():
            barL = np.where(outL != eL, float(np.max(kbarL[cL < eL])), 0.0)
        if (cR > eR).any():
            barR = np.where(outR != eR, float(np.max(kbarR[cR > eR])), 0.0)
    width = outL - outR
    kw = int(np.argmin(width))                                      # (the first of the smallest)
    stats = dict(width_min=float(width[kw]), u_width_min=float(s[kw]) - s0, n_clip_L=int(np.count_nonzero(outL != eL)), n_clip_R=int(np.count_nonzero(outR != eR)),
                 n_blocked=int(np.count_nonzero(width < S["min_width"])), n_centre_out=int(np.count_nonzero(~((outR < 0.0) & (0.0 < outL)))),
                 n_seen=sum(1 for r in report if r["side"] != 0), n_ignored=sum(1 for r in report if r["side"] == 0))
    out = {name: np.array(ch[c]) for c, name in enumerate(CHANNELS)}
    out["edge_L"][:nk] = outL; out["edge_R"][:nk] = outR
    if closed:
        out["edge_L"][nk] = outL[0]; out["edge_R"][nk] = outR[0]
        barL = np.append(barL, barL[0]); barR = np.append(barR, barR[0])
    out.update(stats=stats, report=report, report_bar=report_bar, bar_L=barL, bar_R=barR, margin=margin)
    return out


def channels(r, Lmax):
    """[10][Lmax] in the order of pg_set_trajectories, 0 at and past L"""
    out = np.zeros((10, Lmax))
    for c, name in enumerate(CHANNELS):
        out[c, :len(r[name])] = r[name]
    return out
