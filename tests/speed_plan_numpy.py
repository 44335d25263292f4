"""Float64 numpy twin of pg_plan_speeds, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, set) at a time, every operation rounded on
its own, in the order the header gives.  plan() returns the intermediate arrays too (cap, the backward pass's W, the limiter of every knot), so the host tests can assert
the invariants that hold by construction."""
import math

import numpy as np

CAP, ACCEL, BRAKE = 0, 1, 2
SPEED_PLAN_DEFAULTS = dict(mu_scale=1.0, V_max=30.0, V_floor=1.0, V_start=math.nan, V_end=math.nan, ax_max=math.inf, ax_min=-math.inf, ay_max=math.inf)


def speed_plan(**kw):
    p = dict(SPEED_PLAN_DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = float(v)
    return p


class Limits:
    """the per-set constants and the three limit functions of the scheme"""

    def __init__(self, sp, veh):
        f = np.float64
        self.a_lim = f(sp["mu_scale"]) * f(veh["mu"]) * f(veh["G"])
        self.ay = min(self.a_lim, f(sp["ay_max"]))
        self.Wmax = f(sp["V_max"]) * f(sp["V_max"])
        self.Wfloor = f(sp["V_floor"]) * f(sp["V_floor"])
        self.ax_max, self.nax_min = f(sp["ax_max"]), -f(sp["ax_min"])
        self.m, self.Fx_max, self.nFx_min, self.Px_max = f(veh["m"]), f(veh["Fx_max"]), -f(veh["Fx_min"]), f(veh["Px_max"])
        self.Cd0, self.Cd1, self.Cd2 = f(veh["Cd0"]), f(veh["Cd1"]), f(veh["Cd2"])
        end = lambda v: math.nan if math.isnan(v) else max(f(v), f(sp["V_floor"])) * max(f(v), f(sp["V_floor"]))
        self.Wstart, self.Wend = end(sp["V_start"]), end(sp["V_end"])

    def cap(self, kappa):
        ak = abs(kappa)
        c = min(self.Wmax, self.ay / ak) if ak > 0.0 else self.Wmax
        return max(self.Wfloor, c)

    def _along_drag(self, W, kappa):
        V = np.sqrt(W)
        lat = W * kappa
        along = np.sqrt(max(self.a_lim * self.a_lim - lat * lat, 0.0))
        Fd = self.Cd0 + V * (self.Cd1 + self.Cd2 * V)
        return V, along, Fd

    def acc(self, W, kappa):
        V, along, Fd = self._along_drag(W, kappa)
        F = min(min(self.m * along, self.Fx_max), self.Px_max / V)
        return min((F - Fd) / self.m, self.ax_max)

    def dec(self, W, kappa):
        V, along, Fd = self._along_drag(W, kappa)
        F = min(self.m * along, self.nFx_min)
        return max(min((F + Fd) / self.m, self.nax_min), 0.0)


def first_largest_curvature(kappa, L):
    """i0 of a closed path: the first knot of largest |kappa| among knots 0 .. L-2"""
    return int(np.argmax(np.abs(np.asarray(kappa[:L - 1], dtype=np.float64))))


def plan(s, kappa, sp, veh, closed=False):
    s = np.asarray(s, dtype=np.float64); kappa = np.asarray(kappa, dtype=np.float64)
    L = len(s); n = L - 1
    lim = Limits(sp, veh)
    ds = np.diff(s)                                             # ds[i] = s[i+1] - s[i]; ds[L-2] is the wrap interval of a closed path
    cap = np.array([lim.cap(k) for k in kappa])
    init = cap.copy()
    if closed:
        init[n] = cap[0]
        i0 = first_largest_curvature(kappa, L)
    else:
        i0 = 0
        if not math.isnan(lim.Wstart):
            init[0] = min(cap[0], lim.Wstart)
        if not math.isnan(lim.Wend):
            init[n] = min(cap[n], lim.Wend)
    W = init.copy()
    limiter = np.full(L, CAP, dtype=np.int32)
    # backward pass: open L-2 .. 0; closed i0-1, i0-2, ... once around modulo n, knot i0 itself is never revisited
    order = [(i0 - j) % n for j in range(1, n)] if closed else list(range(n - 1, -1, -1))
    for i in order:
        nx = (i + 1) % n if closed else i + 1
        cand = W[nx] + 2.0 * ds[i] * lim.dec(W[nx], kappa[nx])
        if cand < W[i]:
            W[i] = cand; limiter[i] = BRAKE
    Wb = W.copy()
    # forward pass: open 0 .. L-2; closed from i0 once around, the step that arrives at i0 again leaves it alone
    order = [(i0 + j) % n for j in range(n - 1)] if closed else list(range(n))
    fwd_cand = np.full(L, np.inf)
    for i in order:
        nx = (i + 1) % n if closed else i + 1
        cand = max(W[i] + 2.0 * ds[i] * lim.acc(W[i], kappa[i]), lim.Wfloor)
        fwd_cand[nx] = cand
        if cand < W[nx]:
            W[nx] = cand; limiter[nx] = ACCEL
    if closed:
        W[n] = W[0]; Wb[n] = Wb[0]; limiter[n] = limiter[0]; fwd_cand[n] = fwd_cand[0]
    V = np.sqrt(W)
    A = np.zeros(L)
    A[:n] = (W[1:] - W[:n]) / (2.0 * ds)
    A[n] = A[0] if closed else 0.0
    t = np.concatenate([[0.0], np.cumsum(2.0 * ds / (V[:-1] + V[1:]))])
    lat = W * kappa
    usage = np.sqrt(A * A + lat * lat) / lim.a_lim
    stats = dict(t_end=float(t[-1]), v_min=float(V.min()), v_max=float(V.max()), usage_max=float(usage.max()),
                 n_cap=int((limiter == CAP).sum()), n_accel=int((limiter == ACCEL).sum()), n_brake=int((limiter == BRAKE).sum()))
    return dict(W=W, V=V, A=A, t=t, cap=cap, init=init, Wb=Wb, fwd_cand=fwd_cand, limiter=limiter, i0=i0, stats=stats, lim=lim, ds=ds)
