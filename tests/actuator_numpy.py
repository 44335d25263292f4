"""The yardstick of the actuator-set tests: the law of pg_set_actuator_sets (include/pigeon_mpc.h) in numpy, written from the header's statement, not from the device code.

Per instance and channel j of (delta, Fxf, Fxr), at step k with command c_k:
    g   = c_{k - delay}                                   (entries before the first step = c_0)
    y   = tau == 0 ? g : a_{k-1} + alpha (g - a_{k-1}),    alpha = -expm1(-dt / tau)
    a_k = rate == +Inf ? y : a_{k-1} + clamp(y - a_{k-1}, -rate dt, +rate dt),     a_{-1} = c_0
(tau, rate) = (tau_delta, rate_delta) for delta, (tau_fx, rate_fx) for Fxf and Fxr.  tau == 0 and rate == +Inf are copies.  The delayed command is taken from the command
array by its index, with no ring: a ring-index error of the device code shows as a difference.  dtype float32 rounds every operation to float, as the fp32 library does."""
import math

import numpy as np

FIELDS = ("delay_steps", "tau_delta", "tau_fx", "rate_delta", "rate_fx", "feedback")
MAX_DELAY = 16


def identity(**overrides):
    a = dict(delay_steps=0, tau_delta=0.0, tau_fx=0.0, rate_delta=math.inf, rate_fx=math.inf, feedback=0)
    for k, v in overrides.items():
        assert k in a, k
        a[k] = v
    return a


def six_sets():
    """The sets of the GPU tests: identity; delay 3; delay 16 (the cap); a lag on every channel; a slew limit with delay 1; delay 2 + steering lag + feedback."""
    return [identity(), identity(delay_steps=3), identity(delay_steps=MAX_DELAY), identity(tau_delta=0.05, tau_fx=0.05),
            identity(rate_delta=0.2, rate_fx=5e3, delay_steps=1), identity(delay_steps=2, tau_delta=0.1, feedback=1)]


def is_pure_delay(s):
    return s["tau_delta"] == 0 and s["tau_fx"] == 0 and math.isinf(s["rate_delta"]) and math.isinf(s["rate_fx"])


def actuator_response(sets, idx, commands, dt, dtype=np.float64, a_start=None, g_before=None):
    """commands [steps][B][3] -> applied [steps][B][3].  sets: list of dicts (FIELDS); idx [B] (None: set 0 for everyone).  a_start [B][3]: the position before the first
    step (default commands[0]); g_before [B][3]: the command before the first step (default commands[0])."""
    T = np.dtype(dtype).type
    c = np.asarray(commands, dtype=np.float64).astype(dtype)
    steps, B, _ = c.shape
    idx = np.zeros(B, dtype=int) if idx is None else np.asarray(idx, dtype=int)
    out = np.empty_like(c)
    first = c[0] if g_before is None else np.asarray(g_before).astype(dtype)
    start = c[0] if a_start is None else np.asarray(a_start).astype(dtype)
    dt = T(dt)
    for b in range(B):
        s = sets[idx[b]]
        d = int(s["delay_steps"])
        for j in range(3):
            tau = T(s["tau_delta"] if j == 0 else s["tau_fx"]); rate = T(s["rate_delta"] if j == 0 else s["rate_fx"])
            a = start[b, j]
            alpha = T(-np.expm1(-dt / tau)) if tau != 0 else None
            lim = None if np.isinf(rate) else T(rate * dt)
            for k in range(steps):
                g = c[k - d, b, j] if k - d >= 0 else first[b, j]
                y = g if alpha is None else T(a + T(alpha * T(g - a)))
                if lim is not None:
                    dlt = T(y - a)
                    y = T(a + (-lim if dlt < -lim else (lim if dlt > lim else dlt)))
                a = y
                out[k, b, j] = a
    return out.astype(np.float64)
