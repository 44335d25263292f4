"""The yardstick of the human-set tests: the law of pg_set_human_sets (include/pigeon_mpc.h) in numpy, written from the header's statement, not from the device code.

Per instance at clock step k, with the library's own seed as the Philox key and the instance's 64-bit stream id:
    not active (k < step_on, or step_off >= 0 and k >= step_off)       u_k = (0, 0)
    active and deciding ((k - step_on) % hold_steps == 0, or the first step of the sequence)
        raw = (0, 0) | optimal_disturbance(x7_k, gradV_k) (safety_numpy; (0, 0) without a grid) | script_k | (sigma_w n_w, sigma_a n_a)      for mode 0 | 1 | 2 | 3
        u_k[c] = gain[c] raw[c] (gain 1: raw itself), then omega limited to [-omega_max, omega_max] and a to [a_min, a_max] by compare-and-select
    active and not deciding                                            u_k = u_{k-1}
n is the gust's AR(1) (disturbance_numpy.gust_states: n_k = z_k at the first step or for tau == 0, else rho n_{k-1} + sqrt(-expm1(-2 dt / tau)) z_k) on
z = Box-Muller of words (x0, x1) of Philox4x32-10 block 3, counter (k, 3, stream_lo, stream_hi); it advances at every step.
Everything in double: the fp32 library is held against it at the fp32 bars."""
import numpy as np

import disturbance_numpy
from safety_numpy import optimal_disturbance
from sensor_numpy import philox4x32_10, box_muller, MASK, S32

FIELDS = ("mode", "hold_steps", "step_on", "step_off", "gain", "omega_max", "a_min", "a_max", "sigma", "tau")
HOLD, WORST, SCRIPT, RANDOM = 0, 1, 2, 3
# how a value came about (response(..., explain=True)): a copy or an exact constant (0, the script, a limit) | arithmetic on optimal_disturbance | arithmetic on the draws
EXACT, FROM_WORST, FROM_RANDOM = 0, 1, 3


def identity(mode=0, **overrides):
    d = dict(mode=mode, hold_steps=1, step_on=0, step_off=-1, gain=[1.0, 1.0], omega_max=np.inf, a_min=-np.inf, a_max=np.inf, sigma=[0.0, 0.0], tau=0.0)
    for k, v in overrides.items():
        assert k in d, k
        d[k] = v
    return d


def four_humans():
    """The sets of the GPU tests, spread over the instances by b % 4: hold; the worst case at half authority, re-decided every 3 steps inside the window [2, 11), with
    finite limits; the caller's script at gain 1 inside the window [3, 9) with a limit on a; a coloured random driver with limits that bite now and then."""
    return [identity(HOLD),
            identity(WORST, hold_steps=3, step_on=2, step_off=11, gain=[0.5, 0.5], omega_max=0.15, a_min=-2.0, a_max=1.5),
            identity(SCRIPT, step_on=3, step_off=9, a_min=-0.5, a_max=0.5),
            identity(RANDOM, hold_steps=2, sigma=[0.2, 1.5], tau=0.05, omega_max=0.3, a_min=-2.0, a_max=2.0)]


def block3_words(seed, streams, step0, steps):
    """the four words of Philox block 3 of every (step, stream): [steps][B][4]"""
    seed = int(seed)
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    ctr = np.zeros((steps, len(streams), 4), dtype=np.uint64)
    ctr[..., 0] = (np.arange(step0, step0 + steps, dtype=np.uint64) & MASK)[:, None]
    ctr[..., 1] = 3
    ctr[..., 2] = (streams & MASK)[None, :]
    ctr[..., 3] = (streams >> S32)[None, :]
    return philox4x32_10(ctr, key)


def normals(seed, streams, step0, steps):
    """z [steps][B][2] = (z_w, z_a)"""
    x = block3_words(seed, streams, step0, steps)
    zw, za = box_muller(x[..., 0], x[..., 1])
    return np.stack([zw, za], axis=-1)


def ar_states(sets, idx, seed, streams, step0, steps, dt):
    """n [steps][B][2] from a fresh state at step0: the AR(1) helper of the gust (disturbance_numpy.gust_states) on block 3 in place of block 2"""
    keep = disturbance_numpy.normals
    disturbance_numpy.normals = normals
    try:
        return disturbance_numpy.gust_states([{"tau_gust": s["tau"]} for s in sets], idx, seed, streams, step0, steps, dt)
    finally:
        disturbance_numpy.normals = keep


def response(X, sets, idx, seed, streams, step0, steps, dt, x7=None, vg8=None, script=None, has_hji=True, explain=False):
    """u [steps][B][2] = (omega, a) of the clock steps [step0, step0 + steps), from a fresh state at step0.  sets: list of dicts (FIELDS); idx [B] (None: set 0 for
    everyone); streams [B]; x7 [steps][B][7], vg8 [steps][B][8] = (V, gradV) (read by mode 1 with has_hji), script [steps][B][2] (read by mode 2).  explain=True:
    (u, how [steps][B][2] in (EXACT, FROM_WORST, FROM_RANDOM), decided [steps][B]: the step whose decision u_k is, -1 when not active)."""
    streams = np.asarray(streams).reshape(-1)
    B = len(streams)
    idx = np.zeros(B, dtype=int) if idx is None else np.asarray(idx, dtype=int)
    n = ar_states(sets, idx, seed, streams, step0, steps, dt)
    ivec = lambda f: np.array([int(sets[i][f]) for i in idx])
    col = lambda f: np.array([float(sets[i][f]) for i in idx])
    pair = lambda f: np.array([[float(v) for v in sets[i][f]] for i in idx])
    mode, hold, on, off = ivec("mode"), ivec("hold_steps"), ivec("step_on"), ivec("step_off")
    gain, sigma = pair("gain"), pair("sigma")
    lo = np.stack([-col("omega_max"), col("a_min")], axis=1); hi = np.stack([col("omega_max"), col("a_max")], axis=1)
    u = np.zeros((steps, B, 2)); how = np.full((steps, B, 2), EXACT); decided = np.full((steps, B), -1)
    for j in range(steps):
        k = step0 + j
        active = (k >= on) & ((off < 0) | (k < off))
        deciding = active & (((k - on) % hold == 0) | (j == 0))
        raw = np.zeros((B, 2)); h = np.full((B, 2), EXACT)
        if np.any(mode == WORST) and has_hji:
            w = optimal_disturbance(X, x7[j], vg8[j][:, 1:])
            raw[mode == WORST] = w[mode == WORST]
            h[mode == WORST] = np.where(w[mode == WORST] == 0.0, EXACT, FROM_WORST)          # ((0, 0): no grid value, a speed <= 0 or a flat gradient -- constants)
        if np.any(mode == SCRIPT):
            raw[mode == SCRIPT] = script[j][mode == SCRIPT]
        r = mode == RANDOM
        raw[r] = np.where(sigma[r] == 0.0, 0.0, sigma[r] * n[j][r])
        h[r] = np.where(sigma[r] == 0.0, EXACT, FROM_RANDOM)
        v = np.where(gain == 1.0, raw, gain * raw)
        h = np.where((gain == 1.0) | (raw == 0.0), h, np.where(h == EXACT, FROM_WORST, h))     # (a scaled script value is arithmetic too: held at the tighter bar)
        over, under = v > hi, v < lo
        v = np.where(over, hi, v); v = np.where(under, lo, v)
        h = np.where(over | under, EXACT, h)
        if j > 0:
            u[j] = u[j - 1]; how[j] = how[j - 1]; decided[j] = decided[j - 1]
        u[j][deciding] = v[deciding]; how[j][deciding] = h[deciding]; decided[j][deciding] = k
        u[j][~active] = 0.0; how[j][~active] = EXACT; decided[j][~active] = -1
    return (u, how, decided) if explain else u
