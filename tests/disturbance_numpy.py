"""The yardstick of the disturbance-set tests: the law of pg_set_disturbance_sets (include/pigeon_mpc.h) and the disturbed plant in numpy, written from the header's
statement, not from the device code.

Per instance at clock step k, with the library's seed as the Philox key and the instance's 64-bit stream id:
    (z_x, z_y) = Box-Muller of words (x0, x1) of Philox4x32-10 block 2, counter (k, 2, stream_lo, stream_hi)
    n_k        = z_k                                                          at the first step of the sequence, or when tau_gust == 0
               = rho n_{k-1} + sqrt(-expm1(-2 dt / tau_gust)) z_k,  rho = exp(-dt / tau_gust)     otherwise
    w_k        = (0, 0, 0, 1) outside the window step_on <= k and (step_off < 0 or k < step_off)
               = (Fx + sigma_Fx n_x, Fy + g_y, Mz + x_cp g_y, mu_scale),  g_y = sigma_Fy n_y       inside it (a sigma of 0: the constant itself)
The plant of the step is plant_numpy's RK4 with P["mu"] * wmu in the tire model and wFx / m, wFy / m, wMz / Izz added to (dUx, dUy, dr) in every sub-step.
Everything in double: the fp32 library is held against it at the fp32 bars."""
import numpy as np

import plant_numpy
from sensor_numpy import philox4x32_10, box_muller, MASK, S32

FIELDS = ("step_on", "step_off", "Fx", "Fy", "Mz", "sigma_Fx", "sigma_Fy", "x_cp", "tau_gust", "mu_scale")
IDENTITY_W = np.array([0.0, 0.0, 0.0, 1.0])


def identity(**overrides):
    d = dict(step_on=0, step_off=-1, Fx=0.0, Fy=0.0, Mz=0.0, sigma_Fx=0.0, sigma_Fy=0.0, x_cp=0.0, tau_gust=0.0, mu_scale=1.0)
    for k, v in overrides.items():
        assert k in d, k
        d[k] = v
    return d


def four_disturbances():
    """The sets of the GPU tests, spread over the instances by b % 4: the identity; a side gust in the window [3, 9); a friction window from step 2 on; a headwind with a
    white gust."""
    return [identity(),
            identity(Fy=2000.0, x_cp=1.0, sigma_Fy=800.0, tau_gust=0.3, step_on=3, step_off=9),
            identity(mu_scale=0.55, step_on=2, step_off=-1),
            identity(Fx=-1000.0, sigma_Fx=500.0, tau_gust=0.0)]


def block2_words(seed, streams, step0, steps):
    """the four words of Philox block 2 of every (step, stream): [steps][B][4]"""
    seed = int(seed)
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    ctr = np.zeros((steps, len(streams), 4), dtype=np.uint64)
    ctr[..., 0] = (np.arange(step0, step0 + steps, dtype=np.uint64) & MASK)[:, None]
    ctr[..., 1] = 2
    ctr[..., 2] = (streams & MASK)[None, :]
    ctr[..., 3] = (streams >> S32)[None, :]
    return philox4x32_10(ctr, key)


def normals(seed, streams, step0, steps):
    """z [steps][B][2] = (z_x, z_y)"""
    x = block2_words(seed, streams, step0, steps)
    zx, zy = box_muller(x[..., 0], x[..., 1])
    return np.stack([zx, zy], axis=-1)


def gust_states(sets, idx, seed, streams, step0, steps, dt):
    """n [steps][B][2], from a fresh state at step0"""
    z = normals(seed, streams, step0, steps)
    B = z.shape[1]
    idx = np.zeros(B, dtype=int) if idx is None else np.asarray(idx, dtype=int)
    tau = np.array([float(sets[i]["tau_gust"]) for i in idx])
    white = tau == 0.0
    safe = np.where(white, 1.0, tau)
    rho = np.exp(-dt / safe)
    g = np.sqrt(-np.expm1(-2.0 * dt / safe))
    n = np.empty_like(z)
    n[0] = z[0]
    for k in range(1, steps):
        n[k] = np.where(white[:, None], z[k], rho[:, None] * n[k - 1] + g[:, None] * z[k])
    return n


def response(sets, idx, seed, streams, step0, steps, dt):
    """w [steps][B][4] = (wFx, wFy, wMz, wmu) of the clock steps [step0, step0 + steps).  sets: list of dicts (FIELDS); idx [B] (None: set 0 for everyone); streams [B]."""
    n = gust_states(sets, idx, seed, streams, step0, steps, dt)
    B = n.shape[1]
    idx = np.zeros(B, dtype=int) if idx is None else np.asarray(idx, dtype=int)
    col = lambda f: np.array([float(sets[i][f]) for i in idx])
    on = np.array([int(sets[i]["step_on"]) for i in idx]); off = np.array([int(sets[i]["step_off"]) for i in idx])
    k = np.arange(step0, step0 + steps)[:, None]
    active = (k >= on[None, :]) & ((off[None, :] < 0) | (k < off[None, :]))
    sx, sy = col("sigma_Fx"), col("sigma_Fy")
    gx = np.where(sx[None, :] == 0.0, 0.0, sx[None, :] * n[..., 0])
    gy = np.where(sy[None, :] == 0.0, 0.0, sy[None, :] * n[..., 1])
    w = np.empty((steps, B, 4))
    w[..., 0] = np.where(active, col("Fx")[None, :] + gx, 0.0)
    w[..., 1] = np.where(active, col("Fy")[None, :] + gy, 0.0)
    w[..., 2] = np.where(active, col("Mz")[None, :] + col("x_cp")[None, :] * gy, 0.0)
    w[..., 3] = np.where(active, col("mu_scale")[None, :], 1.0)
    return w


def plant_step_vec_dist(P, q, u3, w, dt, nsub=10):
    """plant_numpy.plant_step_vec with the disturbance w [B][4] held for the step: world_vehicle_model_vec on a vehicle whose mu is P["mu"] * wmu, plus
    (wFx / m, wFy / m, wMz / Izz) on (dUx, dUy, dr), inside the same RK4."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 6); u3 = np.asarray(u3, dtype=np.float64).reshape(-1, 3); w = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    Pv = P if isinstance(P, dict) and np.ndim(P["m"]) == 1 else plant_numpy.stack_vehicles(P, q.shape[0])
    Pw = dict(Pv, mu=Pv["mu"] * w[:, 3])
    u2 = np.stack([u3[:, 0], u3[:, 1] + u3[:, 2]], axis=1)
    add = np.zeros_like(q)
    add[:, 3] = w[:, 0] / Pv["m"]; add[:, 4] = w[:, 1] / Pv["m"]; add[:, 5] = w[:, 2] / Pv["Izz"]
    f = lambda x: plant_numpy.world_vehicle_model_vec(Pw, x, u2) + add
    x = q.copy(); h = dt / nsub
    for _ in range(nsub):
        k1 = f(x); k2 = f(x + k1 * (h * 0.5)); k3 = f(x + k2 * (h * 0.5)); k4 = f(x + k3 * h)
        x = x + (k1 + 2.0 * k2 + 2.0 * k3 + k4) * (h / 6.0)
    return x
