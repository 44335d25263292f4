"""numpy twin of the sensor library's draws (include/pigeon_mpc.h, pg_set_sensor_sets): Philox4x32-10 in the Random123 definition, vectorised over uint64 arithmetic, and
the Box-Muller construction the device uses, in double.  Test infrastructure: the yardstick of tests/test_gpu_sensor_sets.py, pinned by tests/test_sensor_host.py to the
known-answer vectors of the generator and to the block / word assignment spelled out by hand."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
Z_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))           # 5.887: u1 >= 2^-25 truncates the tails there


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (32-bit words, any integer dtype; broadcast against each other) -> the four output words [..., 4] as uint64 holding 32-bit values"""
    c = np.asarray(counter).astype(np.uint64) & MASK
    k = np.asarray(key).astype(np.uint64) & MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0 = M0 * c0; p1 = M1 * c2                          # 32 x 32 -> 64: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + W0) & MASK; k1 = (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def box_muller(xa, xb):
    """two 32-bit words -> two standard normals: u = ((x >> 8) + 0.5) 2^-24, rho = sqrt(-2 ln u1), (rho cos 2 pi u2, rho sin 2 pi u2)"""
    u1 = ((np.asarray(xa).astype(np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((np.asarray(xb).astype(np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    return rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)


def words(seed, streams, step0, steps):
    """the two Philox blocks of every (step, stream): ([steps][B][4], [steps][B][4])"""
    seed = int(seed)
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1)
    B = len(streams)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    ctr = np.zeros((steps, B, 4), dtype=np.uint64)
    ctr[..., 0] = (np.arange(step0, step0 + steps, dtype=np.uint64) & MASK)[:, None]
    ctr[..., 2] = (streams & MASK)[None, :]
    ctr[..., 3] = (streams >> S32)[None, :]
    x0 = philox4x32_10(ctr, key)
    ctr[..., 1] = 1
    return x0, philox4x32_10(ctr, key)


def draws(seed, streams, step0, steps):
    """z [steps][B][6] for the channels (E, N, psi, Ux, Uy, r): block 0 -> (E, N) from (x0, x1) and (psi, Ux) from (x2, x3); block 1 -> (Uy, r) from its (x0, x1)"""
    x0, x1 = words(seed, streams, step0, steps)
    z = np.zeros(x0.shape[:2] + (6,))
    z[..., 0], z[..., 1] = box_muller(x0[..., 0], x0[..., 1])
    z[..., 2], z[..., 3] = box_muller(x0[..., 2], x0[..., 3])
    z[..., 4], z[..., 5] = box_muller(x1[..., 0], x1[..., 1])
    return z


def four_sensors():
    """the test sensors, spread over the instances by b % 4: exact; noisy; biased (+0.2 m on E, -0.05 m/s on Ux); three times as noisy.  [(sigma [6], bias [6])]"""
    sg = np.array([0.05, 0.05, 0.005, 0.1, 0.05, 0.01])
    zero = np.zeros(6)
    return [(zero, zero), (sg, zero), (zero, np.array([0.2, 0.0, 0.0, -0.05, 0.0, 0.0])), (3.0 * sg, zero)]


def measured(sets, idx, true_hist, z):
    """true + bias + sigma z for a history [steps][B][6] under the sets [(sigma, bias)] selected by idx [B]"""
    sg = np.stack([np.asarray(sets[i][0], dtype=np.float64) for i in idx]); bs = np.stack([np.asarray(sets[i][1], dtype=np.float64) for i in idx])
    return true_hist + bs[None] + sg[None] * z
