"""float64 numpy twin of pg_make_starts (include/pigeon_mpc.h states the scheme; pigeon.jl_amd/csrc/pg_start_make.hip is the kernel): the draws, the arclength, the
controller's lookup with its t(s), the placement, the body state and control, the other car, the store.  Test infrastructure: the yardstick of
tests/test_gpu_start_make.py, pinned by tests/test_start_make_host.py to spec_numpy.Trajectory and to the block / word assignment spelled out by hand.  Every operation is
written out in the order the scheme states it and rounded once (numpy contracts nothing).  Philox comes from tests/sensor_numpy.py; steady_state_estimates and
longitudinal_tire_forces from oracle/spec_numpy.py.  single = np.float32 reads the channels and the vehicle as the fp32 library holds them and rounds the store to float."""
import math

import numpy as np

import sensor_numpy
from oracle import spec_numpy as spec

RANGES = ("s", "e", "dpsi", "v", "uy", "dr", "delta", "fx", "dt0", "other_dx", "other_dy", "other_dpsi", "other_v")
MODES = ("s_mode", "e_mode", "steady", "time_mode", "other_mode")
BLOCK0 = 4                                                         # blocks 0-3 belong to the sensor, the disturbance and the human


def start(**kw):
    """a start set as a dict of the structure's fields; a range as one value or a pair (the mirror of vehicles.start, written independently)"""
    p = {}
    for n in RANGES:
        p[n + "_lo"] = p[n + "_hi"] = 1.0 if n == "v" else 0.0
    for m in MODES:
        p[m] = 0
    for k, v in kw.items():
        if k in RANGES:
            lo, hi = v if isinstance(v, (tuple, list)) else (v, v)
            p[k + "_lo"], p[k + "_hi"] = float(lo), float(hi)
        else:
            assert k in p, k
            p[k] = v
    return p


def uniforms(seed, streams):
    """u [B][13]: channel c = word c % 4 of block BLOCK0 + c / 4, key (seed_lo, seed_hi), counter (0, block, stream_lo, stream_hi); u = (x + 0.5) 2^-32"""
    seed = int(seed)
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    u = np.zeros((len(streams), len(RANGES)))
    for blk in range((len(RANGES) + 3) // 4):
        ctr = np.zeros((len(streams), 4), dtype=np.uint64)
        ctr[:, 1] = BLOCK0 + blk
        ctr[:, 2] = streams & sensor_numpy.MASK
        ctr[:, 3] = streams >> sensor_numpy.S32
        x = sensor_numpy.philox4x32_10(ctr, key)
        for k in range(4):
            c = 4 * blk + k
            if c < len(RANGES):
                u[:, c] = (x[:, k].astype(np.float64) + 0.5) * 2.0 ** -32
    return u


def draws(sets, index, seed, streams):
    """value [B][13] = lo + u (hi - lo) under set index[b]"""
    u = uniforms(seed, streams)
    lo = np.array([[sets[i][n + "_lo"] for n in RANGES] for i in index], dtype=np.float64)
    hi = np.array([[sets[i][n + "_hi"] for n in RANGES] for i in index], dtype=np.float64)
    return lo + u * (hi - lo)


def held(tube, single=np.float64):
    """the ten channels the library holds of a tube (pigeon_jl_amd TrajectoryTube or anything with .data [12][L]), rounded to its element type, as float64"""
    d = np.asarray(tube.data, dtype=np.float64)[[0, 1, 2, 3, 4, 5, 6, 7, 10, 11]]
    return dict(zip(("t", "s", "V", "A", "E", "N", "psi", "kappa", "edge_L", "edge_R"), d.astype(single).astype(np.float64)))


def lookup(ch, sq):
    """traj[s] (trajectories.jl:55-68) with t(s), the square root as the reference writes it (:63), and interp_by_s (:32-35) of psi, kappa, E, N, the edges"""
    s, V, t = ch["s"], ch["V"], ch["t"]
    L = len(s)
    sq = np.float64(sq)
    i = min(max(int(np.searchsorted(s, sq, side="left")), 1), L - 1) - 1            # count of knots < s
    A = (V[i + 1] - V[i]) / (t[i + 1] - t[i])
    ds = sq - s[i]
    if abs(A) < 1e-3 or sq > s[L - 1]:
        dt = ds / V[i]; branch = "linear"
    else:
        dt = (np.sqrt(2.0 * A * ds + V[i] * V[i]) - V[i]) / A; branch = "sqrt"
    j = min(max(int(np.searchsorted(s, sq, side="right")), 1), L - 1) - 1           # count of knots <= s
    w = (sq - s[j]) / (s[j + 1] - s[j])
    lin = lambda c: c[j] + w * (c[j + 1] - c[j])
    return dict(V=V[i] + A * dt, A=A, t=t[i] + dt, psi=lin(ch["psi"]), kappa=lin(ch["kappa"]), E=lin(ch["E"]), N=lin(ch["N"]), edge_L=lin(ch["edge_L"]),
                edge_R=lin(ch["edge_R"]), i=i, j=j, branch=branch)


def make(tubes, tube_index, sets, index, seed, streams, vehicle, single=np.float64):
    """the twin of pg_make_starts: tubes = the installed library, tube_index [B], sets = start() dicts, index [B], streams [B], vehicle = the handle's.
    Returns the arrays the call returns (state, control, t0, other, time_offset, placed) and, for the tests, look [B] (the lookups) and steady [B] (bool)."""
    B = len(index)
    val = draws(sets, index, seed, streams)
    P = {k: float(single(v)) for k, v in vehicle.items()}
    chans = [held(t, single) for t in tubes]
    out = dict(state=np.zeros((B, 6)), control=np.zeros((B, 3)), t0=np.zeros(B), other=np.zeros((B, 4)), time_offset=np.zeros(B), placed=np.zeros((B, 4)),
               look=[], steady=np.zeros(B, dtype=bool))
    C = dict(zip(RANGES, range(len(RANGES))))
    for b in range(B):
        S, ch, v = sets[index[b]], chans[tube_index[b]], val[b]
        s_first, s_last = ch["s"][0], ch["s"][-1]
        s = s_first + v[C["s"]] * (s_last - s_first) if S["s_mode"] else s_first + v[C["s"]]
        s = s_first if s < s_first else (s_last if s > s_last else s)
        K = lookup(ch, s)
        e = v[C["e"]]
        if S["e_mode"]:
            mid = 0.5 * (K["edge_L"] + K["edge_R"]); half = 0.5 * (K["edge_L"] - K["edge_R"])
            e = mid + v[C["e"]] * half
        sp, cp = math.sin(K["psi"]), math.cos(K["psi"])
        E = K["E"] - e * cp; N = K["N"] - e * sp; psi = K["psi"] + v[C["dpsi"]]
        vV = v[C["v"]] * K["V"]
        Ux, Uy, r, delta, Fx = vV, 0.0, K["kappa"] * vV, 0.0, 0.0
        if S["steady"]:
            Vr, kr = float(single(vV)), float(single(K["kappa"]))
            est = spec.steady_state_estimates(P, Vr, float(single(K["A"])), kr)      # the reference's defaults: 4 iterations, r = V kappa, the other estimates 0
            Ux, Uy, r, delta, Fx = est["Ux"], est["Uy"], est["r"], est["delta"], est["Fxf"] + est["Fxr"]
            out["steady"][b] = True
        Uy = Uy + v[C["uy"]]; r = r + v[C["dr"]]; delta = delta + v[C["delta"]]; Fx = Fx + v[C["fx"]]
        Fxf, Fxr = spec.longitudinal_tire_forces(P, Fx)
        oth = np.zeros(4)
        if S["other_mode"]:
            so, co = math.sin(psi), math.cos(psi)
            dx, dy = v[C["other_dx"]], v[C["other_dy"]]
            oth[:] = [E + dx * (-so) + dy * (-co), N + dx * co + dy * (-so), psi + v[C["other_dpsi"]], v[C["other_v"]]]
        out["state"][b] = np.array([E, N, psi, Ux, Uy, r]).astype(single)
        out["control"][b] = np.array([delta, Fxf, Fxr]).astype(single)
        out["other"][b] = oth.astype(single)
        out["t0"][b] = K["t"] + v[C["dt0"]]
        out["time_offset"][b] = math.nan if S["time_mode"] else 0.0
        out["placed"][b] = [s, e, v[C["dpsi"]], K["V"]]
        out["look"].append(K)
    return out
