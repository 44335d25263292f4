"""The start maker without a device: the ctypes mirror of pg_start_set against the header text, the defaults, the refusals of pack_starts, and the numpy twin
(tests/start_make_numpy.py) against spec_numpy.Trajectory, against its own inverse and against the block / word assignment of the draws spelled out by hand, over the
shared case of tests/start_make_cases.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sensor_numpy
import start_make_cases as cases
import start_make_numpy as twin
from oracle import spec_numpy as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_fields():
    """[(name, C type, count)] of pg_start_set as include/pigeon_mpc.h declares it"""
    txt = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    body = re.search(r"typedef struct pg_start_set \{(.*?)\} pg_start_set;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.match(r"^\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


def test_struct_size_and_offsets_match_the_header(pkg):
    S = pkg._lib.pg_start_set
    fields = header_fields()
    assert [f[0] for f in fields] == [n for n, _ in S._fields_]
    at = 0
    for name, ctype, count in fields:
        size = {"double": 8, "int32_t": 4}[ctype]
        assert at % size == 0
        assert getattr(S, name).offset == at and getattr(S, name).size == size * count, name
        at += size * count
    assert at == 240 and C.sizeof(S) == 240
    assert S.s_mode.offset == 208                                   # the 26 range fields lead the structure, in the order of the draws
    assert [n for n, _ in S._fields_][:26] == [f"{r}_{end}" for r in twin.RANGES for end in ("lo", "hi")]
    assert tuple(pkg._lib.START_RANGES) == twin.RANGES == tuple(pkg.vehicles.START_RANGES) and tuple(pkg._lib.START_MODES) == twin.MODES


def test_defaults_agree_everywhere(pkg):
    d = pkg.start()
    assert d == twin.start()
    assert all(d[f"{r}_{end}"] == (1.0 if r == "v" else 0.0) for r in twin.RANGES for end in ("lo", "hi")) and all(d[m] == 0 for m in twin.MODES)
    rec = pkg.BatchedTrajectoryTrackingMPC.pack_starts(pkg.start())[0]
    assert all(getattr(rec, k) == v for k, v in d.items()) and list(rec.reserved) == [0, 0, 0]
    src = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    body = re.search(r"pg_start_set pg_default_start_set\(void\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "memset(&s, 0, sizeof(s))" in body and "s.v_lo = 1.0" in body and "s.v_hi = 1.0" in body
    assert pkg.start(s=(2.0, 3.0))["s_hi"] == 3.0 and pkg.start(v=1.1)["v_lo"] == 1.1 and pkg.start(e_hi=0.5)["e_hi"] == 0.5
    with pytest.raises(KeyError):
        pkg.start(speed=1.0)
    c2 = pkg.start_config2(s_range=(5.0, 120.0))
    assert (c2["s_lo"], c2["s_hi"], c2["s_mode"], c2["e_lo"], c2["e_hi"], c2["fx_hi"], c2["dt0_lo"], c2["time_mode"]) == (5.0, 120.0, 0, -0.5, 0.5, 500.0, -0.2, 0)
    assert pkg.start_config2()["s_mode"] == 1 and pkg.start_config2(traj_mode=False)["time_mode"] == 1


def test_pack_starts_refuses_what_the_library_refuses(pkg):
    pack = pkg.BatchedTrajectoryTrackingMPC.pack_starts
    assert len(pack(cases.sets())) == cases.N_SETS and len(pack(pkg.start())) == 1
    bad = {"no set": [], "nan": pkg.start(e_lo=math.nan), "inf": pkg.start(fx_hi=math.inf), "lo > hi": pkg.start(s=(2.0, 1.0)), "v_lo = 0": pkg.start(v=(0.0, 1.0)),
           "v_lo < 0": pkg.start(v=(-1.0, 1.0)), "mode": pkg.start(steady=2), "negative mode": pkg.start(other_mode=-1)}
    for name, s in bad.items():
        with pytest.raises(ValueError):
            pack(s)
    rec = pkg._lib.pg_start_set(); rec.v_lo = rec.v_hi = 1.0; rec.reserved[1] = 1
    with pytest.raises(ValueError):
        pack([rec])


def test_twin_lookup_is_traj_at_s_bit_for_bit():
    """(V, A, psi, kappa) and t of the twin's lookup against spec_numpy.Trajectory's traj[s] at the 64 arclengths of the case: both branches, the pinned knots, the clamped
    ends.  The twin takes the square root as the reference writes it (trajectories.jl:63), so the two are the same operations in the same order."""
    ref = cases.reference()
    branches = set()
    for b in range(cases.B):
        T = spec.Trajectory(cases.tubes()[cases.TUBE_INDEX[b]].data)
        a, k = T.at_s(ref["placed"][b, 0]), ref["look"][b]
        assert (a["V"], a["A"], a["psi"], a["kappa"], a["t"]) == (k["V"], k["A"], k["psi"], k["kappa"], k["t"]), b
        branches.add(k["branch"])
    assert branches == {"linear", "sqrt"}


def test_twin_lookup_is_traj_at_s_in_V_bit_for_bit():
    """... and V over every tube more densely than the case samples it: 2000 arclengths per tube, the knots and the ends among them."""
    for tube in cases.tubes():
        ch, T = twin.held(tube), spec.Trajectory(tube.data)
        differ = [s for s in np.concatenate([np.linspace(tube.s[0], tube.s[-1], 2000), tube.s[:50], tube.s[-50:]]) if T.at_s(s)["V"] != twin.lookup(ch, s)["V"]]
        assert not differ, (len(differ), differ[:3])


def test_twin_time_inverts_traj_of_t_on_variable_speed():
    """s -> t(s) (the twin) -> traj(t).s (spec_numpy.Trajectory.at_time).  The bound, with u = 2^-53.
    Outside the root: t = t_i + dt rounds by u t, which traj(t) reads back as an error of dt; s = s_i + V dt + A dt^2 / 2 turns an error of dt into V_max times it and
    rounds its own three sums and four products by at most 7 u s: V_max u t_end + 7 u s_end <= 2^-52 (V_max t_end + 4 s_end) = 6.0e-14 m on variable_speed (t_end
    10.8 s, s_end 53.1 m, V_max 5.18 m/s).
    The root, dt = (sqrt(2 A ds + V^2) - V) / A: the radicand carries 2 u of itself (a product, a square, a sum), its root u of that and u of its own: 2 u V' with V' the
    root.  The difference cancels without a rounding of its own, so dt carries 2 u V' / |A| and s' - s that times V: 2^-52 V_max^2 / |A_i|, which joins the bound on
    that branch (6e-12 m at |A_i| = 1e-3, the smallest the branch admits).
    On an interval with |A_i| < 1e-3 (two of the 27) traj[s] takes dt = ds / V_i, the reference's own approximation (trajectories.jl:61): it drops the term A dt^2 / 2
    that traj(t) keeps, so there the two formulas differ by |A_i| dt^2 / 2 by construction (up to 2e-5 m on this tube) and the bound carries that term."""
    tube = cases.tubes()[2]
    ch, T = twin.held(tube), spec.Trajectory(tube.data)
    bound = 2.0 ** -52 * (float(tube.V.max()) * float(tube.t[-1]) + 4.0 * float(tube.s[-1]))
    assert 5e-14 < bound < 7e-14
    worst = {"sqrt": 0.0, "linear": 0.0}; over = 0.0
    for s in np.concatenate([np.linspace(tube.s[0], tube.s[-1], 801), tube.s, 0.5 * (tube.s[1:] + tube.s[:-1])]):
        k = twin.lookup(ch, s)
        back = T.at_time(k["t"])["s"]
        dt = k["t"] - tube.t[k["i"]]
        dropped = abs(k["A"]) * dt * dt / 2.0 if k["branch"] == "linear" else 0.0
        # ... and the time it misplaces, dropped / V, may carry t past the knot, where traj(t) runs on under the next interval's acceleration: second order in that time
        across = float(np.max(np.abs(np.diff(tube.V) / np.diff(tube.t)))) * (dropped / float(tube.V.min())) ** 2
        root = 2.0 ** -52 * float(tube.V.max()) ** 2 / abs(k["A"]) if k["branch"] == "sqrt" else 0.0
        worst[k["branch"]] = max(worst[k["branch"]], abs(back - s))
        if k["branch"] == "sqrt":
            over = max(over, abs(back - s) / (bound + root))
        assert abs(back - s) <= bound + root + dropped + across, (s, k["branch"])
    print(f"t(s) inverts traj(t).s on variable_speed: worst |s' - s| = {worst['sqrt']:.3e} m on the square-root branch ({over:.3f} of its bound, {bound:.3e} m + the root's), "
          f"{worst['linear']:.3e} m where |A_i| < 1e-3 (the dropped term)")
    assert worst["sqrt"] > 0.0 and worst["linear"] > 0.0             # both branches were visited


def test_default_set_gives_the_first_knot_exactly(pkg):
    tubes = cases.tubes()
    out = twin.make(tubes, [0, 1, 2], [twin.start()], [0, 0, 0], seed=99, streams=[5, 6, 7], vehicle=pkg.X1())
    for k, t in enumerate(tubes):
        assert out["placed"][k].tolist() == [t.s[0], 0.0, 0.0, t.V[0]]
        assert out["state"][k].tolist() == [t.E[0], t.N[0], t.psi[0], t.V[0], 0.0, t.kappa[0] * t.V[0]]
        assert out["control"][k].tolist() == [0.0, 0.0, 0.0] and out["t0"][k] == t.t[0] and out["time_offset"][k] == 0.0 and not out["other"][k].any()
    ref = cases.reference()                                         # ... and so do the instances of the case that run under set 0
    for b in np.flatnonzero(cases.INDEX == 0):
        t = tubes[cases.TUBE_INDEX[b]]
        assert ref["state"][b].tolist() == [t.E[0], t.N[0], t.psi[0], t.V[0], 0.0, t.kappa[0] * t.V[0]]


def test_draws_are_a_function_of_seed_stream_and_channel_only():
    seed, streams = cases.SEED, cases.STREAMS
    u = twin.uniforms(seed, streams)
    assert u.shape == (cases.B, 13) and np.all(u > 0.0) and np.all(u < 1.0)
    # the block / word assignment by hand: channel c = word c % 4 of block 4 + c / 4
    key = [seed & 0xFFFFFFFF, seed >> 32]
    for b in (0, 1, 37):
        st = int(streams[b])
        for c in range(13):
            x = sensor_numpy.philox4x32_10([0, 4 + c // 4, st & 0xFFFFFFFF, st >> 32], key)
            assert u[b, c] == (float(x[c % 4]) + 0.5) * 2.0 ** -32, (b, c)
    # no dependence on the batch: alone, permuted, in another batch size
    perm = np.random.default_rng(0).permutation(cases.B)
    assert np.array_equal(twin.uniforms(seed, streams[perm]), u[perm])
    assert np.array_equal(twin.uniforms(seed, streams[11:12]), u[11:12])
    # ... and a dependence on both words of the seed and of the stream
    assert not np.any(twin.uniforms(seed + 1, streams) == u) and not np.any(twin.uniforms(seed + (1 << 32), streams) == u)
    assert not np.any(twin.uniforms(seed, streams + np.uint64(1 << 32)) == u)
    # none of the sensor's, the disturbance's or the human's blocks (0-3) is used
    assert twin.BLOCK0 == 4
    # value = lo + u (hi - lo): lo == hi gives lo exactly
    v = twin.draws([twin.start(e=0.3, s=(1.0, 2.0))], np.zeros(cases.B, dtype=int), seed, streams)
    assert np.all(v[:, 1] == 0.3) and np.all((v[:, 0] > 1.0) & (v[:, 0] < 2.0)) and np.all(v[:, 3] == 1.0)
