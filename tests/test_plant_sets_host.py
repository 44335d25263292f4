"""CPU tests of the plant sets (pg_set_plant_sets) and the tracking summary (pg_get_tracking_state): the numpy yardstick of the GPU tests is pinned to the C++ oracle, the
vehicle variants recompute their derived fields, the ctypes packing matches the ABI, the new names are declared and exported, and the numpy tracking summary returns the
known answers of a hand-made history."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import plant_numpy
from conftest import ROOT, make_oracle

NEW_NAMES = ["pg_set_plant_sets", "pg_set_plant_index", "pg_clear_plant_sets", "pg_get_plant_sets", "pg_get_tracking_state"]


def test_numpy_plant_equals_the_oracle_at_x1(pkg, oracle_mod, skidpad):
    """(a) 200 random states, among them steering beyond delta_max, braking beyond Fx_min, drive beyond Fx_max / Px_max and sliding tires: 1e-12 relative."""
    orc = make_oracle(oracle_mod, skidpad)
    P = pkg.X1()
    for k, v in orc.vehicle().items():
        assert P[k] == pytest.approx(v, rel=1e-15), k
    rng = np.random.default_rng(2024)
    n = 200
    q = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-3.5, 3.5, n), rng.uniform(1.5, 16.0, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    delta = rng.uniform(-0.25, 0.25, n); Fx = rng.uniform(-3000.0, 3000.0, n)
    delta[0:25] = rng.uniform(0.32, 0.6, 25) * rng.choice([-1, 1], 25)        # beyond delta_max = 0.314
    Fx[25:50] = rng.uniform(-30000.0, P["Fx_min"] - 1.0, 25)                  # braking beyond Fx_min
    Fx[50:70] = rng.uniform(5700.0, 12000.0, 20)                              # beyond Fx_max, and beyond Px_max / Ux at speed
    q[70:110, 4] = rng.uniform(1.5, 4.0, 40) * rng.choice([-1, 1], 40)        # sliding: slip angles far beyond the peak
    q[90:110, 5] = rng.uniform(0.8, 1.5, 20) * rng.choice([-1, 1], 20)
    u3 = np.stack([delta, np.where(Fx > 0, 0.0, 0.6) * Fx, np.where(Fx > 0, 1.0, 0.4) * Fx], axis=1)
    assert np.sum(np.abs(delta) > P["delta_max"]) >= 25 and np.sum(Fx < P["Fx_min"]) >= 25 and np.sum(Fx > P["Fx_max"]) >= 20
    for dt in (0.01, 0.05):
        got = plant_numpy.plant_step_vec(P, q, u3, dt)
        ref = np.stack([orc.plant_step(q[b], u3[b], dt) for b in range(n)])
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        print(f"dt = {dt}: max relative difference numpy plant - oracle plant = {err.max():.2e}")
        assert err.max() < 1e-12, (dt, err.max(), int(np.argmax(err.max(axis=1))))
    # the scalar statement (spec_numpy.world_vehicle_model as it stands) on every fourth state, and on the saturated and sliding ones
    sel = np.unique(np.concatenate([np.arange(0, n, 4), np.arange(0, 110, 5)]))
    one = plant_numpy.plant_step(P, q[sel], u3[sel], 0.01)
    ref = np.stack([orc.plant_step(q[b], u3[b], 0.01) for b in sel])
    assert np.max(np.abs(one - ref) / np.maximum(1.0, np.abs(ref))) < 1e-12
    # other vehicles, one per instance: the vectorised form against the scalar one (the oracle knows X1 only)
    sets = plant_numpy.four_plants(pkg.X1)
    Ps = [sets[b % 4] for b in range(len(sel))]
    vec = plant_numpy.plant_step_vec(Ps, q[sel], u3[sel], 0.01)
    sca = plant_numpy.plant_step(Ps, q[sel], u3[sel], 0.01)
    assert np.max(np.abs(vec - sca) / np.maximum(1.0, np.abs(sca))) < 1e-12
    assert np.array_equal(vec[0::4], plant_numpy.plant_step_vec(sets[0], q[sel][0::4], u3[sel][0::4], 0.01))       # instance b integrates P[b], no other
    for k in (1, 2, 3):
        assert np.max(np.abs(vec[k::4] - plant_numpy.plant_step_vec(sets[0], q[sel][k::4], u3[sel][k::4], 0.01))) > 1e-6, k


def test_x1_overrides_recompute_the_derived_fields(pkg):
    """(b)"""
    import math
    X = pkg.X1()
    want = dict(G=9.80665, mfl=484.0, mfr=455.0, mrl=521.0, mrr=504.0, m=1964.0, Ixx=175.0, Iyy=1000.0, Izz=2900.0, L=2.87, d=1.63, a=(521.0 + 504.0) / 1964.0 * 2.87,
                b=(484.0 + 455.0) / 1964.0 * 2.87, hf=0.1, hr=0.1, h1=0.37, mu=0.92, Caf=150e3, Car=220e3, Fx_max=5600.0, Px_max=75e3, Cd0=241.0, Cd1=25.1, Cd2=0.0, fwd_frac=0.0,
                rwd_frac=1.0, fwb_frac=0.6, rwb_frac=0.4, delta_max=18 * math.pi / 180)
    want["h"] = 0.1 * want["b"] / 2.87 + 0.1 * want["a"] / 2.87 + 0.37
    want["Fx_min"] = max(-1964.0 * 9.80665 * want["a"] * 0.92 / (2.87 * 0.4 + 0.92 * want["h"]), -1964.0 * 9.80665 * want["b"] * 0.92 / (2.87 * 0.6 - 0.92 * want["h"]))
    want["kappa_max"] = math.tan(want["delta_max"]) / 2.87
    assert set(X) == set(want)
    for k in want:
        assert X[k] == want[k] and isinstance(X[k], float), k
    lo = pkg.X1(mu=0.5)
    fmin = max(-X["m"] * X["G"] * X["a"] * 0.5 / (X["L"] * 0.4 + 0.5 * X["h"]), -X["m"] * X["G"] * X["b"] * 0.5 / (X["L"] * 0.6 - 0.5 * X["h"]))
    assert lo["mu"] == 0.5 and lo["Fx_min"] == fmin and abs(lo["Fx_min"]) < 0.6 * abs(X["Fx_min"])
    assert all(lo[k] == X[k] for k in X if k not in ("mu", "Fx_min"))
    heavy = pkg.X1(mfl=580.8, mrr=604.8)
    assert heavy["m"] == 580.8 + 455.0 + 521.0 + 604.8 and heavy["a"] == (521.0 + 604.8) / heavy["m"] * 2.87 and heavy["b"] == (580.8 + 455.0) / heavy["m"] * 2.87
    assert heavy["h"] == 0.1 * heavy["b"] / 2.87 + 0.1 * heavy["a"] / 2.87 + 0.37 and heavy["Fx_min"] != X["Fx_min"]
    assert pkg.X1(L=3.0)["kappa_max"] == math.tan(X["delta_max"]) / 3.0 and pkg.X1(fwb_frac=0.7)["rwb_frac"] == 1 - 0.7
    with pytest.raises(KeyError):
        pkg.X1(m=2000.0)            # derived: set the corner masses
    with pytest.raises(KeyError):
        pkg.X1(Fx_min=-1.0)


def test_vehicle_arrays_pack_as_the_abi_lays_them_out(pkg):
    """(c)"""
    from pigeon_jl_amd import _lib
    from pigeon_jl_amd.mpc import BatchedTrajectoryTrackingMPC
    lib = pkg.load_library()
    out = (C.c_int32 * 3)()
    assert lib.pg_abi_layout(out, 3) >= 3
    sets = plant_numpy.four_plants(pkg.X1)
    holder = BatchedTrajectoryTrackingMPC.__new__(BatchedTrajectoryTrackingMPC)       # pack_vehicles reads nothing of a handle but its own vehicle
    holder.vehicle = pkg.X1()
    arr = holder.pack_vehicles(sets + [dict(mu=0.3)])
    assert C.sizeof(arr) == 5 * out[1] and out[1] == 22 * 8
    raw = np.frombuffer(bytes(arr), dtype=np.float64).reshape(5, 22)
    for k, v in enumerate(sets):
        assert np.array_equal(raw[k], np.array([v[f] for f in plant_numpy.VEH_FIELDS])), k
    assert [n for n, _ in _lib.pg_vehicle._fields_] == plant_numpy.VEH_FIELDS
    assert raw[4, plant_numpy.VEH_FIELDS.index("mu")] == 0.3 and raw[4, 1] == holder.vehicle["m"]      # a partial dict is completed from the handle's vehicle
    holder.h = None


def test_new_names_are_declared_and_exported(pkg):
    """(d)"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read(), flags=re.S)
    m = re.search(r"global:\s*([^;]+);", open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_exports.map")).read())
    patterns = m.group(1).split()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in pkg.SYMBOLS
    jl = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    for name in NEW_NAMES:
        assert ":" + name in jl, name
    lib = pkg.load_library()
    for name in NEW_NAMES:
        assert getattr(lib, name).argtypes is not None, name


def test_numpy_tracking_summary_on_a_hand_made_history():
    """(e) four instances over five steps: one outside from step 0, one that leaves at step 3 on the right, one that never leaves, one that touches the edge exactly
    (inside: the interval is closed)."""
    e = np.array([[0.30, 0.00, 0.10, 0.25],
                  [0.20, -0.10, -0.10, 0.25],
                  [0.10, -0.20, 0.10, 0.00],
                  [0.00, -0.30, -0.10, 0.00],
                  [0.00, -0.10, 0.10, 0.00]])
    s = np.arange(5.0)[:, None] + np.array([10.0, 20.0, 30.0, 40.0])[None, :]
    Ux = np.full((5, 4), 5.0); Ux[2, 1] = 4.0
    Uy = np.zeros((5, 4)); Uy[1, 0] = -0.5; Uy[4, 2] = 0.25
    r = np.zeros((5, 4)); r[3, 3] = -0.7; r[0, 3] = 0.2
    eL = np.full((5, 4), 0.25); eR = np.full((5, 4), -0.25)
    sm, n, fx, margin = plant_numpy.tracking_summary(s, e, Ux, Uy, r, eL, eR)
    assert np.array_equal(n, [5, 5, 5, 5])
    assert np.array_equal(fx, [0, 3, -1, -1])
    assert np.allclose(sm[:, 0], [0.30, 0.30, 0.10, 0.25], rtol=0, atol=1e-15)
    assert np.allclose(sm[:, 1], [0.14, 0.15, 0.05, 0.125], rtol=0, atol=1e-15)
    assert np.allclose(sm[:, 2], [0.1, 0.0, 0.05, 0.0], rtol=0, atol=1e-15)
    assert np.allclose(sm[:, 3], [0.0, 0.0, 0.0, 0.7], rtol=0, atol=1e-15)
    assert np.array_equal(sm[:, 4], [5.0, 4.0, 5.0, 5.0]) and np.array_equal(sm[:, 5], [14.0, 24.0, 34.0, 44.0])
    assert np.allclose(margin, [0.05, 0.05, 0.15, 0.0], rtol=0, atol=1e-15)
    # a later call's history continues the clock's step indices
    assert np.array_equal(plant_numpy.tracking_summary(s, e, Ux, Uy, r, eL, eR, step0=30)[2], [30, 33, -1, -1])
