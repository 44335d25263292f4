"""The speed planner without a device: the numpy twin (tests/speed_plan_numpy.py) against closed forms and the invariants the scheme has by construction, and the Python
mirror of pg_plan_speeds (struct layouts, defaults, refusals, `closed` broadcasting, the order of the returned tubes)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import speed_plan_cases as cases
import speed_plan_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def no_drag(pkg, **kw):
    v = pkg.X1(Cd0=0.0, Cd1=0.0, Cd2=0.0, **kw)
    return v


# ---- the twin against closed forms ----
def test_circle_with_free_ends_runs_at_the_cap(pkg):
    veh = pkg.X1()
    s = np.linspace(0.0, 60.0, 61); kappa = np.full(61, 0.05)
    for mu_scale, V_max in ((0.5, 30.0), (1.0, 8.0)):
        sp = twin.speed_plan(mu_scale=mu_scale, V_max=V_max)
        # (drag off: at the cap no tire force is left for the tangent, so drag alone would slow the car along the arc)
        r = twin.plan(s, kappa, sp, no_drag(pkg))
        a_lim = np.float64(mu_scale) * veh["mu"] * veh["G"]
        assert np.all(r["V"] == np.sqrt(min(V_max * V_max, a_lim / 0.05))), (mu_scale, V_max)
        assert np.all(r["A"] == 0.0) and r["stats"]["n_cap"] == 61


def test_straight_full_throttle_and_full_braking(pkg):
    veh = no_drag(pkg, Px_max=math.inf)
    s = np.linspace(0.0, 100.0, 201); kappa = np.zeros(201)
    r = twin.plan(s, kappa, twin.speed_plan(V_max=14.0, V_start=2.0), veh)
    W = 4.0 + 2.0 * (veh["Fx_max"] / veh["m"]) * s
    free = W < 196.0
    assert free.sum() > 50 and not free.all()
    assert np.max(np.abs(r["W"][free] - W[free]) / W[free]) < 1e-13 and np.all(r["W"][~free] == 196.0)
    # the same straight planned backward from V_end with Fx_min (mu_scale large enough that the tires are not the limit)
    r = twin.plan(s, kappa, twin.speed_plan(V_max=14.0, V_end=2.0, mu_scale=3.0), veh)
    W = 4.0 + 2.0 * (-veh["Fx_min"] / veh["m"]) * (100.0 - s)
    free = W < 196.0
    assert free.sum() > 20 and not free.all()
    assert np.max(np.abs(r["W"][free] - W[free]) / W[free]) < 1e-13 and np.all(r["W"][~free] == 196.0)
    assert r["stats"]["n_brake"] == free.sum() - 1 and r["stats"]["n_accel"] == 0


def test_power_limit_converges_at_first_order(pkg):
    veh = no_drag(pkg, Fx_max=1e9)
    errs = []
    for n in (200, 400, 800):
        s = np.linspace(0.0, 200.0, n + 1)
        r = twin.plan(s, np.zeros(n + 1), twin.speed_plan(V_max=100.0, V_start=5.0), veh)
        V3 = 125.0 + 3.0 * veh["Px_max"] * s / veh["m"]
        errs.append(float(np.max(np.abs(r["V"] - np.cbrt(V3)))))
    assert 1.8 < errs[0] / errs[1] < 2.2 and 1.8 < errs[1] / errs[2] < 2.2, errs


# ---- invariants by construction, on the shared case and on whole committed paths ----
def every_plan(pkg):
    p, closed, sets, vehs, ref = cases.reference()
    for i in range(len(p)):
        for j in range(0, cases.N_SETS, 3):
            yield p[i], bool(closed[i]), ref[i][j]


def test_invariants_hold_exactly(pkg):
    for path, closed, r in every_plan(pkg):
        W, Wb, init, cap, L = r["W"], r["Wb"], r["init"], r["cap"], len(path)
        n = L - 1
        assert np.all(W <= cap) and np.all(W <= Wb) and np.all(W[:n] <= init[:n])
        cand = (init, Wb, r["fwd_cand"])
        assert np.all((W == cand[0]) | (W == cand[1]) | (W == cand[2]))
        st = r["stats"]
        assert st["n_cap"] + st["n_accel"] + st["n_brake"] == L
        # the forward inequality as computed, over every interval the pass took (a closed path's pass does not take the one that arrives at i0)
        lim = r["lim"]
        for i in range(n):
            nx = (i + 1) % n if closed else i + 1
            if closed and nx == r["i0"]:
                continue
            assert W[nx] <= max(W[i] + 2.0 * r["ds"][i] * lim.acc(W[i], path.kappa[i]), lim.Wfloor)
        if closed:
            assert W[n] == W[0] and r["A"][n] == r["A"][0] and W[r["i0"]] == cap[r["i0"]]


@pytest.mark.parametrize("name,closed", [("skidpadoval", True), ("vail", False)])
def test_more_friction_is_never_slower(pkg, name, closed):
    path = pkg.load_path_fixture(name); veh = pkg.X1()
    prev = None
    for mu_scale in (0.3, 0.5, 0.7, 0.9, 1.0):
        W = twin.plan(path.s, path.kappa, twin.speed_plan(mu_scale=mu_scale, V_max=20.0), veh, closed)["W"]
        assert prev is None or np.all(prev <= W), mu_scale
        prev = W


def test_closed_path_equals_its_rotation_to_i0(pkg):
    path = cases.synthetic_closed(pkg); veh = pkg.X1()
    n = len(path) - 1
    sp = twin.speed_plan(mu_scale=0.8, V_max=25.0)
    r = twin.plan(path.s, path.kappa, sp, veh, True)
    i0 = r["i0"]
    assert i0 == 23
    rot = np.r_[np.arange(i0, n), np.arange(0, i0 + 1)]
    ds = np.diff(path.s)[np.r_[np.arange(i0, n), np.arange(0, i0)]]
    s_rot = np.concatenate([[0.0], np.cumsum(ds)])
    q = twin.plan(s_rot, path.kappa[rot], sp, veh, True)
    assert q["i0"] == 0
    same_ds = np.diff(s_rot) == ds                                  # (the rotated s is a new sum: compare where its intervals are the original ones bit for bit)
    assert same_ds.sum() > n // 2
    if same_ds.all():
        assert q["W"].tobytes() == r["W"][rot].tobytes()
    else:
        assert np.max(np.abs(q["W"] - r["W"][rot]) / r["W"][rot]) < 1e-12


# ---- the mirror ----
def test_struct_layouts_and_defaults(pkg):
    L = pkg._lib if hasattr(pkg, "_lib") else __import__("sys").modules["pigeon_jl_amd._lib"]
    assert C.sizeof(L.pg_speed_plan) == 64 and C.sizeof(L.pg_speed_plan_stats) == 48
    assert [getattr(L.pg_speed_plan, n).offset for n, _ in L.pg_speed_plan._fields_] == list(range(0, 64, 8))
    assert [getattr(L.pg_speed_plan_stats, n).offset for n, _ in L.pg_speed_plan_stats._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    mpc_mod = __import__("sys").modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.SPEED_PLAN_STATS_DTYPE.itemsize == 48 and mpc_mod.SPEED_PLAN_STATS_DTYPE.names == tuple(n for n, _ in L.pg_speed_plan_stats._fields_)
    d = pkg.vehicles.speed_plan()
    assert (d["mu_scale"], d["V_max"], d["V_floor"], d["ax_max"], d["ax_min"], d["ay_max"]) == (1.0, 30.0, 1.0, math.inf, -math.inf, math.inf)
    assert math.isnan(d["V_start"]) and math.isnan(d["V_end"])
    assert {k: v for k, v in d.items() if v == v} == {k: v for k, v in twin.speed_plan().items() if v == v}
    with pytest.raises(KeyError):
        pkg.vehicles.speed_plan(mu=0.5)
    # the header states the same sizes and the same defaults
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_speed_plan;            /* 64 bytes */" in hdr and "} pg_speed_plan_stats;      /* 48 bytes */" in hdr
    assert "/* { 1, 30, 1, NaN, NaN, +Inf, -Inf, +Inf } */\npg_speed_plan pg_default_speed_plan(void);" in hdr
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_speed_plan
        f.restype = L.pg_speed_plan; f.argtypes = []
        r = f()
        assert (r.mu_scale, r.V_max, r.V_floor, r.ax_max, r.ax_min, r.ay_max) == (1.0, 30.0, 1.0, math.inf, -math.inf, math.inf) and math.isnan(r.V_start) and math.isnan(r.V_end)


def test_both_libraries_export_the_two_symbols(pkg):
    for name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", name)], capture_output=True, text=True, check=True).stdout
        syms = set(re.findall(r" T (pg_\w+)", out))
        assert {"pg_plan_speeds", "pg_default_speed_plan"} <= syms, name
    assert {"pg_plan_speeds", "pg_default_speed_plan"} <= set(pkg.SYMBOLS)


def test_mirror_refuses_what_the_library_refuses(pkg):
    M = pkg.BatchedTrajectoryTrackingMPC
    sp = pkg.vehicles.speed_plan
    for bad in (dict(mu_scale=0.0), dict(mu_scale=math.inf), dict(V_max=0.0), dict(V_max=math.nan), dict(V_floor=0.0), dict(V_floor=31.0), dict(V_start=-1.0),
                dict(V_end=math.inf), dict(ax_max=-0.1), dict(ax_min=0.1), dict(ax_min=math.nan), dict(ay_max=0.0)):
        with pytest.raises(ValueError):
            M.pack_speed_plans([sp(), sp(**bad)])
    with pytest.raises(ValueError):
        M.pack_speed_plans([])
    assert len(M.pack_speed_plans(sp(V_start=0.0, ax_min=0.0, ax_max=0.0))) == 1
    path = pkg.load_path_fixture("variable_speed")

    def edited(field, i, value, n=None):
        d = path.data.copy(); d[pkg.trajectories.FIELDS.index(field), i] = value
        d = d[:, :n] if n else d
        return pkg.TrajectoryTube(*[d[k] for k in range(12)])

    for bad, closed in ((edited("s", 5, path.s[4]), None), (edited("kappa", 3, math.nan), None), (edited("edge_L", 0, math.inf), None), (edited("s", 0, 0.0, n=2), True),
                        (edited("s", 0, 0.0, n=1), None)):
        with pytest.raises(ValueError):
            M.pack_paths([path, bad], closed)
    with pytest.raises(ValueError):
        M.pack_paths([])
    with pytest.raises(ValueError):
        M.pack_paths([path, path, path], [True, False])
    # t, V and A are not looked at
    L, ch, cl = M.pack_paths([edited("V", 2, math.nan), edited("t", 2, math.inf)])
    assert list(L) == [28, 28] and list(cl) == [0, 0]


def test_closed_broadcasting_and_tube_order(pkg):
    M = pkg.BatchedTrajectoryTrackingMPC
    p, closed, _, _, _ = cases.reference()
    assert list(M.pack_paths(p)[2]) == [0, 0, 0] and list(M.pack_paths(p, True)[2]) == [1, 1, 1] and list(M.pack_paths(p, [0, 0, 1])[2]) == [0, 0, 1]
    L, ch, cl = M.pack_paths(p, closed)
    assert list(L) == [130, 28, 65] and ch.shape == (3, 10, 130) and np.all(ch[1, :, 28:] == 0)
    L1, ch1, _ = M.pack_paths(ch[:1])                              # the channel array itself: every knot valid
    assert list(L1) == [130] and ch1.tobytes() == ch[:1].tobytes()
    # output trajectory k = path * n_sets + set
    n_sets = 4
    out = np.zeros((3 * n_sets, 10, 130))
    for k in range(3 * n_sets):
        out[k] = ch[k // n_sets]; out[k, 2] = 100 * (k // n_sets) + (k % n_sets)
    tubes = M.tubes_from_channels(out, L, n_sets)
    assert [len(t) for t in tubes] == [130] * 4 + [28] * 4 + [65] * 4
    for k, t in enumerate(tubes):
        assert np.all(t.V == 100 * (k // n_sets) + (k % n_sets)) and np.all(t.theta == 0) and np.all(t.phi == 0)
        assert t.s.tobytes() == p[k // n_sets].s.tobytes() and t.edge_R.tobytes() == p[k // n_sets].edge_R.tobytes()
