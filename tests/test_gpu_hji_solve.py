"""GPU tests of pg_hji_solve (BatchedTrajectoryTrackingMPC.solve_hji_cache) in both libraries: against the numpy twin (tests/hji_solve_numpy.py), the properties the
scheme holds exactly, the CFL mode, the install path and the refusals.  Grids, target and twin runs: tests/hji_solve_cases.py."""
import numpy as np
import pytest

import hji_solve_cases as cases
import hji_solve_numpy as hs

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "f32"]
# max |device - twin| after the 6 fixed sweeps of the shared cases, measured on the MI355X (EXPERIMENTS.md, "pg_hji_solve against its twin"), and the asserted bound =
# 8 x the measured value: the twin is numpy without contraction, the kernels contract to FMA, and V is rounded to float32 after every sweep, so one flipped ulp
# (3.8e-6 for |V| < 32) travels.  alpha is relative.  The fp32 library does its arithmetic in float: its figures are those of float32 rounding in p, f and H.
# Measured 2026-10-19 (both grids and the mu = 0.6 run; the largest of the three): the fp64 library gives the twin's V and gradV BIT FOR BIT after 6 sweeps (alpha differs
# in the last place, 1.565e-16), so its asserted bound on V and gradV is 0: any difference there is a disagreement in the scheme.  fp32: half an ulp of V at 16 <= |V| < 32.
MEASURED = {"f64": {"V": 0.0, "gradV": 0.0, "alpha": 1.565e-16}, "f32": {"V": 1.907e-06, "gradV": 1.982e-06, "alpha": 1.275e-07}}
BOUND = {p: {k: 8 * v for k, v in m.items()} for p, m in MEASURED.items()}


@pytest.fixture(scope="module", params=PRECISIONS)
def mpc(request, pkg, skidpad):
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, 64, precision=request.param, hji_eps=1.0)
    yield m
    m.close()


def run(m, name, periodic, sweeps=cases.SWEEPS, veh=None, install=False, l0=None, **kw):
    knots, t = cases.grid(name, periodic)
    return m.solve_hji_cache(knots, t if l0 is None else l0, 1e9, vehicle=veh, install=install, fixed_dt=cases.FIXED_DT, max_sweeps=sweeps, periodic_psi=periodic, **kw)


def differences(dev, twin):
    (V, g, st), (Vt, gt, stt) = dev, twin
    return {"V": float(np.max(np.abs(V.astype(np.float64) - Vt))), "gradV": float(np.max(np.abs(g.astype(np.float64) - gt))),
            "alpha": float(np.max(np.abs(st["alpha"] - stt["alpha"]) / np.maximum(1.0, np.abs(stt["alpha"]))))}


@pytest.mark.parametrize("name,periodic", cases.CASES)
def test_against_the_twin(mpc, name, periodic):
    dev = run(mpc, name, periodic)
    assert dev[2]["sweeps"] == cases.SWEEPS and dev[2]["reached_horizon"] == 0 and dev[2]["bad_sweep"] == -1
    assert abs(dev[2]["tau"] - cases.SWEEPS * cases.FIXED_DT) < 1e-12 and dev[2]["last_dt"] == cases.FIXED_DT
    d = differences(dev, cases.twin(name, periodic))
    print(f"pg_hji_solve {mpc.precision} grid {name} periodic={periodic}: max |V - twin| = {d['V']:.3e}, max |gradV - twin| = {d['gradV']:.3e}, alpha rel = {d['alpha']:.3e}")
    for k in ("V", "gradV", "alpha"):
        assert d[k] <= BOUND[mpc.precision][k], (k, d[k])
    assert dev[2]["v_min"] == float(dev[0].min()) and dev[2]["v_max"] == float(dev[0].max())
    assert np.any(dev[0] < cases.grid(name, periodic)[1])                                   # the tube moved


@pytest.mark.parametrize("name,periodic", cases.CASES)
def test_exact_properties(mpc, name, periodic):
    knots, l0 = cases.grid(name, periodic)
    V0, g0, st0 = mpc.solve_hji_cache(knots, l0, 0.0, install=False, periodic_psi=periodic)
    assert st0["sweeps"] == 0 and st0["reached_horizon"] == 1 and st0["tau"] == 0.0
    assert np.array_equal(V0.view(np.uint32), l0.view(np.uint32))                           # zero horizon: l0 bit for bit
    gb = 1e-6 if mpc.precision == "f32" else 0.0                                            # (the fp64 library's finite differences of l0 are the twin's, rounded once)
    assert np.max(np.abs(g0.astype(np.float64) - hs.gradient(l0, knots, periodic))) <= gb + 6e-8 * np.max(np.abs(g0))
    V6, g6, st6 = run(mpc, name, periodic)
    V5, _, _ = run(mpc, name, periodic, sweeps=cases.SWEEPS - 1)
    assert np.all(V6 <= l0) and np.all(V6 <= V5) and np.any(V6 < V5)
    again = run(mpc, name, periodic)
    assert np.array_equal(again[0].view(np.uint32), V6.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), g6.view(np.uint32))
    assert np.array_equal(again[2]["alpha"], st6["alpha"])
    V3, _, _ = run(mpc, name, periodic, sweeps=3)
    V33, g33, st33 = run(mpc, name, periodic, sweeps=3, l0=V3)                              # the tube form: a solve continued from its own result
    assert np.array_equal(V33.view(np.uint32), V6.view(np.uint32)) and np.array_equal(g33.view(np.uint32), g6.view(np.uint32))
    assert np.array_equal(st33["alpha"], st6["alpha"])
    if periodic:                                                                            # both copies of the same angle stay bit-identical
        lc = cases.target(knots, cos_psi=0.3)
        dims = [len(k) for k in knots]
        Vc = run(mpc, name, True, sweeps=4, l0=lc)[0].reshape(dims, order="F")
        assert np.array_equal(Vc[:, :, 0], Vc[:, :, -1]) and np.any(Vc.reshape(-1, order="F") < lc)


def test_cfl_mode(mpc):
    knots, l0 = cases.grid("A", False)
    minsp = np.array([np.min(np.diff(k.astype(np.float64))) for k in knots])
    horizon = 0.1
    V, g, st = mpc.solve_hji_cache(knots, l0, horizon, install=False)
    assert st["reached_horizon"] == 1 and st["tau"] == horizon and 2 <= st["sweeps"] <= 20
    assert st["last_dt"] <= 0.8 / np.sum(st["alpha"] / minsp) * (1 + 1e-12)
    total, tau = st["sweeps"], 0.0
    for k in range(1, total):                                                               # every step but the last is the CFL step of the alpha it reports
        _, _, sk = mpc.solve_hji_cache(knots, l0, horizon, install=False, max_sweeps=k)
        assert sk["sweeps"] == k and sk["reached_horizon"] == 0
        assert abs(sk["last_dt"] - 0.8 / np.sum(sk["alpha"] / minsp)) <= 1e-12 * sk["last_dt"]
        tau += sk["last_dt"]
        assert abs(sk["tau"] - tau) <= 1e-12
    _, _, s2 = mpc.solve_hji_cache(knots, l0, 3.0, install=False, max_sweeps=2, cfl=0.5)
    assert s2["sweeps"] == 2 and s2["reached_horizon"] == 0 and s2["tau"] < 3.0
    assert abs(s2["last_dt"] - 0.5 / np.sum(s2["alpha"] / minsp)) <= 1e-12 * s2["last_dt"]


def test_install_equals_set_hji_cache(pkg, skidpad, mpc):
    name, periodic = "B", True
    knots, l0 = cases.grid(name, periodic)
    dims = [len(k) for k in knots]
    V, g, st = run(mpc, name, periodic, install=True)
    got = np.zeros(7, dtype=np.int32)
    import ctypes as C
    mpc._chk(mpc.lib.pg_hji_grid_dims(mpc.h, got.ctypes.data_as(C.POINTER(C.c_int32))), "pg_hji_grid_dims")
    assert list(got) == dims
    # lookups at node coordinates (weights exactly 0 / 1): interior nodes and nodes on the high faces, where the bounds test is <=
    rng = np.random.default_rng(3)
    idx = np.stack([rng.integers(0, n, 96) for n in dims], axis=1)
    idx[:24] = np.minimum(idx[:24], np.array(dims) - 2); idx[:24] = np.maximum(idx[:24], 1 - (np.array(dims) == 2))     # interior where the extent allows
    for k in range(7):
        idx[24 + 8 * k:32 + 8 * k, k] = dims[k] - 1                                         # high face of dimension k
    idx[80:] = np.array(dims) - 1                                                           # the last node: every face at once
    x = np.stack([knots[d][idx[:, d]].astype(np.float64) for d in range(7)], axis=1)
    node = np.ravel_multi_index(tuple(idx.T), dims, order="F")
    Vl, gl = mpc.hji_lookup(x)
    assert np.array_equal(Vl, V[node].astype(np.float64)) and np.array_equal(gl, g[node].astype(np.float64))
    # a second handle that receives the same arrays through pg_set_hji_grid runs the same safety rollout, bit for bit
    B = 64
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=41)
    other = pkg.synthetic.other_cars(state, seed=43)
    ref = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, precision=mpc.precision, hji_eps=1.0)
    ref.set_hji_cache(knots, V, g)
    outs = []
    for m in (mpc, ref):
        m.reset()
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        outs.append(m.simulate_safety_(6, dt=0.01, use_HJI_policy=True, human="worst", record=True))
    ref.close()
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert np.array_equal(a, b, equal_nan=True)
    for key in outs[0][4]:
        assert np.array_equal(outs[0][4][key], outs[1][4][key], equal_nan=True), key
    assert np.any(np.isfinite(outs[0][4]["V"]))                                             # the rollout did read the grid
    mpc.clear_hji_cache()


def test_vehicle_argument(pkg, mpc):
    name, periodic = "A", False
    nominal = run(mpc, name, periodic)
    low = run(mpc, name, periodic, veh=pkg.vehicles.X1(mu=0.6))
    assert not np.array_equal(low[0], nominal[0])
    d = differences(low, cases.twin(name, periodic, veh="mu06"))
    print(f"pg_hji_solve {mpc.precision} grid {name} mu = 0.6: max |V - twin| = {d['V']:.3e}, max |gradV - twin| = {d['gradV']:.3e}, alpha rel = {d['alpha']:.3e}")
    for k in ("V", "gradV", "alpha"):
        assert d[k] <= BOUND[mpc.precision][k], (k, d[k])
    # the handle's own vehicle, handed over explicitly, is the default
    same = run(mpc, name, periodic, veh=mpc.vehicle)
    assert np.array_equal(same[0].view(np.uint32), nominal[0].view(np.uint32))


def test_refusals_leave_the_installed_grid_alone(pkg, skidpad, mpc):
    knots, l0 = cases.grid("A", False)
    pk, pl0 = cases.grid("B", True)
    gk, gV, gg = pkg.synthetic.hji_grid(dims=(5, 4, 4, 3, 3, 3, 3), seed=6)
    mpc.set_hji_cache(gk, gV, gg)
    x = pkg.synthetic.hji_queries(gk, 32, seed=2)
    before = mpc.hji_lookup(x)

    def refused(status, k, t, horizon=0.1, **kw):
        with pytest.raises(pkg.PigeonError) as e:
            mpc.solve_hji_cache(k, t, horizon, install=True, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))
        after = mpc.hji_lookup(x)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])

    one = [knots[0][:1]] + list(knots[1:])                                                  # a dimension below 2
    refused(-2, one, l0[:l0.size // len(knots[0])])
    flat = [k.copy() for k in knots]; flat[3][1] = flat[3][0]                               # knots that do not increase
    refused(-2, flat, l0)
    down = [k.copy() for k in knots]; down[1] = down[1][::-1].copy()
    refused(-2, down, l0)
    short = [k.copy() for k in pk]; short[2][-1] = np.float32(3.0)                          # a periodic flag whose dimension 3 does not span 2 pi
    refused(-2, short, pl0, periodic_psi=True)
    refused(-2, knots, l0, horizon=-0.1)
    for cfl in (0.0, -0.5, 1.5, float("nan")):
        refused(-2, knots, l0, cfl=cfl)
    refused(-2, knots, l0, fixed_dt=-0.01)
    refused(-2, knots, l0, max_sweeps=-1)
    refused(-2, knots, l0, vehicle=dict(mpc.vehicle, mu=-0.1))
    # a NaN in V ends the solve: error code, the sweep's index in the stats, nothing installed
    bad = l0.copy(); bad[bad.size // 2] = np.nan
    with pytest.raises(pkg.PigeonError) as e:
        mpc.solve_hji_cache(knots, bad, 1e9, install=True, fixed_dt=cases.FIXED_DT, max_sweeps=4)
    assert e.value.status == -2 and e.value.stats["bad_sweep"] == 0 and e.value.stats["reached_horizon"] == 0
    after = mpc.hji_lookup(x)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    mpc.clear_hji_cache()
    # install on a decoupled handle: a state error; without install the same handle solves
    dec = pkg.BatchedTrajectoryTrackingMPC(skidpad, 8, precision=mpc.precision, formulation="decoupled")
    with pytest.raises(pkg.PigeonError) as e:
        dec.solve_hji_cache(knots, l0, 0.1, install=True)
    assert e.value.status == -4
    Vd = dec.solve_hji_cache(knots, l0, 1e9, install=False, fixed_dt=cases.FIXED_DT, max_sweeps=2)[0]
    assert np.array_equal(Vd, run(mpc, "A", False, sweeps=2)[0])
    dec.close()
