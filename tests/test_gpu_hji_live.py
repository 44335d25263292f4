"""GPU parity tests of the HJI path (lookup, safety row, fallback policy: HJI_computation.jl:66-72, :90-170, ros_integration.jl:114-124) against the CPU oracle on the
live-gradient grid of tests/hji_live_cases.py.  On synthetic.hji_grid, which every other HJI test uses, dV/dUy and dV/dr are zero at every node and nothing depends on
Uy or r: the steer sign, the line-search winner, the steering terms of the safety row and the handling of dimensions 4 and 6 in the lookup could be wrong unnoticed.
tests/test_hji_live_host.py shows without a GPU that on this grid they cannot; the closed loop on it is in tests/test_gpu_safety_rollout.py."""
import math

import numpy as np
import pytest

from conftest import make_oracle
import hji_live_cases as lc

pytestmark = pytest.mark.gpu

# fp32 lookup on this grid against the oracle at the float-rounded queries, largest over the 348 queries and the three layouts, measured on the MI355X (EXPERIMENTS.md):
# |V - V_o| / max(1, |V_o|) and max_k |gradV_k - gradV_o,k|.  The test asserts 8 x these (the project's rule for fp32 bounds).
MEASURED_F32 = {"V": 1.987e-7, "gradV": 1.602e-7}                           # the same figures in all three layouts


def f32_round(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def lookup_ref(oracle_mod, skidpad):
    """precision -> (queries, V, gradV, in-bounds) of the oracle, computed once; the fp32 library is compared at the float-rounded queries"""
    knots, V, g = lc.live_grid()
    orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(knots, V, g)
    x, fam, _ = lc.lookup_queries(knots)
    out = {}
    for prec in ("f64", "f32"):
        q = x if prec == "f64" else f32_round(x)
        res = [orc.hji_lookup(p) for p in q]
        out[prec] = tuple(a for a in (q, np.array([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res])))
        for a in out[prec]:
            a.setflags(write=False)
    return out, fam


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cell_dims", [7, 5, 3])
def test_lookup_on_the_live_grid(pkg, skidpad, lookup_ref, cell_dims, precision):
    """All three cell layouts, both libraries: V and all seven gradient channels at random points (some outside), the corners of the box, node points (weights exactly
    0 or 1, the high faces of dimensions 4 and 6 among them) and two families that move along x[4] only and along x[6] only.  fp64: 1e-12, the bar of
    test_lookup_matches_oracle.  fp32: 8 x MEASURED_F32."""
    ref, fam = lookup_ref
    x, Vo, Go, inb = ref[precision]
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, 8, precision=precision, options={"hji_cell_dims": cell_dims})
    mpc.set_hji_cache(*lc.live_grid())
    Vg, Gg = mpc.hji_lookup(x)
    mpc.close()
    assert inb.sum() >= 50 and (~inb).sum() >= 50
    assert np.all(np.isposinf(Vg[~inb])) and np.all(Gg[~inb] == 0)
    assert np.all(np.isfinite(Vg[inb]))
    eV = np.abs(Vg[inb] - Vo[inb]) / np.maximum(1.0, np.abs(Vo[inb]))
    eG = np.abs(Gg[inb] - Go[inb])
    print(f"live lookup {precision} cell_dims={cell_dims}: max rel |dV| = {eV.max():.3e}, max |dgradV| per channel = {np.array2string(eG.max(axis=0), precision=3)}")
    tolV, tolG = (1e-12, 1e-12) if precision == "f64" else (8 * MEASURED_F32["V"], 8 * MEASURED_F32["gradV"])
    assert eV.max() <= tolV, (int(np.argmax(eV)), eV.max())
    assert eG.max() <= tolG, (np.unravel_index(np.argmax(eG), eG.shape), eG.max())
    for name in ("along4", "along6"):                                       # non-vacuity: dV/dUy and dV/dr (channels 5 and 7) move along both families on the device
        for k in (4, 6):
            col = Gg[fam[name]][:, k]
            assert len(np.unique(col)) == 16 and np.ptp(col) > 1e-3, (name, k, col)


def _check_rows(pkg, oracle_mod, skidpad, precision):
    """The flow of test_constraint_rows_and_solve_with_hji (fp64) and of test_f32_with_hji_constraint (fp32), with their bars, at B = 48 on the live grid."""
    knots, V, g = lc.live_grid()
    f32 = precision == "f32"
    state, control, t0, toff, other = lc.constraint_inputs(pkg, skidpad)
    B = state.shape[0]
    if f32:
        state, control = f32_round(state), f32_round(control)
        other = f32_round(pkg.synthetic.other_cars(state, seed=5))
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, precision=precision, hji_eps=10.0)      # large eps so that most rows are active
    mpc.set_hji_cache(knots, V, g)
    orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(knots, V, g); orc.set_hji_eps(10.0)
    u, status, iters = mpc.step_(state, control, t0, other_car_state=other, time_offset=toff)
    M, b, Vv = mpc.hji_constraint()
    tolV, tolM = (2e-5, 2e-3) if f32 else (1e-12, 1e-9)
    nact = 0
    worst = np.zeros(3)
    for i in range(B):
        Mo, bo, Vo = orc.hji_constraint(state[i], other[i], control[i])
        Mo = Mo * orc.u_norm                                                     # coupled_lat_long.jl:345
        if math.isinf(Vo):
            assert math.isinf(Vv[i]) and np.all(M[i] == 0) and b[i] == 1.0
            continue
        if f32 and math.isinf(Vv[i]):                                            # (a query within float rounding of the grid boundary may fall on the other side)
            continue
        assert math.isfinite(Vv[i]), i
        if Vo <= 10.0:
            nact += 1
        e = (abs(Vv[i] - Vo) / max(1, abs(Vo)), np.max(np.abs(M[i] - Mo)) / max(1.0, np.max(np.abs(Mo))), abs(b[i] - bo) / max(1.0, abs(bo)))
        worst = np.maximum(worst, e)
        assert e[0] <= tolV and e[1] <= tolM and e[2] <= tolM, (i, e)
    print(f"live safety row {precision}: {nact} active of {B}, worst relative errors V {worst[0]:.3e}, M {worst[1]:.3e}, b {worst[2]:.3e}")
    assert nact >= 24                                                            # (test_hji_live_host: in all of them the steering coefficient comes mostly through dV/dUy, dV/dr)
    return mpc, orc, status


def test_constraint_rows_and_solve_on_the_live_grid(pkg, oracle_mod, skidpad):
    """k_hji_constraint with g[4] d(dUy)/d(delta) + g[6] d(dr)/d(delta) live (on synthetic.hji_grid both are multiplied by zero), then the full solve against the exact
    optimum of the same QP."""
    mpc, orc, status = _check_rows(pkg, oracle_mod, skidpad, "f64")
    assert np.all(status == pkg.SOLVED), status
    qp = mpc.qp_data(); x, sg = mpc.solution()
    worst = max(float(np.max(np.abs(x[i, 1, 6:] - orc.split_x(orc.solve_exact(qp[i])[0])["u"][1]))) for i in range(x.shape[0]))
    assert worst < 1e-6, worst
    mpc.close()


def test_f32_constraint_rows_and_solve_on_the_live_grid(pkg, oracle_mod, skidpad):
    """The fp32 library on the same rows, in the manner and with the bars of test_f32_with_hji_constraint: V 2e-5, M and b 2e-3, the first control 1e-3 (normalised) from
    the exact optimum of the device's QP."""
    mpc, orc, status = _check_rows(pkg, oracle_mod, skidpad, "f32")
    assert np.all(pkg.is_solved(status)), np.bincount(status)
    qp = mpc.qp_data(); x, sg = mpc.solution()
    worst = max(float(np.max(np.abs(x[i, 1, 6:] - orc.split_x(orc.solve_exact(qp[i])[0])["u"][1]))) for i in range(x.shape[0]))
    assert worst <= 1e-3, worst
    mpc.close()


def test_fallback_policy_on_the_live_grid(pkg, oracle_mod, skidpad):
    """The flow of test_hji_fallback_policy where its two exact assertions can fail: on this grid the oracle steers -delta_max for 10 of the 96 instances and +delta_max
    for 86, the line search ends inside the Fx range for 44 of them, on 16 different candidates (synthetic.hji_grid: +delta_max and candidate 49, 96 times).
    Steer sign and winning index equal the oracle's, the chosen Fx bit for bit, outside a tie set: |Bc| < 1e-12 (|g[4]|/m + a |g[6]|/Izz) or best two candidates within
    1e-10 relative -- at most 2 of 96 (measured: none); a tied instance must still pick a candidate within 1e-9 relative of the best under the oracle's objective."""
    knots, V, g = lc.live_grid()
    eps = 0.5
    state, control, t0, toff, other = lc.policy_inputs(pkg, skidpad)
    B = state.shape[0]
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps)
    mpc.set_hji_cache(knots, V, g)
    orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(knots, V, g); orc.set_hji_eps(eps)
    u_mpc, status, _ = mpc.step_(state, control, t0, other_car_state=other, time_offset=toff)
    assert np.all(status == pkg.SOLVED)
    u_on, src_on, u2 = mpc.get_next_control_hji(True)
    u_off, src_off, _ = mpc.get_next_control_hji(False)
    R = lc.policy_reference(orc, state, other)
    inb, win, fx_grid = R["inb"], R["win"], R["fx_grid"]
    # non-vacuity, on the oracle's answers
    assert np.sum(R["u2"][inb, 0] < 0) >= 8 and np.sum(R["u2"][inb, 0] > 0) >= 8
    assert np.sum((win[inb] > 0) & (win[inb] < 49)) >= 24 and len(set(win[inb].tolist())) >= 8
    assert R["tie"].sum() <= lc.TIE_CAP
    P = mpc.vehicle
    assert np.array_equal(fx_grid, np.array([n / 49 * P["Fx_max"] + (1 - n / 49) * P["Fx_min"] for n in range(50)]))
    seen, fx_policy = set(), []
    for i in range(B):
        Vo, u2o = R["V"][i], R["u2"][i]
        unsafe = (not math.isnan(toff[i])) and Vo <= eps
        assert src_on[i] == (1 if unsafe else 0) and src_off[i] == (2 if unsafe else 0), i
        seen.add(int(src_on[i]))
        assert np.array_equal(u_off[i], u_mpc[i])
        if inb[i]:
            j = int(np.argmin(np.abs(fx_grid - u2[i, 1])))
            assert u2[i, 1] == fx_grid[j], i                                                     # a grid point, bit for bit
            if not R["tie"][i]:
                assert u2[i, 0] == u2o[0], (i, R["Bc"][i])                                       # steer sign: exact
                assert j == win[i] and u2[i, 1] == u2o[1], (i, j, win[i])                        # line-search index: exact; the force bit for bit
            else:
                best = R["scores"][i, win[i]]
                assert abs(u2[i, 0]) == P["delta_max"] and R["scores"][i, j] >= best - 1e-9 * abs(best), (i, j, win[i])
        if unsafe:
            Fx = u2[i, 1] if R["tie"][i] else u2o[1]
            fx_policy.append(Fx)
            exp = [u2[i, 0], Fx * (P["fwd_frac"] if Fx > 0 else P["fwb_frac"]), Fx * (P["rwd_frac"] if Fx > 0 else P["rwb_frac"])]
            assert np.allclose(u_on[i], exp, rtol=0, atol=1e-12 * max(1.0, abs(Fx))), i
        else:
            assert np.array_equal(u_on[i], u_mpc[i])
    assert seen == {0, 1}, seen                                      # both outcomes exercised
    fx_policy = np.array(fx_policy)
    assert np.sum(fx_policy > 0) >= 3 and np.sum(fx_policy < 0) >= 3, fx_policy                  # the policy both drives and brakes (measured 9 / 5)
    mpc.close()
