"""GPU tests of the safety rollout (pg_simulate_safety_dev / pg_get_safety_state): simulate (model_predictive_control.jl:80-100) with the control the ROS node sends
(ros_integration.jl:114-124) fed back, against an other car that moves -- held, worst case (optimal_disturbance, HJI_computation.jl:90-131) or scripted."""
import math

import numpy as np
import pytest

from conftest import make_oracle
import hji_live_cases as lc
import safety_numpy as sn

pytestmark = pytest.mark.gpu

DT = 0.01


@pytest.fixture(scope="module")
def grid(pkg):
    return pkg.synthetic.hji_grid(dims=(7, 6, 5, 4, 4, 5, 4), seed=11)


@pytest.fixture(scope="module")
def big_grid(pkg):
    return pkg.synthetic.hji_grid_large()


def _policy_control(X, u2):
    Fx = u2[1]
    return [u2[0], Fx * (X["fwd_frac"] if Fx > 0 else X["fwb_frac"]), Fx * (X["rwd_frac"] if Fx > 0 else X["rwb_frac"])]


def oracle_loop(pkg, oracle_mod, skidpad, grid, human, state, control, t0, toff, other, steps, eps, margin):
    """The host loop the rollout is compared with: the oracle's exact solver with the safety row, HJI lookup, optimal_control, RK4 plant and the loop's clock, and the numpy
    other car.  Returns the histories, the final (q, u, other), the clock, the source of every step's control, keep (instances that stay `margin` away from V = eps and
    V = 0 and whose solves all end verified), and for the steps the policy drove its steer sign and whether optimal_control was within rounding of another answer
    (hji_live_cases.is_tie)."""
    B = state.shape[0]
    X = pkg.vehicles.X1()                                                    # the vehicle of the handle (mpc.vehicle)
    orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(*grid); orc.set_hji_eps(eps)
    clock = np.stack([orc.simulate_times(DT, float(skidpad.t[-1]), steps + 1, t_start=float(t0[b])) for b in range(B)], axis=1)
    q, u, ob, tt = state.copy(), control.copy(), other.copy(), t0.copy()
    keep = np.ones(B, bool)
    hist = {k: [] for k in ("state", "control", "other", "V")}
    src = np.zeros((steps, B), dtype=np.int32)
    steer = np.zeros((steps, B)); tie = np.zeros((steps, B), bool)
    for k in range(steps):
        hist["state"].append(q); hist["control"].append(u); hist["other"].append(ob)
        unext, _, it, st, _ = orc.step_batch(q, u, tt, others4=ob, time_offsets=toff, solver=0)
        x7 = np.stack([orc.hji_relative_state(q[b], ob[b]) for b in range(B)])
        look = [orc.hji_lookup(x7[b]) for b in range(B)]
        V = np.array([l[0] for l in look]); G = np.stack([l[1] for l in look])
        hist["V"].append(V)
        keep &= ~((np.abs(V - eps) < margin) | (np.abs(V) < margin)) & (st == pkg.SOLVED)
        for b in np.nonzero(V <= eps)[0]:                                    # trajectory mode, policy on
            _, u2, Bc, scores = orc.hji_optimal_control_detail(q[b], ob[b])
            unext[b] = _policy_control(X, u2); src[k, b] = 1
            steer[k, b] = np.sign(u2[0]); tie[k, b] = lc.is_tie(X, G[b], Bc, scores)
        hu = sn.optimal_disturbance(X, x7, G) if human == "worst" else np.zeros((B, 2))
        q = np.stack([orc.plant_step(q[b], u[b], DT) for b in range(B)])
        ob = sn.other_car_step(ob, hu, DT)
        u = unext; tt = clock[k + 1]
    un = np.array([orc.u_norm[0], orc.u_norm[1], orc.u_norm[1]])
    return dict(hist=hist, final=(q, u, ob), clock=clock, src=src, keep=keep, steer=steer, tie=tie, un=un)


def _rollout_against_the_oracle_loop(pkg, oracle_mod, skidpad, grid, human, last_step=None):
    """The body of test_rollout_matches_an_oracle_loop.  last_step(oracle loop) -> the last step index that is compared (None: all steps and the final state)."""
    B, steps, eps, margin = 32, 40, 1.0, 1e-3
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=41)
    other = pkg.synthetic.other_cars(state, seed=43)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps)
    mpc.set_hji_cache(*grid)
    mpc.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    parts, dev_st = [], []
    for k in range(steps):                                                  # step by step (a continued rollout is the same bits): the solver's status of every step
        parts.append(mpc.simulate_safety_(1, dt=DT, use_HJI_policy=True, human=human, record=True))
        dev_st.append(mpc.solve_info()[0])
    s, c, t, o = parts[-1][:4]
    H = {key: np.concatenate([p[4][key] for p in parts]) for key in parts[0][4]}
    dev_st = np.array(dev_st)
    L = oracle_loop(pkg, oracle_mod, skidpad, grid, human, state, control, t0, toff, other, steps, eps, margin)
    hist, (q, u, ob), clock, src, keep, un = L["hist"], L["final"], L["clock"], L["src"], L["keep"], L["un"]
    last = steps if last_step is None else last_step(L)
    keep &= np.all(dev_st == pkg.SOLVED, axis=0)
    assert keep.sum() >= B * 3 // 4, (keep.sum(), dev_st)
    # per instance, the largest deviation from the oracle loop over all steps (states, other car, V: relative; controls: normalised)
    rel = lambda a, b: np.abs(a - b) / np.maximum(1.0, np.abs(b))
    dev = np.zeros(B)
    for k in range(last + 1):
        if k < steps:
            dq, du = H["state"][k], H["control"][k]; do = H["other"][k]
            Vd, Vo = H["V"][k], hist["V"][k]
            assert np.array_equal(np.isfinite(Vd)[keep], np.isfinite(Vo)[keep]) and np.all(Vd[keep & ~np.isfinite(Vo)] == np.inf), k
            fin = np.isfinite(Vo) & np.isfinite(Vd)
            dev = np.maximum(dev, np.where(fin, rel(np.where(fin, Vd, 0.0), np.where(fin, Vo, 0.0)), 0.0))
            assert np.array_equal(H["source"][k][keep], src[k][keep]), k
            ref = (hist["state"][k], hist["control"][k], hist["other"][k])
        else:
            dq, du, do = s, c, o
            ref = (q, u, ob)
        dev = np.maximum(dev, rel(dq, ref[0]).max(axis=1))
        dev = np.maximum(dev, (np.abs(du - ref[1]) / un).max(axis=1))
        dev = np.maximum(dev, rel(do, ref[2]).max(axis=1))
    # every kept instance but at most one follows the oracle loop to 1e-5 (observed: one instance of the 32 whose applied control differs by 7.5e-5 (normalised) from step 3 on,
    # both solvers reporting a verified optimum at every step)
    off = np.nonzero(keep & (dev >= 1e-5))[0]
    assert len(off) <= 1, (off, dev[off])
    keep[off] = False
    assert np.array_equal(t, clock[steps])
    pol = (H["source"] == 1).any(axis=0)
    assert (pol & keep).sum() >= 3 and (~pol & keep).sum() >= 3, ((pol & keep).sum(), (~pol & keep).sum())
    if human == "worst":
        assert np.any(H["human"] != 0.0)
    else:
        assert np.all(H["human"] == 0.0)
    return H, L, keep, last


@pytest.mark.parametrize("human", ["hold", "worst"])
def test_rollout_matches_an_oracle_loop(pkg, oracle_mod, skidpad, grid, human):
    """40 steps x 32 instances against a host loop built from the oracle (exact solver with the safety row, HJI lookup, optimal_control, RK4 plant, the loop's clock) and
    the numpy other car.  The selection is discontinuous at V = eps and the breach at V = 0: instances whose oracle V comes within 1e-3 of either are left out, and so are
    instances that either solver did not end at a verified optimum at some step (PG_SOLVED; an unverified interior-point answer is 1e-5-close, not 1e-9-close)."""
    _rollout_against_the_oracle_loop(pkg, oracle_mod, skidpad, grid, human)


def live_last_step(L):
    """The last step of the live-grid rollout that is compared: the first one at which the policy drives an instance whose optimal_control is within rounding of another
    answer (the tie set of test_gpu_hji_live.test_fallback_policy_on_the_live_grid: a bang-bang steer that flips there sends the two loops apart for good); all of them when
    there is none.  It must not come before step 3."""
    hit = np.nonzero((L["tie"] & (L["src"] == 1)).any(axis=1))[0]
    last = int(hit[0]) if len(hit) else L["src"].shape[0]
    assert last >= 3, last
    return last


def test_rollout_matches_an_oracle_loop_on_the_live_grid(pkg, oracle_mod, skidpad):
    """The same comparison, same batch, steps and bars, worst-case human, on hji_live_cases.live_grid: dV/dUy and dV/dr are live, so the policy's steer takes both signs
    (one instance changes sign on the way, at the same step on both sides); the human's optimal_disturbance sees a gradient that depends on every coordinate.  Compared
    up to live_last_step (here: every step, no policy-driven step of the oracle loop is in the tie set)."""
    H, L, keep, last = _rollout_against_the_oracle_loop(pkg, oracle_mod, skidpad, lc.live_grid(), "worst", last_step=live_last_step)
    # the steer the policy handed over at step k is the control at the start of step k + 1
    drove = (H["source"][:last - 1] == 1) & keep[None]
    steer = H["control"][1:last][..., 0][drove]
    assert np.sum(steer > 0) >= 3 and np.sum(steer < 0) >= 3, (np.sum(steer > 0), np.sum(steer < 0))
    assert np.array_equal(np.sign(steer), L["steer"][:last - 1][drove])


def test_reduces_to_the_existing_loop_bit_for_bit(pkg, skidpad):
    """Other car at speed 0, held, policy off, no grid: the state and control histories are those of pg_simulate_dev, bit for bit, at B = 4096 where the cold step takes the
    pipelined nodes + update_QP launch (counted by both handles)."""
    B, steps = 4096, 6
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=2024)
    other = pkg.synthetic.other_cars(state, seed=5); other[:, 3] = 0.0
    a = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, phase_timing=False)
    a.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    sa, ca, ta, qa, ua = a.simulate_(steps, record=True)
    b = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, phase_timing=False)
    b.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    sb, cb, tb, ob, H = b.simulate_safety_(steps, use_HJI_policy=False, human="hold", record=True)
    assert a.get_option("stat_pipelined_launches") >= 1 and b.get_option("stat_pipelined_launches") == a.get_option("stat_pipelined_launches")
    assert np.array_equal(H["state"], qa) and np.array_equal(H["control"], ua)
    assert np.array_equal(sb, sa) and np.array_equal(cb, ca) and np.array_equal(tb, ta)
    assert np.array_equal(ob, other) and np.all(H["other"] == other[None])
    assert np.all(H["V"] == np.inf) and np.all(H["source"] == 0) and np.all(H["human"] == 0.0)
    vmin, fb, ps = b.safety_summary()
    assert np.all(vmin == np.inf) and np.all(fb == -1) and np.all(ps == 0)
    a.close(); b.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("use_policy", [True, False])
def test_selection_equals_the_one_step_call(pkg, skidpad, grid, precision, use_policy):
    """A rollout step applies exactly what pg_step + pg_get_next_control_hji return for the same inputs: the same source and the same bits of the control."""
    B, eps = 96, 0.5
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=33)
    toff[::5] = np.nan                                                      # path-tracking mode never hands over
    other = pkg.synthetic.other_cars(state, seed=9)
    one = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps, precision=precision)
    one.set_hji_cache(*grid)
    one.step_(state, control, t0, other_car_state=other, time_offset=toff)
    u1, src1, _ = one.get_next_control_hji(use_policy)
    ro = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps, precision=precision)
    ro.set_hji_cache(*grid)
    ro.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    s, c, t, o, H = ro.simulate_safety_(1, use_HJI_policy=use_policy, human="worst", record=True)
    assert np.array_equal(H["source"][0], src1)
    assert np.array_equal(c, u1)
    assert set(np.unique(src1).tolist()) == ({0, 1} if use_policy else {0, 2})
    one.close(); ro.close()


def test_scripted_human(pkg, skidpad, grid):
    """human = "script": the other car is the numpy RK4 of the script (1e-12), the human history is the script, and V is the lookup at the relative states formed from the
    recorded histories (1e-12)."""
    B, steps, eps = 64, 15, 1.0
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=7)
    other = pkg.synthetic.other_cars(state, seed=8)
    rng = np.random.default_rng(3)
    hu = np.stack([rng.uniform(-0.5, 0.5, (steps, B)), rng.uniform(-3.0, 3.0, (steps, B))], axis=2)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps)
    mpc.set_hji_cache(*grid)
    mpc.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    s, c, t, o, H = mpc.simulate_safety_(steps, human="script", human_u=hu, record=True)
    assert np.array_equal(H["human"], hu)
    assert np.array_equal(H["other"][0], other)
    rel = lambda a, b: np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    for k in range(steps):
        nxt = sn.other_car_step(H["other"][k], hu[k], DT)
        assert rel(H["other"][k + 1] if k + 1 < steps else o, nxt) < 1e-12, k
        V, _ = mpc.hji_lookup(sn.relative_state(H["state"][k], H["other"][k]))
        fin = np.isfinite(V)
        assert np.array_equal(np.isfinite(H["V"][k]), fin), k
        assert np.all(np.abs(H["V"][k][fin] - V[fin]) <= 1e-12 * np.maximum(1.0, np.abs(V[fin]))), k
    assert fin.sum() > B // 4
    mpc.close()


def _summary_of(H):
    V = H["V"]
    vmin = V.min(axis=0)
    br = V <= 0.0
    fb = np.where(br.any(axis=0), br.argmax(axis=0), -1)
    return vmin, fb, (H["source"] == 1).sum(axis=0)


def test_summary_and_continuation(pkg, skidpad, grid):
    """10 + 20 steps give the bits of 30 steps (histories and summary); the summary is the one the histories imply; pg_set_inputs restarts it and the step index."""
    B, eps = 64, 1.0
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=41)
    other = pkg.synthetic.other_cars(state, seed=43)
    runs = []
    for split in ((30,), (10, 20)):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps)
        m.set_hji_cache(*grid)
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        parts = [m.simulate_safety_(n, human="worst", record=True) for n in split]
        H = {k: np.concatenate([p[4][k] for p in parts]) for k in parts[0][4]}
        runs.append((parts[-1][:4], H, m.safety_summary(), m))
    (fin30, H30, sum30, m30), (fin12, H12, sum12, m12) = runs
    for a, b in zip(fin30, fin12):
        assert np.array_equal(a, b)
    for k in H30:
        assert np.array_equal(H30[k], H12[k]), k
    for a, b in zip(sum30, sum12):
        assert np.array_equal(a, b)
    for a, b in zip(sum30, _summary_of(H30)):
        assert np.array_equal(a, b)
    assert np.any(sum30[1] >= 0) and np.any(sum30[1] == -1) and np.any(sum30[2] > 0)
    # a restart: new inputs, new clock, new summary (the step index starts at 0 again)
    m30.reset()
    m30.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    vmin, fb, ps = m30.safety_summary()
    assert np.all(vmin == np.inf) and np.all(fb == -1) and np.all(ps == 0)
    *_, H5 = m30.simulate_safety_(5, human="worst", record=True)
    assert np.array_equal(H5["state"][0], state) and np.array_equal(H5["other"][0], other)
    after = m30.safety_summary()
    for a, b in zip(after, _summary_of(H5)):
        assert np.array_equal(a, b)
    assert np.all(after[1] < 5) and np.any(after[1] >= 0)
    m30.close(); m12.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rollout_is_reproducible_bit_for_bit(pkg, skidpad, big_grid, precision):
    """The config 3 shape (B = 4096, the full-size synthetic grid, other cars, worst-case human, policy on), 30 steps on two handles: the same bits, histories and summary
    included."""
    B = 4096
    grid = big_grid
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=12345)
    other = pkg.synthetic.other_cars(state, seed=777)
    runs = []
    for rep in range(2):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, precision=precision, phase_timing=False)
        m.set_hji_cache(*grid)
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        s, c, t, o, H = m.simulate_safety_(30, human="worst", record=True)
        st, it, act, mu = m.solve_info()
        runs.append([s, c, t, o, st, it, act] + [H[k] for k in sorted(H)] + list(m.safety_summary()))
        m.close()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    src = runs[0][7 + sorted(H).index("source")]
    assert np.any(src == 1) and np.any(src == 0)


def test_refusals(pkg, skidpad):
    B = 8
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=1)
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    m.set_inputs(state, control, t0, time_offset=toff)
    f = lambda steps, dt, mode, hu=None: m.lib.pg_simulate_safety_dev(m.h, steps, __import__("ctypes").c_double(dt), 1, mode, hu, None, None, None, None, None, None)
    assert f(1, DT, 3) == -2 and f(1, DT, -1) == -2                         # PG_ERR_INVALID
    assert f(1, DT, 2) == -2                                                # scripted without a script
    assert f(0, DT, 0) == -2 and f(1, 0.0, 0) == -2 and f(1, -DT, 0) == -2
    with pytest.raises(ValueError):
        m.simulate_safety_(1, human="script")
    s, c, t, o = m.simulate_safety_(1)                                       # and the handle still works
    assert np.all(np.isfinite(s))
    m.close()
    d = pkg.DecoupledTrajectoryTrackingMPC(pkg.X1(), skidpad, B)
    d.set_inputs(state, control, t0, time_offset=toff)
    assert d.lib.pg_simulate_safety_dev(d.h, 1, __import__("ctypes").c_double(DT), 1, 0, None, None, None, None, None, None, None) == -4   # PG_ERR_STATE
    with pytest.raises(pkg.PigeonError):
        d.simulate_safety_(1)
    d.close()
