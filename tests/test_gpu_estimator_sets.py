"""GPU tests of the estimator sets (pg_set_estimator_sets / pg_set_estimator_index): a fixed-gain observer between the sensor and the controller of the three device
rollouts.

Four estimators -- the identity; gain 0.2 with the controller's model as the prior; gain 0.5 as a plain low-pass; gains (1, 1, 0.2, 0.2, 0, 0.2) with the model -- spread
over the instances by b % 4 (tests/estimator_numpy.py, which tests/test_estimator_host.py pins to closed forms).  Relative differences are |got - ref| / max(1, |ref|) per
component; the bars are 1e-9 in fp64 and 2e-5 in the fp32 library, as in test_gpu_plant_sets.py.  The smallest shapes at which the code can go wrong: B = 70 (a full
wavefront and a ragged one) and 12 steps, split 5 + 7.  Every comparison with the twin is ONE step: the twin's step k starts from the device's estimate of step k - 1."""
import ctypes as C

import numpy as np
import pytest

import actuator_numpy
import disturbance_numpy
import estimator_numpy as en
import node_numpy as nn
import plant_numpy
import sensor_numpy
from conftest import make_oracle
from rollout_libs import NOISE_SEED, inputs, join, make, narrowed, numpy_summary, rel, rollout, start, stream_ids

pytestmark = pytest.mark.gpu

BAR = {"f64": 1e-9, "f32": 2e-5}
DT = 0.01
SETS = en.four_estimators()
SENSORS = sensor_numpy.four_sensors()
KINDS = [("simulate", "coupled"), ("simulate", "decoupled"), ("safety", "coupled"), ("node", "coupled"), ("node", "decoupled")]
DTYPE = {"f64": np.float64, "f32": np.float32}


def check_estimates(r, precision, idx, P, what="", moved_min=0.9):
    """item 2's identity: row k of the estimated history is ONE step of the twin from row k - 1 of it, row k of what the sensor gave and row k - 1 of the control history;
    row 0 and every channel with gain 1 are the sensor's output bit for bit"""
    y = r["measured"] if r["measured"] is not None else r["state"]
    est, u = r["estimated"], r["control"]
    B = est.shape[1]
    g, _ = en.gains(SETS, idx, B)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert np.array_equal(bits(est[0]), bits(y[0]))
    assert np.array_equal(bits(est[:, g == 1.0]), bits(y[:, g == 1.0]))
    worst = 0.0
    for k in range(1, est.shape[0]):
        want = en.step(SETS, idx, est[k - 1], y[k], u[k - 1], DT, P, dtype=DTYPE[precision])
        err = np.where(np.isnan(est[k]) & np.isnan(want), 0.0, rel(est[k], want))      # (a NaN the sensor handed over is a NaN on both sides)
        worst = max(worst, float(err.max()))
        assert err.max() <= BAR[precision], (what, precision, k, int(np.argmax(err.max(axis=1))), float(err.max()))
    moved = float(np.mean(est[1:, g != 1.0] != y[1:, g != 1.0]))
    print(f"{what} {precision}: max |estimate - one twin step| = {worst:.2e} (bar {BAR[precision]:g}); the filtered channels differ from the sensor's output on {moved:.0%} of the entries")
    assert moved >= moved_min
    return worst


# ---- 1: the law alone ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_response_equals_the_twin(pkg, skidpad, precision):
    B, steps = 70, 12
    idx = (np.arange(B) % 4).astype(np.int32)
    m = make(pkg, skidpad, B, precision=precision)
    st = start(m, inputs(pkg, skidpad, B))
    m.set_estimators(SETS, idx)
    P = pkg.X1()
    x = np.empty((steps, B, 6)); x[0] = st[0]
    for k in range(1, steps):
        x[k] = plant_numpy.plant_step_vec(P, x[k - 1], st[1], DT)
    rng = np.random.default_rng(11)
    y = (x + SENSORS[1][0] * rng.standard_normal(x.shape)).astype(DTYPE[precision]).astype(np.float64)
    u = (st[1][None] + 0.01 * rng.standard_normal((steps, B, 3)) * np.array([1.0, 100.0, 100.0])).astype(DTYPE[precision]).astype(np.float64)
    y[3, 4, 1] = -0.0; y[5, 8, 0] = np.nan                   # an identity lane and a copied channel: both survive
    got = m.estimator_response(y, u, DT)
    check_estimates(dict(measured=y, state=None, estimated=got, control=u), precision, idx, P, "pg_estimator_response")
    assert np.signbit(got[3, 4, 1]) and np.isnan(got[5, 8, 0])
    # a non-finite prior restarts that instance alone: the control of step 6 is NaN for instance 1 (gain 0.2, model) -> its estimate of step 7 is the measurement
    bad = u.copy(); bad[6, 1, 0] = np.nan
    got2 = m.estimator_response(y, bad, DT)
    assert np.array_equal(got2[7, 1], y[7, 1]) and np.array_equal(got2[:7], got[:7], equal_nan=True)
    others = np.arange(B) != 1
    assert np.array_equal(got2[:, others], got[:, others], equal_nan=True) and np.all(np.isfinite(got2[8:, 1]))
    assert m.get_option("stat_estimator_steps") == 0
    with pytest.raises(pkg.PigeonError):
        m.estimated_state()                                  # PG_ERR_STATE: the response is no rollout step
    m.close()


# ---- 2, 3: the estimate follows the law in every rollout; the plant moves the true state ---------------------------------------------------------------------------------
_runs = {}


def filtered_run(pkg, traj, kind, formulation, precision, sensor=True):
    """the reference rollout of items 2-4, computed once per case: B = 70, four estimators by b % 4, the noisy sensor for everyone, 12 steps as 5 + 7"""
    key = (kind, formulation, precision, sensor)
    if key not in _runs:
        B = 70
        idx = (np.arange(B) % 4).astype(np.int32)
        m = make(pkg, traj, B, formulation, precision)
        st = start(m, inputs(pkg, traj, B), others=kind != "simulate")
        if sensor:
            m.set_sensors([SENSORS[1]], None, seed=NOISE_SEED, streams=stream_ids(B))
        m.set_estimators(SETS, idx)
        a = rollout(m, kind, 5, DT, measured=sensor, estimated=True)
        last5 = m.estimated_state()
        b = rollout(m, kind, 7, DT, measured=sensor, estimated=True)
        r = join([a, b])
        r.update(idx=idx, last5=last5, last=m.estimated_state(), est_steps=m.get_option("stat_estimator_steps"), clock=m.simulate_clock(12, st[2], DT), inputs=st)
        m.close()
        # the same twelve steps in one call
        m = make(pkg, traj, B, formulation, precision)
        start(m, inputs(pkg, traj, B), others=kind != "simulate")
        if sensor:
            m.set_sensors([SENSORS[1]], None, seed=NOISE_SEED, streams=stream_ids(B))
        m.set_estimators(SETS, idx)
        r["whole"] = rollout(m, kind, 12, DT, measured=sensor, estimated=True)
        m.close()
        _runs[key] = r
    return _runs[key]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind,formulation", KINDS)
def test_the_estimate_is_one_twin_step_from_the_histories(pkg, skidpad, kind, formulation, precision):
    r = filtered_run(pkg, skidpad, kind, formulation, precision)
    assert r["estimated"].shape == (12, 70, 6) and r["est_steps"] == 12
    # (node rollout: the applied command of the history is the message the compute calls read -- k_node_finish writes both, and leaves both alone for a gated-out instance)
    check_estimates(r, precision, r["idx"], pkg.X1(), f"{kind} {formulation}")
    assert np.array_equal(r["last5"], r["estimated"][4]) and np.array_equal(r["last"], r["estimated"][11])      # pg_get_estimated_state: the last row of each call
    for k in ("state", "control", "final_state", "measured", "estimated"):
        assert np.array_equal(r[k], r["whole"][k]), k         # 5 + 7 = 12, bit for bit


def test_the_estimate_filters_the_true_state_without_a_sensor_library(pkg, skidpad):
    r = filtered_run(pkg, skidpad, "simulate", "coupled", "f64", sensor=False)
    assert r["measured"] is None and r["est_steps"] == 12
    # (an exact model on an exact measurement predicts what it is shown: only the low-pass set, which has no model, must leave the truth)
    check_estimates(r, "f64", r["idx"], pkg.X1(), "simulate coupled, no sensor library", moved_min=0.0)
    low = r["idx"] == 2
    assert np.all(r["estimated"][1:, low, :2] != r["state"][1:, low, :2])
    assert np.array_equal(r["estimated"], r["whole"]["estimated"]) and np.array_equal(r["last"], r["estimated"][11])


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind,formulation", KINDS)
def test_the_plant_moves_the_true_state(pkg, skidpad, kind, formulation, precision):
    r = filtered_run(pkg, skidpad, kind, formulation, precision)
    P = pkg.X1(); bar = BAR[precision]; idx = r["idx"]
    qh, uh, eh = r["state"], r["control"], r["estimated"]
    worst = 0.0; apart = np.zeros(70)
    for k in range(12):
        nxt = qh[k + 1] if k + 1 < 12 else r["final_state"]
        err = rel(nxt, plant_numpy.plant_step_vec(P, qh[k], uh[k], DT))
        worst = max(worst, float(err.max()))
        assert err.max() < bar, (kind, formulation, precision, k, int(np.argmax(err.max(axis=1))), float(err.max()))
        apart = np.maximum(apart, rel(nxt, plant_numpy.plant_step_vec(P, eh[k], uh[k], DT)).max(axis=1))
    share = float(np.mean(apart > 100 * bar))
    print(f"{kind} {formulation} {precision}: worst |state - numpy plant from the true state| = {worst:.2e} (bar {bar:g}); "
          f"replay from the estimate misses 100 bars on {share:.0%} of the instances")
    if precision == "f64":                                   # (noise of 5 cm / 0.1 m/s against 1e-7: a plant that integrated the estimate is far off)
        assert share >= 0.9, share


# ---- 4: the controller sees the estimate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("formulation", ["coupled", "decoupled"])
def test_the_controller_sees_the_estimate(pkg, skidpad, formulation):
    """A handle without a library, driven from the host with step_(estimated_hist[k], control_hist[k], clock[k]), computes the control the filtered rollout recorded at
    step k + 1 (the yardstick itself -- the replay of a rollout without a library -- is pinned in test_gpu_sensor_sets.py)."""
    B, steps = 70, 12
    r = filtered_run(pkg, skidpad, "simulate", formulation, "f64")
    idx = r["idx"]; clock = r["clock"]; toff = r["inputs"][3]

    def replay(states):
        h = make(pkg, skidpad, B, formulation)
        us = [h.step_(states[k], r["control"][k], clock[k], time_offset=toff)[0] for k in range(steps - 1)]
        h.close()
        return np.stack(us)
    ue = replay(r["estimated"])
    print(f"{formulation}: replay from the estimates: bit-equal {np.array_equal(ue, r['control'][1:])}, max relative difference {rel(ue, r['control'][1:]).max():.2e}")
    assert np.array_equal(ue, r["control"][1:])
    # not vacuous: neither the measured nor the true states give these controls (the identity set reads the measurement)
    for name in ("measured", "state"):
        off = rel(replay(r[name]), r["control"][1:]).max(axis=(0, 2))
        share = float(np.mean(off[idx != 0] > 1e-6))
        print(f"{formulation}: replay from the {name} history differs by > 1e-6 on {share:.0%} of the instances of sets 2-4")
        assert share >= 0.5
        if name == "measured":
            assert np.all(off[idx == 0] == 0.0) if formulation == "coupled" else np.all(off[idx == 0] < 1e-6)


# ---- 5: nothing changes under the identity set -------------------------------------------------------------------------------------------------------------------------
def histories(pkg, traj, kind, precision, est, others, B=256, steps=8):
    idx = (np.arange(B) % 4).astype(np.int32)
    m = make(pkg, traj, B, precision=precision)
    m.set_option("tracking_summary", 1)
    start(m, inputs(pkg, traj, B), others=kind != "simulate")
    if others:
        m.set_sensors(SENSORS, idx, seed=NOISE_SEED, streams=stream_ids(B))
        m.set_disturbances(disturbance_numpy.four_disturbances(), idx, seed=NOISE_SEED + 1)
        if kind != "node":
            acts = actuator_numpy.six_sets()
            m.set_actuators(acts, (np.arange(B) % len(acts)).astype(np.int32))
    if est is not None:
        m.set_estimators(est, None)
    r = rollout(m, kind, steps, DT, measured=others, estimated=est is not None)
    out = [r["state"], r["control"], r["final_state"]] + [np.asarray(x) for x in m.solve_info()[:3]] + [np.asarray(x) for x in m.tracking_summary()]
    if others:
        out.append(r["measured"])
    if kind != "simulate":
        out += [np.asarray(x) for x in m.safety_summary()]
    if kind == "node":
        out += [r["event"]] + [np.asarray(x) for x in m.node_summary()]
    stat = m.get_option("stat_estimator_steps")
    est_hist = r["estimated"]
    seen = r["measured"] if others else r["state"]
    m.close()
    return out, stat, est_hist, seen


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("others", [False, True])
@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_nothing_changes_under_the_identity_set(pkg, skidpad, kind, others, precision):
    none, s_none, _, _ = histories(pkg, skidpad, kind, precision, None, others)
    assert s_none == 0                                       # a handle that never saw a library
    for pred in (1, 0):
        one, s_one, est, seen = histories(pkg, skidpad, kind, precision, [en.identity(predict=pred)], others)
        assert s_one == 8
        for j, (a, b) in enumerate(zip(none, one)):
            assert np.array_equal(a, b, equal_nan=True), (kind, others, precision, pred, j)
        assert np.array_equal(est.view(np.uint64), seen.view(np.uint64))      # the estimate IS what the sensor gave
    if not others:
        filt, _, _, _ = histories(pkg, skidpad, kind, precision, [SETS[2]], others)
        assert not np.array_equal(filt[2], none[2])          # the other sets are not cosmetic


# ---- 6: the summaries describe the truth (the launch_track condition: an estimator library and NO sensor library) ---------------------------------------------------------
@pytest.mark.parametrize("kind,precision", [("simulate", "f64"), ("simulate", "f32"), ("node", "f64")])
def test_the_summaries_describe_the_truth(pkg, oracle_mod, skidpad, kind, precision):
    B, steps = 70, 12
    bar = BAR[precision]
    idx = (np.arange(B) % 4).astype(np.int32)
    pidx = ((np.arange(B) // 4) % 4).astype(np.int32)
    tube = narrowed(pkg, skidpad)
    orc = make_oracle(oracle_mod, tube if precision == "f64" else pkg.TrajectoryTube(*tube.data.astype(np.float32).astype(np.float64)))
    m = make(pkg, tube, B, precision=precision)
    m.set_option("tracking_summary", 1)
    start(m, inputs(pkg, tube, B), others=kind != "simulate")
    m.set_plants(plant_numpy.four_plants(pkg.X1), pidx)
    m.set_estimators(SETS, idx)
    a = rollout(m, kind, 5, DT, estimated=True); b = rollout(m, kind, 7, DT, estimated=True)
    r = join([a, b])
    sm, n, fx = m.tracking_summary()
    (wsm, wn, wfx, margin), _, _ = numpy_summary([orc], None, r["state"])
    assert np.array_equal(n, wn) and np.all(n == steps)
    err = rel(sm, wsm)
    print(f"{kind} {precision}: tracking summary vs numpy on the TRUE history: {err.max():.2e} (bar {bar:g})")
    assert err.max() < bar, (err.max(axis=0), bar)
    decided = margin > 1e-6
    assert np.mean(~decided) <= 1 / 8 and np.array_equal(fx[decided], wfx[decided])
    # the estimate really left the truth: the low-pass set (gain 0.5, no model) trails the car by v dt (1 - g) / g, a decimetre at 10 m/s
    (msm, _, _, _), ms, me = numpy_summary([orc], None, r["estimated"])
    off = rel(sm, msm).max(axis=1)
    lag = np.linalg.norm(r["estimated"][-1, :, :2] - r["state"][-1, :, :2], axis=1)
    print(f"{kind} {precision}: the summary of the ESTIMATED history is off by > 100 bars on {np.mean(off[idx == 2] > 100 * bar):.0%} of the low-pass instances; "
          f"their estimate trails the truth by {lag[idx == 2].min():.3f} .. {lag[idx == 2].max():.3f} m")
    assert np.all(lag[idx == 2] > 1e-3) and np.all(off[idx == 0] < bar)
    if precision == "f64":
        assert np.mean(off[idx == 2] > 100 * bar) >= 0.9
    # the step's own projection -- the (s, e) a node step publishes -- is the estimate's
    sep = m.path_coordinates(); s_dev = sep[:, 0]
    assert rel(s_dev, ms[-1]).max() < max(bar, 1e-7)
    m.close()


# ---- 7: the gates read the estimate ------------------------------------------------------------------------------------------------------------------------------------
def test_the_gates_read_the_estimate(pkg, skidpad):
    """True Ux 1.02 m/s.  The first measurement is biased to 0.90 (a sensor set replaced by the exact one after one step: installing resets nothing), and a gain of 0.05 on
    Ux without the model holds the estimate below 1 m/s -- 1.02 - 0.12 x 0.95^k -- for the next five steps, while truth and measurement would let the instance run."""
    B, steps = 70, 5
    slow = 3
    state, control, t0, toff, other = inputs(pkg, skidpad, B)
    state = state.copy(); control = control.copy()
    state[slow, 3] = 1.02; state[slow, 4:6] = 0.0; control[slow] = 0.0
    biased = [SENSORS[0], (np.zeros(6), np.array([0, 0, 0, -0.12, 0, 0.0]))]
    sidx = np.zeros(B, dtype=np.int32); sidx[slow] = 1
    est = [en.identity(), en.identity(gain=[1, 1, 1, 0.05, 1, 1], predict=0)]
    eidx = np.zeros(B, dtype=np.int32); eidx[slow] = 1
    res = {}
    for lib in (True, False):
        m = make(pkg, skidpad, B)
        m.set_inputs(state, control, t0, other, toff)
        m.set_sensors(biased, sidx, seed=NOISE_SEED)
        if lib:
            m.set_estimators(est, eidx)
        first = rollout(m, "node", 1, DT, measured=True, estimated=lib)
        assert first["measured"][0, slow, 3] < 1.0 and first["event"][0, slow] == nn.LOW_SPEED
        m.set_sensors([SENSORS[0]], None, seed=NOISE_SEED)
        x0 = [np.asarray(a)[slow].copy() for a in list(m.solution()) + list(m.solve_info())]
        r = rollout(m, "node", steps, DT, measured=True, estimated=lib)
        assert np.all(r["measured"][:, slow, 3] >= 1.0) and np.all(r["state"][:, slow, 3] >= 1.0)
        if lib:
            assert np.all(r["estimated"][:, slow, 3] < 1.0) and np.all(r["estimated"][:, slow, 3] > 0.9)
        x1 = [np.asarray(a)[slow] for a in list(m.solution()) + list(m.solve_info())]
        _, hb, cn = m.node_summary()
        res[lib] = (r["event"], hb, cn, x0, x1)
        m.close()
    ev, hb, cn, x0, x1 = res[True]
    assert np.all(ev[:, slow] == nn.LOW_SPEED) and hb[slow] == 0 and cn[slow, 2] == steps + 1
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x0, x1))                                  # its solver state: untouched
    ev0, hb0, cn0, _, _ = res[False]
    assert np.all(ev0[:, slow] == 0) and hb0[slow] == steps and cn0[slow, 2] == 1                             # without the library it runs from the second step on
    others = np.arange(B) != slow
    assert np.array_equal(ev[:, others], ev0[:, others])


# ---- 8: filtering in the closed loop -----------------------------------------------------------------------------------------------------------------------------------
def test_the_observer_filters_in_the_closed_loop(pkg, skidpad):
    """The bar of tests/test_estimator_host.py (0.5 on every channel; derived 1/3) with the controller in the loop: gain 0.2 and the model for even b, the identity for odd b."""
    B, steps = 70, 200
    idx = (np.arange(B) % 2 == 0).astype(np.int32)            # set 1 for even b, set 0 (the identity) for odd b
    m = make(pkg, skidpad, B)
    start(m, inputs(pkg, skidpad, B))
    m.set_sensors([SENSORS[1]], None, seed=NOISE_SEED, streams=stream_ids(B))
    m.set_estimators([SETS[0], SETS[1]], idx)
    r = rollout(m, "simulate", steps, DT, measured=True, estimated=True)
    m.close()
    x, y, xh = r["state"][50:], r["measured"][50:], r["estimated"][50:]
    rms = lambda a, sel: np.sqrt(np.mean(a[:, sel] ** 2, axis=(0, 1)))
    even = idx == 1
    ratio = rms(xh - x, even) / rms(y - x, even)
    odd = rms(xh - x, ~even) / rms(y - x, ~even)
    print("closed loop, gain 0.2 with the model: RMS(xh - x) / RMS(y - x) per channel (E, N, psi, Ux, Uy, r) = " + ", ".join(f"{v:.3f}" for v in ratio)
          + "; identity: " + ", ".join(f"{v:.3f}" for v in odd))
    assert np.all(np.isfinite(x))
    assert np.all(ratio < 0.5), ratio
    assert np.array_equal(odd, np.ones(6))


# ---- 9: contract -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_contract(pkg, skidpad):
    B, cap = 70, 80
    idx = (np.arange(B) % 4).astype(np.int32)

    def fresh():
        m = make(pkg, skidpad, cap)
        start(m, inputs(pkg, skidpad, B), others=True)
        return m
    m = fresh()
    with pytest.raises(pkg.PigeonError):
        m.simulate_(1, DT, estimated=True)                   # PG_ERR_STATE: an estimated history without a library
    m.set_estimators(SETS, None)

    def rollouts_refuse():
        assert m.lib.pg_simulate_dev(m.h, 1, C.c_double(DT), None, None) == -4
        assert m.lib.pg_simulate_safety_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None, None) == -4
        assert m.lib.pg_simulate_node_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None) == -4
    rollouts_refuse()                                        # n_sets > 1 and no index
    y = np.zeros((1, B, 6)); u = np.zeros((1, B, 3))
    with pytest.raises(pkg.PigeonError):
        m.estimator_response(y, u, DT)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert m.lib.pg_set_estimator_index(m.h, B - 1, i32(idx)) == 0
    rollouts_refuse()                                        # an index shorter than the batch
    assert m.lib.pg_set_estimator_index(m.h, B, i32(idx)) == 0
    before = m.get_estimators()
    assert len(before[0]) == 4 and np.array_equal(before[1], idx) and before[0] == SETS          # the round trip

    def rejected(rc, *words):
        assert rc == -2
        msg = m.lib.pg_last_error(m.h).decode()
        assert all(w in msg for w in words), (msg, words)
        after = m.get_estimators()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    arr = m.pack_estimators(SETS)
    rejected(m.lib.pg_set_estimator_sets(m.h, 0, arr))
    rejected(m.lib.pg_set_estimator_sets(m.h, -1, arr))
    for c in range(6):
        for bad in (float("nan"), float("inf"), -float("inf"), -1e-9, 1.0 + 1e-9):
            one = m.pack_estimators([SETS[0], SETS[1]]); one[1].gain[c] = bad
            rejected(m.lib.pg_set_estimator_sets(m.h, 2, one), "set 1", f"gain[{c}]")
    for bad in (2, -1):
        one = m.pack_estimators([SETS[1]]); one[0].predict = bad
        rejected(m.lib.pg_set_estimator_sets(m.h, 1, one), "set 0", "predict")
    one = m.pack_estimators(SETS); one[2].reserved = 1
    rejected(m.lib.pg_set_estimator_sets(m.h, 4, one), "set 2", "reserved")
    for bad_idx in (np.where(np.arange(B) == 5, 4, idx), np.where(np.arange(B) == 69, -1, idx)):
        rejected(m.lib.pg_set_estimator_index(m.h, B, i32(bad_idx)))
    rejected(m.lib.pg_set_estimator_index(m.h, 0, i32(idx)))
    rejected(m.lib.pg_set_estimator_index(m.h, cap + 1, i32(np.zeros(cap + 1))))
    with pytest.raises(pkg.PigeonError):
        m.estimated_state()                                  # PG_ERR_STATE: before the first step
    # a rollout call that FAILS consumes the one-shot estimated history too: the successful call behind it writes nothing to that buffer
    import torch
    m.set_estimators(SETS, None)
    buf = torch.full((2, B, 6), -7.0, dtype=torch.float64, device=f"cuda:{m.cfg.device}")
    assert m.lib.pg_set_estimated_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == 0
    rollouts_refuse()
    assert m.lib.pg_set_estimator_index(m.h, B, i32(idx)) == 0
    m.simulate_(2, DT); m.synchronize()
    assert bool((buf == -7.0).all()) and m.get_option("stat_estimator_steps") == 2
    assert m.estimated_state().shape == (B, 6)
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    with pytest.raises(pkg.PigeonError):
        m.estimated_state()                                  # forgotten with the inputs
    m.clear_estimators()
    assert m.get_estimators()[0] == [] and m.lib.pg_set_estimator_index(m.h, B, i32(idx)) == -2
    assert m.lib.pg_set_estimated_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == -4
    m.simulate_(2, DT)
    assert m.get_option("stat_estimator_steps") == 2
    m.close()


def test_step_and_node_step_never_read_the_library(pkg, skidpad):
    B = 70
    state, control, t0, toff, other = inputs(pkg, skidpad, B)
    outs = []
    for lib in (False, True):
        m = make(pkg, skidpad, B)
        if lib:
            m.set_estimators(SETS, None)                     # four sets and NO index: pg_step and pg_node_step_dev do not care
        u = m.step_(state, control, t0, time_offset=toff)
        qp = m.qp_data()
        m.set_inputs(state, control, t0, other, toff)
        m.step_dev()
        m.synchronize()
        u_dev = m.get_next_control()
        node = m.node_step_()
        outs.append(list(u) + [qp, u_dev] + list(node) + [m.get_option("stat_estimator_steps")])
        if lib:
            with pytest.raises(pkg.PigeonError):
                m.estimated_state()
        m.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)
    assert outs[1][-1] == 0


def test_installing_resets_nothing_and_clearing_restarts_the_estimate(pkg, skidpad):
    B = 70
    idx = (np.arange(B) % 4).astype(np.int32)

    def run(between):
        m = make(pkg, skidpad, B)
        st = start(m, inputs(pkg, skidpad, B))
        m.set_sensors([SENSORS[1]], None, seed=NOISE_SEED, streams=stream_ids(B))
        m.set_estimators(SETS, idx)
        rollout(m, "simulate", 4, DT, measured=True, estimated=True)
        if between == "restore":
            m.set_estimators([SETS[3]], None); m.set_estimators(SETS, idx)
        elif between == "clear":
            m.clear_estimators(); m.set_estimators(SETS, idx)
        r = rollout(m, "simulate", 4, DT, measured=True, estimated=True)
        r["t"] = m.simulate_(1, DT)[2]
        clock = m.simulate_clock(10, st[2], DT)
        m.close()
        return r, clock
    twin, clock = run(None)
    back, _ = run("restore")
    for k in ("state", "control", "final_state", "measured", "estimated", "t"):
        assert np.array_equal(twin[k], back[k]), k
    assert np.array_equal(twin["t"], clock[9])               # nine steps of ONE clock
    assert not np.array_equal(twin["estimated"][0, idx != 0], twin["measured"][0, idx != 0])      # the fifth step filters on
    cleared, _ = run("clear")
    assert np.array_equal(cleared["state"][0], twin["state"][0]) and np.array_equal(cleared["measured"][0], twin["measured"][0])
    assert np.array_equal(cleared["estimated"][0], cleared["measured"][0])                        # cleared: the estimate starts again from the measurement
    check_estimates(cleared, "f64", idx, pkg.X1(), "after a clear")


# ---- 10: the large-batch launch paths ----------------------------------------------------------------------------------------------------------------------------------
def test_large_batch_takes_the_pipelined_launch_under_a_library(pkg, skidpad):
    B, steps = 2341, 3
    idx = (np.arange(B) % 4).astype(np.int32)
    ids = stream_ids(B)
    m = make(pkg, skidpad, B, options={"pipe_min": 2341})
    start(m, inputs(pkg, skidpad, B))
    m.set_sensors([SENSORS[1]], None, seed=NOISE_SEED, streams=ids)
    m.set_estimators(SETS, idx)
    r = rollout(m, "simulate", steps, DT, measured=True, estimated=True)
    assert m.get_option("stat_pipelined_launches") >= 1 and m.get_option("stat_estimator_steps") == steps
    check_estimates(r, "f64", idx, pkg.X1(), "B = 2341")
    assert np.array_equal(m.estimated_state(), r["estimated"][-1])
    m.close()
