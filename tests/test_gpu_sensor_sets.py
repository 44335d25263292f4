"""GPU tests of the sensor sets (pg_set_sensor_sets / pg_set_sensor_index / pg_set_sensor_seed): seeded measurement noise in the three device rollouts.

Four sensors -- exact; sigma (0.05, 0.05, 0.005, 0.1, 0.05, 0.01); bias +0.2 m on E and -0.05 m/s on Ux; three times the noise -- spread over the instances by b % 4
(tests/sensor_numpy.py, whose draws tests/test_sensor_host.py pins to the known answers of Philox4x32-10).  The seed has a non-zero high word and the stream ids lie above
2^32.  Relative differences are |got - ref| / max(1, |ref|) per component; the node bars are 1e-9 in fp64 and 2e-5 in the fp32 library, as in test_gpu_plant_sets.py.
The smallest shapes at which the code can go wrong: B = 70 (a full wavefront and a ragged one) and 12 steps, split 5 + 7."""
import ctypes as C

import numpy as np
import pytest

import node_numpy as nn
import plant_numpy
import sensor_numpy
from conftest import make_oracle
from rollout_libs import NOISE_SEED, inputs, join, make, narrowed, numpy_summary, rel, rollout, start, stream_ids

pytestmark = pytest.mark.gpu

BAR = {"f64": 1e-9, "f32": 2e-5}          # node bars
MEAS_BAR = {"f64": 1e-12, "f32": 2e-5}    # measured = true + bias + sigma z: three roundings + the draw's 1e-13 / the fp32 draw's 2e-6
DRAW_BAR = {"f64": 1e-13, "f32": 2e-5}
DT = 0.01
SETS = sensor_numpy.four_sensors()
KINDS = [("simulate", "coupled"), ("simulate", "decoupled"), ("safety", "coupled"), ("node", "coupled")]


_noisy = {}


def noisy_run(pkg, traj, kind, formulation, precision):
    """the reference rollout of items 2 and 3, computed once per case: B = 70, four sensors by b % 4, 12 steps as 5 + 7"""
    key = (kind, formulation, precision)
    if key not in _noisy:
        B = 70
        idx = (np.arange(B) % 4).astype(np.int32)
        m = make(pkg, traj, B, formulation, precision)
        st = start(m, inputs(pkg, traj, B), others=kind != "simulate")
        m.set_sensors(SETS, idx, seed=NOISE_SEED, streams=stream_ids(B))
        a = rollout(m, kind, 5, DT, measured=True)
        last5 = m.measured_state()
        b = rollout(m, kind, 7, DT, measured=True)
        r = join([a, b])
        r.update(idx=idx, last5=last5, last=m.measured_state(), sensor_steps=m.get_option("stat_sensor_steps"), clock=m.simulate_clock(12, st[2], DT), inputs=st)
        m.close()
        _noisy[key] = r
    return _noisy[key]


def check_measured(r, precision, idx, streams, steps, step0=0):
    """item 2's identity: measured_hist[k] = state_hist[k] + bias + sigma * twin[k] at MEAS_BAR, the channels without noise and bias bit-equal"""
    z = sensor_numpy.draws(NOISE_SEED, streams, step0, steps)
    want = sensor_numpy.measured(SETS, idx, r["state"], z)
    err = rel(r["measured"], want)
    print(f"{precision}: max |measured - (true + bias + sigma z)| = {err.max():.2e} (bar {MEAS_BAR[precision]:g})")
    assert err.max() <= MEAS_BAR[precision], (float(err.max()), np.unravel_index(np.argmax(err), err.shape))
    sg = np.stack([SETS[i][0] for i in idx]); bs = np.stack([SETS[i][1] for i in idx])
    exact = (sg == 0) & (bs == 0)                                                    # [B][6]
    assert exact[idx == 0].all() and exact[idx == 2].sum() == 4 * np.sum(idx == 2) and not exact[idx % 2 == 1].any()
    assert np.array_equal(r["measured"][:, exact].view(np.uint64), r["state"][:, exact].view(np.uint64))
    assert np.mean(r["measured"][:, ~exact] != r["state"][:, ~exact]) > 0.99          # (a draw smaller than half an ulp of the state may leave it as it is)
    return err.max()


# ---- 1: the draws equal the twin -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_draws_equal_the_twin(pkg, skidpad, precision):
    B = 70
    ids = stream_ids(B)
    m = make(pkg, skidpad, B, precision=precision)
    start(m, inputs(pkg, skidpad, B))
    m.set_sensor_seed(NOISE_SEED, ids)
    small = make(pkg, skidpad, 7, precision=precision)
    start(small, inputs(pkg, skidpad, 7))
    ids7 = np.array([11, 12, ids[5], 1 << 50, 3, 4, 5], dtype=np.uint64)
    small.set_sensor_seed(NOISE_SEED, ids7)
    for step0 in (0, 1000):
        z = m.sensor_draws(step0, 4)
        want = sensor_numpy.draws(NOISE_SEED, ids, step0, 4)
        err = np.abs(z - want)
        print(f"{precision}, steps {step0}..{step0 + 3}: max |z - twin| = {err.max():.2e} (bar {DRAW_BAR[precision]:g}), max |z| = {np.abs(z).max():.3f}")
        assert z.shape == (4, B, 6) and err.max() <= DRAW_BAR[precision]
        z7 = small.sensor_draws(step0, 4)
        assert np.array_equal(z7[:, 2], z[:, 5])                                     # the stream id decides, not the position or the batch size
        assert np.abs(z7 - sensor_numpy.draws(NOISE_SEED, ids7, step0, 4)).max() <= DRAW_BAR[precision]
    # default streams: stream[b] = b, and seed 0 until one is set
    fresh = make(pkg, skidpad, B, precision=precision)
    assert np.abs(fresh.sensor_draws(2, 2, B) - sensor_numpy.draws(0, np.arange(B), 2, 2)).max() <= DRAW_BAR[precision]
    assert m.get_option("stat_sensor_steps") == 0
    for h in (m, small, fresh):
        h.close()


# ---- 2: measured = true + bias + sigma z -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind,formulation", KINDS)
def test_measured_is_true_plus_bias_plus_sigma_z(pkg, skidpad, kind, formulation, precision):
    r = noisy_run(pkg, skidpad, kind, formulation, precision)
    assert r["measured"].shape == (12, 70, 6) and r["sensor_steps"] == 12
    check_measured(r, precision, r["idx"], stream_ids(70), 12)
    assert np.array_equal(r["last5"], r["measured"][4]) and np.array_equal(r["last"], r["measured"][11])      # pg_get_measured_state: the last row of each call


# ---- 3: the plant moves the true state -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind,formulation", KINDS)
def test_the_plant_moves_the_true_state(pkg, skidpad, kind, formulation, precision):
    r = noisy_run(pkg, skidpad, kind, formulation, precision)
    P = pkg.X1(); bar = BAR[precision]; idx = r["idx"]
    qh, uh, mh = r["state"], r["control"], r["measured"]
    worst = 0.0; apart = np.zeros(70)
    for k in range(12):
        nxt = qh[k + 1] if k + 1 < 12 else r["final_state"]
        err = rel(nxt, plant_numpy.plant_step_vec(P, qh[k], uh[k], DT))
        worst = max(worst, float(err.max()))
        assert err.max() < bar, (kind, formulation, precision, k, int(np.argmax(err.max(axis=1))), float(err.max()))
        apart = np.maximum(apart, rel(nxt, plant_numpy.plant_step_vec(P, mh[k], uh[k], DT)).max(axis=1))
    # not vacuous: a plant that integrated the measured state misses the bar by two orders of magnitude
    share = float(np.mean(apart[idx != 0] > 100 * bar))
    print(f"{kind} {formulation} {precision}: worst |state - numpy plant from the true state| = {worst:.2e} (bar {bar:g}); "
          f"replay from the measured state misses 100 bars on {share:.0%} of the instances of sets 2-4")
    assert share >= 0.9, share
    assert np.all(apart[idx == 0] < bar)


# ---- 4: the controller sees the measured state -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("formulation", ["coupled", "decoupled"])
def test_the_controller_sees_the_measured_state(pkg, skidpad, formulation):
    """A handle without a library, driven from the host with step_(measured_hist[k], control_hist[k], clock[k]), computes the control the noisy rollout recorded at
    step k + 1.  First the yardstick itself: the same replay of a rollout WITHOUT a library reproduces that rollout's controls."""
    B, steps = 70, 12
    idx = (np.arange(B) % 4).astype(np.int32)

    def replay(states, controls, clock, toff):
        h = make(pkg, skidpad, B, formulation)
        us = [h.step_(states[k], controls[k], clock[k], time_offset=toff)[0] for k in range(steps - 1)]
        h.close()
        return np.stack(us)
    plain = make(pkg, skidpad, B, formulation)
    st = start(plain, inputs(pkg, skidpad, B))
    clock = plain.simulate_clock(steps, st[2], DT)
    p = rollout(plain, "simulate", steps, DT)
    assert plain.get_option("stat_sensor_steps") == 0
    plain.close()
    up = replay(p["state"], p["control"], clock, st[3])
    exact_plain = np.array_equal(up, p["control"][1:])
    print(f"{formulation}: replay of the rollout without a library: bit-equal {exact_plain}, max relative difference {rel(up, p['control'][1:]).max():.2e}")
    assert exact_plain                                        # the same kernels on the same bits
    r = noisy_run(pkg, skidpad, "simulate", formulation, "f64")
    assert np.array_equal(r["clock"], clock)
    un = replay(r["measured"], r["control"], clock, st[3])
    print(f"{formulation}: replay of the noisy rollout from its measured states: bit-equal {np.array_equal(un, r['control'][1:])}, "
          f"max relative difference {rel(un, r['control'][1:]).max():.2e}")
    assert np.array_equal(un, r["control"][1:])
    # not vacuous: the true states give other controls
    ut = replay(r["state"], r["control"], clock, st[3])
    off = rel(ut, r["control"][1:]).max(axis=(0, 2))
    share = float(np.mean(off[idx % 2 == 1] > 1e-6))
    print(f"{formulation}: replay from the TRUE states differs by > 1e-6 on {share:.0%} of the instances of sets 2 and 4 (exact set: max {off[idx == 0].max():.1e})")
    assert share >= 0.5
    # (the exact set reads the true state: the same controls -- bit for bit where the solve of an instance does not depend on its neighbours, the coupled formulation)
    assert np.all(off[idx == 0] == 0.0) if formulation == "coupled" else np.all(off[idx == 0] < 1e-6)


# ---- 5: nothing changes without noise --------------------------------------------------------------------------------------------------------------------------------
def histories(pkg, traj, B, steps, sets, idx, kind, precision, **kw):
    m = make(pkg, traj, B, precision=precision, **kw)
    start(m, inputs(pkg, traj, B), others=kind != "simulate")
    if sets is not None:
        m.set_sensors(sets, idx, seed=NOISE_SEED, streams=stream_ids(B))
    r = rollout(m, kind, steps, DT)
    out = [r["state"], r["control"], r["final_state"]] + [np.asarray(x) for x in m.solve_info()[:3]]
    stats = (m.get_option("stat_pipelined_launches"), m.get_option("stat_sensor_steps"))
    m.close()
    return out, stats


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_nothing_changes_without_noise(pkg, skidpad, kind, precision):
    B, steps = 256, 8
    idx = (np.arange(B) % 4).astype(np.int32)
    none, s_none = histories(pkg, skidpad, B, steps, None, None, kind, precision)
    mixed, s_mixed = histories(pkg, skidpad, B, steps, SETS, idx, kind, precision)
    assert s_none[1] == 0 and s_mixed[1] == steps
    for k in range(4):
        one, s_one = histories(pkg, skidpad, B, steps, [SETS[k]], None, kind, precision)
        assert s_one[1] == steps
        sel = idx == k
        for a, b in zip(mixed, one):
            assert np.array_equal(a[..., sel, :] if a.ndim == 3 else a[sel], b[..., sel, :] if b.ndim == 3 else b[sel]), (kind, precision, k)
        if k == 0:
            for a, b in zip(none, one):                      # a library of one all-zero set = no library
                assert np.array_equal(a, b), (kind, precision)
            for a, b in zip(none, mixed):                    # ... and so are the instances of the exact set in the mixed library
                assert np.array_equal(a[..., sel, :] if a.ndim == 3 else a[sel], b[..., sel, :] if b.ndim == 3 else b[sel]), (kind, precision)
        else:
            assert not np.array_equal(one[2], none[2]), k    # the other sets are not cosmetic


def test_step_and_node_step_never_read_the_library(pkg, skidpad):
    B = 70
    state, control, t0, toff, other = inputs(pkg, skidpad, B)
    outs = []
    for lib in (False, True):
        m = make(pkg, skidpad, B)
        if lib:
            m.set_sensors(SETS, None, seed=NOISE_SEED)       # four sets and NO index: pg_step and pg_node_step_dev do not care
        u = m.step_(state, control, t0, time_offset=toff)
        qp = m.qp_data()
        m.set_inputs(state, control, t0, other, toff)
        m.step_dev()
        m.synchronize()
        u_dev = m.get_next_control()
        node = m.node_step_()
        outs.append(list(u) + [qp, u_dev] + list(node) + [m.get_option("stat_sensor_steps")])
        if lib:
            with pytest.raises(pkg.PigeonError):
                m.measured_state()                           # PG_ERR_STATE: no rollout step ran under the library
        m.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)
    assert outs[1][-1] == 0


# ---- 6: the gates read the measurement -------------------------------------------------------------------------------------------------------------------------------
def test_the_gates_read_the_measurement(pkg, skidpad):
    B, steps = 70, 6
    slow, fast = 3, 66                                        # true Ux 1.02 measured 0.97: paused; true Ux 0.98 measured 1.03: runs
    state, control, t0, toff, other = inputs(pkg, skidpad, B)
    state = state.copy(); control = control.copy()
    state[slow, 3] = 1.02; state[fast, 3] = 0.98
    state[[slow, fast], 4:6] = 0.0; control[[slow, fast]] = 0.0          # (a paused instance coasts: 60 ms of drag take a few mm/s)
    sets = [SETS[0], (np.zeros(6), np.array([0, 0, 0, -0.05, 0, 0.0])), (np.zeros(6), np.array([0, 0, 0, 0.05, 0, 0.0]))]
    idx = np.zeros(B, dtype=np.int32); idx[slow] = 1; idx[fast] = 2
    res = {}
    for lib in (True, False):
        m = make(pkg, skidpad, B)
        m.set_inputs(state, control, t0, other, toff)
        if lib:
            m.set_sensors(sets, idx, seed=NOISE_SEED)
        x0 = [np.asarray(a)[[slow, fast]].copy() for a in list(m.solution()) + list(m.solve_info())]
        r = rollout(m, "node", steps, DT, measured=lib)
        seen = r["measured"] if lib else r["state"]                                                        # what the gate read: on the intended side of 1 m/s at every step
        assert (np.all(seen[:, slow, 3] < 1.0) and np.all(seen[:, fast, 3] >= 1.0)) if lib else (np.all(seen[:, slow, 3] >= 1.0) and np.all(seen[:, fast, 3] < 1.0))
        if lib:
            assert np.all(r["state"][:, slow, 3] >= 1.0)                                                   # ... while the true speed would have let it run
        x1 = [np.asarray(a)[[slow, fast]] for a in list(m.solution()) + list(m.solve_info())]
        _, hb, cn = m.node_summary()
        res[lib] = (r["event"], hb, cn, x0, x1)
        m.close()
    ev, hb, cn, x0, x1 = res[True]
    assert np.all(ev[:, slow] == nn.LOW_SPEED) and hb[slow] == 0 and cn[slow, 2] == steps
    assert all(np.array_equal(a[0], b[0], equal_nan=True) for a, b in zip(x0, x1))                            # its solver state: untouched
    assert np.all(ev[:, fast] == 0) and hb[fast] == steps and cn[fast, 2] == 0
    others = np.ones(B, bool); others[[slow, fast]] = False
    ev0, hb0, cn0, _, _ = res[False]
    assert np.all(ev0[:, slow] == 0) and hb0[slow] == steps                                                   # without the library the first runs ...
    assert np.all(ev0[:, fast] == nn.LOW_SPEED) and hb0[fast] == 0 and cn0[fast, 2] == steps                  # ... and the second is paused
    assert np.array_equal(ev[:, others], ev0[:, others])


# ---- 7: the summaries describe the truth -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,precision", [("simulate", "f64"), ("simulate", "f32"), ("node", "f64")])
def test_the_summaries_describe_the_truth(pkg, oracle_mod, skidpad, kind, precision):
    B, steps = 70, 12
    bar = BAR[precision]
    idx = (np.arange(B) % 4).astype(np.int32)
    tube = narrowed(pkg, skidpad)
    orc = make_oracle(oracle_mod, tube if precision == "f64" else pkg.TrajectoryTube(*tube.data.astype(np.float32).astype(np.float64)))
    m = make(pkg, tube, B, precision=precision)
    m.set_option("tracking_summary", 1)
    start(m, inputs(pkg, tube, B), others=kind != "simulate")
    m.set_sensors(SETS, idx, seed=NOISE_SEED, streams=stream_ids(B))
    a = rollout(m, kind, 5, DT, measured=True); b = rollout(m, kind, 7, DT, measured=True)
    r = join([a, b])
    sm, n, fx = m.tracking_summary()
    (wsm, wn, wfx, margin), _, _ = numpy_summary([orc], None, r["state"])
    assert np.array_equal(n, wn) and np.all(n == steps)
    err = rel(sm, wsm)
    print(f"{kind} {precision}: tracking summary vs numpy on the TRUE history: {err.max():.2e} (bar {bar:g})")
    assert err.max() < bar, (err.max(axis=0), bar)
    decided = margin > 1e-6
    assert np.mean(~decided) <= 1 / 8 and np.array_equal(fx[decided], wfx[decided])
    (msm, _, _, _), ms, me = numpy_summary([orc], None, r["measured"])
    off = rel(sm, msm).max(axis=1)
    share = float(np.mean(off[idx != 0] > 100 * bar))
    print(f"{kind} {precision}: the summary of the MEASURED history is off by > 100 bars on {share:.0%} of the instances of sets 2-4")
    assert share >= 0.9 and np.all(off[idx == 0] < bar)
    # the step's own projection -- the (s, e) a node step publishes -- is the measured one.  The rollouts have no (s, e) output; k_node_finish copies what it publishes from
    # NodeIO::sep, which node_io() points at the handle's sep buffer, the one path_coordinates() reads (a node_step_ here would not do: the one-shot call never reads the library)
    sep = m.path_coordinates(); s_dev, e_dev = sep[:, 0], sep[:, 1]
    assert rel(s_dev, ms[-1]).max() < max(bar, 1e-7) and np.abs(e_dev - me[-1]).max() < (1e-7 if precision == "f64" else 1e-3)
    (_, ts_, te) = numpy_summary([orc], None, r["state"][-1:])
    assert np.mean(np.abs(e_dev - te[0])[idx != 0] > 1e-3) >= 0.8
    m.close()


# ---- 8: contract -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_contract(pkg, skidpad):
    B, cap = 70, 80
    idx = (np.arange(B) % 4).astype(np.int32)
    ids = stream_ids(B)

    def fresh():
        m = make(pkg, skidpad, cap)
        start(m, inputs(pkg, skidpad, B), others=True)
        return m
    twin = fresh()
    twin.set_sensors(SETS, idx, seed=NOISE_SEED, streams=ids)
    want = rollout(twin, "simulate", 4, DT, measured=True)
    twin.close()
    m = fresh()
    with pytest.raises(pkg.PigeonError):
        m.simulate_(1, DT, measured=True)                    # PG_ERR_STATE: a measured history without a library
    m.set_sensors(SETS, None, seed=NOISE_SEED, streams=ids)

    def rollouts_refuse():
        assert m.lib.pg_simulate_dev(m.h, 1, C.c_double(DT), None, None) == -4
        assert m.lib.pg_simulate_safety_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None, None) == -4
        assert m.lib.pg_simulate_node_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None) == -4
    rollouts_refuse()                                        # n_sets > 1 and no index
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    assert m.lib.pg_set_sensor_index(m.h, B - 1, i32(idx)) == 0
    rollouts_refuse()                                        # an index shorter than the batch
    assert m.lib.pg_set_sensor_index(m.h, B, i32(idx)) == 0
    before = m.sensors()
    assert len(before[0]) == 4 and np.array_equal(before[1], idx)
    assert all(before[0][k]["sigma"] == list(SETS[k][0]) and before[0][k]["bias"] == list(SETS[k][1]) for k in range(4))

    def rejected(rc):
        assert rc == -2
        after = m.sensors()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    arr = m.pack_sensors(SETS)
    rejected(m.lib.pg_set_sensor_sets(m.h, 0, arr))
    rejected(m.lib.pg_set_sensor_sets(m.h, -1, arr))
    for c in range(6):
        for field in ("sigma", "bias"):
            for bad in (float("nan"), float("inf"), -float("inf")):
                one = m.pack_sensors([SETS[0], SETS[1]]); getattr(one[1], field)[c] = bad
                rejected(m.lib.pg_set_sensor_sets(m.h, 2, one))
        one = m.pack_sensors([SETS[1]]); one[0].sigma[c] = -1e-9
        rejected(m.lib.pg_set_sensor_sets(m.h, 1, one))
    for bad_idx in (np.where(np.arange(B) == 5, 4, idx), np.where(np.arange(B) == 69, -1, idx)):
        rejected(m.lib.pg_set_sensor_index(m.h, B, i32(bad_idx)))
    rejected(m.lib.pg_set_sensor_index(m.h, 0, i32(idx)))
    rejected(m.lib.pg_set_sensor_index(m.h, cap + 1, i32(np.zeros(cap + 1))))
    rejected(m.lib.pg_set_sensor_seed(m.h, C.c_uint64(1), 0, u64(ids)))
    rejected(m.lib.pg_set_sensor_seed(m.h, C.c_uint64(1), cap + 1, u64(np.zeros(cap + 1))))
    z = np.zeros((1, cap + 1, 6))
    for args in ((0, 1, 0), (0, 1, cap + 1), (-1, 1, B), (0, 0, B)):
        rejected(m.lib.pg_sensor_draws(m.h, *args, z.ctypes.data_as(C.POINTER(C.c_double))))
    # ... and the histories after all those refusals are the twin's, bit for bit (seed and streams included)
    got = rollout(m, "simulate", 4, DT, measured=True)
    for k in ("state", "control", "final_state", "measured"):
        assert np.array_equal(got[k], want[k]), k
    # pg_set_inputs restarts the sequence: the same four steps again, the same bits; another seed, other bits
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    with pytest.raises(pkg.PigeonError):
        m.measured_state()                                   # forgotten with the inputs
    again = rollout(m, "simulate", 4, DT, measured=True)
    for k in ("state", "control", "final_state", "measured"):
        assert np.array_equal(again[k], want[k]), k
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    m.set_sensor_seed(NOISE_SEED + 1, ids)
    other = rollout(m, "simulate", 4, DT, measured=True)
    assert np.array_equal(other["state"][0], want["state"][0]) and not np.array_equal(other["measured"][0], want["measured"][0])
    assert np.array_equal(other["measured"][:, idx == 0], other["state"][:, idx == 0])
    # installing a library drops the index, keeps seed and streams; clearing restores the no-library launches
    m.set_sensor_seed(NOISE_SEED, ids)
    assert m.lib.pg_set_sensor_sets(m.h, 4, arr) == 0
    assert np.all(m.sensors()[1] == -1)
    rollouts_refuse()
    assert m.lib.pg_set_sensor_index(m.h, B, i32(idx)) == 0
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    third = rollout(m, "simulate", 4, DT, measured=True)
    assert np.array_equal(third["measured"], want["measured"])
    m.clear_sensors()
    assert m.sensors()[0] == [] and m.lib.pg_set_sensor_index(m.h, B, i32(idx)) == -2
    n_before = m.get_option("stat_sensor_steps")
    m.simulate_(2, DT)
    assert m.get_option("stat_sensor_steps") == n_before
    # a rollout call that FAILS consumes the one-shot measured history too: the successful call behind it writes nothing to that buffer
    import torch
    m.set_sensors(SETS, None, seed=NOISE_SEED, streams=ids)
    buf = torch.full((2, B, 6), -7.0, dtype=torch.float64, device=f"cuda:{m.cfg.device}")
    assert m.lib.pg_set_measured_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == 0
    rollouts_refuse()                                        # no index: PG_ERR_STATE
    assert m.lib.pg_set_sensor_index(m.h, B, i32(idx)) == 0
    m.simulate_(2, DT); m.synchronize()
    assert bool((buf == -7.0).all())
    m.close()


def test_installing_a_library_between_rollouts_resets_nothing(pkg, skidpad):
    """The clock runs on, the draws continue at the clock's step index, the safety summary's step indices continue and every instance stays warm: a handle whose library is
    replaced and restored, or cleared and installed again, between two rollout calls equals, bit for bit, its twin whose library was installed once."""
    B = 70
    idx = (np.arange(B) % 4).astype(np.int32)
    ids = stream_ids(B)
    grid = pkg.synthetic.hji_grid(dims=(7, 6, 5, 4, 4, 5, 4), seed=11)

    def run(between):
        m = make(pkg, skidpad, B)
        m.set_hji_cache(*grid)
        st = start(m, inputs(pkg, skidpad, B), others=True)
        m.set_sensors(SETS, idx, seed=NOISE_SEED, streams=ids)
        m.simulate_safety_(4, DT, use_HJI_policy=True, human="worst")
        if between == "restore":
            m.set_sensors([SETS[3]], None, seed=1); m.set_sensors(SETS, idx, seed=NOISE_SEED, streams=ids)
        elif between == "clear":
            m.clear_sensors(); m.set_sensors(SETS, idx, seed=NOISE_SEED, streams=ids)
        elif between == "replace":
            m.set_sensors(SETS, (3 - idx).astype(np.int32), seed=NOISE_SEED, streams=ids)
        s2 = m.simulate_safety_(4, DT, use_HJI_policy=True, human="worst", record=True, measured=True)
        out = dict(state=s2[0], control=s2[1], t=s2[2], iters=m.solve_info()[1], status=m.solve_info()[0], polish=m.polish_info(), fb=m.safety_summary()[1],
                   vmin=m.safety_summary()[0], qh=s2[4]["state"], uh=s2[4]["control"], mh=s2[5])
        clock = m.simulate_clock(9, st[2], DT)
        m.close()
        return out, clock
    twin, clock = run(None)
    for between in ("restore", "clear"):
        back, _ = run(between)
        for k in twin:
            assert np.array_equal(twin[k], back[k]), (between, k)
    assert np.array_equal(twin["t"], clock[8])               # eight steps of ONE clock
    z = sensor_numpy.draws(NOISE_SEED, ids, 4, 4)            # ... and the second call drew at the clock's steps 4..7
    assert rel(twin["mh"], sensor_numpy.measured(SETS, idx, twin["qh"], z)).max() <= MEAS_BAR["f64"]
    swap, _ = run("replace")
    assert np.array_equal(swap["t"], clock[8]) and np.array_equal(swap["qh"][0], twin["qh"][0])
    assert rel(swap["mh"], sensor_numpy.measured(SETS, 3 - idx, swap["qh"], z)).max() <= MEAS_BAR["f64"]      # the new selection acts from the next step on
    early = (twin["fb"] >= 0) & (twin["fb"] < 4)
    assert np.array_equal(swap["fb"][early], twin["fb"][early])                                                # breaches of the first call keep their step index


# ---- 9: the large-batch launch paths ---------------------------------------------------------------------------------------------------------------------------------
def test_large_batch_takes_the_pipelined_launch_under_a_library(pkg, skidpad):
    B, steps = 2341, 3
    idx = (np.arange(B) % 4).astype(np.int32)
    ids = stream_ids(B)
    m = make(pkg, skidpad, B, options={"pipe_min": 2341})
    start(m, inputs(pkg, skidpad, B))
    m.set_sensors(SETS, idx, seed=NOISE_SEED, streams=ids)
    r = rollout(m, "simulate", steps, DT, measured=True)
    assert m.get_option("stat_pipelined_launches") >= 1 and m.get_option("stat_sensor_steps") == steps
    check_measured(r, "f64", idx, ids, steps)
    assert np.array_equal(m.measured_state(), r["measured"][-1])
    m.close()
