"""GPU tests of the disturbance sets (pg_set_disturbance_sets / pg_set_disturbance_index / pg_set_disturbance_seed): forces, a seeded gust and low-friction windows on
the ego plant of the three rollouts.

Four sets -- the identity; a side gust (Fy = 2000 N, x_cp = 1 m, sigma_Fy = 800 N, tau = 0.3 s) in the window [3, 9); mu x 0.55 from step 2 on; a headwind of -1000 N
with a white gust of 500 N -- spread over the instances by b % 4.  The yardstick is tests/disturbance_numpy.py, written from the header and pinned by
tests/test_disturbance_host.py.  Bars: the draws' 1e-13 / 2e-5 (tests/test_gpu_sensor_sets.py) per step of the recursion for the law -- a draw's error enters once per
step and rho < 1 never amplifies it --, relative to max(1, |ref|); the node bars 1e-9 / 2e-5 of DESIGN.md section 5 for the plant.

Not vacuous: the replay with w = (0, 0, 0, 1) must miss by more than 100 bars on at least half of the active instance-steps of the non-identity sets.  The miss is
measured as the derivation of the sizes measures it, in state units: 2000 N over 1964 kg for 0.01 s moves Uy by 1.0e-2, 1000 N moves Ux by 5e-3, both above
2e-3 = 100 x 2e-5.  (Divided by max(1, |ref|) as the replay's own error is, the headwind's 5e-3 on Ux = 5.4 .. 6.6 m/s is 8e-4 and never counts.)
Checked on the CPU with the twin alone before the first GPU visit (tests/test_disturbance_host.py::test_the_replay_test_of_the_gpu_file_is_not_vacuous), `skidpadoval`,
synthetic.config2_inputs(seed = 4), 12 steps from the 70 starts with the start control held: the undisturbed step is more than 2e-3 away on 65 % of the active
instance-steps (side gust 100 %, friction window 16 % -- at 6 m/s few tires are near their limit --, headwind 87 %); with the relative measure on 28 %."""
import ctypes as C

import numpy as np
import pytest

import disturbance_numpy as dn
import plant_numpy
from rollout_libs import check_summary, inputs, join, make, numpy_summary, rel, rollout, start

pytestmark = pytest.mark.gpu

SEED = 4                                  # of the synthetic inputs
GUST_SEED = 0x9E3779B97F4A7C15            # of the draws: high word non-zero
BAR = {"f64": 1e-9, "f32": 2e-5}          # node bars
DRAW_BAR = {"f64": 1e-13, "f32": 2e-5}    # of tests/test_gpu_sensor_sets.py
DT = 0.01
B = 70
STEPS = 12
SETS = dn.four_disturbances()
IDX = (np.arange(B) % 4).astype(np.int32)
KEYS = ("state", "control", "disturbance", "final_state")          # what two runs are compared on
OUTSIDE = dn.identity(Fx=-3000.0, Fy=4000.0, Mz=500.0, sigma_Fx=100.0, sigma_Fy=900.0, x_cp=1.0, tau_gust=0.2, mu_scale=0.3, step_on=1000, step_off=2000)


def active(sets, idx, step0, steps):
    """[steps][B]: the instance's set is inside its window at that clock step"""
    k = np.arange(step0, step0 + steps)[:, None]
    on = np.array([sets[i]["step_on"] for i in idx])[None, :]; off = np.array([sets[i]["step_off"] for i in idx])[None, :]
    return (k >= on) & ((off < 0) | (k < off))


def miss(a, b):
    """per instance: how far two predicted states are apart, in state units (see the module docstring)"""
    return np.abs(np.asarray(a) - np.asarray(b)).max(axis=1)


def replay_share_on_the_starts(pkg, traj):
    """CPU only, STEPS steps from the starts with the start control held: (share of the active instance-steps of the non-identity sets on which the undisturbed step is
    more than 100 x 2e-5 away from the disturbed one, the same per set, the share with the difference divided by max(1, |ref|))"""
    state, control, _, _ = pkg.synthetic.config2_inputs(traj, B, seed=SEED)
    w = dn.response(SETS, IDX, GUST_SEED, np.arange(B), 0, STEPS, DT)
    X1 = pkg.X1()
    ident = np.tile(dn.IDENTITY_W, (B, 1))
    q = state.copy(); far = np.zeros((STEPS, B), dtype=bool); far_rel = np.zeros((STEPS, B), dtype=bool)
    for k in range(STEPS):
        pred = dn.plant_step_vec_dist(X1, q, control, w[k], DT); plain = dn.plant_step_vec_dist(X1, q, control, ident, DT)
        far[k] = miss(plain, pred) > 100 * BAR["f32"]; far_rel[k] = rel(plain, pred).max(axis=1) > 100 * BAR["f32"]
        q = pred
    live = active(SETS, IDX, 0, STEPS) & (IDX != 0)[None, :]
    per_set = [float(np.mean(far[:, IDX == j][live[:, IDX == j]])) for j in (1, 2, 3)]
    return float(np.mean(far[live])), per_set, float(np.mean(far_rel[live]))


def check_law(got, precision, sets, idx, streams, step0, what, seed=GUST_SEED):
    """got [steps][B][4] against the twin from a fresh state at step0: within steps x DRAW_BAR, and bit-equal to (0, 0, 0, 1) outside the window"""
    steps = got.shape[0]
    want = dn.response(sets, idx, seed, streams, step0, steps, DT)
    worst = float(rel(got, want).max())
    bar = steps * DRAW_BAR[precision]
    print(f"{what} {precision}: law vs twin over {steps} steps from step {step0}: worst {worst:.3g} (bar {bar:.3g})")
    assert worst <= bar, (what, worst, bar)
    out = ~active(sets, idx, step0, steps)
    assert out.any() and np.array_equal(got[out], np.broadcast_to(dn.IDENTITY_W, (int(out.sum()), 4))), what
    return worst


# ---- 1: the law, no controller ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_law_equals_the_twin(pkg, skidpad, precision):
    m = make(pkg, skidpad, B, precision=precision)
    start(m, inputs(pkg, skidpad, B))
    m.set_disturbances(SETS, IDX, seed=GUST_SEED)
    check_law(m.disturbance_response(0, 40, DT), precision, SETS, IDX, np.arange(B), 0, "pg_disturbance_response")
    check_law(m.disturbance_response(7, 40, DT), precision, SETS, IDX, np.arange(B), 7, "pg_disturbance_response")
    # the call leaves the handle's gust state and the clock alone: no step has run
    with pytest.raises(pkg.PigeonError):
        m.disturbance_state()
    assert m.get_option("stat_disturbance_steps") == 0
    m.close()


# ---- 2: rollout replay ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_replay(r, precision, plants, sets, idx, what, step0=0):
    """every recorded step replays through the numpy plant with the recorded w; returns (worst difference, share of the active non-identity instance-steps on which the
    replay with w = (0, 0, 0, 1) is more than 100 bars away)"""
    bar = BAR[precision]
    steps, n = r["state"].shape[:2]
    worst = 0.0; apart = np.zeros((steps, n), dtype=bool)
    ident = np.tile(dn.IDENTITY_W, (n, 1))
    for k in range(steps):
        nxt = r["state"][k + 1] if k + 1 < steps else r["final_state"]
        pred = dn.plant_step_vec_dist(plants, r["state"][k], r["control"][k], r["disturbance"][k], DT)
        err = rel(nxt, pred)
        worst = max(worst, float(err.max()))
        assert err.max() < bar, (what, precision, k, int(np.argmax(err.max(axis=1))), float(err.max()))
        apart[k] = miss(dn.plant_step_vec_dist(plants, r["state"][k], r["control"][k], ident, DT), pred) > 100 * bar
    live = active(sets, idx, step0, steps) & (np.asarray(idx) != 0)[None, :]
    return worst, float(np.mean(apart[live]))


@pytest.mark.parametrize("kind,formulation,precision", [("simulate", "coupled", "f64"), ("simulate", "decoupled", "f64"), ("safety", "coupled", "f64"), ("node", "coupled", "f64"),
                                                        ("node", "decoupled", "f64"), ("simulate", "coupled", "f32"), ("safety", "coupled", "f32"), ("node", "coupled", "f32")])
def test_every_step_replays_through_the_disturbed_numpy_plant(pkg, skidpad, kind, formulation, precision):
    m = make(pkg, skidpad, B, formulation=formulation, precision=precision)
    m.set_disturbances(SETS, IDX, seed=GUST_SEED)
    start(m, inputs(pkg, skidpad, B), others=kind != "simulate")
    r = rollout(m, kind, STEPS, DT)
    what = f"{kind} {formulation}"
    check_law(r["disturbance"], precision, SETS, IDX, np.arange(B), 0, what + " record")
    worst, share = check_replay(r, precision, pkg.X1(), SETS, IDX, what)
    print(f"{what} {precision}: worst |state - disturbed numpy plant| = {worst:.2e} (bar {BAR[precision]:g}); the undisturbed replay is > 100 bars away on {share:.0%} of the "
          f"active instance-steps of the non-identity sets")
    assert share >= 0.5, share
    assert np.array_equal(m.disturbance_state(), r["disturbance"][-1])
    assert m.get_option("stat_disturbance_steps") == STEPS
    m.close()


# ---- 3 / 4: identity = no library; mixed = libraries of one ----------------------------------------------------------------------------------------------------------------
def histories(pkg, traj, kind, sets, idx, n=256, steps=8, precision="f64", **kw):
    m = make(pkg, traj, n, precision=precision, **kw)
    if sets is not None:
        m.set_disturbances(sets, idx, seed=GUST_SEED)
    start(m, inputs(pkg, traj, n), others=kind != "simulate")
    r = rollout(m, kind, steps, DT)
    r["stat"] = m.get_option("stat_disturbance_steps"); r["pipelined"] = m.get_option("stat_pipelined_launches")
    m.close()
    return r


@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_the_identity_set_and_a_closed_window_equal_no_library(pkg, skidpad, kind):
    keys = ("state", "control", "final_state")
    none = histories(pkg, skidpad, kind, None, None)
    assert none["stat"] == 0 and none["disturbance"] is None
    for name, s in (("identity", dn.identity()), ("closed window", OUTSIDE)):
        one = histories(pkg, skidpad, kind, [s], None)
        assert one["stat"] == 8
        for k in keys:
            assert np.array_equal(none[k], one[k]), (kind, name, k)
        assert np.array_equal(one["disturbance"], np.broadcast_to(dn.IDENTITY_W, (8, 256, 4)))
    n32 = histories(pkg, skidpad, kind, None, None, precision="f32")
    for name, s in (("identity", dn.identity()), ("closed window", OUTSIDE)):
        o32 = histories(pkg, skidpad, kind, [s], None, precision="f32")
        worst = max(float(rel(o32[k], n32[k]).max()) for k in keys)
        print(f"fp32 library, {kind}, {name}: against no library: max relative difference {worst:.2e}, bit-equal: {all(np.array_equal(n32[k], o32[k]) for k in keys)}")
        assert worst < BAR["f32"]


def test_mixed_library_equals_libraries_of_one_bit_for_bit(pkg, skidpad):
    idx = (np.arange(256) % 4).astype(np.int32)
    mixed = histories(pkg, skidpad, "simulate", SETS, idx)
    base = None
    for j in range(4):
        one = histories(pkg, skidpad, "simulate", [SETS[j]], None)
        sel = idx == j
        for k in ("state", "control", "disturbance"):
            assert np.array_equal(mixed[k][:, sel], one[k][:, sel]), (j, k)
        assert np.array_equal(mixed["final_state"][sel], one["final_state"][sel]), j
        if j == 0:
            base = one["final_state"]
        else:
            assert np.max(np.abs(one["final_state"] - base)) > 1e-5, j          # the sets are not cosmetic


# ---- 5: the controller does not see it -------------------------------------------------------------------------------------------------------------------------------------
def test_the_controller_does_not_see_the_disturbance(pkg, skidpad):
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=SEED)
    plain = make(pkg, skidpad, B); lib = make(pkg, skidpad, B)
    lib.set_disturbances(SETS)                               # four sets and NO index: pg_step does not care
    u0, st0, it0 = plain.step_(state, control, t0, time_offset=toff)
    u1, st1, it1 = lib.step_(state, control, t0, time_offset=toff)
    assert np.array_equal(u0, u1) and np.array_equal(st0, st1) and np.array_equal(it0, it1)
    assert np.array_equal(plain.qp_data(), lib.qp_data())
    assert all(np.array_equal(a, b) for a, b in zip(plain.nodes(), lib.nodes()))
    assert lib.get_option("stat_disturbance_steps") == 0
    # in a rollout: the nodes and the QP of step 0 are those of the handle without a library (the headwind set is active there); the states part company one step after a set's window opens
    fresh = make(pkg, skidpad, B); roll = make(pkg, skidpad, B)
    roll.set_disturbances(SETS, IDX, seed=GUST_SEED)
    for m in (fresh, roll):
        m.set_inputs(state, control, t0, None, toff)
    f0 = rollout(fresh, "simulate", 1, DT); r0 = rollout(roll, "simulate", 1, DT)
    assert np.array_equal(fresh.qp_data(), roll.qp_data()) and all(np.array_equal(a, b) for a, b in zip(fresh.nodes(), roll.nodes()))
    assert np.any(r0["disturbance"][0, IDX == 3, 0] != 0.0)
    f = join([f0, rollout(fresh, "simulate", STEPS - 1, DT)]); r = join([r0, rollout(roll, "simulate", STEPS - 1, DT)])
    for j in range(4):
        sel = IDX == j
        on = SETS[j]["step_on"]
        if j == 0:
            assert np.array_equal(f["state"][:, sel], r["state"][:, sel]) and np.array_equal(f["final_state"][sel], r["final_state"][sel])
            continue
        assert np.array_equal(f["state"][:on + 1, sel], r["state"][:on + 1, sel]) and np.array_equal(f["control"][:on + 1, sel], r["control"][:on + 1, sel]), j
        assert np.all(np.any(f["state"][on + 1, sel] != r["state"][on + 1, sel], axis=1)), j
    for m in (plain, lib, fresh, roll):
        m.close()


# ---- 6: determinism --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_determinism(pkg, skidpad):
    streams = (1000 + np.arange(B)).astype(np.uint64)
    m = make(pkg, skidpad, B)
    start(m, inputs(pkg, skidpad, B))
    m.set_disturbances(SETS, IDX, seed=GUST_SEED, streams=streams)
    w70 = m.disturbance_response(0, STEPS, DT)
    check_law(w70, "f64", SETS, IDX, streams, 0, "streams 1000 + b")
    # (a) a function of the stream id, not of b or B
    pick = np.array([1, 2, 3, 13, 34, 67, 69])
    small = make(pkg, skidpad, 7)
    start(small, inputs(pkg, skidpad, 7))
    small.set_disturbances(SETS, IDX[pick], seed=GUST_SEED, streams=streams[pick])
    assert np.array_equal(small.disturbance_response(0, STEPS, DT), w70[:, pick])
    small.close()
    # (b) 6 + 6 steps in two calls are 12 in one; (c) set_inputs replays them
    whole = rollout(m, "simulate", STEPS, DT)
    assert np.array_equal(whole["disturbance"], w70)
    m.reset(); start(m, inputs(pkg, skidpad, B))
    split = join([rollout(m, "simulate", 6, DT), rollout(m, "simulate", 6, DT)])
    for k in KEYS:
        assert np.array_equal(whole[k], split[k]), k
    assert m.get_option("stat_disturbance_steps") == 2 * STEPS
    # (d) another seed: w changes wherever a sigma is positive and the window open, and nowhere else
    m.set_disturbance_seed(GUST_SEED + 1, streams)
    w2 = m.disturbance_response(0, STEPS, DT)
    live = active(SETS, IDX, 0, STEPS)
    sx = np.array([SETS[i]["sigma_Fx"] for i in IDX]) > 0; sy = np.array([SETS[i]["sigma_Fy"] for i in IDX]) > 0
    moved = w2 != w70
    assert np.array_equal(moved[..., 0], live & sx[None, :]) and np.array_equal(moved[..., 1], live & sy[None, :]) and np.array_equal(moved[..., 2], live & sy[None, :])
    assert not moved[..., 3].any()
    m.close()


# ---- 7: composition ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_composition_with_plants_sensors_actuators_tunings_and_the_summary(pkg, oracle_mod, skidpad):
    import actuator_numpy
    import sensor_numpy
    from conftest import make_oracle
    plants = plant_numpy.four_plants(pkg.X1)
    pidx = ((np.arange(B) // 4) % 4).astype(np.int32)           # every (plant, disturbance) pair occurs
    asets = actuator_numpy.six_sets()
    orc = make_oracle(oracle_mod, skidpad)

    def run(disturbed):
        m = make(pkg, skidpad, B)
        cp = pkg.CoupledControlParams()
        m.set_control_params([cp, dict(cp, Q_e=2.0, R_ddelta=0.2)], ((np.arange(B) // 2) % 2).astype(np.int32))
        m.set_plants(plants, pidx)
        m.set_sensors(sensor_numpy.four_sensors(), ((np.arange(B) // 3) % 4).astype(np.int32), seed=7)
        m.set_actuators(asets, (np.arange(B) % 6).astype(np.int32))
        if disturbed:
            m.set_disturbances(SETS, IDX, seed=GUST_SEED)
        m.set_option("tracking_summary", 1)
        start(m, inputs(pkg, skidpad, B))
        r = rollout(m, "simulate", STEPS, DT)
        got = m.tracking_summary()
        stats = [m.get_option(f"stat_{n}_steps") for n in ("disturbance", "actuator", "sensor")]
        m.close()
        return r, got, stats
    r, got, stats = run(True)
    assert stats == [STEPS, STEPS, STEPS]
    check_law(r["disturbance"], "f64", SETS, IDX, np.arange(B), 0, "composition record")
    own = plant_numpy.stack_vehicles([plants[i] for i in pidx], B)
    worst, share = check_replay(r, "f64", own, SETS, IDX, "composition")      # (the control record under an actuator library is the applied control)
    print(f"composition: worst |state - disturbed numpy plant of the instance's own set (applied control)| = {worst:.2e}; undisturbed replay apart on {share:.0%}")
    assert share >= 0.5
    want, _, _ = numpy_summary([orc], None, r["state"])
    check_summary(got, want, BAR["f64"])
    r0, got0, stats0 = run(False)
    assert stats0[0] == 0
    slick = IDX == 2
    with_w, without = float(got[0][slick, 0].max()), float(got0[0][slick, 0].max())
    print(f"friction-window set (mu x 0.55 from step 2): max |e| over its instances {with_w:.6f} m with the library, {without:.6f} m without")
    assert with_w >= without


# ---- 8: contract -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_contract(pkg, skidpad):
    import torch
    cap = 80
    m = make(pkg, skidpad, cap)
    start(m, inputs(pkg, skidpad, B), others=True)
    none = rollout(m, "simulate", 3, DT)
    assert m.get_option("stat_disturbance_steps") == 0 and m.disturbances()[0] == []
    buf = torch.full((2, B, 4), -7.0, dtype=torch.float64, device=f"cuda:{m.cfg.device}")
    assert m.lib.pg_set_disturbance_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == -4          # no library
    assert m.lib.pg_get_disturbance_state(m.h, np.zeros((B, 4)).ctypes.data_as(C.POINTER(C.c_double))) == -4
    with pytest.raises(pkg.PigeonError):
        m.disturbance_response(0, 2, DT)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert m.lib.pg_set_disturbance_index(m.h, B, i32(IDX)) == -2          # no library to index
    m.set_disturbances(SETS, seed=GUST_SEED)

    def rollouts_refuse():
        assert m.lib.pg_simulate_dev(m.h, 1, C.c_double(DT), None, None) == -4
        assert m.lib.pg_simulate_safety_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None, None) == -4
        assert m.lib.pg_simulate_node_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None) == -4
        assert "disturbance" in m.lib.pg_last_error(m.h).decode()
    rollouts_refuse()                                            # several sets and no index
    with pytest.raises(pkg.PigeonError):
        m.disturbance_response(0, 2, DT)
    m.set_disturbance_index(IDX[:B - 1])
    rollouts_refuse()                                            # an index shorter than the batch
    m.set_disturbance_index(IDX)
    assert m.lib.pg_get_disturbance_state(m.h, np.zeros((B, 4)).ctypes.data_as(C.POINTER(C.c_double))) == -4      # a library, and no step under it yet
    before = m.disturbances()
    assert before[0] == SETS and np.array_equal(before[1], IDX)          # round trip

    def rejected(rc, word=None):
        assert rc == -2
        if word:
            msg = m.lib.pg_last_error(m.h).decode()
            assert word in msg and "set 1" in msg, msg
        after = m.disturbances()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    arr = m.pack_disturbances(SETS)
    rejected(m.lib.pg_set_disturbance_sets(m.h, 0, arr))
    rejected(m.lib.pg_set_disturbance_sets(m.h, -1, arr))

    def two(**bad):
        a = m.pack_disturbances([SETS[0], SETS[1]])
        for k, v in bad.items():
            setattr(a[1], k, v)
        return a
    nan, inf = float("nan"), float("inf")
    for field in ("Fx", "Fy", "Mz", "sigma_Fx", "sigma_Fy", "x_cp", "tau_gust", "mu_scale"):
        for v in (nan, inf, -inf):
            rejected(m.lib.pg_set_disturbance_sets(m.h, 2, two(**{field: v})), field)
    for field, values in (("sigma_Fx", (-1e-9,)), ("sigma_Fy", (-1.0,)), ("tau_gust", (-1e-9,)), ("mu_scale", (0.0, -0.5)), ("step_on", (-1,))):
        for v in values:
            rejected(m.lib.pg_set_disturbance_sets(m.h, 2, two(**{field: v})), field)
    for bad_idx in (np.where(np.arange(B) == 5, 4, IDX), np.where(np.arange(B) == 69, -1, IDX)):
        rejected(m.lib.pg_set_disturbance_index(m.h, B, i32(bad_idx)))
    rejected(m.lib.pg_set_disturbance_index(m.h, 0, i32(IDX)))
    rejected(m.lib.pg_set_disturbance_index(m.h, cap + 1, i32(np.zeros(cap + 1))))
    # pg_node_step_dev ignores the library
    m.node_step_()
    assert m.get_option("stat_disturbance_steps") == 0
    # a rollout call that FAILS consumes the one-shot history: the successful call behind it writes nothing to that buffer
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    m.set_disturbances(SETS, seed=GUST_SEED)                     # (installing a library drops the index)
    assert np.all(m.disturbances()[1] == -1)
    assert m.lib.pg_set_disturbance_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == 0
    rollouts_refuse()
    m.set_disturbance_index(IDX)
    m.simulate_(2, DT); m.synchronize()
    assert bool((buf == -7.0).all())
    assert m.get_option("stat_disturbance_steps") == 2
    assert np.array_equal(m.disturbance_state(), m.disturbance_response(0, 2, DT)[1])          # (both from a fresh gust state at step 0)
    # clearing: the launches and the bits of before; seed and streams persist across it
    m.clear_disturbances()
    assert m.disturbances()[0] == []
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    again = rollout(m, "simulate", 3, DT)
    for k in KEYS:
        assert np.array_equal(none[k], again[k]), k
    assert m.get_option("stat_disturbance_steps") == 2
    arr = m.pack_disturbances(SETS)
    assert m.lib.pg_set_disturbance_sets(m.h, 4, arr) == 0       # the C call: the seed installed above still holds
    m.set_disturbance_index(IDX)
    check_law(m.disturbance_response(0, 10, DT), "f64", SETS, IDX, np.arange(B), 0, "after clear and re-install")
    m.close()


# ---- 9: the large-batch launch path ------------------------------------------------------------------------------------------------------------------------------------------
def test_large_batch_takes_the_pipelined_launch_under_a_library(pkg, skidpad):
    n, steps = 2341, 3
    idx = (np.arange(n) % 4).astype(np.int32)
    sets = [SETS[0], dict(SETS[1], step_on=1), SETS[2], SETS[3]]          # (three steps: the side gust opens at step 1 here)
    r = histories(pkg, skidpad, "simulate", sets, idx, n, steps, options={"pipe_min": 2341})
    assert r["pipelined"] >= 1 and r["stat"] == steps
    check_law(r["disturbance"], "f64", sets, idx, np.arange(n), 0, "B = 2341")
    worst, share = check_replay(r, "f64", pkg.X1(), sets, idx, "B = 2341")
    print(f"B = 2341: worst |state - disturbed numpy plant| = {worst:.2e}; undisturbed replay apart on {share:.0%}")
    assert share >= 0.5
