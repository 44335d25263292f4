"""GPU tests of the actuator sets (pg_set_actuator_sets / pg_set_actuator_index): command delay, first-order lag and slew limit between the controller and the plant of
pg_simulate_dev and pg_simulate_safety_dev.

Six sets spread over the instances by b % 6 (actuator_numpy.six_sets): identity; delay 3; delay 16 (the cap); tau = 0.05 s on every channel; a slew limit (0.2 rad/s,
5e3 N/s) with delay 1; delay 2 + tau_delta = 0.1 s + feedback = 1.  `skidpadoval`, synthetic.config2_inputs(seed = 4), dt = 0.01, B = 70 (one full wavefront and a ragged
one), 24 steps (more than PG_ACT_MAX_DELAY: the ring wraps).  The yardsticks: tests/actuator_numpy.py for the law (pinned by closed forms in tests/test_actuator_host.py)
and tests/plant_numpy.py for the plant.

Bars.  The law: bit equality wherever a set only delays (no arithmetic); otherwise UNITS = 64 units of eps(real) x max |command| of the channel -- the recurrence
a <- a + alpha (g - a) contracts (alpha >= 0.095 for these sets), so a rounding error of one step has decayed after ~1 / alpha steps and the errors of ~10 steps, a few
eps each, are all that can stand at once.  The plant replay: the node bars of tests/test_gpu_plant_sets.py, 1e-9 (fp64) and 2e-5 (fp32 library) with the same `rel`."""
import ctypes as C

import numpy as np
import pytest

import actuator_numpy
import plant_numpy
from rollout_libs import inputs, join, make, rel, rollout, same, start

pytestmark = pytest.mark.gpu

SEED = 4
DT = 0.01
B = 70
STEPS = 24
UNITS = 64
BAR = {"f64": 1e-9, "f32": 2e-5}
SETS = actuator_numpy.six_sets()
IDX = (np.arange(B) % 6).astype(np.int32)
PURE = np.array([actuator_numpy.is_pure_delay(s) for s in SETS])
DTYPE = {"f64": np.float64, "f32": np.float32}
KEYS = ("state", "control", "command", "applied", "final_state", "final_control")          # what two runs are compared on


def law_bar(commands, precision):
    """[3]: UNITS x eps(real) x max |command| per channel"""
    return UNITS * float(np.finfo(DTYPE[precision]).eps) * np.max(np.abs(commands), axis=(0, 1))


# ---- the command sequence of test 1 (no controller): seeded random walks about a slow sine, steps of the size of the slew limit ------------------------------------------
def law_commands(steps=40):
    rng = np.random.default_rng(20261018)
    k = np.arange(steps)[:, None]
    delta = 0.1 * np.sin(2 * np.pi * k / 37.0 + rng.uniform(0, 6.28, B)[None]) + np.cumsum(0.003 * rng.standard_normal((steps, B)), axis=0)
    fxf = np.cumsum(80.0 * rng.standard_normal((steps, B)), axis=0) - 500.0
    fxr = 800.0 * np.sin(2 * np.pi * k / 23.0 + rng.uniform(0, 6.28, B)[None]) + np.cumsum(60.0 * rng.standard_normal((steps, B)), axis=0)
    c = np.stack([delta, fxf, fxr], axis=2)
    c[5, 0, 0] = -0.0; c[7, 1, 1] = np.nan; c[9, 2, 2] = np.inf          # instances 0 .. 2: identity and the two pure delays carry these through untouched
    return c, IDX


def law_shares(sets, idx, c):
    """(share of (step, instance, channel) on which the slew limit of set 4 binds, share on which the lag of set 3 differs from its input by > 100 fp32 bars), twin alone"""
    finite = np.where(np.isfinite(c), c, 0.0)
    a = actuator_numpy.actuator_response(sets, idx, finite, DT)
    bar = law_bar(finite, "f32")
    sel = idx == 4
    prev = np.concatenate([finite[:1, sel], a[:-1, sel]])
    lim = np.array([sets[4]["rate_delta"], sets[4]["rate_fx"], sets[4]["rate_fx"]]) * DT
    slew = float(np.mean(np.abs(a[:, sel] - prev) >= lim * (1 - 1e-9)))
    lag = float(np.mean(np.abs(a[:, idx == 3] - finite[:, idx == 3]) > 100 * bar))
    return slew, lag


def check_law(applied, commands, precision, sets=SETS, idx=IDX, what=""):
    """applied == twin(commands): bit for bit where the set only delays, within the bar elsewhere; returns the worst difference in units of eps x max |command|"""
    want = actuator_numpy.actuator_response(sets, idx, commands, DT, DTYPE[precision])
    pure = np.array([actuator_numpy.is_pure_delay(s) for s in sets])[idx]
    assert same(applied[:, pure], want[:, pure]), what
    fin = np.where(np.isfinite(commands), commands, 0.0)
    unit = law_bar(fin, precision) / UNITS
    with np.errstate(invalid="ignore"):
        worst = float(np.nanmax(np.abs(applied[:, ~pure] - want[:, ~pure]) / unit))
    print(f"{what} {precision}: law vs twin on the lag / slew sets: worst {worst:.3g} units of eps x max |command| (bar {UNITS}); pure delays bit-equal")
    assert worst <= UNITS, (what, worst)
    return worst


# ---- 1: the law, no controller ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_law_equals_the_twin(pkg, skidpad, precision):
    c, idx = law_commands()
    slew, lag = law_shares(SETS, idx, c)
    print(f"command sequence: slew limit of set 4 binds on {slew:.0%} of its steps, lag of set 3 apart from its input by > 100 bars on {lag:.0%}")
    assert slew >= 0.25 and lag >= 0.5
    m = make(pkg, skidpad, B, precision=precision)
    start(m, inputs(pkg, skidpad, B))
    m.set_actuators(SETS, idx)
    got = m.actuator_response(c, DT)
    c_real = c.astype(DTYPE[precision]).astype(np.float64)
    # the instances with the special values (-0.0, NaN, Inf) only delay: checked by bits; the bar applies to the others, whose commands are finite
    assert PURE[idx[0]] and PURE[idx[1]] and PURE[idx[2]]
    check_law(got, c_real, precision, what="pg_actuator_response")
    # a library of one without an index, and the handle's own state untouched by the call
    m.set_actuators(SETS[5])
    one = m.actuator_response(c, DT)
    check_law(one, c_real, precision, [SETS[5]], np.zeros(B, dtype=int), what="library of one")
    assert same(m.actuator_state(), start(m, inputs(pkg, skidpad, B))[1].astype(DTYPE[precision]))
    m.close()


# ---- 2: rollout replay ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_replay(r, precision, plants, what):
    """2 (a): applied = twin(command); 2 (b): every step replays through the numpy plant with the APPLIED control; 2 (c): ... and not with the command"""
    check_law(r["applied"], r["command"], precision, what=what)
    assert same(r["control"], r["applied"]), what           # the control record under a library is the applied control
    bar = BAR[precision]
    steps = r["state"].shape[0]
    worst = 0.0; apart = np.zeros(r["state"].shape[1])
    for k in range(steps):
        nxt = r["state"][k + 1] if k + 1 < steps else r["final_state"]
        pred = plant_numpy.plant_step_vec(plants, r["state"][k], r["applied"][k], DT)
        err = rel(nxt, pred)
        worst = max(worst, float(err.max()))
        assert err.max() < bar, (what, precision, k, int(np.argmax(err.max(axis=1))), float(err.max()))
        apart = np.maximum(apart, rel(plant_numpy.plant_step_vec(plants, r["state"][k], r["command"][k], DT), pred).max(axis=1))
    return worst, apart


@pytest.mark.parametrize("kind,formulation,precision", [("simulate", "coupled", "f64"), ("simulate", "decoupled", "f64"), ("safety", "coupled", "f64"),
                                                        ("simulate", "coupled", "f32"), ("safety", "coupled", "f32")])
def test_every_step_replays_with_the_applied_control(pkg, skidpad, kind, formulation, precision):
    m = make(pkg, skidpad, B, formulation=formulation, precision=precision)
    m.set_actuators(SETS, IDX)
    start(m, inputs(pkg, skidpad, B), others=kind == "safety")
    # 20 steps in one call, then four calls of one step: behind each of those the control the step computed can be read back (2 (d))
    parts = [rollout(m, kind, STEPS - 4, DT)]
    computed = []
    for _ in range(4):
        computed.append(m.get_next_control())
        parts.append(rollout(m, kind, 1, DT))
    computed.append(m.get_next_control())
    r = join(parts)
    what = f"{kind} {formulation}"
    worst, apart = check_replay(r, precision, pkg.X1(), what)
    share = float(np.mean(apart[IDX != 0] > 100 * BAR[precision]))
    print(f"{what} {precision}: worst |state - numpy plant(applied)| = {worst:.2e} (bar {BAR[precision]:g}); replay with the command apart by > 100 bars on {share:.0%} of the "
          f"instances with a non-identity set")
    assert share >= 0.5, share
    # (d) the command of the next step is the control the step computed; the last one is the handle's control now
    real = DTYPE[precision]
    for i in range(4):
        assert same(r["command"][STEPS - 4 + i], computed[i].astype(real)), i
    assert same(r["final_control"], computed[4].astype(real))
    assert same(m.actuator_state(), r["applied"][-1])
    assert m.get_option("stat_actuator_steps") == STEPS
    m.close()


# ---- 3: identity = no library, bit for bit -------------------------------------------------------------------------------------------------------------------------------
def histories(pkg, traj, kind, sets, idx, formulation="coupled", steps=STEPS):
    m = make(pkg, traj, B, formulation=formulation)
    if sets is not None:
        m.set_actuators(sets, idx)
    start(m, inputs(pkg, traj, B), others=kind == "safety")
    r = rollout(m, kind, steps, DT)
    m.close()
    return r


@pytest.mark.parametrize("kind,formulation", [("simulate", "coupled"), ("simulate", "decoupled"), ("safety", "coupled")])
def test_the_identity_set_equals_no_library_bit_for_bit(pkg, skidpad, kind, formulation):
    none = histories(pkg, skidpad, kind, None, None, formulation)
    assert none["applied"] is None
    for fb in (0, 1):
        one = histories(pkg, skidpad, kind, [actuator_numpy.identity(feedback=fb)], None, formulation)
        for k in ("state", "control", "final_state", "final_control"):
            assert same(none[k], one[k]), (kind, formulation, fb, k)
        assert same(one["applied"], one["command"]) and same(one["applied"], none["control"])
    mixed = histories(pkg, skidpad, kind, SETS, IDX, formulation)
    sel = IDX == 0
    for k in ("state", "control"):
        assert same(none[k][:, sel], mixed[k][:, sel]), (kind, formulation, k)
    assert same(none["final_state"][sel], mixed["final_state"][sel]) and same(none["final_control"][sel], mixed["final_control"][sel])


def test_mixed_library_equals_libraries_of_one_bit_for_bit(pkg, skidpad):
    mixed = histories(pkg, skidpad, "simulate", SETS, IDX)
    base = None
    for j in range(6):
        one = histories(pkg, skidpad, "simulate", [SETS[j]], None)
        sel = IDX == j
        for k in ("state", "control", "command", "applied"):
            assert same(mixed[k][:, sel], one[k][:, sel]), (j, k)
        assert same(mixed["final_state"][sel], one["final_state"][sel]), j
        if j == 0:
            base = one["final_state"]
        else:
            assert np.max(np.abs(one["final_state"] - base)) > 1e-5, j          # the sets are not cosmetic


# ---- 4: what the controller sees -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_controller_sees_the_command_or_the_position(pkg, skidpad):
    m = make(pkg, skidpad, B)
    m.set_actuators(SETS, IDX)
    start(m, inputs(pkg, skidpad, B))
    r = rollout(m, "simulate", STEPS, DT)
    fb = np.array([s["feedback"] for s in SETS])[IDX] == 1
    seen = np.where(fb[:, None], r["applied"][-1], r["command"][-1])
    un = m.u_normalization
    want = np.stack([seen[:, 0] / un[0], (seen[:, 1] + seen[:, 2]) / un[1]], axis=1)
    u_curr = m.qp_data()[:, -5:-3]
    assert same(u_curr, want)
    gap = np.max(np.abs(r["applied"][-1] - r["command"][-1])[fb], axis=1)
    print(f"feedback = 1 set at the last step: |applied - command| between {gap.min():.2e} and {gap.max():.2e}")
    assert np.all(gap > 1e-6)
    m.close()


# ---- 5: continuation and restart -----------------------------------------------------------------------------------------------------------------------------------------
def test_continuation_and_restart(pkg, skidpad):
    whole = histories(pkg, skidpad, "simulate", SETS, IDX)
    m = make(pkg, skidpad, B)
    m.set_actuators(SETS, IDX)
    start(m, inputs(pkg, skidpad, B))
    split = join([rollout(m, "simulate", 10, DT), rollout(m, "simulate", 14, DT)])
    for k in KEYS:
        assert same(whole[k], split[k]), k                  # ring and position continue across calls
    m.reset(); start(m, inputs(pkg, skidpad, B))                            # the clock restarts: the same 24 steps again
    assert same(m.actuator_state(), split["command"][0])
    again = rollout(m, "simulate", STEPS, DT)
    for k in KEYS:
        assert same(whole[k], again[k]), k
    # a new index between two calls resets nothing: instances that keep their set stay bit-identical, the others change from the next step on
    idx2 = np.where(np.arange(B) % 7 == 3, (IDX + 1) % 6, IDX).astype(np.int32)
    m.reset(); start(m, inputs(pkg, skidpad, B))
    first = rollout(m, "simulate", 10, DT)
    m.set_actuator_index(idx2)
    swapped = join([first, rollout(m, "simulate", 14, DT)])
    keep = idx2 == IDX
    for k in ("state", "control", "command", "applied"):
        assert same(swapped[k][:, keep], whole[k][:, keep]), k
        assert same(swapped[k][:10], whole[k][:10]), k
    assert not same(swapped["applied"][10:, ~keep], whole["applied"][10:, ~keep])
    # ... an instance whose delay grew reads commands that were already in the ring: the twin over the whole command history with the new sets from step 10 on
    grew = np.flatnonzero((IDX == 0) & (idx2 == 1))              # identity -> delay 3
    assert grew.size >= 1
    assert same(swapped["applied"][10:, grew], swapped["command"][7:21, grew])
    m.close()


# ---- 6: composition ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_composition_with_plants_sensors_tunings_and_the_summary(pkg, skidpad):
    import sensor_numpy
    plants = plant_numpy.four_plants(pkg.X1)
    pidx = (np.arange(B) % 4).astype(np.int32)
    m = make(pkg, skidpad, B)
    cp = pkg.CoupledControlParams()
    m.set_control_params([cp, dict(cp, Q_e=2.0, R_ddelta=0.2)], ((np.arange(B) // 2) % 2).astype(np.int32))
    m.set_plants(plants, pidx)
    m.set_sensors(sensor_numpy.four_sensors(), ((np.arange(B) // 3) % 4).astype(np.int32), seed=7)
    m.set_actuators(SETS, IDX)
    m.set_option("tracking_summary", 1)
    start(m, inputs(pkg, skidpad, B))
    r = rollout(m, "simulate", STEPS, DT)
    own = plant_numpy.stack_vehicles([plants[i] for i in pidx], B)
    worst, apart = check_replay(r, "f64", own, "composition")
    share = float(np.mean(apart[IDX != 0] > 100 * BAR["f64"]))
    print(f"composition: worst |state - numpy plant of the instance's own set (applied)| = {worst:.2e}; the command apart on {share:.0%}")
    assert share >= 0.5
    sm, n, fx = m.tracking_summary()
    assert np.all(n == STEPS) and np.all(np.isfinite(sm))
    assert m.get_option("stat_actuator_steps") == STEPS and m.get_option("stat_sensor_steps") == STEPS
    m.close()


def test_large_batch_takes_the_pipelined_launch_under_a_library(pkg, skidpad):
    n, steps = 2341, 3
    idx = (np.arange(n) % 6).astype(np.int32)
    m = make(pkg, skidpad, n, options={"pipe_min": 2341})
    start(m, inputs(pkg, skidpad, n))
    m.set_actuators(SETS, idx)
    r = rollout(m, "simulate", steps, DT)
    assert m.get_option("stat_pipelined_launches") >= 1 and m.get_option("stat_actuator_steps") == steps
    check_law(r["applied"], r["command"], "f64", idx=idx, what="B = 2341")
    for k in range(steps):
        nxt = r["state"][k + 1] if k + 1 < steps else r["final_state"]
        assert rel(nxt, plant_numpy.plant_step_vec(pkg.X1(), r["state"][k], r["applied"][k], DT)).max() < BAR["f64"], k
    m.close()


# ---- 7: contract ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_contract(pkg, skidpad):
    import torch
    from pigeon_jl_amd import _lib
    cap = 80
    m = make(pkg, skidpad, cap)
    start(m, inputs(pkg, skidpad, B), others=True)
    # a handle that never installed a library: the launch counter stays at zero, the state call returns the control, the histories are refused
    none = rollout(m, "simulate", 3, DT)
    assert m.get_option("stat_actuator_steps") == 0 and m.get_actuators()[0] == []
    assert same(m.actuator_state(), none["final_control"])
    buf = torch.full((2, B, 3), -7.0, dtype=torch.float64, device=f"cuda:{m.cfg.device}")
    assert m.lib.pg_set_applied_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == -4 and m.lib.pg_set_command_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == -4
    with pytest.raises(pkg.PigeonError):
        m.actuator_response(np.zeros((2, B, 3)), DT)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert m.lib.pg_set_actuator_index(m.h, B, i32(IDX)) == -2          # no library to index
    m.set_actuators(SETS)

    def rollouts_refuse():
        assert m.lib.pg_simulate_dev(m.h, 1, C.c_double(DT), None, None) == -4
        assert m.lib.pg_simulate_safety_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None, None) == -4
    rollouts_refuse()                                            # several sets and no index
    with pytest.raises(pkg.PigeonError):
        m.actuator_response(np.zeros((2, B, 3)), DT)
    m.set_actuator_index(IDX[:B - 1])
    rollouts_refuse()                                            # an index shorter than the batch
    m.set_actuator_index(IDX)
    before = m.get_actuators()
    assert before[0] == SETS and np.array_equal(before[1], IDX)          # round trip

    def rejected(rc, word=None):
        assert rc == -2
        if word:
            msg = m.lib.pg_last_error(m.h).decode()
            assert word in msg and "set 1" in msg, msg
        after = m.get_actuators()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    arr = m.pack_actuators(SETS)
    rejected(m.lib.pg_set_actuator_sets(m.h, 0, arr))
    rejected(m.lib.pg_set_actuator_sets(m.h, -1, arr))

    def two(**bad):
        a = m.pack_actuators([SETS[0], SETS[3]])
        for k, v in bad.items():
            setattr(a[1], k, v)
        return a
    nan, inf = float("nan"), float("inf")
    for field, values in (("tau_delta", (-1e-9, nan, inf)), ("tau_fx", (-1.0, nan, inf)), ("rate_delta", (0.0, -1.0, nan)), ("rate_fx", (0.0, -inf, nan)),
                          ("delay_steps", (17, -1)), ("feedback", (2, -1))):
        for v in values:
            rejected(m.lib.pg_set_actuator_sets(m.h, 2, two(**{field: v})), field)
    for bad_idx in (np.where(np.arange(B) == 5, 6, IDX), np.where(np.arange(B) == 69, -1, IDX)):
        rejected(m.lib.pg_set_actuator_index(m.h, B, i32(bad_idx)))
    rejected(m.lib.pg_set_actuator_index(m.h, 0, i32(IDX)))
    rejected(m.lib.pg_set_actuator_index(m.h, cap + 1, i32(np.zeros(cap + 1))))
    # the node callback is out of scope under a library: PG_ERR_STATE, and it works again once the library is cleared
    assert m.lib.pg_simulate_node_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None) == -4
    assert "actuator" in m.lib.pg_last_error(m.h).decode()
    assert m.lib.pg_node_step_dev(m.h, 0, None, None, None, None) == -4
    assert "actuator" in m.lib.pg_last_error(m.h).decode()
    # pg_step ignores the library
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=SEED)
    plain = make(pkg, skidpad, cap)
    u0 = plain.step_(state, control, t0, time_offset=toff)
    m.reset()
    u1 = m.step_(state, control, t0, time_offset=toff)
    assert all(np.array_equal(a, b) for a, b in zip(u0, u1))
    plain.close()
    # a rollout call that FAILS consumes the one-shot histories: the successful call behind it writes nothing to those buffers
    start(m, inputs(pkg, skidpad, B), others=True)
    m.set_actuators(SETS)                                        # (installing a library drops the index)
    assert np.all(m.get_actuators()[1] == -1)
    cbuf = torch.full((2, B, 3), -7.0, dtype=torch.float64, device=f"cuda:{m.cfg.device}")
    assert m.lib.pg_set_applied_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == 0 and m.lib.pg_set_command_history_dev(m.h, C.c_void_p(cbuf.data_ptr()), 2) == 0
    rollouts_refuse()
    m.set_actuator_index(IDX)
    m.simulate_(2, DT); m.synchronize()
    assert bool((buf == -7.0).all()) and bool((cbuf == -7.0).all())
    assert m.get_option("stat_actuator_steps") == 2
    m.clear_actuators()
    assert m.get_actuators()[0] == []
    m.reset(); start(m, inputs(pkg, skidpad, B), others=True)
    again = rollout(m, "simulate", 3, DT)                            # the no-library bits are back, and the counter stands
    for k in KEYS:
        assert same(none[k], again[k]), k
    assert m.get_option("stat_actuator_steps") == 2
    m.simulate_node_(2, DT); m.node_step_()                      # ... and the node callback runs again
    m.close()
