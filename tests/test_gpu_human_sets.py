"""GPU tests of the human sets (pg_set_human_sets / pg_set_human_index / pg_set_human_seed): the driver of the other car per instance in pg_simulate_safety_dev and
pg_simulate_node_dev.

`skidpadoval`, synthetic.hji_grid(dims = (7, 6, 5, 4, 4, 5, 4), seed = 11), synthetic.other_cars, DT = 0.01, B = 96 (a full wavefront and a ragged one), 12 steps.  The
yardstick of the law is tests/human_numpy.py, written from the header and pinned by tests/test_human_host.py.  Bars, both taken from existing files: mode 1 arithmetic
1e-5 relative to max(1, |ref|), the bar tests/test_gpu_safety_rollout.py holds the loop driven by safety_numpy.optimal_disturbance to; mode 3 the gust's
steps x (1e-13 | 2e-5) of tests/test_gpu_disturbance_sets.py.  Everything that is a copy -- modes 0 and 2 at gain 1, held steps, steps outside the window, values on a
limit -- and every comparison between two device runs is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import human_numpy as hn
import rollout_libs as rl
import safety_numpy as sn
from rollout_libs import grid  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SEED = 4                                  # of the synthetic inputs
OTHER_SEED = 43                           # of the other cars: the worst case is non-zero for at least half of the instances at step 0 (asserted in test 1)
DRIVER_SEED = 0x9E3779B97F4A7C15          # of the draws: high word non-zero
WORST_BAR = 1e-5                          # tests/test_gpu_safety_rollout.py
DRAW_BAR = {"f64": 1e-13, "f32": 2e-5}    # tests/test_gpu_disturbance_sets.py, per step of the recursion
DTYPE = {"f64": np.float64, "f32": np.float32}
DT = 0.01
B = 96
STEPS = 12
SETS = hn.four_humans()
IDX = (np.arange(B) % 4).astype(np.int32)
MIXED = [hn.identity(0), hn.identity(1), hn.identity(2)]
MODE_NAME = ("hold", "worst", "script")
RUN = dict(use_HJI_policy=True, summary=True)          # of every rollout here but the decoupled one: the policy on, the safety summary read


@pytest.fixture(scope="module")
def inputs(pkg, skidpad):
    """state, control, t0, toff, other of the 96 instances and the script [STEPS][B][2]"""
    rng = np.random.default_rng(3)
    script = np.stack([rng.uniform(-0.5, 0.5, (STEPS, B)), rng.uniform(-3.0, 3.0, (STEPS, B))], axis=2)
    return rl.inputs(pkg, skidpad, B, SEED, OTHER_SEED) + (script,)


def assert_same_run(a, b, what, cols=None, skip=("human_u",)):
    """two runs, every history and final state bit for bit (cols: the instances compared, as (columns of a, columns of b))"""
    keys = [k for k in a if k not in skip and a[k] is not None]
    assert keys == [k for k in b if k not in skip and b[k] is not None], (what, keys)          # both runs produced the same records
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if cols is not None:
            ax = 1 if k in rl.RECORDS else 0
            x = np.take(x, cols[0], axis=ax); y = np.take(y, cols[1], axis=ax)
        assert rl.same(x, y), (what, k)


def other_libraries(pkg, m, kind):
    """the other six libraries (five under the node rollout, which refuses an actuator library) at non-identity sets"""
    import actuator_numpy
    import disturbance_numpy
    import estimator_numpy
    import plant_numpy
    import sensor_numpy
    n = np.arange(B)
    cp = pkg.CoupledControlParams()
    m.set_control_params([cp, dict(cp, Q_e=2.0, R_ddelta=0.2)], ((n // 2) % 2).astype(np.int32))
    m.set_plants(plant_numpy.four_plants(pkg.X1), ((n // 4) % 4).astype(np.int32))
    m.set_sensors(sensor_numpy.four_sensors(), ((n // 3) % 4).astype(np.int32), seed=7)
    if kind == "safety":
        m.set_actuators(actuator_numpy.six_sets(), (n % 6).astype(np.int32))
    m.set_disturbances(disturbance_numpy.four_disturbances(), (n % 4).astype(np.int32), seed=11)
    m.set_estimators(estimator_numpy.four_estimators(), ((n // 5) % 4).astype(np.int32))
    m.set_option("tracking_summary", 1)


def lookups(m, states, others):
    """x7 [steps][B][7] and vg8 [steps][B][8] of recorded states and other cars, through relative_state and pg_hji_lookup"""
    x7 = np.stack([sn.relative_state(s, o) for s, o in zip(states, others)])
    vg8 = np.zeros(x7.shape[:2] + (8,))
    for k in range(x7.shape[0]):
        V, g = m.hji_lookup(x7[k])
        vg8[k, :, 0] = V; vg8[k, :, 1:] = g
    return x7, vg8


def check_law(pkg, got, precision, sets, idx, streams, step0, x7, vg8, script, what, has_hji=True, lanes=None):
    """got [steps][B][2] against the twin from a fresh state at step0.  Copies bit for bit -- exact values against the twin (the script and the limits as the library's
    element type holds them), held steps against the device's own decision --, mode 1 arithmetic within WORST_BAR, mode 3 arithmetic within steps x DRAW_BAR"""
    steps = got.shape[0]
    cast = lambda a: None if a is None else np.asarray(a, dtype=np.float64).astype(DTYPE[precision]).astype(np.float64)
    sets_r = [dict(s, omega_max=float(cast(s["omega_max"])), a_min=float(cast(s["a_min"])), a_max=float(cast(s["a_max"]))) for s in sets]
    want, how, decided = hn.response(pkg.X1(), sets_r, idx, DRIVER_SEED, streams, step0, steps, DT, cast(x7), cast(vg8), cast(script), has_hji=has_hji, explain=True)
    k = np.arange(step0, step0 + steps)[:, None]
    held = (decided >= 0) & (decided != k)
    lanes = np.ones(got.shape[1], dtype=bool) if lanes is None else lanes
    worst = {hn.FROM_WORST: 0.0, hn.FROM_RANDOM: 0.0}; count = {hn.EXACT: 0, hn.FROM_WORST: 0, hn.FROM_RANDOM: 0, "held": 0}
    for j in range(steps):
        for b in np.nonzero(lanes)[0]:
            if held[j, b]:
                assert rl.same(got[j, b], got[decided[j, b] - step0, b]), (what, "held", j, b)
                count["held"] += 1
                continue
            for c in range(2):
                h = int(how[j, b, c])
                count[h] += 1
                if h == hn.EXACT:
                    assert rl.same(got[j, b, c], want[j, b, c]), (what, "copy", j, b, c, got[j, b, c], want[j, b, c])
                else:
                    worst[h] = max(worst[h], float(rl.rel(got[j, b, c], want[j, b, c])))
    bar3 = steps * DRAW_BAR[precision]
    print(f"{what} {precision}: {count[hn.EXACT]} copies and {count['held']} held steps bit for bit; mode 1 arithmetic ({count[hn.FROM_WORST]} values) worst "
          f"{worst[hn.FROM_WORST]:.3g} (bar {WORST_BAR:.3g}); mode 3 arithmetic ({count[hn.FROM_RANDOM]} values) worst {worst[hn.FROM_RANDOM]:.3g} (bar {bar3:.3g})")
    assert worst[hn.FROM_WORST] <= WORST_BAR and worst[hn.FROM_RANDOM] <= bar3, (what, worst)
    return count


# ---- 1: the law, no controller ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_response_equals_the_twin(pkg, skidpad, grid, inputs, precision):
    state, control, t0, toff, other, script = inputs
    m = rl.make(pkg, skidpad, B, grid=grid, precision=precision)
    rl.start(m, inputs, others=True)
    # the other car drives on at its speed while the ego stands: twelve different relative states per instance
    others = [other]
    for _ in range(STEPS - 1):
        others.append(sn.other_car_step(others[-1], np.zeros((B, 2)), 0.3))
    x7, vg8 = lookups(m, [state] * STEPS, others)
    cast = lambda a: a.astype(DTYPE[precision]).astype(np.float64)
    w0 = sn.optimal_disturbance(pkg.X1(), cast(x7[0]), cast(vg8[0])[:, 1:])
    live = int(np.count_nonzero(np.any(w0 != 0.0, axis=1)))
    print(f"worst case non-zero at step 0 on {live} of {B} instances")
    assert live >= B // 2
    m.set_humans(SETS, IDX, seed=DRIVER_SEED, streams=rl.stream_ids(B))
    for step0 in (0, 4):
        got = m.human_response(step0, x7, vg8, DT, script)
        count = check_law(pkg, got, precision, SETS, IDX, rl.stream_ids(B), step0, x7, vg8, script, f"pg_human_response from step {step0}")
        assert count[hn.FROM_WORST] > 0 and count[hn.FROM_RANDOM] > 0 and count["held"] > 0
    # the call leaves the handle's driver state and the clock alone: no step has run
    with pytest.raises(pkg.PigeonError):
        m.human_state()
    assert m.get_option("stat_human_steps") == 0
    m.close()


# ---- 2: the identity sets are the three human modes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_others", [False, True], ids=["alone", "with_the_other_libraries"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["safety", "node"])
def test_the_identity_set_reproduces_the_human_mode(pkg, skidpad, grid, inputs, kind, precision, with_others):
    script = inputs[5]
    for mode in (0, 1, 2):
        runs = []
        for lib in (False, True):
            m = rl.make(pkg, skidpad, B, grid=grid, precision=precision)
            if with_others:
                other_libraries(pkg, m, kind)
            if lib:
                m.set_humans(hn.identity(mode), seed=DRIVER_SEED)
            rl.start(m, inputs, others=True)
            # (under the library the argument no longer decides: the call asks for another mode, the set's is what runs)
            human = MODE_NAME[(mode + 1) % 2] if lib else MODE_NAME[mode]
            runs.append(rl.rollout(m, kind, STEPS, DT, human=human, human_u=script if mode == 2 else None, **RUN))
            if lib:
                assert m.get_option("stat_human_steps") == STEPS and rl.same(m.human_state(), runs[1]["human_u"][-1])
            else:
                assert m.get_option("stat_human_steps") == 0
            m.close()
        assert_same_run(runs[0], runs[1], (kind, precision, mode))
        if kind == "safety":
            assert rl.same(runs[1]["human_u"], runs[1]["human"])
            if mode == 1:
                assert np.count_nonzero(runs[0]["human"]) > 0
            if mode == 2:
                assert rl.same(runs[1]["human"], script.astype(DTYPE[precision]))


# ---- 3: a mixed library is the per-instance composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["safety", "node"])
def test_a_mixed_library_is_the_composition_per_instance(pkg, skidpad, grid, inputs, kind, precision):
    script = inputs[5]
    idx = (np.arange(B) % 3).astype(np.int32)
    m = rl.make(pkg, skidpad, B, grid=grid, precision=precision)
    m.set_humans(MIXED, idx)
    rl.start(m, inputs, others=True)
    mixed = rl.rollout(m, kind, STEPS, DT, human_u=script, **RUN)
    m.close()
    for mode in (0, 1, 2):
        u = rl.make(pkg, skidpad, B, grid=grid, precision=precision)
        rl.start(u, inputs, others=True)
        uniform = rl.rollout(u, kind, STEPS, DT, human=MODE_NAME[mode], human_u=script if mode == 2 else None, **RUN)
        u.close()
        cols = np.nonzero(idx == mode)[0]
        assert_same_run(mixed, uniform, (kind, precision, mode), cols=(cols, cols))


# ---- 4: the window ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_window_is_the_script_zeroed_outside_it(pkg, skidpad, grid, inputs):
    script = inputs[5]
    m = rl.make(pkg, skidpad, B, grid=grid)
    m.set_humans(hn.identity(2, step_on=3, step_off=6))
    rl.start(m, inputs, others=True)
    lib = rl.rollout(m, "safety", STEPS, DT, human_u=script, **RUN)
    m.close()
    cut = script.copy(); cut[:3] = 0.0; cut[6:] = 0.0
    u = rl.make(pkg, skidpad, B, grid=grid)
    rl.start(u, inputs, others=True)
    ref = rl.rollout(u, "safety", STEPS, DT, human="script", human_u=cut, **RUN)
    u.close()
    assert_same_run(lib, ref, "window")
    assert rl.same(lib["human_u"], cut)


# ---- 5: hold ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_held_worst_case(pkg, skidpad, grid, inputs):
    m = rl.make(pkg, skidpad, B, grid=grid)
    held = hn.identity(1, hold_steps=3)
    m.set_humans(held)
    rl.start(m, inputs, others=True)
    r = rl.rollout(m, "safety", STEPS, DT, **RUN)
    H = r["human"]
    for k in range(STEPS):
        assert rl.same(H[k], H[k - k % 3]), k
    decisions = H[[0, 3, 6, 9]]
    assert np.any(np.any(decisions != decisions[:1], axis=(0, 2)))
    x7, vg8 = lookups(m, r["state"], r["other"])
    got = m.human_response(0, x7, vg8, DT)
    err = float(rl.rel(H, got).max())
    print(f"held worst case: the rollout's history against pg_human_response on the reconstructed x7 / vg8: worst {err:.3g} (bar {WORST_BAR:.3g})")
    assert err <= WORST_BAR
    check_law(pkg, H, "f64", [held], None, np.arange(B), 0, x7, vg8, None, "held worst case, rollout history")
    m.close()


# ---- 6: clock rules -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["safety", "node"])
def test_clock_rules(pkg, skidpad, grid, inputs, kind):
    script = inputs[5]
    ids = rl.stream_ids(B)

    def run(split, between=None):
        m = rl.make(pkg, skidpad, B, grid=grid)
        m.set_humans(SETS, IDX, seed=DRIVER_SEED, streams=ids)
        rl.start(m, inputs, others=True)
        parts = []; k0 = 0
        for i, n in enumerate(split):
            if i and between == "reinstall":
                m.set_humans([SETS[0]], None); m.set_humans(SETS, IDX, seed=1); m.set_human_index(IDX); m.set_human_seed(DRIVER_SEED, ids)
            if i and between == "clear":
                m.clear_humans(); m.set_humans(SETS, IDX, seed=DRIVER_SEED, streams=ids)
            parts.append(rl.rollout(m, kind, n, DT, human_u=script[k0:k0 + n], **RUN)); k0 += n
        return m, rl.join(parts)
    m, whole = run([STEPS])
    assert m.get_option("stat_human_steps") == STEPS
    m.reset(); rl.start(m, inputs, others=True)                               # pg_set_inputs: the clock restarts and the run replays (pg_reset: from cold solvers, as the first run)
    again = rl.rollout(m, kind, STEPS, DT, human_u=script, **RUN)
    assert_same_run(whole, again, "replay", skip=())
    m.close()
    for between in (None, "reinstall"):
        m, split = run([5, 7], between)
        assert_same_run(whole, split, ("5 + 7", between), skip=())
        m.close()
    # the hold phase and the AR state did continue: the random lanes decide at even steps only, and step 5 holds step 4
    rnd = IDX == 3
    assert rl.same(whole["human_u"][5][rnd], whole["human_u"][4][rnd]) and not rl.same(whole["human_u"][6][rnd], whole["human_u"][4][rnd])
    # after a clear the next install starts fresh: a decision at step 5, and the law from a fresh state there (the worst-case lanes need x7: left out)
    m, cleared = run([5, 7], "clear")
    m.close()
    assert rl.same(cleared["human_u"][:5], whole["human_u"][:5]) and not rl.same(cleared["human_u"][5][rnd], cleared["human_u"][4][rnd])
    check_law(pkg, cleared["human_u"][5:], "f64", SETS, IDX, ids, 5, None, None, script[5:], "after a clear", has_hji=False, lanes=IDX != 1)


def test_a_stream_draws_the_same_sequence_in_any_batch(pkg, skidpad, grid, inputs):
    ids = rl.stream_ids(B)
    rnd = hn.identity(3, sigma=[0.2, 1.5], tau=0.05)
    z7 = np.zeros((STEPS, B, 7)); z8 = np.zeros((STEPS, B, 8))
    big = rl.make(pkg, skidpad, B, grid=grid)
    rl.start(big, inputs, others=True)
    big.set_humans(rnd, seed=DRIVER_SEED, streams=ids)
    u96 = big.human_response(0, z7, z8, DT)
    r96 = rl.rollout(big, "safety", STEPS, DT, **RUN)
    big.close()
    slots = np.arange(B - 1, B - 33, -1)                      # the last 32 instances, in reverse order
    small = rl.make(pkg, skidpad, B, grid=grid)
    rl.start(small, [a[slots] for a in inputs[:5]] + [None], 32, others=True)
    small.set_humans(rnd, seed=DRIVER_SEED, streams=ids[slots])
    u32 = small.human_response(0, z7[:, :32], z8[:, :32], DT)
    r32 = rl.rollout(small, "safety", STEPS, DT, **RUN)
    small.close()
    assert rl.same(u32, u96[:, slots]) and np.count_nonzero(u96) == u96.size
    assert rl.same(r32["human_u"], r96["human_u"][:, slots]) and rl.same(r32["human"], r96["human"][:, slots])
    assert rl.same(r96["human_u"], u96)


# ---- 7: contract --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_contract(pkg, skidpad, grid, inputs):
    import torch
    script = inputs[5]
    m = rl.make(pkg, skidpad, B, grid=grid)
    rl.start(m, inputs, others=True)
    m.set_humans(SETS, IDX, seed=DRIVER_SEED)
    before = m.humans()
    bad = [dict(mode=4), dict(mode=-1), dict(hold_steps=0), dict(step_on=-1), dict(gain=[1.5, 1.0]), dict(gain=[1.0, -0.1]), dict(gain=[np.nan, 1.0]),
           dict(omega_max=np.nan), dict(omega_max=-1.0), dict(a_min=0.5), dict(a_min=np.nan), dict(a_max=-0.5), dict(a_max=np.nan), dict(sigma=[-1.0, 0.0]),
           dict(sigma=[0.0, np.inf]), dict(tau=-1.0), dict(tau=np.inf), dict(tau=np.nan)]
    for field in bad:
        with pytest.raises(pkg.PigeonError) as e:
            m.set_humans([hn.identity(0), hn.identity(**{"mode": 0, **field})], IDX % 2)
        assert "set 1" in str(e.value) and list(field)[0] in str(e.value), (field, str(e.value))
        after = m.humans()
        assert str(after[0]) == str(before[0]) and np.array_equal(after[1], before[1]), field
    with pytest.raises(pkg.PigeonError):
        m.human_state()                                       # no step yet
    with pytest.raises(pkg.PigeonError):
        m.simulate_safety_(2, DT, human="hold")               # a set has mode 2: the script is wanted whatever the argument says
    with pytest.raises(pkg.PigeonError):
        m.human_response(0, np.zeros((2, B, 7)), np.zeros((2, B, 8)), DT)
    with pytest.raises(pkg.PigeonError):
        m.set_human_index(np.full(B, 4, dtype=np.int32))
    m.set_humans(SETS, IDX[:B - 1])                           # an index that does not cover the batch
    with pytest.raises(pkg.PigeonError):
        m.simulate_safety_(2, DT, human_u=script[:2])
    m.set_human_index(IDX)
    # the one-shot history is consumed by a failing call
    buf = torch.full((2, B, 2), -7.0, dtype=torch.float64, device="cuda")
    assert m.lib.pg_set_human_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) == 0
    with pytest.raises(pkg.PigeonError):
        m.simulate_safety_(2, DT)                             # (no script)
    m.simulate_safety_(2, DT, human_u=script[:2]); m.synchronize()
    assert bool((buf == -7.0).all()) and m.get_option("stat_human_steps") == 2
    assert m.human_state().shape == (B, 2)
    # pg_simulate_dev never reads the library: no script wanted, nothing counted
    m.simulate_(2, DT)
    assert m.get_option("stat_human_steps") == 2
    rl.start(m, inputs, others=True)
    with pytest.raises(pkg.PigeonError):
        m.human_state()                                       # forgotten with the inputs
    m.clear_humans()
    assert m.humans()[0] == [] and m.lib.pg_set_human_history_dev(m.h, C.c_void_p(buf.data_ptr()), 2) != 0
    m.simulate_safety_(2, DT, human="hold")
    assert m.get_option("stat_human_steps") == 2
    m.close()


def test_the_other_entry_points_never_read_the_library(pkg, skidpad, grid, inputs):
    state, control, t0, toff, other, _ = inputs
    outs = []
    for lib in (False, True):
        m = rl.make(pkg, skidpad, B, grid=grid)
        if lib:
            m.set_humans(SETS, None, seed=DRIVER_SEED)        # four sets, a script set among them, and NO index: none of these calls cares
        u = m.step_(state, control, t0, other_car_state=other, time_offset=toff)
        qp = m.qp_data()
        m.set_inputs(state, control, t0, other, toff)
        m.compute_time_steps_(); m.compute_linearization_nodes_(); m.update_QP_(); m.solve_()
        u_phase = m.get_next_control()
        m.set_inputs(state, control, t0, other, toff)
        m.step_dev(); m.synchronize()
        u_dev = m.get_next_control()
        node = m.node_step_()
        sim = m.simulate_(3, DT, record=True)
        outs.append(list(u) + [qp, u_phase, u_dev] + list(node) + [x for x in sim if x is not None] + [m.get_option("stat_human_steps")])
        m.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)
    assert outs[1][-1] == 0


# ---- 8: the decoupled node rollout ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_decoupled_node_rollout_has_no_worst_case(pkg, skidpad, inputs):
    runs = []
    for lib in (False, True):
        m = rl.make(pkg, skidpad, B, formulation="decoupled", hji_eps=1.0)        # (a lateral handle takes no grid: there is no safety row)
        if lib:
            m.set_humans(hn.identity(1))
        rl.start(m, inputs, others=True)
        runs.append(rl.rollout(m, "node", STEPS, DT, human="worst", summary=True))
        m.close()
    assert_same_run(runs[0], runs[1], "decoupled node")
    assert rl.same(runs[1]["human_u"], np.zeros((STEPS, B, 2)))


# ---- 9: one large batch -------------------------------------------------------------------------------------------------------------------------------------------------
def test_large_batch_takes_the_pipelined_launch_under_a_library(pkg, skidpad, grid):
    n, steps = 2341, 2
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, n, seed=SEED)
    other = pkg.synthetic.other_cars(state, seed=OTHER_SEED)
    rng = np.random.default_rng(3)
    script = np.stack([rng.uniform(-0.5, 0.5, (steps, n)), rng.uniform(-3.0, 3.0, (steps, n))], axis=2)
    inp = (state, control, t0, toff, other, script)
    idx = (np.arange(n) % 3).astype(np.int32)
    big = rl.make(pkg, skidpad, n, grid=grid, options={"pipe_min": n})
    big.set_humans(MIXED, idx)
    rl.start(big, inp, n, others=True)
    rb = rl.rollout(big, "safety", steps, DT, human_u=script, **RUN)
    assert big.get_option("stat_pipelined_launches") >= 1 and big.get_option("stat_human_steps") == steps
    assert rl.same(big.human_state(), rb["human_u"][-1])
    big.close()
    small = rl.make(pkg, skidpad, B, grid=grid)
    small.set_humans(MIXED, idx[:B])
    rl.start(small, inp, B, others=True)
    rs = rl.rollout(small, "safety", steps, DT, human_u=script[:, :B], **RUN)
    small.close()
    assert_same_run(rb, rs, "B = 2341 against B = 96", cols=(np.arange(B), np.arange(B)), skip=())
    assert rl.same(rb["human_u"][:, idx == 0], np.zeros((steps, int(np.sum(idx == 0)), 2))) and rl.same(rb["human_u"][:, idx == 2], script[:, idx == 2])
    assert np.count_nonzero(rb["human_u"][:, idx == 1]) > 0
