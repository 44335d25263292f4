"""GPU tests of the plant sets (pg_set_plant_sets / pg_set_plant_index) and of the tracking summary (pg_get_tracking_state).

Four plants -- X1, mu = 0.5, corner masses + 20 % with Izz x 1.2, Caf / Car - 30 % with Fx_max = 3000 -- spread over the instances by b % 4.  The yardstick is
tests/plant_numpy.py (pinned to the oracle by tests/test_plant_sets_host.py); tolerances are the node bars of DESIGN.md section 5: 1e-9 relative in fp64, 2e-5 in the
fp32 library, relative meaning |got - ref| / max(1, |ref|) per component (the states are O(1) .. O(100) in SI units).

Checked on the CPU with numpy alone before the first GPU visit, `skidpadoval`, synthetic.config2_inputs(seed = 4): after ONE step from the 70 starts the plant under an
instance's own set differs from the plant under X1 by more than 100 x 2e-5 for 96 % of the instances with idx != 0 (median 8e-3 / 4e-3 / 8e-3 for sets 1 / 2 / 3); with
the tube narrowed to +-0.25 m, 50 of the 96 starts lie outside it, 12 leave within 30 steps under the held start control, 34 never do."""
import numpy as np
import pytest

import plant_numpy
from conftest import make_oracle
from rollout_libs import check_summary, inputs, make, narrowed, numpy_summary, rel, rollout, start

pytestmark = pytest.mark.gpu

SEED = 4
BAR = {"f64": 1e-9, "f32": 2e-5}
DT = 0.01


@pytest.fixture(scope="module")
def plants(pkg):
    return plant_numpy.four_plants(pkg.X1)


# ---- 1 / 7: replay of every recorded step against the numpy plant ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,formulation,precision", [("simulate", "coupled", "f64"), ("simulate", "decoupled", "f64"), ("safety", "coupled", "f64"), ("node", "coupled", "f64"),
                                                        ("node", "decoupled", "f64"), ("simulate", "coupled", "f32"), ("safety", "coupled", "f32"), ("node", "coupled", "f32")])
def test_every_step_replays_through_the_numpy_plant_of_its_own_set(pkg, skidpad, plants, kind, formulation, precision):
    B, steps = 70, 12
    idx = (np.arange(B) % 4).astype(np.int32)
    m = make(pkg, skidpad, B, formulation, precision)
    m.set_plants(plants, idx)
    start(m, inputs(pkg, skidpad, B), others=kind != "simulate")
    r = rollout(m, kind, steps, DT)
    qh, uh, final = r["state"], r["control"], r["final_state"]
    own = plant_numpy.stack_vehicles([plants[i] for i in idx], B)
    bar = BAR[precision]
    worst = 0.0; apart = np.zeros(B)
    for k in range(steps):
        nxt = qh[k + 1] if k + 1 < steps else final
        pred = plant_numpy.plant_step_vec(own, qh[k], uh[k], DT)            # (the recorded inputs: float-rounded in the fp32 library)
        err = rel(nxt, pred)
        worst = max(worst, float(err.max()))
        assert err.max() < bar, (kind, formulation, precision, k, int(np.argmax(err.max(axis=1))), float(err.max()))
        apart = np.maximum(apart, rel(plant_numpy.plant_step_vec(plants[0], qh[k], uh[k], DT), pred).max(axis=1))
    # not vacuous: an implementation that ignores the index (X1 for everyone) misses the bar by two orders of magnitude on most instances of the other sets
    share = float(np.mean(apart[idx != 0] > 100 * bar))
    print(f"{kind} {formulation} {precision}: worst |state - numpy plant| = {worst:.2e} (bar {bar:g}); own set vs X1 apart by > 100 bars on {share:.0%} of the instances with idx != 0")
    assert share >= 0.5, share
    m.close()


# ---- 2: the same bits as a library of one; a library of one equal to the handle's vehicle = no library ----------------------------------------------------------------
def histories(pkg, traj, B, steps, sets, idx, kind="simulate", precision="f64", **kw):
    m = make(pkg, traj, B, precision=precision, **kw)
    if sets is not None:
        m.set_plants(sets, idx)
    start(m, inputs(pkg, traj, B), others=kind != "simulate")
    r = rollout(m, kind, steps, DT)
    stat = m.get_option("stat_pipelined_launches")
    m.close()
    return r["state"], r["control"], r["final_state"], stat


def test_mixed_library_equals_libraries_of_one_bit_for_bit(pkg, skidpad, plants):
    B, steps = 256, 8
    idx = (np.arange(B) % 4).astype(np.int32)
    mq, mu, mf, _ = histories(pkg, skidpad, B, steps, plants, idx)
    base = None
    for k in range(4):
        q1, u1, f1, _ = histories(pkg, skidpad, B, steps, [plants[k]], None)
        sel = idx == k
        assert np.array_equal(mq[:, sel], q1[:, sel]) and np.array_equal(mu[:, sel], u1[:, sel]) and np.array_equal(mf[sel], f1[sel]), k
        if k == 0:
            base = f1
        else:
            assert np.max(np.abs(f1 - base)) > 1e-5, k          # the sets are not cosmetic


@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_a_library_of_the_handles_own_vehicle_equals_no_library(pkg, skidpad, kind):
    B, steps = 256, 8
    none = histories(pkg, skidpad, B, steps, None, None, kind)
    one = histories(pkg, skidpad, B, steps, [pkg.X1()], None, kind)
    for a, b in zip(none[:3], one[:3]):
        assert np.array_equal(a, b), kind
    n32 = histories(pkg, skidpad, B, steps, None, None, kind, "f32")
    o32 = histories(pkg, skidpad, B, steps, [pkg.X1()], None, kind, "f32")
    worst = max(float(rel(b, a).max()) for a, b in zip(n32[:3], o32[:3]))
    print(f"fp32 library, {kind}: library of one (X1) vs no library: max relative difference {worst:.2e}, bit-equal: {all(np.array_equal(a, b) for a, b in zip(n32[:3], o32[:3]))}")
    assert worst < BAR["f32"]


# ---- 3: the controller does not see the plant ------------------------------------------------------------------------------------------------------------------------
def test_the_controller_does_not_see_the_plant(pkg, skidpad, plants):
    B = 70
    idx = (np.arange(B) % 4).astype(np.int32)
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=SEED)
    plain = make(pkg, skidpad, B); lib = make(pkg, skidpad, B)
    lib.set_plants(plants)                                   # four sets and NO index: pg_step does not care
    u0, st0, it0 = plain.step_(state, control, t0, time_offset=toff)
    u1, st1, it1 = lib.step_(state, control, t0, time_offset=toff)
    assert np.array_equal(u0, u1) and np.array_equal(st0, st1) and np.array_equal(it0, it1)
    assert np.array_equal(plain.qp_data(), lib.qp_data())
    n0 = plain.nodes(); n1 = lib.nodes()
    assert all(np.array_equal(a, b) for a, b in zip(n0, n1))
    # ... and the first control a rollout computes (recorded as the control of its second step) is the one a handle without a library computes from the same start
    fresh = make(pkg, skidpad, B)
    fresh.set_inputs(state, control, t0, None, toff)
    uf = fresh.simulate_(2, DT, record=True)[4]
    roll = make(pkg, skidpad, B)
    roll.set_plants(plants, idx)
    roll.set_inputs(state, control, t0, None, toff)
    ur = roll.simulate_(2, DT, record=True)[4]
    assert np.array_equal(ur[0], uf[0]) and np.array_equal(ur[1], uf[1]) and np.array_equal(ur[1], u0)
    for m in (plain, lib, fresh, roll):
        m.close()


# ---- 4: contract -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_contract(pkg, skidpad, plants):
    import ctypes as C
    from pigeon_jl_amd import _lib
    B, cap = 70, 80
    idx = (np.arange(B) % 4).astype(np.int32)
    m = make(pkg, skidpad, cap)
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=SEED)
    m.set_inputs(state, control, t0, pkg.synthetic.other_cars(state), toff)
    none = m.simulate_(3, DT, record=True)
    m.set_plants(plants)

    def rollouts_refuse():
        assert m.lib.pg_simulate_dev(m.h, 1, C.c_double(DT), None, None) == -4
        assert m.lib.pg_simulate_safety_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None, None) == -4
        assert m.lib.pg_simulate_node_dev(m.h, 1, C.c_double(DT), 0, 0, None, None, None, None, None, None) == -4
    rollouts_refuse()                                        # n_sets > 1 and no index
    m.set_plant_index(idx[:B - 1])
    rollouts_refuse()                                        # an index shorter than the batch
    m.set_plant_index(idx)
    before = m.plant_sets()
    assert len(before[0]) == 4 and np.array_equal(before[1], idx) and all(before[0][k][f] == plants[k][f] for k in range(4) for f in plant_numpy.VEH_FIELDS)

    def rejected(rc):
        assert rc == -2
        after = m.plant_sets()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    arr = m.pack_vehicles(plants)
    rejected(m.lib.pg_set_plant_sets(m.h, 0, arr))
    rejected(m.lib.pg_set_plant_sets(m.h, -1, arr))
    for field in ["G", "m", "Izz", "L", "a", "b", "mu", "Caf", "Car", "Fx_max", "Px_max", "delta_max"]:
        for bad in (0.0, -1.0):
            rejected(m.lib.pg_set_plant_sets(m.h, 2, m.pack_vehicles([plants[0], dict(plants[1], **{field: bad})])))
    rejected(m.lib.pg_set_plant_sets(m.h, 2, m.pack_vehicles([plants[0], dict(plants[1], Fx_min=0.0)])))
    rejected(m.lib.pg_set_plant_sets(m.h, 2, m.pack_vehicles([plants[0], dict(plants[1], Fx_min=10.0)])))
    for field in plant_numpy.VEH_FIELDS:
        for bad in (float("nan"), float("inf")):
            rejected(m.lib.pg_set_plant_sets(m.h, 1, m.pack_vehicles([dict(plants[2], **{field: bad})])))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    for bad_idx in (np.where(np.arange(B) == 5, 4, idx), np.where(np.arange(B) == 69, -1, idx)):
        rejected(m.lib.pg_set_plant_index(m.h, B, i32(bad_idx)))
    rejected(m.lib.pg_set_plant_index(m.h, 0, i32(idx)))
    rejected(m.lib.pg_set_plant_index(m.h, cap + 1, i32(np.zeros(cap + 1))))
    # clearing restores the no-library bits
    m.clear_plants()
    assert m.plant_sets()[0] == []
    assert m.lib.pg_set_plant_index(m.h, B, i32(idx)) == -2          # no library to index
    m.reset()                                                # (cold again, as the first rollout found the handle)
    m.set_inputs(state, control, t0, pkg.synthetic.other_cars(state), toff)
    again = m.simulate_(3, DT, record=True)
    assert all(np.array_equal(a, b) for a, b in zip(none, again))
    m.close()


def test_installing_an_index_between_rollouts_resets_nothing(pkg, skidpad, plants):
    """The clock runs on, the safety summary's step indices continue and every instance stays warm: a handle whose index is replaced and restored between two rollout
    calls equals, bit for bit, its twin whose index was installed once before the first call -- states, controls, times, iteration counts, polish rounds, first breach."""
    B = 70
    idx = (np.arange(B) % 4).astype(np.int32)
    other = (3 - idx).astype(np.int32)
    grid = pkg.synthetic.hji_grid(dims=(7, 6, 5, 4, 4, 5, 4), seed=11)

    def run(between):
        m = make(pkg, skidpad, B)
        m.set_hji_cache(*grid)
        st = start(m, inputs(pkg, skidpad, B), others=True)
        m.set_plants(plants, idx)
        m.simulate_safety_(4, DT, use_HJI_policy=True, human="worst")
        if between == "restore":
            m.set_plant_index(other); m.set_plant_index(idx)
        elif between == "replace":
            m.set_plant_index(other)
        s2 = m.simulate_safety_(4, DT, use_HJI_policy=True, human="worst", record=True)
        out = dict(state=s2[0], control=s2[1], t=s2[2], iters=m.solve_info()[1], status=m.solve_info()[0], polish=m.polish_info(), fb=m.safety_summary()[1],
                   qh=s2[4]["state"], uh=s2[4]["control"])
        clock = m.simulate_clock(9, st[2], DT)
        m.close()
        return out, clock
    twin, clock = run(None)
    back, _ = run("restore")
    for k in twin:
        assert np.array_equal(twin[k], back[k]), k
    assert np.array_equal(twin["t"], clock[8])               # eight steps of ONE clock
    swap, _ = run("replace")
    assert np.array_equal(swap["t"], clock[8])
    assert np.array_equal(swap["qh"][0], twin["qh"][0]) and not np.array_equal(swap["qh"][1], twin["qh"][1])      # the new plants act from the next step on
    early = twin["fb"][(twin["fb"] >= 0) & (twin["fb"] < 4)]
    assert np.array_equal(swap["fb"][(twin["fb"] >= 0) & (twin["fb"] < 4)], early)                                  # breaches of the first call keep their step index
    late = swap["fb"][swap["fb"] >= 4]
    print(f"first breaches: {np.sum(twin['fb'] >= 0)} of {B} (twin), {late.size} of them in the second call after a replaced index")
    assert np.all(swap["fb"] < 8)

# ---- 5: the large-batch launch paths ---------------------------------------------------------------------------------------------------------------------------------
def test_large_batch_takes_the_pipelined_launch_under_a_library(pkg, skidpad, plants):
    B, steps = 2341, 3
    idx = (np.arange(B) % 4).astype(np.int32)
    opts = dict(options={"pipe_min": 2341})
    mq, mu, mf, stat = histories(pkg, skidpad, B, steps, plants, idx, **opts)
    assert stat >= 1
    for k in range(4):
        q1, u1, f1, stat1 = histories(pkg, skidpad, B, steps, [plants[k]], None, **opts)
        assert stat1 >= 1
        sel = idx == k
        assert np.array_equal(mq[:, sel], q1[:, sel]) and np.array_equal(mu[:, sel], u1[:, sel]) and np.array_equal(mf[sel], f1[sel]), k


# ---- 6 / 7: tracking summary -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_tracking_summary_equals_numpy_on_the_recorded_history(pkg, oracle_mod, skidpad, plants, precision):
    B, steps = 96, 30
    bar = BAR[precision]
    idx = (np.arange(B) % 4).astype(np.int32)
    tube = narrowed(pkg, skidpad)
    # (the reference receives the inputs as the library holds them: in the fp32 library the tube's channels are float-rounded, like the recorded states)
    orc = make_oracle(oracle_mod, tube if precision == "f64" else pkg.TrajectoryTube(*tube.data.astype(np.float32).astype(np.float64)))
    tidx = np.zeros(B, dtype=int)
    m = make(pkg, tube, B, precision=precision)
    m.set_plants(plants, idx)
    start(m, inputs(pkg, tube, B))
    with pytest.raises(pkg.PigeonError):
        m.tracking_summary()                                 # option off: PG_ERR_STATE
    m.set_option("tracking_summary", 1)
    sm0, n0, fx0 = m.tracking_summary()
    assert np.all(n0 == 0) and np.all(fx0 == -1)              # nothing counted yet
    qh = m.simulate_(steps, DT, record=True)[3]
    want, _, e = numpy_summary([orc], tidx, qh)
    out = (e > 0.25) | (e < -0.25)
    n_start, n_leave, n_never = int(out[0].sum()), int((~out[0] & out.any(axis=0)).sum()), int((~out.any(axis=0)).sum())
    print(f"{precision}: start outside {n_start}, leave {n_leave}, never {n_never}")
    assert min(n_start, n_leave, n_never) >= 8
    worst = check_summary(m.tracking_summary(), want, bar)
    # a second call with the same dt continues the sums and the step indices
    qh2 = m.simulate_(10, DT, record=True)[3]
    both = np.concatenate([qh, qh2])
    want2, _, _ = numpy_summary([orc], tidx, both)
    worst = max(worst, check_summary(m.tracking_summary(), want2, bar))
    assert np.all(m.tracking_summary()[1] == 40)
    # another dt restarts them (and the clock)
    qh3 = m.simulate_(5, 0.02, record=True)[3]
    want3, _, _ = numpy_summary([orc], tidx, qh3)
    worst = max(worst, check_summary(m.tracking_summary(), want3, bar))
    # set_inputs restarts them
    start(m, inputs(pkg, tube, B))
    assert np.all(m.tracking_summary()[1] == 0)
    qh4 = m.simulate_(3, 0.02, record=True)[3]
    want4, _, _ = numpy_summary([orc], tidx, qh4)
    worst = max(worst, check_summary(m.tracking_summary(), want4, bar))
    print(f"{precision}: tracking summary vs numpy, worst relative difference {worst:.2e} (bar {bar:g})")
    m.close()


def test_tracking_summary_off_adds_no_launch_and_changes_no_bit(pkg, skidpad):
    B, steps = 96, 6
    outs = []
    for on in (False, True):
        m = make(pkg, skidpad, B)
        if on:
            m.set_option("tracking_summary", 1)
        start(m, inputs(pkg, skidpad, B))
        r = m.simulate_(steps, DT, record=True)
        stats = [m.get_option(n) for n in ("stat_pipelined_launches", "stat_split_solve_launches", "stat_single_solve_launches", "stat_whole_batch_solves")]
        outs.append((r, stats))
        if not on:
            assert m.lib.pg_get_tracking_state(m.h, None, None, None) == -4
        m.close()
    assert outs[0][1] == outs[1][1]                          # the solver's launch counters: the sequence of the handle without the option
    assert all(np.array_equal(a, b) for a, b in zip(outs[0][0], outs[1][0]))


def test_tracking_summary_with_a_trajectory_library_and_in_the_node_rollout(pkg, oracle_mod, skidpad, plants):
    B, steps = 96, 30
    idx = (np.arange(B) % 4).astype(np.int32)
    tubes = [narrowed(pkg, skidpad), narrowed(pkg, skidpad, half=0.3, shift=0.1)]
    orcs = [make_oracle(oracle_mod, t) for t in tubes]
    tidx = ((np.arange(B) // 3) % 2).astype(np.int32)
    m = make(pkg, tubes[0], B)
    m.set_trajectories(tubes, tidx)
    m.set_plants(plants, idx)
    m.set_option("tracking_summary", 1)
    start(m, inputs(pkg, tubes[0], B), others=True)
    qh = m.simulate_(steps, DT, record=True)[3]
    want, _, _ = numpy_summary(orcs, tidx, qh)
    check_summary(m.tracking_summary(), want, BAR["f64"])
    assert len(set(want[2][tidx == 0]) | set(want[2][tidx == 1])) > 2
    # node rollout, pre_flag off on a third of the steps (for every other instance): the steps still count, the summaries still match
    start(m, inputs(pkg, tubes[0], B), others=True)
    pre = np.ones((steps, B), dtype=np.uint8); pre[::3, ::2] = 0
    out = m.simulate_node_(steps, DT, pre_flag=pre, record=True)
    hist = out[5]
    assert np.all(hist["event"][::3, ::2] == m.NODE_EVENTS["pre_flag_off"])
    want, _, _ = numpy_summary(orcs, tidx, hist["state"])
    got = m.tracking_summary()
    assert np.all(got[1] == steps)
    check_summary(got, want, BAR["f64"])
    # ... and in the safety rollout
    start(m, inputs(pkg, tubes[0], B), others=True)
    sh = m.simulate_safety_(8, DT, use_HJI_policy=False, record=True)[4]["state"]
    want, _, _ = numpy_summary(orcs, tidx, sh)
    check_summary(m.tracking_summary(), want, BAR["f64"])
    m.close()
