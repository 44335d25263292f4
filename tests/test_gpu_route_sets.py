"""GPU tests of the route library (pg_set_route_sets; k_route): an instance changes trajectory during a rollout.

Handles come from rollout_libs.make: capacity 8, B = 6, 5 steps.  The trajectory library has three tubes cut from the skidpad oval, so they overlap in space and a switched
car can track: 300 knots (a lane of the projection strides its loop five times), every eighth knot of the first 401 (51 knots: lanes 50 to 63 never see a segment) and the
first 200 knots under a slower profile (another time base).  dt = 2^-6 and the start times are multiples of 2^-6, so every clock element is exact whether the clock runs
on or restarts: final_t is asserted equal bit for bit wherever a split run is compared.

The manual twin of an event is what a host had to do before: stop, read the state back, pg_set_trajectory_index, pg_set_inputs with the same state, control and t0 and the
new offsets, pg_reset with the mask of the switched instances, start again.  Without other libraries the two are the same computation, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import actuator_numpy
import disturbance_numpy
import estimator_numpy
import human_numpy
import rollout_libs as rl
import route_numpy as rn
import sensor_numpy
from rollout_libs import grid  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

CAP, B, STEPS, DT = 8, 6, 5, 2.0 ** -6
N_TRAJ = 3
HOME = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
T_JOIN = 3.0


@pytest.fixture(scope="module")
def tubes(pkg, skidpad):
    d = skidpad.data
    slow = d[:, :200].copy(); slow[0] = slow[0] / 0.75; slow[2] = slow[2] * 0.75; slow[3] = slow[3] * 0.75 ** 2
    t = [pkg.TrajectoryTube(*d[:, :300]), pkg.TrajectoryTube(*d[:, 0:401:8]), pkg.TrajectoryTube(*slow)]
    assert [len(x) for x in t] == [300, 51, 200]
    return t


@pytest.fixture(scope="module")
def inp(pkg, tubes):
    """B instances on the first 30 m of the oval (inside all three tubes), trajectory mode, start times on the 2^-6 grid, with other cars"""
    state, control, t0, toff = pkg.synthetic.config2_inputs(tubes[2], B, seed=21, s_range=(5.0, 30.0))
    t0 = np.round(t0 * 64.0) / 64.0
    return state, control, t0, toff, pkg.synthetic.other_cars(state, seed=43)


def make(pkg, tubes, formulation="coupled", precision="f64", home=HOME, **kw):
    m = rl.make(pkg, tubes, CAP, formulation=formulation, precision=precision, **kw)
    m.set_trajectory_index(home)
    return m


def start(m, inp, others, toff=None, state=None):
    state_, control, t0, toff_, other = inp
    m.set_inputs(state_ if state is None else state, control, t0, other if others else None, toff_ if toff is None else toff)


def run(m, kind, steps, **kw):
    return rl.rollout(m, kind, steps, DT, **kw)


def assert_same(got, want, keys=rl.KEYS, sel=None, what=""):
    for k in keys:
        a, b = got[k], want[k]
        if sel is not None and a is not None and b is not None:
            a, b = (a[:, sel], b[:, sel]) if k in rl.RECORDS else (a[sel], b[sel])
        assert rl.same(a, b), (what, k)


def manual_switch(m, kind, part, new_index, new_toff, switched):
    """what a host did before the library: the state read back (the finals of `part`), the new index, the same state, control and t0 with the new offsets, the switched cold"""
    m.set_trajectory_index(new_index)
    m.set_inputs(part["final_state"], part["final_control"], part["final_t"], part["final_other"] if kind != "simulate" else None, new_toff)
    m.reset(np.asarray(switched, dtype=np.uint8))


KINDS = [("simulate", "coupled"), ("simulate", "decoupled"), ("safety", "coupled")]


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_sets_without_events_reproduce_the_handle_without_a_library(pkg, tubes, inp, kind, precision):
    others = kind != "simulate"
    ref = make(pkg, tubes, precision=precision); start(ref, inp, others)
    want = run(ref, kind, STEPS, summary=others)
    ref.close()
    for sets, index in (([rn.route()], None), ([rn.route(), rn.route()], np.arange(B) % 2)):
        m = make(pkg, tubes, precision=precision)
        m.set_routes(sets, index); start(m, inp, others)
        plain = run(m, kind, 2)
        assert m.get_option("stat_route_steps") == 0            # no event in any set: the launches of a handle without a library
        hist = m.record_route(3)                                # ... and with a record every wavefront writes its history word and leaves
        rest = run(m, kind, 3, summary=others)
        assert m.get_option("stat_route_steps") == 3 and np.array_equal(hist.cpu().numpy(), np.tile(HOME, (3, 1)))
        st = m.route_state()
        assert np.array_equal(st["traj"], HOME) and not st["fired"].any() and np.all(st["last_step"] == -1) and np.isnan(st["t_at"]).all() and np.isnan(st["e_at"]).all()
        m.close()
        assert_same(rl.join([plain, rest]), want, what=(kind, precision, len(sets)))


# ---- 2. the manual twin -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchor", [rn.KEEP, rn.PATH, rn.STAMP])
@pytest.mark.parametrize("kind,formulation", KINDS)
def test_an_event_equals_the_manual_switch(pkg, tubes, inp, kind, formulation, anchor):
    others = kind != "simulate"
    tj = T_JOIN if anchor == rn.STAMP else 0.0
    sets = [rn.route(), rn.route(rn.event(2, 2, anchor, t_join=tj)), rn.route(rn.event(2, -1, anchor, relative=True, t_join=tj))]
    index = np.array([0, 1, 2, 0, 1, 2])
    m = make(pkg, tubes, formulation); m.set_routes(sets, index); start(m, inp, others)
    hist = m.record_route(STEPS)
    got = run(m, kind, STEPS)
    ran, fired, last = rn.schedule(sets, index, HOME, N_TRAJ, 0, STEPS)
    assert np.array_equal(hist.cpu().numpy(), ran) and ran[-1].tolist() == [0, 2, 2, 1, 2, 0]
    st = m.route_state()
    assert np.array_equal(st["traj"], ran[-1]) and np.array_equal(st["fired"], fired) and np.array_equal(st["last_step"], last)
    m.close()

    w = make(pkg, tubes, formulation); start(w, inp, others)
    first = run(w, kind, 2)
    switched = index != 0
    new_toff = inp[3].copy(); t_at = np.full(B, np.nan)
    for b in np.flatnonzero(switched):
        new_toff[b], t_at[b] = rn.offset_of(sets[index[b]][0], first["final_t"][b], inp[3][b])
    manual_switch(w, kind, first, ran[-1], new_toff, switched)
    second = run(w, kind, 3)
    w.close()
    want = rl.join([first, second])
    assert rl.same(got["final_t"], want["final_t"])             # the precondition: the clock that ran on and the one that restarted hold the same times
    assert_same(got, want, what=(kind, formulation, anchor))
    assert np.array_equal(st["t_at"], t_at, equal_nan=True) and np.isnan(st["e_at"]).all()


@pytest.mark.parametrize("missing", ["nothing", "event", "offset", "cold start", "index"])
def test_the_twin_comparison_sees_each_ingredient_of_an_event(pkg, tubes, inp, missing):
    """A PATH event on every instance at step 2 against a manual twin that leaves one ingredient out -- the whole switch, the new offset, the reset of the switched
    instances, the new index.  The complete twin is equal; each incomplete one gives the records of steps 0 to 2 (the control recorded at step 2 was computed at step 1)
    and another control from step 3 on, for every instance.  (PATH, because the controller reads of a time offset only whether it is NaN -- trajectory mode feeds the
    arclength error into the commanded acceleration --: the VALUE a STAMP or PROJECT event writes is pinned by the test below.)"""
    ev = rn.event(2, 2, rn.PATH)
    m = make(pkg, tubes); m.set_routes([rn.route(ev)]); start(m, inp, False)
    got = run(m, "simulate", STEPS); m.close()
    w = make(pkg, tubes); start(w, inp, False)
    first = run(w, "simulate", 2)
    if missing != "event":
        new_toff = inp[3] if missing == "offset" else np.full(B, np.nan)
        w.set_trajectory_index(HOME if missing == "index" else np.full(B, 2, dtype=np.int32))
        w.set_inputs(first["final_state"], first["final_control"], first["final_t"], None, new_toff)
        if missing != "cold start":
            w.reset(np.ones(B, dtype=np.uint8))
    second = run(w, "simulate", 3); w.close()
    want = rl.join([first, second])
    assert rl.same(got["final_t"], want["final_t"])
    assert rl.same(got["state"][:3], want["state"][:3]) and rl.same(got["control"][:3], want["control"][:3])
    if missing == "nothing":
        assert_same(got, want)
    else:
        assert np.all(np.any(got["control"][3] != want["control"][3], axis=1)), missing


def test_the_offset_an_event_writes_is_what_a_later_keep_event_reads(pkg, tubes, inp):
    """No getter returns time_offset and the kernels read only its NaN-ness, so the value is observed through t_at of a KEEP event, which is t0 - time_offset: a STAMP
    (b0 to b2) or PROJECT (b3 to b5) event at step 1, a KEEP event at step 3.  All times are on the 2^-6 grid but t_proj, and the arithmetic is the twin's."""
    first = [rn.event(1, 2, rn.STAMP, t_join=T_JOIN), rn.event(1, 0, rn.PROJECT, t_join=0.5)]
    index = np.array([0, 0, 0, 1, 1, 1])
    m = make(pkg, tubes); m.set_routes([rn.route(e) for e in first], index); start(m, inp, False)
    run(m, "simulate", 2)
    one = m.route_state(); m.close()
    assert np.all(one["fired"] == 1) and np.all(one["t_at"][:3] == T_JOIN) and np.isfinite(one["t_at"]).all()
    m = make(pkg, tubes); m.set_routes([rn.route(e, rn.event(3, 1, rn.KEEP)) for e in first], index); start(m, inp, False)
    run(m, "simulate", STEPS)
    two = m.route_state(); m.close()
    t1, t3 = inp[2] + DT, inp[2] + 3 * DT
    toff = np.array([rn.offset_of(first[index[b]], t1[b], inp[3][b], t_proj=one["t_at"][b])[0] for b in range(B)])
    assert np.all(two["fired"] == 2) and np.all(two["traj"] == 1) and rl.same(two["t_at"], t3 - toff)
    assert np.all(two["t_at"][:3] == T_JOIN + 2 * DT)


# ---- 3. event placement -----------------------------------------------------------------------------------------------------------------------------------------------
def test_an_event_at_step_zero_equals_installing_target_and_offset_up_front(pkg, tubes, inp):
    sets = [rn.route(), rn.route(rn.event(0, 2, rn.STAMP, t_join=T_JOIN))]
    index = np.array([0, 1, 0, 1, 1, 0])
    m = make(pkg, tubes); m.set_routes(sets, index); start(m, inp, False)
    got = run(m, "simulate", STEPS); m.close()
    home = np.where(index == 1, 2, HOME).astype(np.int32)
    w = make(pkg, tubes, home=home); start(w, inp, False, toff=np.where(index == 1, inp[2] - T_JOIN, inp[3]))
    want = run(w, "simulate", STEPS); w.close()
    assert_same(got, want)


def placement_sets():
    return ([rn.route(), rn.route(rn.event(7, 1)), rn.route(rn.event(1, 1, rn.KEEP), rn.event(3, 0, rn.STAMP, t_join=T_JOIN)), rn.route(rn.event(2, -1, rn.PATH, relative=True))],
            np.array([0, 1, 2, 3, 2, 1]))


@pytest.mark.parametrize("kind", ["simulate", "safety"])
def test_call_boundaries_restarts_and_the_recorded_route(pkg, tubes, inp, kind):
    others = kind != "simulate"
    sets, index = placement_sets()
    ran, fired, last = rn.schedule(sets, index, HOME, N_TRAJ, 0, STEPS)
    assert fired.tolist() == [0, 0, 2, 1, 2, 0] and last.tolist() == [-1, -1, 3, 2, 3, -1]
    m = make(pkg, tubes); m.set_routes(sets, index); start(m, inp, others)
    hist = m.record_route(STEPS)
    one = run(m, kind, STEPS)
    assert np.array_equal(hist.cpu().numpy(), ran)              # the recorded route is the twin's schedule
    st = m.route_state()
    assert np.array_equal(st["traj"], ran[-1]) and np.array_equal(st["fired"], fired) and np.array_equal(st["last_step"], last)
    # an event that never fires (step 7) and the identity set: the run without a library, per instance
    w = make(pkg, tubes); start(w, inp, others)
    plain = run(w, kind, STEPS); w.close()
    assert_same(one, plain, sel=fired == 0)
    assert not rl.same(one["control"][:, fired > 0], plain["control"][:, fired > 0])
    # new inputs restart the clock: nothing fired; the return home is applied when the next rollout starts, and until then `traj` reports what the phase calls run on
    m.reset(); start(m, inp, others)
    st = m.route_state()
    assert np.array_equal(st["traj"], ran[-1]) and not st["fired"].any() and np.all(st["last_step"] == -1) and np.isnan(st["t_at"]).all()
    # 2 + 3 steps with the event of step 2 at the call boundary
    h1 = m.record_route(2); a = run(m, kind, 2)
    h2 = m.record_route(3); b = run(m, kind, 3)
    assert np.array_equal(np.concatenate([h1.cpu().numpy(), h2.cpu().numpy()]), ran)
    st = m.route_state()
    assert np.array_equal(st["traj"], ran[-1]) and np.array_equal(st["fired"], fired) and np.array_equal(st["last_step"], last)
    two = rl.join([a, b])
    assert rl.same(two["final_t"], one["final_t"])
    assert_same(two, one, what="2 + 3 against 5, replayed from home")
    # after the rollout the phase calls run on the trajectory switched to; pg_set_trajectory_index installs home and current together
    m.compute_time_steps_(); m.compute_linearization_nodes_()
    m.set_trajectory_index(HOME)
    assert np.array_equal(m.route_state()["traj"], HOME)
    m.clear_routes()
    m.close()


# ---- 4. PROJECT -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_project_joins_the_target_where_k_project_puts_the_seen_state(pkg, tubes, inp, precision):
    """b0 identity; b1, b2 project on tube 1 at step 2 (t_join 0.5 and -0.25); b3 sits exactly on interior knot 10 of tube 1 (two segments tie at distance 0: the lower
    index must win) and b4 has a NaN position, both with the event at step 0, where the seen state is the installed one; b5 projects on tube 0 (300 knots) at step 2."""
    state = inp[0].copy()
    state[3, 0] = tubes[1].E[10]; state[3, 1] = tubes[1].N[10]
    state[4, 0] = np.nan
    sets = [rn.route(), rn.route(rn.event(2, 1, rn.PROJECT, t_join=0.5)), rn.route(rn.event(2, 1, rn.PROJECT, t_join=-0.25)), rn.route(rn.event(0, 1, rn.PROJECT)),
            rn.route(rn.event(2, -1, rn.PROJECT, relative=True, t_join=0.125))]
    index = np.array([0, 1, 2, 3, 3, 4]); home = np.array([0, 0, 2, 0, 2, 1], dtype=np.int32)
    ran, fired, last = rn.schedule(sets, index, home, N_TRAJ, 0, STEPS)
    assert ran[-1].tolist() == [0, 1, 1, 1, 1, 0]
    m = make(pkg, tubes, precision=precision, home=home); m.set_routes(sets, index); start(m, inp, False, state=state)
    hist = m.record_route(STEPS)
    got = run(m, "simulate", STEPS)
    st = m.route_state(); m.close()
    assert np.array_equal(hist.cpu().numpy(), ran) and np.array_equal(st["traj"], ran[-1]) and np.array_equal(st["fired"], fired)
    # the recorded pre-switch states on a handle whose index is the target: its projection is what the event used
    seen = np.stack([got["state"][max(last[b], 0), b] for b in range(B)])
    p = make(pkg, tubes, precision=precision, home=ran[-1]); start(p, inp, False, state=seen)
    p.compute_time_steps_(); p.compute_linearization_nodes_()
    sep = p.path_coordinates(); p.close()
    ev = fired > 0
    fin = ev & (np.arange(B) != 4)
    assert rl.same(st["t_at"][fin], sep[fin, 2]) and rl.same(st["e_at"][fin], sep[fin, 1])
    assert np.isnan(st["t_at"][4]) and np.isnan(st["e_at"][4]) and np.isnan(sep[4, 2]) and np.isnan(st["t_at"][0]) and np.isnan(st["e_at"][0])
    assert st["e_at"][3] == 0.0 and abs(st["t_at"][3] - tubes[1].t[10]) < 1e-4       # on the knot: segments 9 and 10 tie at distance 0, and the equality above says which one won
    tw = rn.project(tubes[1].data, seen[1, 0], seen[1, 1])
    bar = 2e-5 if precision == "f32" else 1e-9                                  # (the bars of tests/test_gpu_f32.py and tests/test_gpu_parity.py)
    assert abs(st["t_at"][1] - tw[2]) <= bar * max(1.0, abs(tw[2])) and abs(st["e_at"][1] - tw[1]) <= bar * max(1.0, abs(tw[1]))
    # ... and the manual twin with the offset computed from the read-back
    tj = np.array([sets[index[b]][0]["t_join"] for b in range(B)])
    w = make(pkg, tubes, precision=precision, home=np.where(last == 0, ran[-1], home).astype(np.int32))
    toff0 = np.where(last == 0, inp[2] - (st["t_at"] + tj), inp[3])
    assert np.isnan(toff0[4]) and np.isfinite(toff0[3])
    start(w, inp, False, state=state, toff=toff0)
    first = run(w, "simulate", 2)
    at2 = last == 2
    new_toff = np.where(at2, first["final_t"] - (st["t_at"] + tj), toff0)
    manual_switch(w, "simulate", first, ran[-1], new_toff, at2)
    second = run(w, "simulate", 3); w.close()
    want = rl.join([first, second])
    assert rl.same(got["final_t"], want["final_t"])
    assert_same(got, want, what=("project", precision))
    assert np.isnan(got["final_state"][4]).any() and np.isfinite(np.delete(got["final_state"], 4, axis=0)).all()


# ---- 5. node rollout --------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_stamp_event_brings_an_instance_back_inside_the_window(pkg, tubes, inp):
    """the window of the node callback is [0, trajectory.t[end]] of the instance's own tube: instance 1 starts on the slow tube (it ends at 10.4 s) at t = 11 s, outside;
    at step 2 it is handed tube 1, which ends at 15.7 s"""
    state, control, t0, toff, other = inp
    late = t0.copy(); late[1] = 11.0
    assert tubes[2].t[-1] < 11.0 < tubes[0].t[-1] < tubes[1].t[-1]
    late_inp = (state, control, late, toff, other)
    sets = [rn.route(), rn.route(rn.event(2, 1, rn.STAMP, t_join=T_JOIN))]
    index = np.array([0, 1, 0, 0, 0, 0]); home = np.array([0, 2, 0, 1, 1, 1], dtype=np.int32)
    m = make(pkg, tubes, home=home); m.set_routes(sets, index); start(m, late_inp, True)
    got = run(m, "node", STEPS)
    _, heartbeat, counts = m.node_summary(); m.close()
    w = make(pkg, tubes, home=home); start(w, late_inp, True)
    plain = run(w, "node", STEPS)
    _, hb_plain, _ = w.node_summary(); w.close()
    OUT = pkg.BatchedTrajectoryTrackingMPC.NODE_EVENTS["outside_trajectory"]
    assert plain["event"][:, 1].tolist() == [OUT] * 5 and hb_plain[1] == 0
    assert got["event"][:2, 1].tolist() == [OUT, OUT] and np.all(got["event"][2:, 1] != OUT)
    assert heartbeat[1] == 3 and counts[1, 1] == 2
    others = np.arange(B) != 1
    assert_same(got, plain, sel=others)
    assert np.array_equal(heartbeat[others], hb_plain[others])


# ---- 6. cold = 0 ------------------------------------------------------------------------------------------------------------------------------------------------------
def rel_inf(a, b, floor=1.0):
    a = np.asarray(a); b = np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(floor, float(np.max(np.abs(b)))))


def test_cold_zero_keeps_the_warm_start_and_both_loops_follow_the_oracle_on_the_switched_trajectory(pkg, oracle_mod, tubes, inp):
    """b1 and b4 go to tube 1 at step 2 with cold = 1, b2 and b5 with cold = 0 (KEEP: tubes 0 and 1 share a time base); b0 and b3 run the identity set.  The rollout is
    taken one step per call, so that every step's nodes, QP data, solution and solve_info can be read.  What a warm and a cold start are is what the reference makes of
    mpc.solved: the warm branch of compute_linearization_nodes! seeds the nodes from the previous solution, the cold one from the steady state.  Per step and instance the
    oracle ON THE TRAJECTORY THE INSTANCE IS ON NOW, told solved = true or false as the event's flag says, gives the nodes within 1e-9, and the applied (normalised)
    control is within 1e-6 of the exact optimum of the step's QP data: the bars of tests/test_gpu_parity.py::test_warm_second_step, no new number.  On the event step the
    flag is seen both ways: the cold = 0 instances do not match the cold oracle, the cold = 1 instances do not match the warm one; solve_info reports both SOLVED."""
    from conftest import make_oracle
    orcs = [make_oracle(oracle_mod, t) for t in tubes]
    sets = [rn.route(), rn.route(rn.event(2, 1, rn.KEEP, cold=True)), rn.route(rn.event(2, 1, rn.KEEP, cold=False))]
    index = np.array([0, 1, 2, 0, 1, 2])
    ran, _, _ = rn.schedule(sets, index, HOME, N_TRAJ, 0, STEPS)
    state, control, t, toff = pkg.synthetic.config2_inputs(tubes[0], B, seed=7, s_range=(5.0, 30.0))      # on the profile of tubes 0 and 1, as the parity tests start
    t = np.round(t * 64.0) / 64.0
    m = make(pkg, tubes); m.set_routes(sets, index); m.set_inputs(state, control, t, None, toff)
    x_prev = None
    worst_nodes = worst_u = 0.0
    for k in range(STEPS):
        out = m.simulate_(1, DT)
        qs, us, ps = m.nodes(); qp = m.qp_data(); x, _ = m.solution(); st, it, _, _ = m.solve_info(); pol = m.polish_info()
        print(f"step {k}: status {st.tolist()} iters {it.tolist()} polish {pol.tolist()}")
        assert np.all(st == pkg.SOLVED), (k, st)
        for b in range(B):
            orc = orcs[ran[k, b]]
            ts, dt = orc.time_steps(t[b])
            cold_ev = k == 2 and index[b] == 1
            warm = k > 0 and not cold_ev
            node = lambda solved: orc.nodes(state[b], control[b], ts, dt, time_offset=toff[b], **(dict(solved=True, prev_ts=ts, prev_q=x_prev[b, :, :6], prev_u=x_prev[b, :, 6:]) if solved else {}))
            oq, ou, op = node(warm)
            err = max(rel_inf(qs[b], oq), rel_inf(us[b], ou), rel_inf(ps[b], op))
            worst_nodes = max(worst_nodes, err)
            assert err < 1e-9, (k, b, warm, err)
            if k == 2 and index[b] != 0:                         # the event step: the other start is NOT what ran
                oq2, ou2, _ = node(not warm)
                assert max(rel_inf(qs[b], oq2), rel_inf(us[b], ou2)) > 1e-6, (b, warm)
            xe, ye, info = orc.solve_exact(qp[b])
            assert info["status"] == 1
            eu = rel_inf(x[b, 1, 6:], orc.split_x(xe)["u"][1])
            worst_u = max(worst_u, eu)
            assert eu < 1e-6, (k, b, eu)
        x_prev = x
        state, control, t = out[0], out[1], out[2]
    print(f"worst nodes {worst_nodes:.2e} (bar 1e-9), worst applied control {worst_u:.2e} (bar 1e-6)")
    rs = m.route_state()
    assert rs["traj"].tolist() == [0, 1, 1, 1, 1, 1] and rs["fired"].tolist() == [0, 1, 1, 0, 1, 1]
    m.close()


# ---- 7. together with the seven other libraries -------------------------------------------------------------------------------------------------------------------------
SEED = rl.NOISE_SEED
ACTUATORS = [actuator_numpy.identity(tau_delta=0.05, tau_fx=0.05), actuator_numpy.identity(delay_steps=1, tau_delta=0.1, feedback=1)]


def everything(pkg, tubes, inp, grid, precision, kind):
    m = rl.make(pkg, tubes, CAP, precision=precision, grid=grid, N_short=1, N_long=0)
    m.set_trajectory_index(HOME)
    m.set_control_params([{"Q_e": 1.0}, {"Q_e": 2.0}], np.arange(B) % 2)
    m.set_plants([pkg.X1(), pkg.X1(mu=0.8)], (np.arange(B) // 2) % 2)
    m.set_sensors([sensor_numpy.four_sensors()[1]], seed=SEED, streams=rl.stream_ids(B))
    m.set_estimators([estimator_numpy.identity(gain=[0.2, 0.3, 0.4, 0.5, 0.6, 0.7], predict=1)])
    m.set_disturbances([disturbance_numpy.identity(Fy=500.0, sigma_Fx=300.0, sigma_Fy=800.0, x_cp=1.0, tau_gust=0.3)], seed=SEED + 1)
    if kind != "node":
        m.set_actuators(ACTUATORS, (np.arange(B) % 2).astype(np.int32))
    if kind != "simulate":
        m.set_humans([human_numpy.four_humans()[3]], seed=SEED + 2)
    m.set_routes([rn.route(), rn.route(rn.event(1, 1, rn.PROJECT, relative=True, t_join=0.25)), rn.route(rn.event(2, 2, rn.STAMP, t_join=T_JOIN))], np.arange(B) % 3)
    start(m, inp, kind != "simulate")
    return m


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_three_steps_equal_two_and_one_under_every_library_at_once(pkg, tubes, inp, grid, kind, precision):
    """the other libraries' states (gust, streams, actuator ring, estimate, driver) do not restart at a switch: one call against two, the events inside and at the boundary"""
    kw = dict(measured=True, estimated=True, use_HJI_policy=True, summary=kind != "simulate")
    a = everything(pkg, tubes, inp, grid, precision, kind)
    ha = a.record_route(3)
    A = run(a, kind, 3, **kw)
    sa = a.route_state(); a.close()
    b = everything(pkg, tubes, inp, grid, precision, kind)
    h1 = b.record_route(2); B1 = run(b, kind, 2, **kw)
    h2 = b.record_route(1); B2 = run(b, kind, 1, **kw)
    sb = b.route_state(); b.close()
    ran, fired, last = rn.schedule([rn.route(), rn.route(rn.event(1, 1, relative=True)), rn.route(rn.event(2, 2))], np.arange(B) % 3, HOME, N_TRAJ, 0, 3)
    assert np.array_equal(ha.cpu().numpy(), ran) and np.array_equal(np.concatenate([h1.cpu().numpy(), h2.cpu().numpy()]), ran)
    assert np.array_equal(sa["fired"], fired) and all(rl.same(sa[k], sb[k]) for k in sa)
    AB = rl.join([B1, B2])
    assert {"state", "control", "measured", "estimated", "disturbance"} <= {k for k in rl.KEYS if A[k] is not None}
    for k in rl.KEYS:
        assert rl.same(AB[k], A[k]), (kind, precision, k)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(pkg, tubes, skidpad, inp):
    ev = rn.event
    # every text of route_set_problem, as the library says it, with the set named
    m = make(pkg, tubes); start(m, inp, False)
    bad = {rn.BAD_TARGET_MODE: dict(ev(1, 0), target_mode=2), rn.BAD_ANCHOR: dict(ev(1, 0), anchor=4), rn.BAD_COLD: dict(ev(1, 0), cold=2), rn.BAD_RESERVED: dict(ev(1, 0), reserved=1),
           rn.BAD_T_JOIN: ev(1, 0, t_join=np.inf), rn.T_JOIN_UNUSED: ev(1, 0, rn.KEEP, t_join=0.5), rn.NEGATIVE_TARGET: ev(1, -1)}
    lists = {why: rn.route(e) for why, e in bad.items()}
    lists[rn.USED_BEHIND_UNUSED] = [ev(-1, 0), ev(2, 1), ev(-1, 0), ev(-1, 0)]
    lists[rn.NOT_INCREASING] = rn.route(ev(2, 0), ev(2, 1))
    assert set(lists) == set(rn.PROBLEMS)
    for why, rset in lists.items():
        assert rn.problem(rset) == why
        with pytest.raises(pkg.PigeonError, match="status -2"):
            m.set_routes([rn.route(), rset])
        assert rl.last_error(m) == "pg_set_route_sets: set 1: " + why
        assert m.routes()[0] == []                              # the handle is left without a library
    # a route history without a library; a null buffer; fewer than one step
    assert m.lib.pg_set_route_history_dev(m.h, None, 0) == rl.OK
    with pytest.raises(pkg.PigeonError, match="no route library installed"):
        m.record_route(2)
    m.set_routes([rn.route(ev(1, 5))])                          # (an absolute target beyond the library is refused when a rollout starts, not here)
    assert m.lib.pg_set_route_history_dev(m.h, None, 3) == rl.INVALID and "a device buffer" in rl.last_error(m)
    buf = m.record_route(2)
    assert m.lib.pg_set_route_history_dev(m.h, C.c_void_p(buf.data_ptr()), 0) == rl.INVALID and "steps >= 1" in rl.last_error(m)
    assert m.lib.pg_set_route_history_dev(m.h, None, 0) == rl.OK
    # an absolute target >= n_traj
    assert rl.rollout_status(m, "sensor") == rl.STATE and "absolute target 5 outside the installed trajectory library of 3" in rl.last_error(m)
    # several sets without an index that covers the batch
    m.set_routes([rn.route(), rn.route(ev(1, 1))], np.zeros(B - 1, dtype=np.int32))
    assert rl.rollout_status(m, "sensor") == rl.STATE and "pg_set_route_index does not cover the batch" in rl.last_error(m)
    m.set_route_index(np.arange(B) % 2)
    assert rl.rollout_status(m, "sensor") == rl.OK
    assert m.route_state()["fired"].tolist() == [0, 1] * 3
    # a trajectory index that does not cover B; no trajectory library
    m.set_trajectories(tubes)                                   # (a new library drops the index)
    assert rl.rollout_status(m, "sensor") == rl.STATE and "pg_set_trajectory_index does not cover the batch" in rl.last_error(m)
    m.set_trajectory_index(HOME[:B - 1])
    assert rl.rollout_status(m, "sensor") == rl.STATE and "does not cover the batch" in rl.last_error(m)
    m.set_trajectory(skidpad)
    assert rl.rollout_status(m, "sensor") == rl.STATE and "no trajectory library of at least two trajectories" in rl.last_error(m)
    # ... and the handle still runs: without the library, and with it on a library again
    m.clear_routes()
    assert rl.rollout_status(m, "sensor") == rl.OK
    m.set_trajectories(tubes, HOME); m.set_routes([rn.route(ev(0, 1))]); start(m, inp, False)
    got = run(m, "simulate", 2)
    assert np.array_equal(m.route_state()["traj"], np.ones(B, dtype=np.int32)) and np.isfinite(got["final_state"]).all()
    m.close()
