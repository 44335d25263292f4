"""The device-resident entry points (pg_set_inputs_dev, pg_step_dev, pg_get_next_control_dev, pg_get_next_control_hji_dev, pg_hji_lookup_dev, pg_hji_lookup8_dev) against
their host twins, bit for bit, in every arrangement of the step's launches.

The path the benchmark times and a multi-GPU rank runs is: inputs already in device memory, pg_step_dev writing the controls into the CALLER's array (SolveOut::u_out2, written by
every k_solve instantiation itself; the lateral kernel's controls are copied by pg_get_next_control_dev), on a stream the caller chose.  The host twins (pg_step, ...) never pass
such an array.  Instances are independent and both paths run the same kernels on the same per-instance data: only where the inputs come from and where the controls go differs, so
every comparison here is on raw bits and takes no tolerance.

Every stepping case runs two handles of the same capacity, options, precision and formulation through the same call sequence -- one through set_inputs_dev / step_dev on a
non-default stream into a sentinel-filled tensor of capacity + 8 rows, one through step_ -- and checks (Pair.step): rows < B of the caller's array are the host's u, no sentinel
left; rows >= B still hold the sentinel; status and iteration counts are equal; get_next_control() and get_next_control_dev of the device-side handle return the same bits as the
caller's array; both handles took the same launches, and the case says which (the "stat_*" counters, read as tests/test_gpu_launch_paths.py reads them).

Two anchors outside the code under test: the caller's array of the plain coupled cold step and of the plain lateral N = 20 cold step against the oracle, at the bounds
tests/test_gpu_parity.py::test_solve_matches_exact_optimum and tests/test_gpu_decoupled.py::test_decoupled_matches_oracle apply to u; the fp32 cold step at the bound of
tests/test_gpu_f32.py::test_f32_end_to_end_against_the_oracle_on_identical_inputs."""
import math

import numpy as np
import pytest

from conftest import make_oracle
from rollout_libs import grid  # noqa: F401  (the fixture)
from test_gpu_launch_paths import COUPLED_STATS, LATERAL_STATS, PLAIN_LATERAL, only

pytestmark = pytest.mark.gpu

SENTINEL = -777.25                  # finite, exact in both element types, no control of these batches
SRC_SENTINEL = -7
INVALID, STATE = -2, -4             # PG_ERR_INVALID, PG_ERR_STATE (include/pigeon_mpc.h)
STATS = COUPLED_STATS + ("stat_pipelined_launches",) + LATERAL_STATS
PIPED = {"pipe_min": 64}            # (tests/test_gpu_launch_paths.py: the pipelined nodes + update_QP launch from 64 instances on)
_stream = []


def stream():
    """the ONE non-default stream every device-side handle of this file runs on"""
    import torch
    if not _stream:
        _stream.append(torch.cuda.Stream())
    return _stream[0]


def bits(a):
    """a float array as unsigned integers of its own width (-0.0 is not 0.0, a NaN equals itself); an integer array as it is"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def wide(t):
    """a device tensor of the library's element type as float64 on the host (exact: what the host calls return)"""
    return t.cpu().numpy().astype(np.float64)


def f32_round(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def filled(m, shape, value=SENTINEL, dtype=None):
    torch, tdt, dev = m._torch()
    return torch.full(shape, value, dtype=tdt if dtype is None else dtype, device=dev)


def on_stream(m):
    """everything torch queued so far has finished; the handle runs on the file's stream from here on"""
    import torch
    torch.cuda.synchronize()
    m.set_stream(stream().cuda_stream)


def refused(pkg, call, what, status, text):
    """the wrapper raises with the status and the whole text of pg_last_error"""
    with pytest.raises(pkg.PigeonError) as e:
        call()
    assert str(e.value) == f"{what} failed with status {status}: {text}"


def dev_step(m, state, control, t0, toff=None, other=None):
    """One step through the device-resident calls: numpy inputs as tensors of the library's element type (t0, time_offset: float64), the caller's control array with
    capacity + 8 sentinel rows.  Returns (the array as float64 [capacity + 8, 3], status, iters)."""
    torch, tdt, dev = m._torch()
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dt).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    B = len(t0)
    s, c, o = up(state, tdt), up(control, tdt), up(other, tdt)
    t, f = up(t0, torch.float64), up(toff, torch.float64)
    u = filled(m, (m.capacity + 8, 3))
    on_stream(m)
    m.set_inputs_dev(B, ptr(s), ptr(c), ptr(t), ptr(o), ptr(f))
    m.step_dev(u.data_ptr())
    m.synchronize()                 # (s, c, o, t, f, u are alive until here)
    st, it = m.solve_info()[:2]
    return wide(u), st, it


class Pair:
    """two handles made alike: `dev` stepped through the device-resident calls, `ref` through the host calls"""

    def __init__(self, pkg, traj, cap, formulation="coupled", fusion=None, pipeline=None, grid=None, **kw):
        self.pkg = pkg
        self.f32 = kw.get("precision") == "f32"
        self.both = [pkg.BatchedTrajectoryTrackingMPC(traj, cap, formulation=formulation, phase_timing=False, **kw) for _ in range(2)]
        self.dev, self.ref = self.both
        for m in self.both:
            if fusion is not None:
                m.set_fusion(fusion)
            if pipeline is not None:
                m.set_pipeline(pipeline)
            if grid is not None:
                m.set_hji_cache(*grid)

    def stats(self):
        return [{n: m.get_option(n) for n in STATS} for m in self.both]

    def step(self, state, control, t0, toff=None, other=None):
        """the same step on both handles and every check the two paths share; returns (the caller's array rows < B, status, iters, what the step added to the counters)"""
        if self.f32:                # (both sides see the same float32 values)
            state, control, other = f32_round(state), f32_round(control), f32_round(other)
        B = len(t0)
        before = self.stats()
        u, st, it = dev_step(self.dev, state, control, t0, toff, other)
        uh, sth, ith = self.ref.step_(state, control, t0, other_car_state=other, time_offset=toff)
        grew = [{n: a[n] - b[n] for n in STATS} for a, b in zip(self.stats(), before)]
        assert same(u[:B], uh), f"{int(np.sum(np.any(bits(u[:B]) != bits(uh), axis=1)))} of {B} rows of the caller's array differ from the host's u"
        assert not np.any(u[:B] == SENTINEL)
        assert np.all(u[B:] == SENTINEL), "pg_step_dev wrote beyond row B of the caller's array"
        assert np.array_equal(st, sth) and np.array_equal(it, ith)
        assert same(self.dev.get_next_control(), u[:B])
        v = filled(self.dev, (self.dev.capacity + 8, 3))
        on_stream(self.dev)
        self.dev.get_next_control_dev(v.data_ptr())
        self.dev.synchronize()
        v = wide(v)
        assert same(v[:B], u[:B]) and np.all(v[B:] == SENTINEL)
        assert grew[0] == grew[1], grew
        return u[:B], st, it, grew[0]

    def close(self):
        for m in self.both:
            m.close()


def coupled_pair(pkg, traj, cap, N_long=20, options=None, **kw):
    return Pair(pkg, traj, cap, N_short=10, N_long=N_long, options=options, **kw)


def lateral_pair(pkg, traj, cap, N_long=10, options=None, **kw):
    p = Pair(pkg, traj, cap, formulation="decoupled", vehicle=pkg.X1(), N_short=10, N_long=N_long, options=options, **kw)
    assert all(m.get_option("lateral_solver_in_use") == 1.0 for m in p.both)
    return p


def split_piped(grew, piped):
    return (grew["stat_pipelined_launches"] > 0) == piped and only(grew, COUPLED_STATS, "stat_split_solve_launches")


@pytest.fixture(scope="module")
def inputs(pkg, skidpad):
    """config2_inputs of 128 instances, the seed of tests/test_gpu_launch_paths.py; a case of B instances takes the B it draws itself (the draws depend on B)"""
    return {B: pkg.synthetic.config2_inputs(skidpad, B, seed=12345) for B in (128, 96, 77, 64)}


# ---- coupled formulation -------------------------------------------------------------------------------------------------------------------------------------------------
def test_plain_cold_and_warm_and_the_oracle(pkg, oracle_mod, skidpad, inputs):
    """One launch per phase, one solve kernel; the cold step's array also against the exact optimum of the QP data the handle solved, the bound of
    tests/test_gpu_parity.py:143 (test_solve_matches_exact_optimum: 1e-6 relative-inf on normalised controls)."""
    B = 128
    p = coupled_pair(pkg, skidpad, B, options={"solve_split": 0}, fusion=0, pipeline=0)
    u, st, _, grew = p.step(*inputs[B])
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, "stat_single_solve_launches"), grew
    assert np.all(st == pkg.SOLVED), st
    orc = make_oracle(oracle_mod, skidpad)
    qp = p.dev.qp_data()
    un = np.array([orc.u_norm[0], orc.u_norm[1], orc.u_norm[1]])
    worst = 0.0
    for b in range(B):
        xe, _, info = orc.solve_exact(qp[b])
        assert info["status"] == 1
        uo = orc.next_control(orc.split_x(xe)["u"][1]) / un
        worst = max(worst, float(np.max(np.abs(u[b] / un - uo)) / max(1.0, float(np.max(np.abs(uo))))))
    print(f"plain coupled cold step, caller's array against the oracle: worst {worst:.2e} (bound 1e-6)")
    assert worst < 1e-6, worst
    u2, st2, _, grew = p.step(*inputs[B])
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, "stat_single_solve_launches"), grew
    assert np.all(pkg.is_solved(st2)), st2
    p.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_split_solve_behind_the_pipelined_launch_cold_and_warm(pkg, oracle_mod, skidpad, inputs, precision):
    """Rounds-only launch + list-mode launch; the cold step behind the pipelined nodes + update_QP launch, the warm one (no recurrence) behind the warm nodes kernel.  On this
    batch the rounds verify every instance and the list stays empty (printed): the list-mode launch's own writes are held by the cold_guess = 0 and lateral-embedding cases below.  fp32: the cold step's array also against the exact optimum of the ORACLE's own QP on the same float32 inputs, the bound of
    tests/test_gpu_f32.py:53 (median <= 2e-4, 99th percentile <= 2e-3, max <= 1e-2 on normalised controls)."""
    B = 128
    p = coupled_pair(pkg, skidpad, B, options=PIPED, precision=precision)
    u, st, it, grew = p.step(*inputs[B])
    assert split_piped(grew, True), grew
    assert np.all(pkg.is_solved(st)), st
    print(f"{precision} split cold: {int((it > 0).sum())} of {B} instances went to the interior point (list mode)")
    if precision == "f32":
        state, control, t0, toff = inputs[B]
        state, control = f32_round(state), f32_round(control)
        orc = make_oracle(oracle_mod, skidpad)
        un = np.array([orc.u_norm[0], orc.u_norm[1], orc.u_norm[1]])
        err = []
        for b in range(B):
            ts, dt = orc.time_steps(t0[b])
            oq, ou, op = orc.nodes(state[b], control[b], ts, dt, time_offset=toff[b])
            xe, _, info = orc.solve_exact(orc.update_qp(oq, ou, op, dt, state[b], control[b]))
            assert info["status"] == 1
            err.append(np.max(np.abs(u[b] - orc.next_control(orc.split_x(xe)["u"][1])) / un))
        print(f"fp32 cold step, caller's array against the oracle: median {np.median(err):.2e}, 99th percentile {np.percentile(err, 99):.2e}, max {np.max(err):.2e} (bounds 2e-4, 2e-3, 1e-2)")
        assert np.median(err) <= 2e-4 and np.percentile(err, 99) <= 2e-3 and np.max(err) <= 1e-2
    _, st, it, grew = p.step(*inputs[B])
    assert split_piped(grew, False), grew
    assert np.all(pkg.is_solved(st)), st
    print(f"{precision} split warm: {int((it > 0).sum())} of {B} instances went to the interior point (list mode)")
    p.close()


def test_fused_update_and_solve(pkg, skidpad, inputs):
    B = 128
    p = coupled_pair(pkg, skidpad, B, options=PIPED, fusion=1)
    _, st, _, grew = p.step(*inputs[B])
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, None), grew      # (the fused kernel is neither of the counted solve launches)
    assert np.all(pkg.is_solved(st)), st
    p.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ring_solve_cold_and_warm(pkg, skidpad, inputs, precision):
    """N = 40: the dynamics blocks stream through the four-slot ring (no counter of its own)."""
    B = 64
    p = coupled_pair(pkg, skidpad, B, N_long=30, precision=precision)
    for _ in range(2):
        _, st, _, grew = p.step(*inputs[B])
        assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, None), grew
        assert np.all(pkg.is_solved(st)), st
    p.close()


def test_mixed_cold_and_warm_batch_after_a_masked_reset(pkg, skidpad, inputs):
    """Every third instance cold, the others warm: the nodes kernels file a launch order (SolveOut::order_in) and the split solve runs behind the pipelined launch again
    (the rounds verify every instance here too; a mixed batch that reaches the list-mode launch: the lateral-embedding case below)."""
    B = 128
    p = coupled_pair(pkg, skidpad, B, options=PIPED)
    p.step(*inputs[B])
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    for m in p.both:
        m.reset(mask)
    _, st, it, grew = p.step(*inputs[B])
    assert split_piped(grew, True), grew
    assert np.all(pkg.is_solved(st)), st
    print(f"mixed batch: {int((it > 0).sum())} of {B} instances went to the interior point (list mode), {int((it[mask == 1] > 0).sum())} of them cold")
    p.close()


def whole_batch_solves(p):
    """launches in which the full k_solve took the whole batch (counted by the kernel itself), per handle"""
    return [m.get_option("stat_whole_batch_solves") for m in p.both]


def test_list_mode_launch_and_whole_batch_launch_write_their_instances(pkg, skidpad, inputs):
    """On the tracking batches above every instance verifies in the rounds-only launch and the list behind it stays empty (measured: 0 of 128 with interior-point iterations,
    cold, warm and mixed).  pg_config.cold_guess = 0 gives a cold instance no active-set attempt of its own: the rounds-only launch files it and the LIST-MODE launch solves it.
    Step 1, cold: the list-mode launch serves the whole batch.  Steps 2 (warm) and 3 (every third instance cold): the launch before left work for the interior point, so the
    device-side switch (SolveOut::mode) hands the whole batch to the full kernel, in the launch order the nodes kernels filed."""
    B = 128
    p = coupled_pair(pkg, skidpad, B, options=PIPED, cold_guess=0)
    w0 = whole_batch_solves(p)
    _, st, it, grew = p.step(*inputs[B])
    assert split_piped(grew, True) and whole_batch_solves(p) == w0, (grew, whole_batch_solves(p))
    assert np.all(pkg.is_solved(st)) and np.all(it > 0), (st, it)
    _, st, it, grew = p.step(*inputs[B])
    assert split_piped(grew, False) and whole_batch_solves(p) == [w + 1 for w in w0], (grew, whole_batch_solves(p))
    assert np.all(pkg.is_solved(st)), st
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    for m in p.both:
        m.reset(mask)
    _, st, it, grew = p.step(*inputs[B])
    assert split_piped(grew, True) and whole_batch_solves(p) == [w + 2 for w in w0], (grew, whole_batch_solves(p))
    assert np.all(pkg.is_solved(st)) and np.all(it[mask == 1] > 0), (st, it)
    p.close()


def test_lateral_embedding_is_written_by_both_launches_of_the_split_solve(pkg, skidpad, inputs):
    """N = 20 under the library's own solver choice: the lateral QP embedded in k_solve ("lateral_solver_in_use" = 2), which writes the caller's array itself.  On this cold
    batch the rounds-only launch verifies part of the instances and files the others: the two launches of the split solve each write the rows they finish, into one array, in one
    step (an instance with interior-point iterations came through the list-mode launch; measured 18 of 96).  The warm step behind it takes the whole batch through the full
    kernel (the launch before left work for the interior point) and leaves none, so the step after it, every third instance cold, is split again: warm and cold instances from
    the rounds-only launch, the cold ones it files from the list-mode launch (measured 3), in the launch order of a mixed batch."""
    B = 96
    p = Pair(pkg, skidpad, B, formulation="decoupled", vehicle=pkg.X1(), N_short=10, N_long=10)
    assert all(m.get_option("lateral_solver_in_use") == 2.0 for m in p.both)
    w0 = whole_batch_solves(p)
    _, st, it, grew = p.step(*inputs[B])
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS + LATERAL_STATS, "stat_split_solve_launches") and whole_batch_solves(p) == w0, (grew, whole_batch_solves(p))
    assert np.all(pkg.is_solved(st)), st
    n_list = int((it > 0).sum())
    print(f"lateral embedding, cold: {n_list} of {B} instances through the list-mode launch")
    assert 0 < n_list < B
    _, st, it, grew = p.step(*inputs[B])
    assert only(grew, COUPLED_STATS + LATERAL_STATS, "stat_split_solve_launches") and whole_batch_solves(p) == [w + 1 for w in w0], (grew, whole_batch_solves(p))
    assert np.all(pkg.is_solved(st)), st
    print(f"lateral embedding, warm: {int((it > 0).sum())} of {B} instances with interior-point iterations")
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    for m in p.both:
        m.reset(mask)
    _, st, it, grew = p.step(*inputs[B])
    assert only(grew, COUPLED_STATS + LATERAL_STATS, "stat_split_solve_launches") and whole_batch_solves(p) == [w + 1 for w in w0], (grew, whole_batch_solves(p))
    assert np.all(pkg.is_solved(st)), st
    n_list = int((it > 0).sum())
    print(f"lateral embedding, every third cold: {n_list} of {B} instances through the list-mode launch")
    assert 0 < n_list < B
    p.close()


def test_ragged_batch_leaves_the_rows_beyond_B_alone(pkg, skidpad, inputs):
    """B = 77 of capacity 128: neither the five input copies nor any launch may reach beyond row 77 (Pair.step holds rows 77 .. 135 of the caller's array against the sentinel)."""
    B = 77
    p = coupled_pair(pkg, skidpad, 128, options=PIPED)
    _, st, _, grew = p.step(*inputs[B])
    assert split_piped(grew, True), grew
    assert np.all(pkg.is_solved(st)), st
    p.close()


def test_path_mode_through_a_null_time_offset(pkg, skidpad, inputs):
    """time_offset_dev = NULL (a memset of 0xFF: every instance in path-tracking mode) against host time_offset = None."""
    B = 64
    state, control, t0, _ = inputs[B]
    p = coupled_pair(pkg, skidpad, B)
    _, st, _, grew = p.step(state, control, t0, None)
    assert split_piped(grew, False), grew
    assert np.all(pkg.is_solved(st)), st
    sep = [m.path_coordinates() for m in p.both]
    assert same(*sep)
    p.close()


# ---- lateral formulation: the kernel does not write the caller's array, pg_step_dev copies ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lateral_oracle(oracle_mod, skidpad, inputs):
    """the oracle's applied control of the 96 lateral N = 20 problems, as test_decoupled_matches_oracle computes it"""
    state, control, t0, toff = inputs[96]
    orc = oracle_mod.OracleDecoupled(N_short=10, N_long=10); orc.set_trajectory(skidpad.data)
    out = np.zeros((96, 3))
    for b in range(96):
        ts, dt = orc.time_steps(t0[b])
        oq, ou, op = orc.nodes(state[b], control[b], ts, dt, time_offset=toff[b])
        xe, _, info = orc.solve_exact(orc.update_qp(oq, ou, op, dt))
        assert info["status"] == 1
        out[b] = orc.next_control(orc.split_x(xe)["delta"][1], ou[1, 1])
    return out


LATERAL_CASES = [("plain", PLAIN_LATERAL, 1, None),
                 ("one per wavefront", {"lateral_solver": 1}, 1, "stat_lat_one_per_wavefront_solves"),
                 ("hand-over", {"lateral_solver": 1, "lat_single_max": 0, "lat_hand_batch": 64}, 1, "stat_lat_handover_solves"),
                 ("two-launch warm", {"lateral_solver": 1}, 2, "stat_lat_two_launch_solves")]


@pytest.mark.parametrize("name,options,steps,counter", LATERAL_CASES, ids=[c[0].replace(" ", "_") for c in LATERAL_CASES])
def test_lateral_arrangements(pkg, skidpad, inputs, lateral_oracle, name, options, steps, counter):
    """N = 20 through k_solve_lat, B = 96; the plain arrangement's cold step also against the oracle, the bound of tests/test_gpu_decoupled.py:45
    (test_decoupled_matches_oracle: steering within 1e-6, the forces to 1e-9 relative)."""
    B = 96
    p = lateral_pair(pkg, skidpad, B, options=options)
    for k in range(steps):
        u, st, _, grew = p.step(*inputs[B])
        assert np.all(pkg.is_solved(st)), st
    assert only(grew, LATERAL_STATS, counter), grew
    if name == "plain":
        uo = lateral_oracle
        d = (float(np.max(np.abs(u[:, 0] - uo[:, 0]))), float(np.max(np.abs(u[:, 1:] - uo[:, 1:]) / np.maximum(1.0, np.max(np.abs(uo), axis=1, keepdims=True)))))
        print(f"plain lateral cold step, caller's array against the oracle: steering {d[0]:.2e} (bound 1e-6), forces {d[1]:.2e} relative (bound 1e-9)")
        for b in range(B):
            assert abs(u[b, 0] - uo[b, 0]) < 1e-6 and np.max(np.abs(u[b, 1:] - uo[b, 1:])) <= 1e-9 * max(1.0, np.max(np.abs(uo[b]))), b
    p.close()


@pytest.mark.parametrize("walls", [True, False])
def test_lateral_long_horizon(pkg, skidpad, inputs, walls):
    """N = 50 (k_solve_lat by default), with and without the wall rows; a cold batch of 64 runs one instance per wavefront."""
    B = 64
    p = lateral_pair(pkg, skidpad, B, N_long=40, walls=walls)
    _, st, _, grew = p.step(*inputs[B])
    assert only(grew, LATERAL_STATS, "stat_lat_one_per_wavefront_solves"), grew
    assert np.all(pkg.is_solved(st)), st
    p.close()


# ---- with a safety grid: other_car_dev, pg_get_next_control_hji_dev -------------------------------------------------------------------------------------------------------
def hji_dev(m, use, with_source=True):
    """pg_get_next_control_hji_dev into sentinel-filled arrays of capacity + 8 rows: (u as float64, source)"""
    import torch
    u = filled(m, (m.capacity + 8, 3)); src = filled(m, (m.capacity + 8,), SRC_SENTINEL, torch.int32)
    on_stream(m)
    m.get_next_control_hji_dev(use, u.data_ptr(), src.data_ptr() if with_source else None)
    m.synchronize()
    return wide(u), src.cpu().numpy()


def test_safety_row_and_fallback_policy(pkg, skidpad, grid):
    """The situation of tests/test_gpu_hji.py::test_hji_fallback_policy (eps 0.5, every fifth instance in path mode, other cars of seed 9), 64 instances, the other cars
    through other_car_dev: the selection of the ROS loop from device arrays against pg_get_next_control_hji of the host-stepped handle."""
    B = 64
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=33)
    toff[::5] = np.nan
    other = pkg.synthetic.other_cars(state, seed=9)
    p = coupled_pair(pkg, skidpad, B, hji_eps=0.5, grid=grid)
    u, st, _, grew = p.step(state, control, t0, toff, other)
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, "stat_single_solve_launches"), grew      # (a safety row: never the split solve)
    assert np.all(st == pkg.SOLVED), st
    assert all(same(a, b) for a, b in zip(p.dev.hji_constraint(), p.ref.hji_constraint()))      # other_car_dev arrived
    seen = {}
    for use in (True, False):
        uh, sh, _ = p.ref.get_next_control_hji(use)
        ud, sd = hji_dev(p.dev, use)
        assert same(ud[:B], uh) and np.array_equal(sd[:B], sh)
        assert np.all(ud[B:] == SENTINEL) and np.all(sd[B:] == SRC_SENTINEL)
        ud, sd = hji_dev(p.dev, use, with_source=False)
        assert same(ud[:B], uh) and np.all(ud[B:] == SENTINEL) and np.all(sd == SRC_SENTINEL)
        seen[use] = set(sh.tolist())
    assert seen[True] == {0, 1} and seen[False] == {0, 2}, seen
    # the same step without the other cars: other_car_dev = NULL (a memset) against host other_car_state = None
    for m in p.both:
        m.reset()
    p.step(state, control, t0, toff, None)
    assert all(same(a, b) for a, b in zip(p.dev.hji_constraint(), p.ref.hji_constraint()))
    # without a grid the device call returns the MPC control and source 0
    for m in p.both:
        m.clear_hji_cache(); m.reset()
    u, _, _, _ = p.step(state, control, t0, toff, other)
    ud, sd = hji_dev(p.dev, True)
    assert same(ud[:B], u) and np.all(sd[:B] == 0) and np.all(ud[B:] == SENTINEL) and np.all(sd[B:] == SRC_SENTINEL)
    uh, sh, _ = p.ref.get_next_control_hji(True)
    assert same(uh, u) and np.all(sh == 0)
    p.close()


def test_the_policy_is_refused_on_a_lateral_handle(pkg, skidpad, inputs):
    B = 64
    m = pkg.DecoupledTrajectoryTrackingMPC(pkg.X1(), skidpad, B, N_short=10, N_long=10, phase_timing=False)
    u, _, _ = dev_step(m, *inputs[B])
    v = filled(m, (B, 3))
    on_stream(m)
    refused(pkg, lambda: m.get_next_control_hji_dev(True, v.data_ptr()), "pg_get_next_control_hji_dev", STATE, "the HJI policy belongs to the coupled controller (ros_integration.jl:56,114)")
    m.get_next_control_dev(v.data_ptr()); m.synchronize()
    assert same(wide(v), u[:B])
    m.close()


# ---- lookups ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def lookup_points(knots):
    """the 500 points of tests/test_gpu_hji.py::test_lookup_matches_oracle: ~30 % outside the grid, the two corners, an interior knot point"""
    rng = np.random.default_rng(0)
    lo = np.array([k[0] for k in knots], dtype=np.float64); hi = np.array([k[-1] for k in knots], dtype=np.float64)
    x = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (500, 7))
    x[0] = lo; x[1] = hi
    x[2] = [float(k[len(k) // 2]) for k in knots]
    return x, lo, hi


@pytest.mark.parametrize("B", [500, 1])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_lookups_from_device_arrays(pkg, oracle_mod, skidpad, grid, precision, B):
    """pg_hji_lookup8_dev (the kernel's [B][8] rows) and pg_hji_lookup_dev (the same unpacked by two pitched copies, in its three argument shapes) against pg_hji_lookup.
    Every output tensor is 5 elements longer than needed and sentinel-filled: a wrong pitch shows as a clobbered tail or a left-over sentinel."""
    knots, V, g = grid
    x, lo, hi = lookup_points(knots)
    x = x[:B] if B > 1 else x[2:3]
    if precision == "f32":
        x = f32_round(x)
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, 8, precision=precision, phase_timing=False)
    m.set_hji_cache(knots, V, g)
    Vh, Gh = m.hji_lookup(x)
    inb = np.all((x >= lo) & (x <= hi), axis=1)
    assert np.all(np.isposinf(Vh[~inb])) and np.all(bits(Gh[~inb]) == 0) and np.all(np.isfinite(Vh[inb]))
    if B > 1:
        assert 50 < inb.sum() < B and inb[0] and inb[1] and inb[2]
    torch, tdt, dev = m._torch()
    xd = torch.from_numpy(x).to(tdt).to(dev)
    out8 = filled(m, (B * 8 + 5,))
    on_stream(m)
    m.hji_lookup8_dev(B, xd.data_ptr(), out8.data_ptr())
    m.synchronize()
    o = wide(out8)
    rows = o[:B * 8].reshape(B, 8)
    assert same(rows[:, 0], Vh) and same(rows[:, 1:], Gh) and np.all(o[B * 8:] == SENTINEL)
    for V_given, G_given in ((True, True), (True, False), (False, True)):
        Vd = filled(m, (B + 5,)); Gd = filled(m, (B * 7 + 5,))
        on_stream(m)
        m.hji_lookup_dev(B, xd.data_ptr(), Vd.data_ptr() if V_given else None, Gd.data_ptr() if G_given else None)
        Vd, Gd = wide(Vd), wide(Gd)
        if V_given:
            assert same(Vd[:B], Vh) and np.all(Vd[B:] == SENTINEL), (V_given, G_given)
        else:
            assert np.all(Vd == SENTINEL)
        if G_given:
            assert same(Gd[:B * 7].reshape(B, 7), Gh) and np.all(Gd[B * 7:] == SENTINEL), (V_given, G_given)
        else:
            assert np.all(Gd == SENTINEL)
    if precision == "f64":          # the oracle loop of test_lookup_matches_oracle once more, on the packed rows
        orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(knots, V, g)
        for i in range(B):
            Vo, Go, ok = orc.hji_lookup(x[i])
            assert ok == inb[i]
            if ok:
                assert abs(rows[i, 0] - Vo) <= 1e-12 * max(1.0, abs(Vo)) and np.max(np.abs(rows[i, 1:] - Go)) <= 1e-12, i
            else:
                assert math.isinf(rows[i, 0]) and rows[i, 0] > 0 and np.all(rows[i, 1:] == 0), i
    m.close()


# ---- refusals: status and the whole text, and the next valid call works -----------------------------------------------------------------------------------------------------
def test_refusals(pkg, skidpad, grid, inputs):
    cap, B = 8, 5
    state, control, t0, toff = (a[:B] for a in inputs[64])
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, cap, phase_timing=False)
    ref = pkg.BatchedTrajectoryTrackingMPC(skidpad, cap, phase_timing=False)
    torch, tdt, dev = m._torch()
    s, c, t, f = (torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev) for a, dt in ((state, tdt), (control, tdt), (t0, torch.float64), (toff, torch.float64)))
    u = filled(m, (cap + 8, 3))
    on_stream(m)
    # before any inputs (check_ready)
    not_ready = "no inputs installed (call pg_set_inputs first)"
    refused(pkg, lambda: m.get_next_control_dev(u.data_ptr()), "pg_get_next_control_dev", STATE, not_ready)
    refused(pkg, lambda: m.step_dev(u.data_ptr()), "pg_step_dev", STATE, not_ready)
    # pg_set_inputs_dev
    size, need = "batch size outside [1, batch_capacity]", "state, control and t0 are required"
    good = (s.data_ptr(), c.data_ptr(), t.data_ptr(), None, f.data_ptr())
    for bad_B in (0, cap + 1):
        refused(pkg, lambda: m.set_inputs_dev(bad_B, *good), "pg_set_inputs_dev", INVALID, size)
        refused(pkg, lambda: m.step_dev(u.data_ptr()), "pg_step_dev", STATE, not_ready)          # (a refused call installs nothing)
    for k in range(3):
        refused(pkg, lambda: m.set_inputs_dev(B, *[None if i == k else a for i, a in enumerate(good)]), "pg_set_inputs_dev", INVALID, need)
    m.synchronize()
    assert np.all(wide(u) == SENTINEL)
    m.set_inputs_dev(B, *good)
    m.step_dev(u.data_ptr())
    # pg_get_next_control_dev(NULL): PG_OK, nothing written
    m.get_next_control_dev(None)
    m.synchronize()
    uh, sth, ith = ref.step_(state, control, t0, time_offset=toff)
    got = wide(u)
    assert same(got[:B], uh) and np.all(got[B:] == SENTINEL)
    assert np.array_equal(m.solve_info()[0], sth) and np.array_equal(m.solve_info()[1], ith)
    # the lookups
    x = torch.from_numpy(lookup_points(grid[0])[0][:B]).to(tdt).to(dev)
    out8 = filled(m, (B * 8 + 5,)); Vd = filled(m, (B + 5,))
    on_stream(m)
    calls = (("pg_hji_lookup_dev", m.hji_lookup_dev, Vd), ("pg_hji_lookup8_dev", m.hji_lookup8_dev, out8))      # (the third argument: V_dev / out8_dev)
    for what, call, out in calls:
        refused(pkg, lambda: call(B, x.data_ptr(), out.data_ptr()), what, INVALID, "no HJI grid installed")
    m.set_hji_cache(*grid)
    for what, call, out in calls:
        refused(pkg, lambda: call(0, x.data_ptr(), out.data_ptr()), what, INVALID, f"{what}: bad arguments")
        refused(pkg, lambda: call(B, None, out.data_ptr()), what, INVALID, f"{what}: bad arguments")
    refused(pkg, lambda: m.hji_lookup8_dev(B, x.data_ptr(), None), "pg_hji_lookup8_dev", INVALID, "pg_hji_lookup8_dev: bad arguments")
    m.synchronize()
    assert np.all(wide(out8) == SENTINEL) and np.all(wide(Vd) == SENTINEL)
    Vh, Gh = m.hji_lookup(wide(x))
    for what, call, out in calls:
        call(B, x.data_ptr(), out.data_ptr())
    m.synchronize()
    rows = wide(out8)[:B * 8].reshape(B, 8)
    assert same(rows[:, 0], Vh) and same(rows[:, 1:], Gh) and same(wide(Vd)[:B], Vh)
    m.close(); ref.close()
