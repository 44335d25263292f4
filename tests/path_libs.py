"""What the GPU tests of the two path makers share (tests/test_gpu_speed_plan.py, tests/test_gpu_path_make.py; tests/test_gpu_trajectory_library.py for the ways a library
arrives): the smallest handle a maker call needs, the access to the ctypes structures, the state after a rollout, and the three checks both files make in the same words --
an installed library equals pg_set_trajectories with the returned channels, a refusal leaves the installed library alone, a tube is drivable in closed loop.
A plain module, imported as tests/rollout_libs.py is: no fixtures."""
import ctypes as C
import sys

import numpy as np

OK, INVALID, STATE = 0, -2, -4
c_i32p = C.POINTER(C.c_int32)
c_dp = C.POINTER(C.c_double)


def handle(pkg, precision="f64", cap=8, **kw):
    return pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), cap, N_short=1, N_long=0, precision=precision, **kw)


def lib():                                                          # the module of the ctypes structures (pg_speed_plan_stats, pg_path_spec, ...)
    return sys.modules["pigeon_jl_amd"]._lib


def get_state(m, B):
    q = np.zeros((B, 6)); u = np.zeros((B, 3)); t = np.zeros(B)
    assert m.lib.pg_get_state(m.h, q.ctypes.data_as(c_dp), u.ctypes.data_as(c_dp), t.ctypes.data_as(c_dp)) == OK, m.lib.pg_last_error(m.h)
    return np.concatenate([q, t[:, None]], axis=1), u


def step_bits(m, pkg):
    state, control, t0, toff = pkg.synthetic.config2_inputs(m.trajectories[0], 5, seed=4)
    u, status, _ = m.step_(state, control, t0, time_offset=toff)
    return u.tobytes() + status.tobytes()


def install_equals_set_trajectories(pkg, a, b, channels, L, Lmax, index, start_tube):
    """a: a handle whose library a maker (or a setter) has just installed; b: a handle that is handed the same library as channels [len(L)][10][Lmax] by
    pg_set_trajectories.  Five instances that start on start_tube: the same bits after 6 steps, and the same clock"""
    state, control, t0, toff = pkg.synthetic.config2_inputs(start_tube, 5, seed=4, s_range=(2.0, 20.0))
    a.set_inputs(state, control, t0, time_offset=toff)
    # a library of several needs an index, as after pg_set_trajectories: the phase calls return PG_ERR_STATE until one is installed
    assert a.lib.pg_compute_time_steps(a.h) == STATE and a.lib.pg_compute_linearization_nodes(a.h) == STATE
    assert a.lib.pg_step_dev(a.h, None) == STATE
    L = np.ascontiguousarray(L, dtype=np.int32)
    assert b.lib.pg_set_trajectories(b.h, len(L), Lmax, L.ctypes.data_as(c_i32p), np.ascontiguousarray(channels).ctypes.data_as(c_dp)) == OK
    b.set_inputs(state, control, t0, time_offset=toff)
    res = []
    for m in (a, b):
        m.set_trajectory_index(index)
        rc = m.lib.pg_simulate_dev(m.h, 6, C.c_double(0.01), None, None)
        assert rc == OK, m.lib.pg_last_error(m.h)
        res.append(get_state(m, 5))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
    assert np.all(np.isfinite(res[0][0]))
    # the clock of pg_simulate_dev reads trajectory.t[end] of trajectory 0: the same times on both handles, for a step that has an exact rational and one that has not
    for dt in (0.01, 0.37):
        ca, cb = a.simulate_clock(7, t0, dt=dt), b.simulate_clock(7, t0, dt=dt)
        assert ca.tobytes() == cb.tobytes() and np.all(np.isfinite(ca)), dt


def refusals(m, pkg, call, cases, prefix, before):
    """every call(**kw) of cases {name: kw} is refused with PG_ERR_INVALID in the entry point's name and leaves the installed library alone (before: its step_bits)"""
    for name, kw in cases.items():
        assert call(**kw) == INVALID, name
        assert m.lib.pg_last_error(m.h).decode().startswith(prefix), name
        assert step_bits(m, pkg) == before, name


def drive(m, tube, knots, steps):
    """one instance per knot starts on the installed tube at its knot's speed (Uy = 0, e = 0, r = V kappa) and runs `steps` steps of 0.01 s in trajectory mode.
    Returns (status [steps][n], summary, first_exit) with the tracking summary of the handle (option "tracking_summary")"""
    n = len(knots); at = np.asarray(knots)
    state = np.stack([tube.E[at], tube.N[at], tube.psi[at], tube.V[at], np.zeros(n), tube.V[at] * tube.kappa[at]], axis=1)
    m.set_inputs(state, np.zeros((n, 3)), tube.t[at], time_offset=np.zeros(n))
    status = np.zeros((steps, n), dtype=np.int32)
    for k in range(steps):                                          # (one step per call: consecutive calls continue the clock, and the step's statuses can be read)
        m.simulate_(1, dt=0.01)
        status[k] = m.solve_info()[0]
    summary, _, first_exit = m.tracking_summary()
    return status, summary, first_exit
