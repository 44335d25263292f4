"""What the GPU tests of the rollout libraries share.

The rollout harness of the six library files (tests/test_gpu_{plant,sensor,actuator,disturbance,estimator,human}_sets.py): the measures `rel` and `same`, the stream ids, how
a handle is made (`make`) and started (`inputs`, `start`), and `rollout` / `join` -- THE place that knows what simulate_, simulate_safety_ and simulate_node_ return: one
dictionary with the keys KEYS whatever the rollout and whatever libraries are installed, None where the call produced nothing (pinned without a GPU by
tests/test_rollout_harness_host.py).  With them the `grid` fixture of the safety rollouts and the tracking-summary yardstick (`narrowed`, `numpy_summary`, `check_summary`).

The host-side state tests (tests/test_gpu_index_rule.py, tests/test_gpu_history_slots.py, tests/test_gpu_restart_rules.py): the smallest handle that still runs a rollout --
capacity 8, B = 5, the shortest horizon pg_create accepts (N_short = 1, N_long = 0), 3 steps -- and, per library, how it is installed, its identity set, its rollout and
its history setters with the refusal each one answers without the library (the texts of csrc/pg_api.hip)."""
import ctypes as C

import numpy as np
import pytest

import actuator_numpy
import disturbance_numpy
import estimator_numpy
import human_numpy
import plant_numpy

# ---- the rollout harness ---------------------------------------------------------------------------------------------------------------------------------------------
NOISE_SEED = 0x9E3779B97F4A7C15           # of the sensor's draws: high word non-zero
# per-step records [steps][B]..., under the names the wrapper gives them ("control" of the node rollout: its "applied" record, the control the plant integrates)
RECORDS = ("state", "control", "other", "human", "V", "source", "event", "command", "applied", "disturbance", "human_u", "measured", "estimated")
FINALS = ("final_state", "final_control", "final_t", "final_other", "final_applied")          # after the call, in the order the three methods return them
SUMMARY = ("V_min", "first_breach", "policy_steps")                                           # safety_summary(), read on request only
KEYS = RECORDS + FINALS + SUMMARY


def rel(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)) / np.maximum(1.0, np.abs(ref))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """two device results, bit for bit (-0.0 is not 0.0, a NaN equals itself); a record neither call produced (None) equals itself"""
    if a is None or b is None:
        return a is b
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and (np.array_equal(bits(a), bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b))


def stream_ids(n):
    """64-bit ids, all but the first above 2^32, no two alike in either word"""
    b = np.arange(n, dtype=np.uint64)
    return b * np.uint64(0x100000001) + np.uint64(7) + (b % np.uint64(3)) * np.uint64(1 << 40)


@pytest.fixture(scope="module")
def grid(pkg):
    """the grid of the safety rollouts under a human library"""
    return pkg.synthetic.hji_grid(dims=(7, 6, 5, 4, 4, 5, 4), seed=11)


def make(pkg, traj, cap, formulation="coupled", precision="f64", grid=None, **kw):
    """a handle of capacity `cap`; with a grid: hji_eps = 1 and the grid installed, as the safety rollouts under a human library want it"""
    if grid is not None:
        kw.setdefault("hji_eps", 1.0)
    m = pkg.BatchedTrajectoryTrackingMPC(traj, cap, formulation=formulation, precision=precision, **kw)
    if grid is not None:
        m.set_hji_cache(*grid)
    return m


def inputs(pkg, traj, n, seed=4, other_seed=None):
    """(state, control, t0, toff, other) of n instances; other_seed None: the default seed of synthetic.other_cars"""
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, n, seed=seed)
    other = pkg.synthetic.other_cars(state) if other_seed is None else pkg.synthetic.other_cars(state, seed=other_seed)
    return state, control, t0, toff, other


def start(m, inp, n=None, others=False):
    """installs the first n instances of inp = inputs(...), with or without the other cars; returns inp"""
    state, control, t0, toff, other = inp[:5]
    m.set_inputs(state[:n], control[:n], t0[:n], other[:n] if others else None, toff[:n])
    return inp


def rollout(m, kind, steps, dt, measured=False, estimated=False, use_HJI_policy=False, human="hold", human_u=None, pre_flag=None, summary=False):
    """One recorded rollout -- kind "simulate" (simulate_), "safety" (simulate_safety_) or "node" (simulate_node_) -- as a dictionary with the keys KEYS: every per-step
    record, the measured / estimated histories, the state after the call and, with summary=True, safety_summary().  None: the call did not produce it."""
    opts = dict(record=True, measured=measured, estimated=estimated)
    if kind == "simulate":
        out = m.simulate_(steps, dt, **opts)
        finals, records, tail = out[:3], dict(state=out[3], control=out[4]), list(out[5:])
        if tail and isinstance(tail[-1], dict):                  # under an actuator or a disturbance library
            records.update(tail.pop())
    elif kind == "safety":
        out = m.simulate_safety_(steps, dt, use_HJI_policy=use_HJI_policy, human=human, human_u=human_u, **opts)
        finals, records, tail = out[:4], out[4], list(out[5:])
    else:
        assert kind == "node", kind
        out = m.simulate_node_(steps, dt, use_HJI_policy=use_HJI_policy, human=human, human_u=human_u, pre_flag=pre_flag, **opts)
        finals, records, tail = out[:5], dict(out[5], control=out[5]["applied"]), list(out[6:])
    assert set(records) <= set(RECORDS), sorted(records)         # a record this harness does not know yet
    r = dict.fromkeys(KEYS)
    r.update(records)
    r.update(zip(FINALS, finals))
    if measured:
        r["measured"] = tail.pop(0)
    if estimated:
        r["estimated"] = tail.pop(0)
    assert not tail, len(tail)
    if summary:
        r.update(zip(SUMMARY, m.safety_summary()))
    return r


def join(parts):
    """consecutive calls as one: the records concatenated along the steps, everything else as the last call left it"""
    return {k: parts[-1][k] if k not in RECORDS else None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in parts[0]}


# ---- the tracking summary against numpy --------------------------------------------------------------------------------------------------------------------------------
def narrowed(pkg, traj, half=0.25, shift=0.0):
    """the trajectory with a tube of +-half about e = shift"""
    d = traj.data.copy()
    d[10] = half + shift; d[11] = -half + shift
    return pkg.TrajectoryTube(*d)


def numpy_summary(orcs, tidx, qh, step0=0):
    """(the numpy tracking summary of a recorded state history [steps][B][6], s, e [steps][B]); orcs: one oracle per trajectory, tidx [B] (None: orcs[0] for everyone)"""
    K, B = qh.shape[:2]
    tidx = np.zeros(B, dtype=int) if tidx is None else tidx
    s = np.zeros((K, B)); e = np.zeros((K, B))
    for k in range(K):
        for b in range(B):
            s[k, b], e[k, b] = orcs[tidx[b]].path_coordinates(qh[k, b, 0], qh[k, b, 1])[:2]
    eL = np.zeros((K, B)); eR = np.zeros((K, B))
    for j, o in enumerate(orcs):
        sel = tidx == j
        eL[:, sel], eR[:, sel] = plant_numpy.tube_edges(o.traj, s[:, sel])
    return plant_numpy.tracking_summary(s, e, qh[..., 3], qh[..., 4], qh[..., 5], eL, eR, step0), s, e


def check_summary(got, want, bar):
    """pg_get_tracking_state against numpy_summary's: the sums within the bar, the counts equal, the first exit equal wherever the margin decides it"""
    (sm, n, fx), (wsm, wn, wfx, margin) = got, want
    assert np.array_equal(n, wn)
    err = rel(sm, wsm)
    assert err.max() < bar, (err.max(axis=0), bar)
    decided = margin > 1e-6
    assert np.mean(~decided) <= 1 / 8, float(np.mean(~decided))
    assert np.array_equal(fx[decided], wfx[decided]), np.flatnonzero(decided & (fx != wfx))
    return float(err.max())


# ---- the host-side state tests -----------------------------------------------------------------------------------------------------------------------------------------
CAP, B, DT, STEPS = 8, 5, 0.01, 3
OK, INVALID, STATE = 0, -2, -4
ZERO6 = np.zeros(6)

# library -> (installer, identity set, its index setter, its rollout)
LIBRARIES = {
    "sensor": ("set_sensors", (ZERO6, ZERO6), "pg_set_sensor_index", "simulate"),
    "actuator": ("set_actuators", actuator_numpy.identity(), "pg_set_actuator_index", "simulate"),
    "disturbance": ("set_disturbances", disturbance_numpy.identity(), "pg_set_disturbance_index", "simulate"),
    "estimator": ("set_estimators", estimator_numpy.identity(), "pg_set_estimator_index", "simulate"),
    "human": ("set_humans", human_numpy.identity(0), "pg_set_human_index", "safety"),
}
# history setter -> (library, record width, the advice its refusal ends with)
HISTORIES = {
    "pg_set_measured_history_dev": ("sensor", 6, "(the measured state is the true one: record state_hist)"),
    "pg_set_applied_history_dev": ("actuator", 3, "(applied = command: record control_hist)"),
    "pg_set_command_history_dev": ("actuator", 3, "(applied = command: record control_hist)"),
    "pg_set_disturbance_history_dev": ("disturbance", 4, "(w = (0, 0, 0, 1) at every step)"),
    "pg_set_estimated_history_dev": ("estimator", 6, "(the controller reads the sensor's output: record that)"),
    "pg_set_human_history_dev": ("human", 2, "(the rollouts' human_mode decides: human_hist_dev of pg_simulate_safety_dev records that)"),
}


def make_small(pkg, traj, grid):
    """a coupled handle of capacity 8 at the shortest horizon, with the grid the safety rollout's human library wants"""
    return make(pkg, traj, CAP, grid=grid, N_short=1, N_long=0)


def small_inputs(pkg, traj):
    """the arguments of set_inputs for the B = 5 instances"""
    state, control, t0, toff, other = inputs(pkg, traj, B, other_seed=43)
    return state, control, t0, other, toff


def install(m, library, sets=None, index=None, **kw):
    """the library's identity set (or `sets`), through the Python installer"""
    installer, identity = LIBRARIES[library][:2]
    getattr(m, installer)([identity] if sets is None else sets, index, **kw)


def clear(m, library):
    getattr(m.lib, f"pg_clear_{library}_sets")(m.h)


def rollout_status(m, library, steps=STEPS, dt=DT):
    """the library's rollout through the C call, no record of the call's own: the status"""
    if LIBRARIES[library][3] == "simulate":
        return m.lib.pg_simulate_dev(m.h, int(steps), C.c_double(dt), None, None)
    return m.lib.pg_simulate_safety_dev(m.h, int(steps), C.c_double(dt), 1, 0, None, None, None, None, None, None, None)


def register(m, setter, buf, steps):
    """buf: a torch tensor on the device, or None"""
    return getattr(m.lib, setter)(m.h, C.c_void_p(buf.data_ptr()) if buf is not None else None, int(steps))


def last_error(m):
    return m.lib.pg_last_error(m.h).decode()
