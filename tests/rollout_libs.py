"""What the GPU tests of the rollout libraries' host-side state share (tests/test_gpu_index_rule.py, tests/test_gpu_history_slots.py, tests/test_gpu_restart_rules.py): the
smallest handle that still runs a rollout -- capacity 8, B = 5, the shortest horizon pg_create accepts (N_short = 1, N_long = 0), 3 steps -- and, per library, how it is
installed, its identity set, its rollout and its history setters with the refusal each one answers without the library (the texts of csrc/pg_api.hip)."""
import ctypes as C

import numpy as np

import actuator_numpy
import disturbance_numpy
import estimator_numpy
import human_numpy

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


def make(pkg, traj, grid):
    """a coupled handle of capacity 8 at the shortest horizon, with the grid the safety rollout's human library wants"""
    m = pkg.BatchedTrajectoryTrackingMPC(traj, CAP, N_short=1, N_long=0, hji_eps=1.0)
    m.set_hji_cache(*grid)
    return m


def inputs(pkg, traj):
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=4)
    return state, control, t0, pkg.synthetic.other_cars(state, seed=43), toff


def install(m, library, sets=None, index=None, **kw):
    """the library's identity set (or `sets`), through the Python installer"""
    installer, identity = LIBRARIES[library][:2]
    getattr(m, installer)([identity] if sets is None else sets, index, **kw)


def clear(m, library):
    getattr(m.lib, f"pg_clear_{library}_sets")(m.h)


def rollout(m, library, steps=STEPS, dt=DT):
    """the library's rollout through the C call, no record of the call's own: the status"""
    if LIBRARIES[library][3] == "simulate":
        return m.lib.pg_simulate_dev(m.h, int(steps), C.c_double(dt), None, None)
    return m.lib.pg_simulate_safety_dev(m.h, int(steps), C.c_double(dt), 1, 0, None, None, None, None, None, None, None)


def register(m, setter, buf, steps):
    """buf: a torch tensor on the device, or None"""
    return getattr(m.lib, setter)(m.h, C.c_void_p(buf.data_ptr()) if buf is not None else None, int(steps))


def last_error(m):
    return m.lib.pg_last_error(m.h).decode()
