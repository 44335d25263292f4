"""Between rollout calls the handle's inputs are the truth and the command, under every library at once.

A rollout step hands the controller a view of its own -- the estimate of a noisy measurement as the state, the actuator's position as the control where a set has
feedback = 1 -- while the plant, the records and the getters keep the handle's pair.  The per-library files install one library at a time; here a noisy sensor set, an
estimator set with gains inside (0, 1) on the model's prior, an actuator library of two sets (one with feedback = 1 behind a delay of one step, selected per instance) and a
disturbance set with a force and a gust are installed together, with a random driver (mode 3) in the rollouts that have another car.  The node rollout refuses an actuator
library and runs under the other four.

Per rollout kind, on fresh handles from the same inputs (the small handle of tests/rollout_libs.py: capacity 8, B = 5, the shortest horizon): A, one recorded call of 3 steps
with every record and history the harness knows, against B, a call of 2 steps, the getters, a call of 1 step.  The joined calls equal the one call bit for bit on every key,
and what the getters return between the calls is what the first call left: the true state, the command (not the applied control, not what the controller saw), the last
measured, estimated and applied rows."""
import ctypes as C

import numpy as np
import pytest

import actuator_numpy
import disturbance_numpy
import estimator_numpy
import human_numpy
import rollout_libs as rl
import sensor_numpy
from rollout_libs import grid  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SEED = rl.NOISE_SEED
DP = C.POINTER(C.c_double)
ACTUATORS = [actuator_numpy.identity(tau_delta=0.05, tau_fx=0.05), actuator_numpy.identity(delay_steps=1, tau_delta=0.1, feedback=1)]
ACT_IDX = (np.arange(rl.B) % 2).astype(np.int32)


def handle(pkg, traj, grid, precision, kind):
    """a small handle with the libraries of the rollout `kind` installed and the inputs in place"""
    m = rl.make(pkg, traj, rl.CAP, precision=precision, grid=grid, N_short=1, N_long=0)
    m.set_sensors([sensor_numpy.four_sensors()[1]], seed=SEED, streams=rl.stream_ids(rl.B))
    m.set_estimators([estimator_numpy.identity(gain=[0.2, 0.3, 0.4, 0.5, 0.6, 0.7], predict=1)])
    m.set_disturbances([disturbance_numpy.identity(Fy=500.0, sigma_Fx=300.0, sigma_Fy=800.0, x_cp=1.0, tau_gust=0.3)], seed=SEED + 1)
    if kind != "node":
        m.set_actuators(ACTUATORS, ACT_IDX)
    if kind != "simulate":
        m.set_humans([human_numpy.four_humans()[3]], seed=SEED + 2)
    m.set_inputs(*rl.small_inputs(pkg, traj))
    return m


def recorded(m, kind, steps):
    return rl.rollout(m, kind, steps, rl.DT, measured=True, estimated=True, use_HJI_policy=True, summary=kind != "simulate")


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["simulate", "safety", "node"])
def test_two_calls_equal_one_and_the_getters_between_them_read_truth_and_command(pkg, skidpad, grid, kind, precision):
    a = handle(pkg, skidpad, grid, precision, kind)
    A = recorded(a, kind, 3)
    a.close()

    b = handle(pkg, skidpad, grid, precision, kind)
    B1 = recorded(b, kind, 2)
    state = np.zeros((rl.B, 6)); control = np.zeros((rl.B, 3))
    b._chk(b.lib.pg_get_state(b.h, state.ctypes.data_as(DP), control.ctypes.data_as(DP), None), "pg_get_state")
    assert rl.same(state, B1["final_state"])
    assert rl.same(control, B1["final_control"])
    assert rl.same(b.measured_state(), B1["measured"][-1])
    assert rl.same(b.estimated_state(), B1["estimated"][-1])
    if kind != "node":
        assert rl.same(b.actuator_state(), B1["applied"][-1])
        assert rl.same(control, A["command"][2])                 # the command the third step finds
    assert np.any(B1["measured"][-1] != state) and np.any(B1["estimated"][-1] != B1["measured"][-1])      # noise and gains inside (0, 1): three states, no two alike
    B2 = recorded(b, kind, 1)
    b.close()

    AB = rl.join([B1, B2])
    produced = [k for k in rl.KEYS if A[k] is not None]
    assert {"state", "control", "measured", "estimated", "disturbance", "final_state", "final_control"} <= set(produced)
    for k in rl.KEYS:
        assert rl.same(AB[k], A[k]), (kind, precision, k)
