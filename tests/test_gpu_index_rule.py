"""One index rule for the four per-instance libraries (trajectories, control parameters, plants, sensors): pg_set_*_index writes the WHOLE [capacity] device array,
entries beyond the indexed batch as 0, and a library of several sets wants an index that covers the batch.

Per library, on a handle of capacity 80: a library of four sets with an index over 80 instances that uses set 3; then a library of two sets with an index over 70
instances (one full wavefront and a partial one).  A batch of 80 is refused with PG_ERR_STATE; a batch of 70 runs three rollout steps bit for bit as on a fresh handle
that only ever saw the second library.  No tolerance: whatever the first library left behind must be invisible."""
import ctypes as C

import numpy as np
import pytest

import plant_numpy
import sensor_numpy

pytestmark = pytest.mark.gpu

CAP, B, DT = 80, 70, 0.01
PATHS = ["skidpadoval", "vail", "EastPaddock", "variable_speed"]
CONTROL_SETS = [{}, {"Q_e": 2.0}, {"Q_e": 4.0, "deltadot_max": 0.2}, {"W_r": 30.0, "R_ddelta": 0.2}]
REFUSAL = {"trajectory": "a trajectory library is installed but pg_set_trajectory_index does not cover the batch",
           "control": "a control-parameter library is installed but pg_set_control_param_index does not cover the batch",
           "plant": "a plant library is installed but pg_set_plant_index does not cover the batch",
           "sensor": "a sensor library is installed but pg_set_sensor_index does not cover the batch"}


def install(m, library, sets, index):
    {"trajectory": m.set_trajectories, "control": m.set_control_params, "plant": m.set_plants, "sensor": m.set_sensors}[library](sets, index)


def set_inputs(pkg, m, tubes, idx):
    """installs starts on the tube each instance selects (idx: one entry per instance)"""
    n = len(idx)
    state = np.zeros((n, 6)); control = np.zeros((n, 3)); t0 = np.zeros(n); toff = np.zeros(n)
    for k in sorted(set(idx.tolist())):
        sel = np.where(idx == k)[0]; t = tubes[k]
        state[sel], control[sel], t0[sel], toff[sel] = pkg.synthetic.config2_inputs(t, len(sel), seed=40 + k, s_range=None if t.s[-1] > 90 else (2.0, 0.4 * t.s[-1]))
    m.set_inputs(state, control, t0, time_offset=toff)


@pytest.mark.parametrize("library", ["trajectory", "control", "plant", "sensor"])
def test_a_smaller_library_and_a_shorter_index_leave_nothing_of_the_earlier_ones(pkg, library):
    tubes = [pkg.load_path_fixture(p) for p in PATHS]
    four = {"trajectory": tubes, "control": CONTROL_SETS, "plant": plant_numpy.four_plants(pkg.X1), "sensor": sensor_numpy.four_sensors()}[library]
    idx4 = (np.arange(CAP) % 4).astype(np.int32); idx4[B:] = 3                 # set 3 in every entry beyond the later batch
    idx2 = ((np.arange(B) // 3) % 2).astype(np.int32)
    on_tube = (lambda idx: idx) if library == "trajectory" else (lambda idx: np.zeros(len(idx), dtype=np.int32))

    m = pkg.BatchedTrajectoryTrackingMPC(tubes[0], CAP)
    install(m, library, four, idx4)
    install(m, library, four[:2], idx2)
    set_inputs(pkg, m, tubes, on_tube(np.concatenate([idx2, np.zeros(CAP - B, dtype=np.int32)])))
    assert m.lib.pg_simulate_dev(m.h, 3, C.c_double(DT), None, None) == -4
    assert m.lib.pg_last_error(m.h).decode() == REFUSAL[library]
    set_inputs(pkg, m, tubes, on_tube(idx2))
    got = m.simulate_(3, DT, record=True)
    m.close()

    fresh = pkg.BatchedTrajectoryTrackingMPC(tubes[0], CAP)
    install(fresh, library, four[:2], idx2)
    set_inputs(pkg, fresh, tubes, on_tube(idx2))
    want = fresh.simulate_(3, DT, record=True)
    fresh.close()
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
