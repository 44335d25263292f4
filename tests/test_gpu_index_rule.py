"""One index rule for the eight per-instance libraries (trajectories, control parameters, plants, sensors; below them actuators, disturbances, estimators, humans): pg_set_*_index writes the WHOLE [capacity] device array,
entries beyond the indexed batch as 0, and a library of several sets wants an index that covers the batch.

Per library, on a handle of capacity 80: a library of four sets with an index over 80 instances that uses set 3; then a library of two sets with an index over 70
instances (one full wavefront and a partial one).  A batch of 80 is refused with PG_ERR_STATE; a batch of 70 runs three rollout steps bit for bit as on a fresh handle
that only ever saw the second library.  No tolerance: whatever the first library left behind must be invisible."""
import ctypes as C

import numpy as np
import pytest

import plant_numpy
import rollout_libs as rl
import sensor_numpy
from rollout_libs import grid  # noqa: F401  (the fixture)

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


RESPONSE = {"actuator": lambda m: m.actuator_response(np.zeros((3, rl.B, 3)), DT),
            "disturbance": lambda m: m.disturbance_response(0, 3, DT),
            "estimator": lambda m: m.estimator_response(np.zeros((3, rl.B, 6)), np.zeros((3, rl.B, 3)), DT),
            "human": lambda m: m.human_response(0, np.zeros((3, rl.B, 7)), np.zeros((3, rl.B, 8)), DT)}


@pytest.mark.parametrize("library", ["actuator", "disturbance", "estimator", "human"])
def test_the_other_four_libraries_want_an_index_that_covers_the_batch(pkg, skidpad, grid, library):
    """The same rule for the libraries of the rollouts' actuator, disturbance, estimator and human: two sets and an index over B - 1 of the B = 5 instances.  The rollout
    (three steps asked for) and the library's *_response call both refuse with PG_ERR_STATE and the index rule's one message."""
    _, identity, setter, _ = rl.LIBRARIES[library]
    refusal = f"a {library} library is installed but {setter} does not cover the batch"
    m = rl.make_small(pkg, skidpad, grid)
    state, control, t0, other, toff = rl.small_inputs(pkg, skidpad)
    m.set_inputs(state, control, t0, other, toff)
    rl.install(m, library, [identity, identity], np.array([0, 1, 0, 1], dtype=np.int32))
    assert rl.rollout_status(m, library, 3) == rl.STATE
    assert rl.last_error(m) == refusal
    with pytest.raises(pkg.PigeonError) as e:
        RESPONSE[library](m)
    assert str(e.value) == f"pg_{library}_response failed with status {rl.STATE}: {refusal}"
    m.close()
