"""What restarts when, for the libraries whose law carries state from step to step (disturbance: the gust; estimator: the estimate; human: the random driver).
New inputs void what the *_state getter reads until a rollout step has run again; a rollout call with another dt restarts the clock, and the law with it: the first
step's record is, bit for bit, the first step's record of a fresh handle started from the same state with the same seed.

A handle of capacity 8, B = 5, the shortest horizon, 3 rollout steps per call (tests/rollout_libs.py); per library ONE set whose law has state: a coloured gust, a gain
of 0.2 on the model's prior, the coloured random driver of tests/human_numpy.py."""
import ctypes as C

import numpy as np
import pytest

import disturbance_numpy
import estimator_numpy
import human_numpy
import rollout_libs as rl
from rollout_libs import grid  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
DP = C.POINTER(C.c_double)
# library -> (the set, the installer's seed, the getter, the article in its refusal, the history setter)
CASES = {
    "disturbance": (disturbance_numpy.identity(Fy=500.0, sigma_Fx=300.0, sigma_Fy=800.0, x_cp=1.0, tau_gust=0.3), dict(seed=SEED), "disturbance_state", "a disturbance",
                    "pg_set_disturbance_history_dev"),
    "estimator": (estimator_numpy.identity(gain=0.2, predict=1), {}, "estimated_state", "an estimator", "pg_set_estimated_history_dev"),
    "human": (human_numpy.four_humans()[3], dict(seed=SEED), "human_state", "a human", "pg_set_human_history_dev"),
}


def first_record(m, library, setter, dt):
    """three steps at `dt` with the history registered: record 0"""
    torch, tdt, dev = m._torch()
    buf = torch.zeros((3, rl.B, rl.HISTORIES[setter][1]), dtype=tdt, device=dev)
    assert rl.register(m, setter, buf, 3) == rl.OK
    assert rl.rollout_status(m, library, 3, dt) == rl.OK
    m.synchronize()
    return buf.cpu().numpy().astype(np.float64)[0]


@pytest.mark.parametrize("library", sorted(CASES))
def test_new_inputs_void_the_state_and_another_dt_restarts_the_law(pkg, skidpad, grid, library):
    one_set, seed, getter, article, setter = CASES[library]
    state, control, t0, other, toff = rl.small_inputs(pkg, skidpad)
    m = rl.make_small(pkg, skidpad, grid)
    rl.install(m, library, [one_set], **seed)
    m.set_inputs(state, control, t0, other, toff)
    # after a rollout step the getter answers
    assert rl.rollout_status(m, library) == rl.OK
    assert getattr(m, getter)().shape[0] == rl.B
    # after new inputs it refuses
    m.set_inputs(state, control, t0, other, toff)
    with pytest.raises(pkg.PigeonError) as e:
        getattr(m, getter)()
    name = {"disturbance_state": "pg_get_disturbance_state", "estimated_state": "pg_get_estimated_state", "human_state": "pg_get_human_state"}[getter]
    assert str(e.value) == f"{name} failed with status {rl.STATE}: {name}: no rollout step under {article} library since the inputs were installed"
    # three steps at DT, then a call at 2 DT: the clock restarts.  Its first record against a fresh handle's, started from the state the second call found
    assert rl.rollout_status(m, library) == rl.OK
    s = np.zeros((rl.B, 6)); c = np.zeros((rl.B, 3)); t = np.zeros(rl.B); o = np.zeros((rl.B, 4))
    m._chk(m.lib.pg_get_state(m.h, s.ctypes.data_as(DP), c.ctypes.data_as(DP), t.ctypes.data_as(DP)), "pg_get_state")
    m._chk(m.lib.pg_get_safety_state(m.h, o.ctypes.data_as(DP), None, None, None), "pg_get_safety_state")
    got = first_record(m, library, setter, 2 * rl.DT)
    m.close()

    fresh = rl.make_small(pkg, skidpad, grid)
    rl.install(fresh, library, [one_set], **seed)
    fresh.set_inputs(s, c, t, o, toff)
    want = first_record(fresh, library, setter, 2 * rl.DT)
    fresh.close()
    assert np.all(np.isfinite(want)) and np.any(want != 0.0)
    assert got.tobytes() == want.tobytes()
