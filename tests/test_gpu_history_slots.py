"""The one-shot history registrations of the rollout libraries (pg_set_measured_ / applied_ / command_ / disturbance_ / estimated_ / human_history_dev), setter by setter:
what each refuses, that a registration of `steps` records serves exactly the next rollout call and exactly that many steps, and what drops it.

A handle of capacity 8, B = 5, the shortest horizon, the library's identity set, 3 rollout steps (tests/rollout_libs.py).  Every buffer is a 3-step device tensor filled with a
sentinel no record can hold; "written" = no sentinel left in the record, "untouched" = nothing but the sentinel."""
import numpy as np
import pytest

import rollout_libs as rl
from rollout_libs import grid  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SETTERS = sorted(rl.HISTORIES)


def sentinel_buffer(m, width):
    torch, tdt, dev = m._torch()
    return torch.full((3, rl.B, width), SENTINEL, dtype=tdt, device=dev)


def records(m, buf):
    m.synchronize()
    return buf.cpu().numpy().astype(np.float64)


def started(pkg, skidpad, grid, library=None):
    m = rl.make_small(pkg, skidpad, grid)
    m.set_inputs(*rl.small_inputs(pkg, skidpad))
    if library:
        rl.install(m, library)
    return m


@pytest.mark.parametrize("setter", SETTERS)
def test_what_a_history_setter_refuses_and_what_clears_its_slot(pkg, skidpad, grid, setter):
    library, width, hint = rl.HISTORIES[setter]
    m = started(pkg, skidpad, grid)
    buf = sentinel_buffer(m, width)
    # without the library: PG_ERR_STATE, the library's message and its hint
    assert rl.register(m, setter, buf, 3) == rl.STATE
    assert rl.last_error(m) == f"{setter}: no {library} library installed {hint}"
    # steps = 0 with a buffer: PG_ERR_INVALID (with or without the library)
    assert rl.register(m, setter, buf, 0) == rl.INVALID
    assert rl.last_error(m) == f"{setter}: steps >= 1 required"
    rl.install(m, library)
    assert rl.register(m, setter, buf, 0) == rl.INVALID
    assert rl.last_error(m) == f"{setter}: steps >= 1 required"
    # a null buffer: PG_OK, and a pending registration is gone
    assert rl.register(m, setter, buf, 3) == rl.OK
    assert rl.register(m, setter, None, 3) == rl.OK
    assert rl.rollout_status(m, library) == rl.OK
    assert np.all(records(m, buf) == SENTINEL)
    # pg_clear_*_sets drops a pending registration
    assert rl.register(m, setter, buf, 3) == rl.OK
    rl.clear(m, library)
    rl.install(m, library)
    assert rl.rollout_status(m, library) == rl.OK
    assert np.all(records(m, buf) == SENTINEL)
    m.close()


@pytest.mark.parametrize("setter", SETTERS)
def test_a_registration_serves_the_next_rollout_call_and_no_step_beyond_it(pkg, skidpad, grid, setter):
    library, width, _ = rl.HISTORIES[setter]
    m = started(pkg, skidpad, grid, library)
    buf = sentinel_buffer(m, width)
    # 2 steps registered, 3 run: records 0 and 1 are written, record 2 is not
    assert rl.register(m, setter, buf, 2) == rl.OK
    assert rl.rollout_status(m, library, 3) == rl.OK
    first = records(m, buf)
    assert np.all(np.isfinite(first[:2])) and not np.any(first[:2] == SENTINEL)
    assert np.all(first[2] == SENTINEL)
    # one-shot: a second rollout without registering again writes nothing
    assert rl.rollout_status(m, library, 3) == rl.OK
    assert records(m, buf).tobytes() == first.tobytes()
    # a rollout call that fails its argument check (dt = 0) has consumed the registration all the same
    fresh = sentinel_buffer(m, width)
    assert rl.register(m, setter, fresh, 3) == rl.OK
    assert rl.rollout_status(m, library, 3, dt=0.0) == rl.INVALID
    assert rl.rollout_status(m, library, 3) == rl.OK
    assert np.all(records(m, fresh) == SENTINEL)
    m.close()
