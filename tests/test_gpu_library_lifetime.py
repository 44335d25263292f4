"""The lifetime of the seven set libraries on ONE handle (control parameters, plants, sensors, actuators, disturbances, estimators, humans): each in turn is installed
(two sets and an index), run for a 3-step recorded rollout, cleared and installed again.  The rollout after the second install equals, bit for bit and in every record
the harness knows, the rollout of a fresh handle that only ever saw that one install: whatever the clear freed, whatever it kept and whatever the earlier libraries
left on the handle is invisible.  Capacity 8, B = 5, 3 steps (tests/rollout_libs.py) at the default horizon: at the shortest one (N_short = 1, N_long = 0) the control parameters do not reach
the applied control, and the comparison of that library would be one of two plain rollouts."""
import numpy as np
import pytest

import actuator_numpy
import disturbance_numpy
import estimator_numpy
import human_numpy
import plant_numpy
import rollout_libs as rl
import sensor_numpy
from rollout_libs import grid  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
INDEX = np.array([0, 1, 1, 0, 1], dtype=np.int32)


def libraries(pkg):
    """name -> (installer, its keywords, clearer, two sets whose law acts within three steps, the rollout, the histories to record)"""
    seeded = dict(seed=SEED, streams=rl.stream_ids(rl.B))
    return {
        "control": ("set_control_params", {}, "clear_control_params", [{"R_dFx": 50.0, "deltadot_max": 0.02}, {"Q_e": 40.0, "R_ddelta": 5.0, "deltadot_max": 0.05}], "simulate", {}),
        "plant": ("set_plants", {}, "clear_plants", plant_numpy.four_plants(pkg.X1)[1:3], "simulate", {}),
        "sensor": ("set_sensors", seeded, "clear_sensors", sensor_numpy.four_sensors()[1:3], "simulate", dict(measured=True)),
        "actuator": ("set_actuators", {}, "clear_actuators", [actuator_numpy.six_sets()[k] for k in (1, 5)], "simulate", {}),
        "disturbance": ("set_disturbances", seeded, "clear_disturbances", disturbance_numpy.four_disturbances()[2:4], "simulate", {}),
        "estimator": ("set_estimators", {}, "clear_estimators", estimator_numpy.four_estimators()[1:3], "simulate", dict(estimated=True)),
        "human": ("set_humans", seeded, "clear_humans", [human_numpy.four_humans()[k] for k in (1, 3)], "safety", {}),
    }


def test_install_run_clear_install_again_equals_a_fresh_handle(pkg, skidpad, grid):
    inp = rl.inputs(pkg, skidpad, rl.B, other_seed=43)

    def run(m, kind, hist):
        m.reset()
        rl.start(m, inp, others=True)
        return rl.rollout(m, kind, rl.STEPS, rl.DT, **hist)

    one = rl.make(pkg, skidpad, rl.CAP, grid=grid)
    plain = {kind: run(one, kind, {}) for kind in ("simulate", "safety")}
    for name, (installer, kw, clearer, sets, kind, hist) in libraries(pkg).items():
        getattr(one, installer)(sets, INDEX, **kw)
        first = run(one, kind, hist)
        getattr(one, clearer)()
        getattr(one, installer)(sets, INDEX, **kw)
        second = run(one, kind, hist)
        getattr(one, clearer)()
        fresh = rl.make(pkg, skidpad, rl.CAP, grid=grid)
        getattr(fresh, installer)(sets, INDEX, **kw)
        want = run(fresh, kind, hist)
        fresh.close()
        differ = [k for k in rl.KEYS if not rl.same(second[k], want[k])]
        assert not differ, (name, differ)
        assert not [k for k in rl.KEYS if not rl.same(first[k], want[k])], name
        assert all(want[k] is None or np.all(np.isfinite(want[k])) for k in ("state", "control", "final_state", "measured", "estimated")), name
        assert not (rl.same(want["final_state"], plain[kind]["final_state"]) and rl.same(want["final_control"], plain[kind]["final_control"])), name      # (the library acted)
    # ... and without any of them the handle rolls out as it did before the first
    for kind in plain:
        again = run(one, kind, {})
        assert not [k for k in rl.KEYS if not rl.same(again[k], plain[kind][k])], kind
    one.close()
