"""CPU tests of the actuator library (pg_set_actuator_sets): the numpy twin of the law pinned by closed forms -- a pure delay shifts, a lag answers a step with
1 - exp(-k dt / tau), a slew limit turns a step into a ramp that stops at the target --, the packer's range check, the ctypes structure against the header as the C compiler
lays it out, and the new names declared, exported and mirrored."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import actuator_numpy
from conftest import ROOT

NEW_NAMES = ["pg_set_actuator_sets", "pg_set_actuator_index", "pg_clear_actuator_sets", "pg_get_actuator_sets", "pg_set_applied_history_dev", "pg_set_command_history_dev",
             "pg_get_actuator_state", "pg_actuator_response"]
DT = 0.01


def test_a_pure_delay_shifts_the_sequence_bit_for_bit():
    rng = np.random.default_rng(1)
    c = rng.standard_normal((40, 5, 3))
    c[3, 0, 0] = -0.0; c[4, 1, 1] = np.nan
    for d in (0, 1, 3, 16):
        for dtype in (np.float64, np.float32):
            a = actuator_numpy.actuator_response([actuator_numpy.identity(delay_steps=d)], None, c, DT, dtype)
            want = np.concatenate([np.broadcast_to(c[0], (d, 5, 3)), c[:40 - d]]).astype(dtype).astype(np.float64)
            assert np.array_equal(a.view(np.uint64), want.view(np.uint64)), (d, dtype)


@pytest.mark.parametrize("tau", [0.05, 0.1, 0.2])
def test_a_step_through_the_lag_is_one_minus_exp(tau):
    steps = 60
    c = np.ones((steps, 1, 3)); c[0] = 0.0                       # a_{-1} = c_0 = 0, the step arrives at k = 1
    a = actuator_numpy.actuator_response([actuator_numpy.identity(tau_delta=tau, tau_fx=2 * tau)], None, c, DT)
    k = np.arange(steps)
    assert np.max(np.abs(a[:, 0, 0] - (1 - np.exp(-k * DT / tau)))) < 1e-13
    assert np.max(np.abs(a[:, 0, 1] - (1 - np.exp(-k * DT / (2 * tau))))) < 1e-13 and np.array_equal(a[:, 0, 1], a[:, 0, 2])
    a32 = actuator_numpy.actuator_response([actuator_numpy.identity(tau_delta=tau, tau_fx=2 * tau)], None, c, DT, np.float32)
    assert np.max(np.abs(a32 - a)) < 64 * np.finfo(np.float32).eps


def test_a_slew_limited_step_is_a_ramp_that_stops_at_the_target():
    steps, rate, target = 50, 0.2, 0.05                          # 0.2 rad/s x 0.01 s = 0.002 rad per step: 25 steps to 0.05
    c = np.full((steps, 1, 3), target); c[0] = 0.0
    c[:, :, 1:] *= -1e5                                          # forces: a step DOWN to -5000 N at 5e3 N/s = 50 N per step: never there within 50 steps
    a = actuator_numpy.actuator_response([actuator_numpy.identity(rate_delta=rate, rate_fx=5e3)], None, c, DT)
    k = np.arange(steps)
    assert np.max(np.abs(a[:, 0, 0] - np.minimum(k * rate * DT, target))) < 1e-15
    assert a[-1, 0, 0] == target and np.all(np.diff(a[:, 0, 0]) >= 0)
    assert np.max(np.abs(a[:, 0, 1] + k * 5e3 * DT)) < 1e-9 and np.array_equal(a[:, 0, 1], a[:, 0, 2])
    # delay, lag and slew compose in that order: the delayed step enters the lag, the lag's output is slew-limited
    s = actuator_numpy.identity(delay_steps=2, tau_delta=0.05, rate_delta=0.2)
    a = actuator_numpy.actuator_response([s], None, c, DT)[:, 0, 0]
    assert np.all(a[:3] == 0) and a[3] == pytest.approx(min(0.002, target * -math.expm1(-DT / 0.05)), rel=1e-12)


def test_the_packer_accepts_the_cap_and_refuses_beyond_it(pkg):
    from pigeon_jl_amd import _lib
    M = pkg.BatchedTrajectoryTrackingMPC
    arr = M.pack_actuators([pkg.actuator(), pkg.actuator(delay_steps=16, tau_delta=0.1, rate_fx=5e3, feedback=1), {"delay_steps": 2}])
    assert len(arr) == 3 and _lib.PG_ACT_MAX_DELAY == 16 == actuator_numpy.MAX_DELAY
    assert (arr[0].delay_steps, arr[0].feedback, arr[0].tau_delta, arr[0].tau_fx, arr[0].rate_delta, arr[0].rate_fx) == (0, 0, 0.0, 0.0, math.inf, math.inf)
    assert (arr[1].delay_steps, arr[1].feedback, arr[1].tau_delta, arr[1].rate_delta, arr[1].rate_fx) == (16, 1, 0.1, math.inf, 5e3)
    assert arr[2].delay_steps == 2 and arr[2].rate_delta == math.inf
    assert pkg.actuator() == actuator_numpy.identity() and pkg.vehicles.actuator is pkg.actuator
    for bad in (17, -1, 2.5):
        with pytest.raises(ValueError) as e:
            M.pack_actuators([pkg.actuator(delay_steps=bad)])
        assert "delay_steps" in str(e.value) and "16" in str(e.value)
    with pytest.raises(KeyError):
        pkg.actuator(tau=0.1)
    again = M.pack_actuators([arr[1]])
    assert bytes(again[0]) == bytes(arr[1]) and isinstance(again[0], _lib.pg_actuator_set)


def test_structure_layout_equals_the_headers(pkg, tmp_path):
    """sizeof / offsetof of pg_actuator_set as the C compiler lays out include/pigeon_mpc.h, against the ctypes mirror"""
    from pigeon_jl_amd import _lib
    src = tmp_path / "layout.c"
    fields = [n for n, _ in _lib.pg_actuator_set._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pigeon_mpc.h"\nint main(void) { printf("%zu %d", sizeof(pg_actuator_set), PG_ACT_MAX_DELAY);\n'
                   + "".join(f'printf(" %zu", offsetof(pg_actuator_set, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.pg_actuator_set), _lib.PG_ACT_MAX_DELAY] + [getattr(_lib.pg_actuator_set, f).offset for f in fields]
    assert got[0] == 40 and sorted(fields) == sorted(actuator_numpy.FIELDS)


def test_names_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint " + name + r"\(pg_handle\*", header), name
        assert name in pkg.SYMBOLS
    assert '"stat_actuator_steps"' in header and "ros_integration.jl:51" in header and "model_predictive_control.jl:94-95" in header
    from pigeon_jl_amd import _lib
    assert sorted(_lib.ACTUATOR_SET_PROTOTYPES) == sorted(NEW_NAMES)
    for lib_name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib_name)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW_NAMES) <= exported, sorted(set(NEW_NAMES) - exported)
    M = pkg.BatchedTrajectoryTrackingMPC
    for meth in ("set_actuators", "set_actuator_index", "get_actuators", "clear_actuators", "actuator_response", "actuator_state"):
        assert callable(getattr(M, meth)), meth


def test_the_sequence_of_the_gpu_law_test_is_not_vacuous():
    """The seeded command sequence tests/test_gpu_actuator_sets.py feeds pg_actuator_response, checked with the twin alone: the slew limit of set 5 binds on >= 25 % of the
    steps, the lag's output differs from its input by > 100 bars on >= 50 % of them."""
    import test_gpu_actuator_sets as g
    c, idx = g.law_commands()
    sets = actuator_numpy.six_sets()
    slew, lag = g.law_shares(sets, idx, c)
    assert slew >= 0.25 and lag >= 0.5, (slew, lag)
