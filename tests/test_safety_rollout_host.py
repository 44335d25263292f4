"""CPU tests of the safety rollout (pg_simulate_safety_dev / pg_get_safety_state, include/pigeon_mpc.h): the ABI carries both entry points, and the numpy restatement of
the other car (tests/safety_numpy.py) that the GPU tests check the device against is right on hand-built cases of every branch."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import safety_numpy as sn

NEW = ("pg_simulate_safety_dev", "pg_get_safety_state")


def test_header_declares_the_safety_entry_points():
    txt = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    for name in NEW:
        assert f"int {name}(pg_handle* h" in txt, name


@pytest.mark.parametrize("name", ["libpigeon_hip.so", "libpigeon_hip_f32.so"])
def test_release_libraries_export_the_safety_entry_points(name):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", name)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    for s in NEW:
        assert s in exported, s


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_bindings_carry_the_safety_entry_points(pkg, precision):
    for s in NEW:
        assert s in pkg.SYMBOLS
    lib = pkg.load_library(precision)
    for s in NEW:
        assert hasattr(lib, s)
    assert callable(pkg.BatchedTrajectoryTrackingMPC.simulate_safety_) and callable(pkg.BatchedTrajectoryTrackingMPC.safety_summary)


# ---- optimal_disturbance (HJI_computation.jl:90-131, dMode :min) on hand-built cases --------------------------------------------------------------------------------------

def _case(V, lam_w, lam_Ax):
    x = np.zeros(7); x[5] = V; x[3] = 8.0
    g = np.zeros(7); g[2] = lam_w; g[5] = lam_Ax
    return x, g


@pytest.fixture(scope="module")
def X(pkg):
    return pkg.X1()


def _limits(X, V):
    Ax_max = X["Fx_max"] / X["m"]; maxA = 0.9 * X["mu"] * X["G"]
    return min(Ax_max, X["Px_max"] / X["m"] / V), X["kappa_max"] * V * V, maxA


def test_disturbance_small_gradient_is_zero(X):
    for lam_w, lam_Ax in ((0.0, 0.0), (0.0, 5e-4), (3e-3, 2e-4)):          # lam_norm < 1e-3 (:106-107): at V = 10, lam_Ay = lam_w / 10
        x, g = _case(10.0, lam_w, lam_Ax)
        assert np.array_equal(sn.optimal_disturbance(X, x, g)[0], [0.0, 0.0])


def test_disturbance_accel_beyond_limit_inside_lateral_limit(X):
    V = 10.0; x, g = _case(V, 0.1 * V, -1.0)                                # desAx ~ 8.1 > maxAx ~ 2.85, |desAy| ~ 0.8 < maxAy ~ 11.3
    maxAx, maxAy, maxA = _limits(X, V)
    desAy = -0.1 * maxA / math.hypot(1.0, 0.1)
    assert maxA / math.hypot(1.0, 0.1) > maxAx and abs(desAy) < maxAy
    w, a = sn.optimal_disturbance(X, x, g)[0]
    assert a == maxAx and w == pytest.approx(-min(maxAy, math.sqrt(maxA ** 2 - maxAx ** 2)) / V, rel=1e-15)


def test_disturbance_accel_beyond_limit_outside_lateral_limit(X):
    V = 2.0; x, g = _case(V, -0.5 * V, -1.0)                                # desAx ~ 7.3 > maxAx, desAy ~ 3.6 > maxAy ~ 0.45: maxAy unchanged
    maxAx, maxAy, maxA = _limits(X, V)
    n = math.hypot(1.0, 0.5)
    assert maxA / n > maxAx and 0.5 * maxA / n > maxAy
    w, a = sn.optimal_disturbance(X, x, g)[0]
    assert a == maxAx and w == pytest.approx(maxAy / V, rel=1e-15)


def test_disturbance_lateral_beyond_limit_accelerating(X):
    V = 5.0; x, g = _case(V, 1.0 * V, -0.2)                                 # desAx ~ 1.6 in (0, maxAx], |desAy| ~ 8 > maxAy ~ 2.8
    maxAx, maxAy, maxA = _limits(X, V)
    n = math.hypot(0.2, 1.0)
    assert 0 < 0.2 * maxA / n <= maxAx and maxA / n > maxAy
    w, a = sn.optimal_disturbance(X, x, g)[0]
    assert w == pytest.approx(-maxAy / V, rel=1e-15) and a == pytest.approx(min(math.sqrt(maxA ** 2 - maxAy ** 2), maxAx), rel=1e-15)


def test_disturbance_lateral_beyond_limit_braking(X):
    V = 5.0; x, g = _case(V, 1.0 * V, 0.2)                                  # desAx ~ -1.6 <= 0, |desAy| > maxAy
    maxAx, maxAy, maxA = _limits(X, V)
    w, a = sn.optimal_disturbance(X, x, g)[0]
    assert w == pytest.approx(-maxAy / V, rel=1e-15) and a == pytest.approx(-math.sqrt(maxA ** 2 - maxAy ** 2), rel=1e-15)


def test_disturbance_interior(X):
    V = 10.0; x, g = _case(V, 0.5 * V, 0.5)                                 # desAx = desAy ~ -5.7: inside both limits
    maxAx, maxAy, maxA = _limits(X, V)
    desAy = -0.5 * maxA / math.hypot(0.5, 0.5)
    assert abs(desAy) <= maxAy
    w, a = sn.optimal_disturbance(X, x, g)[0]
    assert w == pytest.approx(desAy / V, rel=1e-15) and a == maxAx


def test_disturbance_at_nonpositive_speed_is_zero(X):
    for V in (0.0, -1.0):                                                   # the reference divides by V: build-defined (0, 0)
        x, g = _case(V, 0.3, -1.0)
        assert np.array_equal(sn.optimal_disturbance(X, x, g)[0], [0.0, 0.0])


def test_disturbance_is_vectorised(X):
    cases = [_case(10.0, 0.0, 0.0), _case(10.0, 1.0, -1.0), _case(5.0, 5.0, 0.2), _case(0.0, 1.0, 1.0)]
    xs = np.stack([c[0] for c in cases]); gs = np.stack([c[1] for c in cases])
    both = sn.optimal_disturbance(X, xs, gs)
    for i, (x, g) in enumerate(cases):
        assert np.array_equal(both[i], sn.optimal_disturbance(X, x, g)[0])


# ---- the other car's RK4 and clamp --------------------------------------------------------------------------------------------------------------------------------------

def test_other_car_straight_line_is_exact():
    o = np.array([[3.0, -2.0, 0.4, 7.5]])
    x = sn.other_car_step(o, [[0.0, 0.0]], 0.01)
    assert np.allclose(x[0], [3.0 - 7.5 * math.sin(0.4) * 0.01, -2.0 + 7.5 * math.cos(0.4) * 0.01, 0.4, 7.5], rtol=0, atol=1e-14)


def test_other_car_constant_turn_follows_the_circle():
    E0, N0, p0, V, w, dt = 1.0, 2.0, -0.3, 9.0, 0.8, 0.05
    x = sn.other_car_step([[E0, N0, p0, V]], [[w, 0.0]], dt)[0]
    p1 = p0 + w * dt
    exact = [E0 + V / w * (math.cos(p1) - math.cos(p0)), N0 + V / w * (math.sin(p1) - math.sin(p0)), p1, V]
    assert np.allclose(x, exact, rtol=0, atol=1e-12)


def test_other_car_accelerating_in_a_straight_line():
    x = sn.other_car_step([[0.0, 0.0, 0.0, 4.0]], [[0.0, 2.0]], 0.1)[0]     # heading North: N = V t + a t^2 / 2 (RK4 is exact on a quadratic)
    assert x[0] == 0.0 and x[3] == pytest.approx(4.2, rel=1e-15) and x[1] == pytest.approx(0.41, rel=1e-14)


def test_other_car_speed_is_clamped_at_zero():
    """V <- max(V, 0) after every sub-step: braking at 10 m/s^2 from 0.05 m/s stops the car after 5 of 10 sub-steps and its speed stays exactly 0.  (The clamp acts at the
    ends of the sub-steps: inside one the speed goes negative, and a car at rest that is still commanded to brake moves back by a h^2 / 2 per sub-step.)"""
    h, a = 0.001, -10.0
    x = sn.other_car_step([[0.0, 0.0, 0.0, 0.05]], [[0.0, a]], 0.01, nsub=10)[0]
    assert x[3] == 0.0 and x[0] == 0.0 and x[2] == 0.0
    speeds = [max(0.05 - 0.01 * i, 0.0) for i in range(10)]                     # at the start of each sub-step
    assert x[1] == pytest.approx(sum(h * v + a * h * h / 2 for v in speeds), rel=1e-9, abs=1e-15)   # (RK4 is exact on each sub-step's quadratic)
    free = sn.other_car_step([[0.0, 0.0, 0.0, 0.05]], [[0.0, a]], 0.01, nsub=1)[0]
    assert free[3] == 0.0                                                       # one sub-step: -0.05 at its end, clamped


def test_relative_state_matches_the_frame_convention():
    us = np.array([[10.0, 20.0, 0.0, 8.0, 0.1, 0.02]])
    th = np.array([[10.0, 25.0, 0.2, 6.0]])                                  # 5 m straight ahead (heading North), turned 0.2 rad left
    x = sn.relative_state(us, th)[0]
    assert np.allclose(x, [5.0, 0.0, 0.2, 8.0, 0.1, 6.0, 0.02], atol=1e-14)
