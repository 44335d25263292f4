"""CPU tests of the estimator library (pg_set_estimator_sets): the numpy twin of the law pinned by closed forms -- all gains 1 is the measurement itself, gain 0 with the
model as the prior is dead reckoning, without the model every channel is the exponential low-pass in closed form --, the noise reduction a fixed gain of 0.2 buys on an
exact model (sqrt(L / (2 - L)) = 1/3 on a marginally stable channel), the restart of one instance whose prior is not finite, the ctypes structure against the header as
the C compiler lays it out, and the new names declared, exported and mirrored."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import estimator_numpy as en
import plant_numpy
import sensor_numpy
from conftest import ROOT

NEW_NAMES = ["pg_set_estimator_sets", "pg_set_estimator_index", "pg_clear_estimator_sets", "pg_get_estimator_sets", "pg_get_estimated_state",
             "pg_set_estimated_history_dev", "pg_estimator_response"]
DT = 0.01


def open_loop(pkg, traj, B, steps, seed=4):
    """true states [steps][B][6] of the controller's own vehicle with the start control held, and that control [steps][B][3]"""
    state, control, _, _ = pkg.synthetic.config2_inputs(traj, B, seed=seed)
    X1 = pkg.X1()
    x = np.empty((steps, B, 6)); x[0] = state
    for k in range(1, steps):
        x[k] = plant_numpy.plant_step_vec(X1, x[k - 1], control, DT)
    return x, np.broadcast_to(control, (steps, B, 3)).copy(), X1


def test_the_closed_forms(pkg, skidpad):
    B, steps = 6, 20
    x, u, X1 = open_loop(pkg, skidpad, B, steps)
    rng = np.random.default_rng(7)
    y = x + 0.05 * rng.standard_normal(x.shape)
    y[3, 2, 1] = -0.0; y[5, 1, 4] = np.nan                     # copies keep what arithmetic would not
    # all gains 1: the measurement, bit for bit, whatever predict says
    for pred in (0, 1):
        got = en.response([en.identity(predict=pred)], None, y, u, DT, X1)
        assert np.array_equal(got.view(np.uint64), y.view(np.uint64))
    # gain 0 with the model: dead reckoning from the first measurement
    y = np.nan_to_num(y)
    got = en.response([en.identity(gain=0.0, predict=1)], None, y, u, DT, X1)
    want = y[0].copy()
    for k in range(1, steps):
        want = plant_numpy.plant_step_vec(X1, want, u[k - 1], DT)
        assert np.array_equal(got[k], want), k
    # no model: xh_k = (1 - g)^k y_0 + g sum_{j=1..k} (1 - g)^(k - j) y_j
    for g in (0.2, 0.5):
        got = en.response([en.identity(gain=g, predict=0)], None, y, u, DT, X1)
        for k in range(steps):
            want = (1 - g) ** k * y[0] + g * sum((1 - g) ** (k - j) * y[j] for j in range(1, k + 1))
            assert np.max(np.abs(got[k] - want)) < 1e-12 * max(1.0, np.max(np.abs(want))), (g, k)
    # the mixed set: E, N copied, Uy dead-reckoned through the model of the whole estimate
    mix = en.four_estimators()[3]
    got = en.response([mix], None, y, u, DT, X1)
    assert np.array_equal(got[..., :2], y[..., :2])
    for k in range(1, steps):
        assert np.array_equal(got[k, :, 4], plant_numpy.plant_step_vec(X1, got[k - 1], u[k - 1], DT)[:, 4])
    # a library of four, selected per instance, is each set on its own instances
    idx = np.arange(B) % 4
    sets = en.four_estimators()
    both = en.response(sets, idx, y, u, DT, X1)
    for s in range(4):
        assert np.array_equal(both[:, idx == s], en.response([sets[s]], None, y[:, idx == s], u[:, idx == s], DT, X1))


def noise_reduction_ratios(pkg, traj, gain, predict=1, B=64, steps=250, seed=2026):
    """RMS(xh - x) / RMS(y - x) per channel over the steps 50 and up: X1, B instances, `steps` steps of 10 ms, open loop, the noise of sensor_numpy.four_sensors()[1]"""
    x, u, X1 = open_loop(pkg, traj, B, steps)
    sigma = sensor_numpy.four_sensors()[1][0]
    y = x + sigma * np.random.default_rng(seed).standard_normal(x.shape)
    xh = en.response([en.identity(gain=gain, predict=predict)], None, y, u, DT, X1)
    rms = lambda a: np.sqrt(np.mean(a[50:] ** 2, axis=(0, 1)))
    return rms(xh - x) / rms(y - x)


def test_a_gain_of_one_fifth_filters_the_noise(pkg, skidpad):
    """The bar of 0.5 on every channel: the derived value on an exact model and a marginally stable channel is sqrt(L / (2 - L)) = 1/3 at L = 0.2; 0.5 leaves room for
    sample noise and fails an estimator that does not filter (gain 1: exactly 1)."""
    r = noise_reduction_ratios(pkg, skidpad, 0.2)
    print("gain 0.2, predict 1: RMS(xh - x) / RMS(y - x) per channel (E, N, psi, Ux, Uy, r) = " + ", ".join(f"{v:.3f}" for v in r))
    assert np.all(r < 0.5), r
    r5 = noise_reduction_ratios(pkg, skidpad, 0.5)
    print("gain 0.5, predict 1: " + ", ".join(f"{v:.3f}" for v in r5))
    assert np.all(r5 > r) and np.all(r5 < 1.0)
    assert np.array_equal(noise_reduction_ratios(pkg, skidpad, 1.0), np.ones(6))


def test_a_non_finite_prior_reseeds_that_instance_only(pkg, skidpad):
    B, steps = 8, 12
    x, u, X1 = open_loop(pkg, skidpad, B, steps)
    y = x + 0.02 * np.random.default_rng(3).standard_normal(x.shape)
    sets = [en.identity(gain=0.2, predict=1)]
    clean = en.response(sets, None, y, u, DT, X1)
    bad = u.copy(); bad[4, 5, 0] = np.nan                      # the control of step 4 drives the prior of step 5
    got = en.response(sets, None, y, bad, DT, X1)
    others = np.arange(B) != 5
    assert np.array_equal(got[:, others], clean[:, others])
    assert np.array_equal(got[:5, 5], clean[:5, 5]) and np.array_equal(got[5, 5], y[5, 5])
    assert np.all(np.isfinite(got))
    # ... and it filters again from there: step 6 is one step of the law from y_5
    assert np.array_equal(got[6, 5], en.step(sets, None, y[5, 5:6], y[6, 5:6], u[5, 5:6], DT, X1)[0])
    assert not np.array_equal(got[6, 5], y[6, 5])
    # without the model a non-finite ESTIMATE is the prior: an infinite measurement is replaced by the next one
    y2 = y.copy(); y2[3, 2, 3] = np.inf
    lp = en.response([en.identity(gain=0.5, predict=0)], None, y2, u, DT, X1)
    assert np.isinf(lp[3, 2, 3]) and np.array_equal(lp[4, 2], y2[4, 2]) and np.all(np.isfinite(lp[4:]))


def test_structure_layout_equals_the_headers(pkg, tmp_path):
    """sizeof / offsetof of pg_estimator as the C compiler lays out include/pigeon_mpc.h, against the ctypes mirror"""
    from pigeon_jl_amd import _lib
    src = tmp_path / "layout.c"
    fields = [n for n, _ in _lib.pg_estimator._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pigeon_mpc.h"\nint main(void) { printf("%zu", sizeof(pg_estimator));\n'
                   + "".join(f'printf(" %zu", offsetof(pg_estimator, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.pg_estimator)] + [getattr(_lib.pg_estimator, f).offset for f in fields]
    assert got == [56, 0, 4, 8] and tuple(fields) == en.FIELDS == pkg.vehicles.ESTIMATOR_FIELDS


def test_names_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    julia = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint " + name + r"\(pg_handle\*", header), name
        assert name in pkg.SYMBOLS and ":" + name in julia and name in integration, name
    assert '"stat_estimator_steps"' in header and "IDENTITY" in header
    from pigeon_jl_amd import _lib
    assert sorted(_lib.ESTIMATOR_SET_PROTOTYPES) == sorted(NEW_NAMES)
    # the export map lets pg_* through and nothing else: the dynamic symbol table is the check
    assert "pg_*" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_exports.map")).read()
    for lib_name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib_name)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW_NAMES) <= exported, sorted(set(NEW_NAMES) - exported)
    M = pkg.BatchedTrajectoryTrackingMPC
    for meth in ("set_estimators", "set_estimator_index", "clear_estimators", "get_estimators", "estimated_state", "estimator_response"):
        assert callable(getattr(M, meth)), meth


def test_the_packer_and_the_identity(pkg):
    from pigeon_jl_amd import _lib
    M = pkg.BatchedTrajectoryTrackingMPC
    assert pkg.estimator() == en.identity() and pkg.vehicles.estimator is pkg.estimator
    assert pkg.estimator(gain=np.float32(0.5)) == en.identity(gain=0.5) and pkg.estimator(gain=np.float64(0.2)) == en.identity(gain=0.2)
    assert pkg.estimator(gain=0.2) == en.identity(gain=0.2) and pkg.estimator(gain={"Ux": 0.3})["gain"] == [1.0, 1.0, 1.0, 0.3, 1.0, 1.0]
    with pytest.raises(KeyError):
        pkg.estimator(gains=0.5)
    with pytest.raises(KeyError):
        pkg.vehicles.estimator(gain={"beta": 0.5})
    with pytest.raises(ValueError):
        pkg.estimator(gain=[0.5] * 5)
    arr = M.pack_estimators(en.four_estimators() + [{"predict": 0}])
    assert len(arr) == 5 and isinstance(arr[0], _lib.pg_estimator)
    assert (arr[0].predict, arr[0].reserved, list(arr[0].gain)) == (1, 0, [1.0] * 6)
    assert (arr[1].predict, list(arr[1].gain)) == (1, [0.2] * 6) and (arr[2].predict, list(arr[2].gain)) == (0, [0.5] * 6)
    assert (arr[3].predict, list(arr[3].gain)) == (1, [1.0, 1.0, 0.2, 0.2, 0.0, 0.2])
    assert (arr[4].predict, list(arr[4].gain)) == (0, [1.0] * 6)
    with pytest.raises(ValueError):
        M.pack_estimators([pkg.estimator(predict=0.5)])
    again = M.pack_estimators([arr[3]])
    assert bytes(again[0]) == bytes(arr[3])
