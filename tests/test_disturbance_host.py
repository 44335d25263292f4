"""CPU tests of the disturbance library (pg_set_disturbance_sets): the numpy twin of the law pinned by closed forms -- outside its window a set is exactly (0, 0, 0, 1), a
white gust is the draw itself, the coloured gust has unit variance and lag-1 correlation exp(-dt / tau) --, block 2 of the generator apart from the sensor's blocks, the
disturbed plant against an exact identity of the model (a constant Fx is a shift of the drag constant), the ctypes structure against the header as the C compiler lays it
out, and the new names declared, exported and mirrored."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import disturbance_numpy as dn
import plant_numpy
import sensor_numpy
from conftest import ROOT

NEW_NAMES = ["pg_set_disturbance_sets", "pg_set_disturbance_index", "pg_set_disturbance_seed", "pg_clear_disturbance_sets", "pg_get_disturbance_sets",
             "pg_disturbance_response", "pg_get_disturbance_state", "pg_set_disturbance_history_dev"]
DT = 0.01
SEED = 0x9E3779B97F4A7C15


def test_outside_the_window_w_is_exactly_zero_zero_zero_one():
    sets = dn.four_disturbances()
    B = 8
    idx = np.arange(B) % 4
    w = dn.response(sets, idx, SEED, np.arange(B), 0, 14, DT)
    k = np.arange(14)
    for b in range(B):
        s = sets[idx[b]]
        inside = (k >= s["step_on"]) & ((s["step_off"] < 0) | (k < s["step_off"]))
        assert np.array_equal(w[~inside, b], np.broadcast_to(dn.IDENTITY_W, (int((~inside).sum()), 4))), b
        assert np.all(w[inside, b, 3] == s["mu_scale"])
    assert np.array_equal(w[:, idx == 0], np.broadcast_to(dn.IDENTITY_W, (14, 2, 4)))          # the identity set: inside its window, and still nothing
    assert np.all(w[2:, idx == 2, :3] == 0.0) and np.all(w[:2, idx == 2, 3] == 1.0) and np.all(w[2:, idx == 2, 3] == 0.55)
    side = w[3:9, idx == 1]
    assert np.all(side[..., 0] == 0.0) and np.all(side[..., 1] != 2000.0)
    assert np.max(np.abs(side[..., 2] - (side[..., 1] - 2000.0))) < 1e-9                        # gust moment = x_cp x gust Fy (x_cp = 1, Mz = 0)


def test_a_white_gust_is_the_draw():
    B, steps = 5, 30
    streams = 1000 + np.arange(B)
    z = dn.normals(SEED, streams, 4, steps)
    n = dn.gust_states([dn.identity(tau_gust=0.0)], None, SEED, streams, 4, steps, DT)
    assert np.array_equal(n, z)
    w = dn.response([dn.identity(Fx=-1000.0, sigma_Fx=500.0, Fy=3.0, sigma_Fy=2.0, x_cp=0.5, Mz=7.0)], None, SEED, streams, 4, steps, DT)
    assert np.array_equal(w[..., 0], -1000.0 + 500.0 * z[..., 0]) and np.array_equal(w[..., 1], 3.0 + 2.0 * z[..., 1])
    assert np.array_equal(w[..., 2], 7.0 + 0.5 * (2.0 * z[..., 1])) and np.all(w[..., 3] == 1.0)
    # a coloured gust starts from the draw too, and a set's window does not stop its state
    n2 = dn.gust_states([dn.identity(tau_gust=0.3)], None, SEED, streams, 4, steps, DT)
    assert np.array_equal(n2[0], z[0]) and not np.array_equal(n2[1], z[1])
    rho, g = np.exp(-DT / 0.3), np.sqrt(-np.expm1(-2 * DT / 0.3))
    assert np.array_equal(n2[1], rho * z[0] + g * z[1])
    assert abs(rho * rho + g * g - 1.0) < 1e-15                                                  # stationary: unit variance is kept


def test_the_coloured_gust_has_unit_variance_and_lag_one_correlation_rho():
    """2 x 10^5 draws per component: 200 streams x 1000 steps, tau = 0.05 s at dt = 0.01 s (rho = 0.819).  Every stream starts in the stationary law (n_0 = z_0), so all
    draws count.  Standard errors of a Gaussian AR(1) (Bartlett): Cov(n_i^2, n_j^2) = 2 rho^(2 |i - j|), so Var(mean n^2) = 2 (1 + rho^2) / ((1 - rho^2) N); the lag-1
    sample correlation has variance (1 - rho^2) / N.  Both within 3 standard errors."""
    S, T, tau = 200, 1000, 0.05
    n = dn.gust_states([dn.identity(tau_gust=tau)], None, SEED, np.arange(S), 0, T, DT)
    rho = np.exp(-DT / tau); N = S * T
    se_var = np.sqrt(2.0 * (1.0 + rho ** 2) / ((1.0 - rho ** 2) * N)); se_r = np.sqrt((1.0 - rho ** 2) / N)
    for c in range(2):
        x = n[..., c]
        var = float(np.mean(x * x)); r1 = float(np.mean(x[1:] * x[:-1]) / np.mean(x * x))
        print(f"component {c}: variance {var:.5f} (1 +- {3 * se_var:.5f}), lag-1 correlation {r1:.5f} ({rho:.5f} +- {3 * se_r:.5f}), mean {np.mean(x):+.4f}")
        assert abs(var - 1.0) <= 3 * se_var and abs(r1 - rho) <= 3 * se_r
    assert abs(float(np.mean(n[..., 0] * n[..., 1]))) <= 3 * np.sqrt((1.0 + rho ** 2) / ((1.0 - rho ** 2) * N))      # the two components are independent


def test_block_two_is_apart_from_the_sensors_blocks():
    streams = np.array([0, 1, 69, 2 ** 40 + 3], dtype=np.uint64)
    b0, b1 = sensor_numpy.words(SEED, streams, 5, 12)
    b2 = dn.block2_words(SEED, streams, 5, 12)
    assert b2.shape == b0.shape
    for other in (b0, b1):
        assert not np.any(b2 == other)                          # 192 words of 32 bits: a chance equality has probability 4e-8
    # the counter's second word alone tells the blocks apart
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint64)
    one = sensor_numpy.philox4x32_10(np.array([5, 2, 69, 0], dtype=np.uint64), key)
    assert np.array_equal(one, b2[0, 2])


def test_a_constant_force_is_a_shift_of_the_drag_constant(pkg, skidpad):
    """dUx = (Fxf cos d - Fyf sin d + Fxr - Cd0 - ...) / m + r Uy: a body-frame Fx is Cd0 - Fx, exactly, in the model (not in the rounding: (a + F) / m against
    a / m + F / m differ by an ulp of the acceleration, 1e-15 relative, which ten RK4 sub-steps do not amplify beyond 1e-13).  The tire forces read Fxf, Fxr and the
    load transfer, none of which sees Cd0."""
    B = 70
    state, control, _, _ = pkg.synthetic.config2_inputs(skidpad, B, seed=4)
    X1 = pkg.X1()
    for Fx in (-1000.0, 350.0):
        w = np.tile(np.array([Fx, 0.0, 0.0, 1.0]), (B, 1))
        got = dn.plant_step_vec_dist(X1, state, control, w, DT)
        want = plant_numpy.plant_step_vec(dict(X1, Cd0=X1["Cd0"] - Fx), state, control, DT)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        assert err.max() < 1e-13, (Fx, float(err.max()))
        assert np.max(np.abs(got[:, 3] - plant_numpy.plant_step_vec(X1, state, control, DT)[:, 3])) > 1e-3          # ... and the force is felt
    # w = (0, 0, 0, 1) is the undisturbed plant, bit for bit; mu_scale is a plant with that mu
    ident = np.tile(dn.IDENTITY_W, (B, 1))
    assert np.array_equal(dn.plant_step_vec_dist(X1, state, control, ident, DT), plant_numpy.plant_step_vec(X1, state, control, DT))
    slip = np.tile(np.array([0.0, 0.0, 0.0, 0.55]), (B, 1))
    assert np.array_equal(dn.plant_step_vec_dist(X1, state, control, slip, DT), plant_numpy.plant_step_vec(dict(X1, mu=X1["mu"] * 0.55), state, control, DT))


def test_the_replay_test_of_the_gpu_file_is_not_vacuous(pkg, skidpad):
    """The share tests/test_gpu_disturbance_sets.py asserts (>= 50 %), with the twin alone: 12 steps from the 70 starts with the start control held, the undisturbed step
    against the disturbed one on the active instance-steps of the non-identity sets, apart by more than 100 fp32 bars (2e-3) in state units."""
    import test_gpu_disturbance_sets as g
    share, per_set, share_rel = g.replay_share_on_the_starts(pkg, skidpad)
    print(f"held control, 12 steps: undisturbed vs disturbed step apart by > 100 x 2e-5 on {share:.0%} of the active instance-steps (side gust, friction window, headwind: "
          f"{per_set}); divided by max(1, |ref|): {share_rel:.0%}")
    assert share >= 0.5


def test_structure_layout_equals_the_headers(pkg, tmp_path):
    """sizeof / offsetof of pg_disturbance as the C compiler lays out include/pigeon_mpc.h, against the ctypes mirror"""
    from pigeon_jl_amd import _lib
    src = tmp_path / "layout.c"
    fields = [n for n, _ in _lib.pg_disturbance._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pigeon_mpc.h"\nint main(void) { printf("%zu", sizeof(pg_disturbance));\n'
                   + "".join(f'printf(" %zu", offsetof(pg_disturbance, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.pg_disturbance)] + [getattr(_lib.pg_disturbance, f).offset for f in fields]
    assert got == [72, 0, 4, 8, 16, 24, 32, 40, 48, 56, 64] and tuple(fields) == dn.FIELDS == pkg.vehicles.DISTURBANCE_FIELDS


def test_names_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    julia = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint " + name + r"\(pg_handle\*", header), name
        assert name in pkg.SYMBOLS and ":" + name in julia and name in integration, name
    assert '"stat_disturbance_steps"' in header and "model_predictive_control.jl:94" in header and "ZERO RULE" in header
    from pigeon_jl_amd import _lib
    assert sorted(_lib.DISTURBANCE_SET_PROTOTYPES) == sorted(NEW_NAMES)
    # the export map lets pg_* through and nothing else: the dynamic symbol table is the check
    assert "pg_*" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_exports.map")).read()
    for lib_name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib_name)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW_NAMES) <= exported, sorted(set(NEW_NAMES) - exported)
    M = pkg.BatchedTrajectoryTrackingMPC
    for meth in ("set_disturbances", "set_disturbance_index", "set_disturbance_seed", "clear_disturbances", "disturbances", "disturbance_response", "disturbance_state"):
        assert callable(getattr(M, meth)), meth


def test_the_packer_and_the_identity(pkg):
    from pigeon_jl_amd import _lib
    M = pkg.BatchedTrajectoryTrackingMPC
    assert pkg.disturbance() == dn.identity() and pkg.vehicles.disturbance is pkg.disturbance
    with pytest.raises(KeyError):
        pkg.disturbance(sigma=1.0)
    with pytest.raises(KeyError):
        pkg.vehicles.disturbance(mu=0.5)
    arr = M.pack_disturbances(dn.four_disturbances() + [{"Mz": 5.0}])
    assert len(arr) == 5 and isinstance(arr[0], _lib.pg_disturbance)
    assert (arr[0].step_on, arr[0].step_off, arr[0].Fx, arr[0].sigma_Fy, arr[0].mu_scale) == (0, -1, 0.0, 0.0, 1.0)
    assert (arr[1].step_on, arr[1].step_off, arr[1].Fy, arr[1].x_cp, arr[1].sigma_Fy, arr[1].tau_gust) == (3, 9, 2000.0, 1.0, 800.0, 0.3)
    assert (arr[2].step_on, arr[2].step_off, arr[2].mu_scale) == (2, -1, 0.55) and (arr[3].Fx, arr[3].sigma_Fx, arr[3].tau_gust) == (-1000.0, 500.0, 0.0)
    assert arr[4].Mz == 5.0 and arr[4].mu_scale == 1.0
    with pytest.raises(ValueError):
        M.pack_disturbances([pkg.disturbance(step_on=2.5)])
    again = M.pack_disturbances([arr[1]])
    assert bytes(again[0]) == bytes(arr[1])
