"""CPU tests of the human library (pg_set_human_sets): the numpy twin of the law against itself -- the identity sets are the three human modes of the rollouts, a set
outside its window is exactly (0, 0), a decision is kept for hold_steps steps from step_on and forced on a fresh state, gain 1 and limits at infinity copy the bits, the
random driver has the moments of its (sigma, tau) --, block 3 of the generator apart from the blocks taken, the ctypes structure against the header as the C compiler lays
it out, vehicles.human, and the new names declared, exported and mirrored."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import disturbance_numpy
import human_numpy as hn
import safety_numpy
import sensor_numpy
from conftest import ROOT

NEW_NAMES = ["pg_set_human_sets", "pg_set_human_index", "pg_set_human_seed", "pg_clear_human_sets", "pg_get_human_sets", "pg_get_human_state", "pg_set_human_history_dev",
             "pg_human_response"]
DT = 0.01
SEED = 0x9E3779B97F4A7C15


def inputs(pkg, B, steps, seed=5):
    """relative states with a live other car, gradients that make optimal_disturbance take every branch, and a script with signed zeros and a NaN in it"""
    rng = np.random.default_rng(seed)
    x7 = rng.normal(size=(steps, B, 7)); x7[..., 5] = rng.uniform(0.5, 30.0, size=(steps, B)); x7[:, ::7, 5] = 0.0
    vg8 = rng.normal(size=(steps, B, 8)); vg8[:, 3::11, 1:] = 0.0
    script = rng.normal(size=(steps, B, 2)); script[0, 0] = (-0.0, np.nan); script[1, 1] = (0.0, -0.0)
    return pkg.X1(), x7, vg8, script


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_identity_sets_are_the_three_human_modes(pkg):
    B, steps = 23, 9
    X, x7, vg8, script = inputs(pkg, B, steps)
    st = np.arange(B)
    hold = hn.response(X, [hn.identity(0)], None, SEED, st, 0, steps, DT, x7, vg8, script)
    assert np.array_equal(bits(hold), bits(np.zeros((steps, B, 2))))
    worst = hn.response(X, [hn.identity(1)], None, SEED, st, 0, steps, DT, x7, vg8, script)
    want = np.stack([safety_numpy.optimal_disturbance(X, x7[k], vg8[k][:, 1:]) for k in range(steps)])
    assert np.array_equal(bits(worst), bits(want)) and np.count_nonzero(worst[..., 1]) > steps * B // 2
    assert np.all(worst[:, ::7] == 0.0) and np.all(worst[:, 3::11] == 0.0)                      # speed 0, flat gradient
    assert np.array_equal(hn.response(X, [hn.identity(1)], None, SEED, st, 0, steps, DT, x7, vg8, script, has_hji=False), np.zeros((steps, B, 2)))
    scr = hn.response(X, [hn.identity(2)], None, SEED, st, 0, steps, DT, x7, vg8, script)
    assert np.array_equal(bits(scr), bits(script))                                              # -0.0 and the NaN included
    # ... and a mixed library is the composition per instance
    idx = st % 3
    mixed = hn.response(X, [hn.identity(m) for m in range(3)], idx, SEED, st, 0, steps, DT, x7, vg8, script)
    for m, ref in enumerate((hold, worst, scr)):
        assert np.array_equal(bits(mixed[:, idx == m]), bits(ref[:, idx == m]))


def test_window_edges(pkg):
    B, steps = 6, 12
    X, x7, vg8, script = inputs(pkg, B, steps)
    for on, off in ((3, 6), (0, 1), (11, -1), (4, 4)):
        u, how, decided = hn.response(X, [hn.identity(2, step_on=on, step_off=off)], None, SEED, np.arange(B), 0, steps, DT, x7, vg8, script, explain=True)
        k = np.arange(steps)
        inside = (k >= on) & ((off < 0) | (k < off))
        assert np.array_equal(bits(u[inside]), bits(script[inside])) and np.array_equal(bits(u[~inside]), bits(np.zeros_like(u[~inside]))), (on, off)
        assert np.all(decided[~inside] == -1) and np.all(decided[inside] == k[inside][:, None]) and np.all(how == hn.EXACT)
    # a sequence that starts inside the window: the same values, whatever step0
    late = hn.response(X, [hn.identity(2, step_on=3, step_off=6)], None, SEED, np.arange(B), 4, 5, DT, x7[4:9], vg8[4:9], script[4:9])
    assert np.array_equal(bits(late[:2]), bits(script[4:6])) and np.all(late[2:] == 0.0)


def test_hold_phase_and_the_forced_decision_on_a_fresh_state(pkg):
    B, steps = 5, 14
    X, x7, vg8, script = inputs(pkg, B, steps)
    script = np.nan_to_num(script)
    s = hn.identity(2, hold_steps=3, step_on=2)
    u, _, decided = hn.response(X, [s], None, SEED, np.arange(B), 0, steps, DT, x7, vg8, script, explain=True)
    want = [-1, -1, 2, 2, 2, 5, 5, 5, 8, 8, 8, 11, 11, 11]                                       # the phase counts from step_on, not from 0
    assert decided[:, 0].tolist() == want
    for k, d in enumerate(want):
        assert np.array_equal(bits(u[k]), bits(script[d] if d >= 0 else np.zeros((B, 2))))
    # a fresh state in the middle of a hold: a decision at once, then the set's own phase again
    u2, _, d2 = hn.response(X, [s], None, SEED, np.arange(B), 6, 8, DT, x7[6:], vg8[6:], script[6:], explain=True)
    assert d2[:, 0].tolist() == [6, 6, 8, 8, 8, 11, 11, 11]
    assert np.array_equal(bits(u2[0]), bits(script[6])) and np.array_equal(bits(u2[2:]), bits(u[8:]))
    # hold_steps = 1 decides at every step
    assert hn.response(X, [hn.identity(2)], None, SEED, np.arange(B), 0, steps, DT, x7, vg8, script, explain=True)[2][:, 0].tolist() == list(range(steps))


def test_gain_one_and_limits_at_infinity_copy_the_bits(pkg):
    B, steps = 23, 4
    X, x7, vg8, script = inputs(pkg, B, steps)
    st = np.arange(B)
    same = hn.response(X, [hn.identity(2, gain=[1.0, 1.0], omega_max=np.inf, a_min=-np.inf, a_max=np.inf)], None, SEED, st, 0, steps, DT, x7, vg8, script)
    assert np.array_equal(bits(same), bits(script))
    # finite limits touch only what lies outside them: -0.0 and the NaN stay, everything inside keeps its bits
    lim = hn.response(X, [hn.identity(2, omega_max=0.5, a_min=-0.25, a_max=0.75)], None, SEED, st, 0, steps, DT, x7, vg8, script)
    w, a = script[..., 0], script[..., 1]
    inside_w = ~(np.abs(w) > 0.5); inside_a = ~((a < -0.25) | (a > 0.75))
    assert np.array_equal(bits(lim[..., 0][inside_w]), bits(w[inside_w])) and np.array_equal(bits(lim[..., 1][inside_a]), bits(a[inside_a]))
    assert np.array_equal(lim[..., 0][~inside_w], 0.5 * np.sign(w[~inside_w])) and np.array_equal(lim[..., 1][~inside_a], np.where(a[~inside_a] > 0, 0.75, -0.25))
    assert np.signbit(lim[0, 0, 0]) and np.isnan(lim[0, 0, 1]) and np.signbit(lim[1, 1, 1])
    # a gain is one product, and a gain of 0 silences the driver
    half = hn.response(X, [hn.identity(1, gain=[0.5, 0.25])], None, SEED, st, 0, steps, DT, x7, vg8, script)
    worst = hn.response(X, [hn.identity(1)], None, SEED, st, 0, steps, DT, x7, vg8, script)
    assert np.array_equal(half, worst * np.array([0.5, 0.25])) and np.all(hn.response(X, [hn.identity(1, gain=[0.0, 0.0])], None, SEED, st, 0, steps, DT, x7, vg8, script) == 0.0)


def test_the_random_driver_has_the_moments_of_its_set():
    """10^5 draws per component: 100 streams x 1000 steps, tau = 0.05 s at dt = 0.01 s (rho = 0.819), hold_steps = 1, no limits, so u = sigma n.  The bars of the gust
    (tests/test_disturbance_host.py): Var(mean n^2) = 2 (1 + rho^2) / ((1 - rho^2) N), the lag-1 sample correlation has variance (1 - rho^2) / N; both within 3 standard
    errors.  A white driver (tau = 0) is sigma times the draw itself, and a sigma of 0 is exactly 0."""
    S, T, tau = 100, 1000, 0.05
    sg = np.array([0.2, 1.5])
    u = hn.response(None, [hn.identity(3, sigma=list(sg), tau=tau)], None, SEED, np.arange(S), 0, T, DT)
    rho = np.exp(-DT / tau); N = S * T
    se_var = np.sqrt(2.0 * (1.0 + rho ** 2) / ((1.0 - rho ** 2) * N)); se_r = np.sqrt((1.0 - rho ** 2) / N)
    for c in range(2):
        x = u[..., c] / sg[c]
        var = float(np.mean(x * x)); r1 = float(np.mean(x[1:] * x[:-1]) / np.mean(x * x))
        print(f"component {c}: variance {var:.5f} (1 +- {3 * se_var:.5f}), lag-1 correlation {r1:.5f} ({rho:.5f} +- {3 * se_r:.5f}), mean {np.mean(x):+.4f}")
        assert abs(var - 1.0) <= 3 * se_var and abs(r1 - rho) <= 3 * se_r
    z = hn.normals(SEED, np.arange(7), 3, 20)
    white = hn.response(None, [hn.identity(3, sigma=[0.2, 0.0])], None, SEED, np.arange(7), 3, 20, DT)
    assert np.array_equal(white[..., 0], 0.2 * z[..., 0]) and np.array_equal(bits(white[..., 1]), bits(np.zeros((20, 7))))
    # the state advances while a decision is held and outside the window
    held = hn.response(None, [hn.identity(3, sigma=list(sg), tau=tau, hold_steps=4, step_on=2)], None, SEED, np.arange(S), 0, 12, DT)
    assert np.all(held[:2] == 0.0) and np.array_equal(held[2], u[2]) and np.array_equal(held[5], u[2]) and np.array_equal(held[6], u[6]) and np.array_equal(held[10], u[10])


def test_block_three_is_apart_from_the_blocks_taken():
    streams = np.array([0, 1, 69, 2 ** 40 + 3], dtype=np.uint64)
    b0, b1 = sensor_numpy.words(SEED, streams, 5, 12)
    b2 = disturbance_numpy.block2_words(SEED, streams, 5, 12)
    b3 = hn.block3_words(SEED, streams, 5, 12)
    for other in (b0, b1, b2):
        assert b3.shape == other.shape and not np.any(b3 == other)
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint64)
    assert np.array_equal(sensor_numpy.philox4x32_10(np.array([5, 3, 69, 0], dtype=np.uint64), key), b3[0, 2])
    # the AR helper is the gust's, fed block 3 -- and the gust's own draws are what they were afterwards
    n = hn.ar_states([hn.identity(3, tau=0.3)], None, SEED, streams, 5, 12, DT)
    z = hn.normals(SEED, streams, 5, 12)
    assert np.array_equal(n[0], z[0]) and np.array_equal(n[1], np.exp(-DT / 0.3) * z[0] + np.sqrt(-np.expm1(-2 * DT / 0.3)) * z[1])
    zg = disturbance_numpy.normals(SEED, streams, 5, 12)
    assert not np.any(zg == z) and np.array_equal(disturbance_numpy.gust_states([disturbance_numpy.identity()], None, SEED, streams, 5, 12, DT), zg)


def test_structure_layout_equals_the_headers(pkg, tmp_path):
    """sizeof / offsetof of pg_human as the C compiler lays out include/pigeon_mpc.h, against the ctypes mirror"""
    from pigeon_jl_amd import _lib
    assert C.sizeof(_lib.pg_human) == 80
    src = tmp_path / "layout.c"
    fields = [n for n, _ in _lib.pg_human._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pigeon_mpc.h"\nint main(void) { printf("%zu", sizeof(pg_human));\n'
                   + "".join(f'printf(" %zu", offsetof(pg_human, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.pg_human)] + [getattr(_lib.pg_human, f).offset for f in fields]
    assert got == [80, 0, 4, 8, 12, 16, 32, 40, 48, 56, 72] and tuple(fields) == hn.FIELDS == pkg.vehicles.HUMAN_FIELDS


def test_names_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    julia = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint " + name + r"\(pg_handle\*", header), name
        assert name in pkg.SYMBOLS and ":" + name in julia and name in integration, name
    assert '"stat_human_steps"' in header and "IDENTITY" in header
    from pigeon_jl_amd import _lib
    assert sorted(_lib.HUMAN_SET_PROTOTYPES) == sorted(NEW_NAMES)
    for lib_name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib_name)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW_NAMES) <= exported, sorted(set(NEW_NAMES) - exported)
    M = pkg.BatchedTrajectoryTrackingMPC
    for meth in ("set_humans", "set_human_index", "set_human_seed", "clear_humans", "humans", "human_response", "human_state"):
        assert callable(getattr(M, meth)), meth


def test_vehicles_human_overrides_and_refusals(pkg):
    from pigeon_jl_amd import _lib
    M = pkg.BatchedTrajectoryTrackingMPC
    assert pkg.human() == hn.identity(0) and pkg.vehicles.human is pkg.human
    for m, name in enumerate(("hold", "worst", "script", "random")):
        assert pkg.human(mode=name) == hn.identity(m) == pkg.human(mode=m)
    h = pkg.human(mode="worst", hold_steps=30, gain=0.6, step_on=40, sigma=(0.1, 0.2))
    assert (h["mode"], h["hold_steps"], h["gain"], h["step_on"], h["sigma"], h["omega_max"]) == (1, 30, [0.6, 0.6], 40, [0.1, 0.2], np.inf)
    with pytest.raises(KeyError):
        pkg.human(sigma_w=1.0)
    with pytest.raises(KeyError):
        pkg.human(mode="aggressive")
    with pytest.raises(ValueError):
        pkg.human(gain=[1.0, 1.0, 1.0])
    arr = M.pack_humans(hn.four_humans() + [{"mode": "random", "tau": 0.3}])
    assert len(arr) == 5 and isinstance(arr[0], _lib.pg_human)
    assert (arr[0].mode, arr[0].hold_steps, arr[0].step_on, arr[0].step_off, list(arr[0].gain), arr[0].omega_max, arr[0].a_min, arr[0].a_max) == (0, 1, 0, -1, [1.0, 1.0], np.inf, -np.inf, np.inf)
    assert (arr[1].mode, arr[1].hold_steps, arr[1].step_on, arr[1].step_off, list(arr[1].gain), arr[1].omega_max) == (1, 3, 2, 11, [0.5, 0.5], 0.15)
    assert (arr[3].mode, list(arr[3].sigma), arr[3].tau) == (3, [0.2, 1.5], 0.05) and (arr[4].mode, arr[4].tau, list(arr[4].sigma)) == (3, 0.3, [0.0, 0.0])
    with pytest.raises(ValueError):
        M.pack_humans([pkg.human(hold_steps=2.5)])
    assert bytes(M.pack_humans([arr[1]])[0]) == bytes(arr[1])
