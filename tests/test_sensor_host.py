"""CPU tests of the sensor library (pg_set_sensor_sets): the numpy twin of the draws reproduces the known-answer vectors of Philox4x32-10 and the block / word assignment
the header states, the Box-Muller construction has the moments of a standard normal within four standard errors and respects the stated truncation, the new names are
declared, exported and mirrored with the right signatures, and the ctypes structure matches the ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sensor_numpy
from conftest import ROOT

NEW_NAMES = ["pg_set_sensor_sets", "pg_set_sensor_index", "pg_set_sensor_seed", "pg_clear_sensor_sets", "pg_get_sensor_sets", "pg_sensor_draws", "pg_get_measured_state",
             "pg_set_measured_history_dev"]

# counter | key -> output (the Random123 known-answer vectors of philox4x32_10)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def scalar_philox(ctr, key):
    """the ten rounds stated with Python integers, one counter at a time: the twin's vectorised uint64 form must agree with it"""
    c = list(ctr); k = list(key)
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]; p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert scalar_philox(ctr, key) == list(want)
    got = sensor_numpy.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(x) for x in got] == list(want)


def test_vectorised_philox_equals_the_scalar_statement():
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(50, 4), dtype=np.uint64); key = rng.integers(0, 2 ** 32, size=(50, 2), dtype=np.uint64)
    got = sensor_numpy.philox4x32_10(ctr, key)
    for i in range(50):
        assert [int(x) for x in got[i]] == scalar_philox([int(x) for x in ctr[i]], [int(x) for x in key[i]]), i


def test_block_and_word_assignment_spelled_out_by_hand():
    import math
    seed = 0x0123456789ABCDEF
    for stream, step in ((5, 0), (2 ** 32 + 17, 3), (0xFEDCBA9876543210, 1001)):
        z = sensor_numpy.draws(seed, [stream], step, 1)[0, 0]
        key = (seed & 0xFFFFFFFF, seed >> 32)
        b0 = scalar_philox((step, 0, stream & 0xFFFFFFFF, stream >> 32), key)
        b1 = scalar_philox((step, 1, stream & 0xFFFFFFFF, stream >> 32), key)

        def bm(xa, xb):
            u1 = ((xa >> 8) + 0.5) * 2.0 ** -24; u2 = ((xb >> 8) + 0.5) * 2.0 ** -24
            rho = math.sqrt(-2.0 * math.log(u1))
            return rho * math.cos(2.0 * math.pi * u2), rho * math.sin(2.0 * math.pi * u2)
        want = bm(b0[0], b0[1]) + bm(b0[2], b0[3]) + bm(b1[0], b1[1])
        assert np.allclose(z, want, rtol=0, atol=1e-14), (stream, step, z, want)
    # a draw belongs to its stream, not to its position: the same ids in another order and another batch size
    a = sensor_numpy.draws(seed, [9, 2 ** 40 + 1, 3], 10, 4)
    b = sensor_numpy.draws(seed, [3, 9], 10, 4)
    assert np.array_equal(a[:, 0], b[:, 1]) and np.array_equal(a[:, 2], b[:, 0])
    # ... a split sequence continues, another seed is another realisation
    assert np.array_equal(sensor_numpy.draws(seed, [9, 3], 12, 2), sensor_numpy.draws(seed, [9, 3], 10, 4)[2:])
    assert not np.array_equal(sensor_numpy.draws(seed + 1, [9, 3], 10, 4), sensor_numpy.draws(seed, [9, 3], 10, 4))


def test_moments_and_truncation():
    """64 steps x 1024 streams x 6 = 393,216 draws on the Philox words: |mean| < 4 / sqrt(n), |std - 1| < 4 / sqrt(2 n), max |z| <= sqrt(-2 ln 2^-25)"""
    z = sensor_numpy.draws(0xA5A5A5A55A5A5A5A, np.arange(1024, dtype=np.uint64) + np.uint64(2 ** 33), 0, 64)
    n = z.size
    assert n == 393216
    mean, std, zmax = float(z.mean()), float(z.std()), float(np.abs(z).max())
    print(f"n = {n}: mean {mean:+.5f} (bar {4 / np.sqrt(n):.4f}), std {std:.5f} (bar 1 +- {4 / np.sqrt(2 * n):.4f}), max |z| {zmax:.3f} (bound {sensor_numpy.Z_MAX:.3f})")
    assert abs(mean) < 4 / np.sqrt(n) and abs(std - 1.0) < 4 / np.sqrt(2 * n)
    assert zmax <= 5.887 and sensor_numpy.Z_MAX < 5.8871
    per = z.reshape(-1, 6)
    assert np.all(np.abs(per.mean(axis=0)) < 4 / np.sqrt(n / 6)) and np.all(np.abs(per.std(axis=0) - 1.0) < 4 / np.sqrt(2 * n / 6))      # every channel by itself
    c = np.corrcoef(per.T)
    assert np.max(np.abs(c - np.eye(6))) < 4 / np.sqrt(n / 6)                                                                            # ... and no pair correlated
    # the extreme words: u1 = 2^-25 gives the bound, not an infinity
    a, b = sensor_numpy.box_muller(np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF]))
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and abs(np.hypot(a[0], b[0]) - sensor_numpy.Z_MAX) < 1e-12


def test_names_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint " + name + r"\(pg_handle\*", header), name
        assert name in pkg.SYMBOLS
    assert "typedef struct pg_sensor { double sigma[6]; double bias[6]; } pg_sensor;" in header
    assert '"stat_sensor_steps"' in header
    from pigeon_jl_amd import _lib
    assert sorted(_lib.SENSOR_SET_PROTOTYPES) == sorted(NEW_NAMES)
    assert C.sizeof(_lib.pg_sensor) == 96
    for lib_name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib_name)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW_NAMES) <= exported, sorted(set(NEW_NAMES) - exported)
    # the mirror: every call of the issue's list exists, and the rollouts take the keyword
    import inspect
    M = pkg.BatchedTrajectoryTrackingMPC
    for meth in ("set_sensors", "clear_sensors", "sensors", "sensor_draws", "measured_state"):
        assert callable(getattr(M, meth)), meth
    assert list(inspect.signature(M.set_sensors).parameters)[1:] == ["sets", "index", "seed", "streams"]
    for meth in ("simulate_", "simulate_safety_", "simulate_node_"):
        assert inspect.signature(getattr(M, meth)).parameters["measured"].default is False, meth


def test_packing_sensors(pkg):
    from pigeon_jl_amd import _lib
    M = pkg.BatchedTrajectoryTrackingMPC
    sets = sensor_numpy.four_sensors()
    arr = M.pack_sensors(M, sets + [{"sigma": {"Ux": 0.1}, "bias": {"E": 0.2, "r": -0.01}}, {"bias": [1, 2, 3, 4, 5, 6]}])
    assert len(arr) == 6
    for k, (sg, bs) in enumerate(sets):
        assert list(arr[k].sigma) == list(sg) and list(arr[k].bias) == list(bs)
    assert list(arr[4].sigma) == [0, 0, 0, 0.1, 0, 0] and list(arr[4].bias) == [0.2, 0, 0, 0, 0, -0.01]
    assert list(arr[5].sigma) == [0] * 6 and list(arr[5].bias) == [1, 2, 3, 4, 5, 6]
    again = M.pack_sensors(M, [arr[4]])
    assert bytes(again[0]) == bytes(arr[4]) and isinstance(again[0], _lib.pg_sensor)


def test_numpy_measured_state():
    sets = sensor_numpy.four_sensors()
    idx = np.arange(8) % 4
    true = np.arange(2 * 8 * 6, dtype=np.float64).reshape(2, 8, 6)
    z = sensor_numpy.draws(3, np.arange(8), 0, 2)
    m = sensor_numpy.measured(sets, idx, true, z)
    assert np.array_equal(m[:, idx == 0], true[:, idx == 0])
    assert np.allclose(m[:, idx == 2] - true[:, idx == 2], np.broadcast_to(sets[2][1], (2, 2, 6)), rtol=0, atol=1e-12)
    assert np.allclose((m[:, idx == 3] - true[:, idx == 3]) / (3 * sets[1][0]), z[:, idx == 3], rtol=0, atol=1e-9)
