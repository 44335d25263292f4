"""The path library x plan-set grid the speed-plan tests share (tests/test_gpu_speed_plan.py, tests/test_speed_plan_host.py), and the twin's result over it, computed once.

Three paths, Lmax = 130: skidpadoval cut to its first 130 knots and declared open, the whole variable_speed (28 knots, non-uniform
ds), a synthetic closed path of 65 knots whose largest curvature is not at knot 0.  65 sets (one past a wavefront): mu_scale over 0.3-1.0, V_max over 5-25, one in eight
with V_start / V_end, one in eight with finite ax / ay caps, two with a second vehicle (mu = 0.6; heavier)."""
import functools
import math

import numpy as np

import speed_plan_numpy as twin

N_SETS, LMAX = 65, 130
ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]


def synthetic_closed(pkg, L=65):
    """a closed path of L knots (knot L-1 = knot 0): a circle of radius 20 m whose curvature channel is modulated, the largest |kappa| at knot 23; non-uniform spacing"""
    u = np.linspace(0.0, 1.0, L) ** 1.15
    th = 2 * np.pi * u
    s = 20.0 * th
    kappa = 0.05 * (1.0 + 0.6 * np.sin(th - 2 * np.pi * u[23] + np.pi / 2))
    kappa[-1] = kappa[0]
    V = np.full(L, 5.0)
    return pkg.TrajectoryTube(twin_t(V, s), s, V, 0 * s, 20 * np.sin(th), -20 * np.cos(th), th, kappa)


def twin_t(V, s):
    return np.concatenate([[0.0], np.cumsum(2 * np.diff(s) / (V[:-1] + V[1:]))])


def cut(pkg, t, n):
    d = t.data[:, :n]
    return pkg.TrajectoryTube(*[d[i] for i in range(12)])


def paths(pkg):
    p = [cut(pkg, pkg.load_path_fixture("skidpadoval"), 130), pkg.load_path_fixture("variable_speed"), synthetic_closed(pkg)]
    assert [len(t) for t in p] == [130, 28, 65] and int(np.argmax(np.abs(p[2].kappa[:-1]))) == 23
    return p, [0, 0, 1]


def sets_and_vehicles(pkg):
    X1 = pkg.vehicles.X1
    sets, vehs = [], []
    for j in range(N_SETS):
        kw = dict(mu_scale=0.3 + 0.7 * j / (N_SETS - 1), V_max=5.0 + 20.0 * ((j * 7) % N_SETS) / (N_SETS - 1))
        if j % 8 == 3:
            kw.update(V_start=2.0 + 0.1 * j, V_end=0.5 + 0.05 * j)
        if j % 8 == 5:
            kw.update(ax_max=1.5, ax_min=-2.5, ay_max=3.0)
        sets.append(pkg.vehicles.speed_plan(**kw))
        vehs.append(X1(mu=0.6) if j == 10 else X1(mfl=600.0, mfr=580.0, mrl=640.0, mrr=620.0) if j == 40 else X1())
    return sets, vehs


@functools.lru_cache(maxsize=None)
def _reference():
    from conftest import load_pkg
    pkg = load_pkg()
    p, closed = paths(pkg)
    sets, vehs = sets_and_vehicles(pkg)
    out = [[twin.plan(t.s, t.kappa, sp, v, closed=bool(c)) for sp, v in zip(sets, vehs)] for t, c in zip(p, closed)]
    return p, closed, sets, vehs, out


def reference():
    """(paths, closed, sets, vehicles, twin results [path][set]); computed once, shared, never modified"""
    return _reference()


def channels_of(tubes, Lmax):
    ch = np.zeros((len(tubes), 10, Lmax))
    for k, t in enumerate(tubes):
        ch[k, :, :len(t)] = t.data[ROWS]
    return ch
