"""The shared case of the pg_smooth_waypoints tests (host twin and device): PATHS x SETS, the smallest shapes at which each code path can go wrong.

Paths (name, closed, waypoints), coordinates rounded to a centimetre as a survey's are, unequal chords throughout:
  open  2 (no row: a copy), 3 (one row), 4, 5 waypoints;  closed 5 (the smallest: band and border just apart), 6, 7;
  257 and 300 waypoints, open and closed: past one stride of 256 threads, blocked prefix and blocked sums with c = 2;
  1100 open and 1030 closed: more rows than the 1024 the kernel keeps in LDS, so the recurrence's state is in the call's scratch;
  skidpadoval (999, closed: the file's repeated last knot dropped) and vail (1000, open) from tests/golden/paths/.
Sets: the identity; lambda = 0.1; lambda = 10 with pin_ends; lambda = 1 with a window of factor 0 and an overlapping, later one of factor 4; lambda = 0.5 with keep_walls.
The twin's results are computed once (reference()) and shared."""
import functools
import math
import os

import numpy as np

import wp_smooth_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = (0.0, 1e-3, 1e-2, 1e-1, 1.0, 10.0)      # the lambda ladder of the oval's table (EXPERIMENTS 41)

SETS = [twin.smooth_set(), twin.smooth_set(lam=0.1), twin.smooth_set(lam=10.0, pin_ends=True),
        twin.smooth_set(lam=1.0, windows=[(2.0, 6.0, 0.0), (5.0, 40.0, 4.0)]), twin.smooth_set(lam=0.5, keep_walls=True)]


def wp(E, N, eL=4.0, eR=-4.0):
    return dict(E=float(E), N=float(N), edge_L=float(eL), edge_R=float(eR))


def golden(name, closed):
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", name + ".npz")))
    n = len(d["posE_m"]) - 1 if closed else len(d["posE_m"])
    return [wp(d["posE_m"][i], d["posN_m"][i], d["edgeL_m"][i], d["edgeR_m"][i]) for i in range(n)]


def arc(n, closed, seed):
    """n waypoints on a circle of R = 30 m (the whole of it when closed, 240 degrees when open) at unequal steps, rounded to a centimetre, the edges varying"""
    rng = np.random.RandomState(seed)
    steps = 0.5 + rng.rand(n)
    th = np.cumsum(steps) / np.sum(steps) * (2.0 * math.pi if closed else 4.0 * math.pi / 3.0)
    return [wp(round(100.0 + 30.0 * math.cos(t), 2), round(-50.0 + 30.0 * math.sin(t), 2), round(3.0 + math.sin(3.0 * t), 2), round(-2.5 + 0.5 * math.cos(2.0 * t), 2)) for t in th]


@functools.lru_cache(maxsize=None)
def paths():
    small = [(0.0, 0.0), (3.0, 0.5), (5.0, 2.5), (9.5, 3.0), (12.0, 7.0)]
    poly = [(0.0, 0.0), (4.0, -1.0), (8.5, 1.5), (9.0, 6.0), (5.0, 9.5), (1.0, 8.0), (-2.0, 4.0)]
    out = [("open%d" % n, False, [wp(E, N, 3.0 + 0.25 * i, -2.0 - 0.5 * i) for i, (E, N) in enumerate(small[:n])]) for n in (2, 3, 4, 5)]
    out += [("closed%d" % n, True, [wp(E, N) for E, N in poly[:n]]) for n in (5, 6, 7)]
    out += [("open257", False, arc(257, False, 1)), ("open300", False, arc(300, False, 2)), ("closed257", True, arc(257, True, 3)), ("closed300", True, arc(300, True, 4))]
    out += [("open1100", False, arc(1100, False, 5)), ("closed1030", True, arc(1030, True, 6))]
    out += [("skidpadoval", True, golden("skidpadoval", True)), ("vail", False, golden("vail", False))]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference():
    """ref[path][set]: the twin's result of every pair"""
    return tuple(tuple(twin.smooth(w, closed, s) for s in SETS) for _, closed, w in paths())


def fit_paths_list():
    """the paths as mpc.smooth_waypoints takes them"""
    return [dict(waypoints=w, closed=closed) for _, closed, w in paths()]


def as_bits(r):
    """[n][4] float64: E, N, edge_L, edge_R of a twin result"""
    return np.stack([r["E"], r["N"], r["edge_L"], r["edge_R"]], axis=1)
