"""The case the tube-clip tests share (tests/test_gpu_tube_clip.py, tests/test_tube_clip_host.py): the six sources of tests/path_offset_cases.py x thirteen obstacle sets in
one call, Lmax = 300, and the twin's result over it, computed once.  The sources' knot counts are 40, 64, 64, 259, 28 and 2: the 259 is the first to give a thread a
second knot, the 2-knot line is the smallest call, the circles have a seam.  The discs are placed with vehicles.obstacle_at, so they sit where the paths are; those on
the line (source 0) lie 120 m and more from its start, far from every other source, which ignore them (that is part of the contract: n_ignored).

The obstacle array (72 discs) and the sets, (first, count):
   0  the identity                                                          (0, 0)
   1  a disc 0.4 m left of the line's centre at 130 m that covers it, R = 1: n_centre_out; taper +Inf            (0, 1)
   2  the same disc, taper 0.25                                             (0, 1)
   3  a disc straddling the line's left edge at 140.3 m, taper 0.5          (1, 1)
   4  a disc wholly outside the tube at 160.2 m: seen by no knot            (2, 1)
   5  two discs at 180.1 m, 2.6 m left and right, R = 1.2: 2.8 m are left, min_width 3   (3, 2)
   6 .. 9  one disc at 250.2 m, 0.8 m right of the centre, margin 0.3, under the policies CENTRE, WIDER, LEFT, RIGHT     (5, 1)
  10  a disc about 1 m from knot 0 of the circles (1.0 m along the counter-clockwise one, 0.5 m to its left, R = 1.5) and one on the oval 199.5 m along it (knot 256 of
      its 258, 0.6 m to the right, R = 1.2: the second knots of the threads 0 and 1), taper 0.25: both tapers wrap the seam   (6, 2)
  11  a disc of R = 1.5 m on the line at 214 m, between the knots at 210 and 220 m: seen by neither   (8, 1)
  12  64 discs (the bound) along the line from 121.3 m on, every 4.07 m, alternately left and right, margin 0.1, taper 0.5; its range starts with the disc of set 11   (8, 64)

Every decision stays away from a floating-point tie: decision_margin() is the smallest |quantity| the twin compared with zero over all sight tests, side tests and the
best-versus-runner-up gap of every argmin (metres, or square metres for q); tests/test_tube_clip_host.py asserts it is >= 1e-6.  The disc of set 11 is at 214 m, not at
215 m, for that reason: at 215 m the knots at 210 and 220 m are equally far (the host test pins the 215 m disc on its own, through the twin)."""
import functools

import numpy as np

import path_offset_cases as offset_cases
import tube_clip_numpy as twin

LMAX = offset_cases.LMAX
N_KNOTS = offset_cases.N_KNOTS
CLOSED = offset_cases.CLOSED
N_PATH, N_SETS = 6, 13
N_OBS = 72


def sources():
    """channels_in [6][10][LMAX] float64, those of the path-offset case"""
    return offset_cases.sources()


@functools.lru_cache(maxsize=None)
def _obstacles():
    from conftest import load_pkg
    at = load_pkg().vehicles.obstacle_at
    ch = sources()
    line = ch[0][:, :N_KNOTS[0]]; circle = ch[1][:, :N_KNOTS[1]]; oval = ch[3][:, :N_KNOTS[3]]
    obs = [at(line, 130.0, 0.4, 1.0), at(line, 140.3, 4.2, 1.0), at(line, 160.2, 7.0, 1.0), at(line, 180.1, 2.6, 1.2), at(line, 180.1, -2.6, 1.2), at(line, 250.2, -0.8, 0.7),
           at(circle, 1.0, 0.5, 1.5), at(oval, 199.5, -0.6, 1.2), at(line, 214.0, 0.0, 1.5)]
    for j in range(63):
        obs.append(at(line, 121.3 + 4.07 * j, (3.2 + 0.013 * j) * (1.0 if j % 2 == 0 else -1.0), 0.5 + 0.003 * j))
    assert len(obs) == N_OBS
    out = np.array([[o["E"], o["N"], o["radius"]] for o in obs])
    out.setflags(write=False)
    return out


def obstacles():
    """[72][3] float64: E, N, radius; computed once, shared, never modified"""
    return _obstacles()


def sets():
    S = twin.obstacle_set
    return [S(), S(first=0, count=1), S(first=0, count=1, taper=0.25), S(first=1, count=1, taper=0.5), S(first=2, count=1), S(first=3, count=2, min_width=3.0, taper=1.0),
            S(first=5, count=1, margin=0.3, policy=twin.CENTRE), S(first=5, count=1, margin=0.3, policy=twin.WIDER), S(first=5, count=1, margin=0.3, policy=twin.LEFT),
            S(first=5, count=1, margin=0.3, policy=twin.RIGHT), S(first=6, count=2, taper=0.25), S(first=8, count=1), S(first=8, count=64, margin=0.1, taper=0.5)]


MAX_COUNT = 64


@functools.lru_cache(maxsize=None)
def _reference():
    ch = sources()
    return [[twin.clip(ch[p][:, :N_KNOTS[p]], S, obstacles(), bool(CLOSED[p])) for S in sets()] for p in range(N_PATH)]


def reference():
    """the twin's results [path][set]; computed once, shared, never modified"""
    return _reference()


def expected_channels():
    """[78][10][LMAX] float64 of the twin, k = path * N_SETS + set"""
    return np.stack([twin.channels(r, LMAX) for row in reference() for r in row])


def decision_margin():
    return min(r["margin"] for row in reference() for r in row)


def packed(which_paths=range(N_PATH), which_sets=range(N_SETS), Lmax=LMAX):
    """(L int32, closed int32, channels_in float64 [n][10][Lmax], sets: a ctypes array of pg_obstacle_set, obstacles: a ctypes array of the 72 pg_obstacle) of the call over
    the chosen paths and sets"""
    Lc = __import__("sys").modules["pigeon_jl_amd"]._lib
    which_paths, which_sets = list(which_paths), list(which_sets)
    L = np.array([N_KNOTS[p] for p in which_paths], dtype=np.int32)
    cl = np.array([CLOSED[p] for p in which_paths], dtype=np.int32)
    ch = np.ascontiguousarray(sources()[which_paths][:, :, :Lmax])
    all_sets = sets()
    arr = (Lc.pg_obstacle_set * len(which_sets))()
    for j, q in enumerate(which_sets):
        for name in ("first", "count", "margin", "taper", "min_width", "policy", "reserved"):
            setattr(arr[j], name, all_sets[q][name])
    obs = (Lc.pg_obstacle * N_OBS)()
    for j, (E, N, r) in enumerate(obstacles()):
        obs[j].E, obs[j].N, obs[j].radius = float(E), float(N), float(r)
    return L, cl, ch, arr, obs
