"""The case the path-offset tests share (tests/test_gpu_path_offset.py, tests/test_path_offset_host.py): six sources x seven offset sets in one call, Lmax = 300, and the
twin's result over it, computed once.  The sources are made by the existing twins (path_make_numpy) or read from the committed fixture, so no device is needed.

  0  a straight line of 390 m, 40 knots 10 m apart, from the pose (3, -2, 0.4) -- the only source longer than the closed ones, see below
  1  a counter-clockwise circle of R = 20 m, closed, 64 knots
  2  the same circle clockwise
  3  oval_segments(40, 14.5, 15), closed, 259 knots: 258 intervals, so the blocked prefix runs with c = 2 and its last block is short
  4  the recorded variable_speed fixture: 28 knots, non-constant V, non-uniform spacing
  5  a line of 2 knots: the smallest call (both knots one-sided)

  0  the identity
  1  lane(+3.5)        2  lane(-3.5)
  3  lane_change(0, 1.5, 212, 217): both window ends inside ONE knot interval of the line (210 .. 220 m): only the quadrature sees it
  4  lane_change(0, 5, 230, 330): a window over ten knots; d1 = 5 m takes the line past its own left edge (n_outside)
  5  pass_by(3, 20, 35, 45, 60): on the oval the plateau and the fall lie on the clothoid into the first bend (40 .. 55 m); on the circles on the arc
  6  lane(2, edge_mode=1)

Every pair of one call must be one the scheme accepts, and a closed path refuses a lane change inside its own length (the offset curve would not close).  So the two lane
changes start past the longest closed source (the oval, 201 m) and act on the line alone -- the other sources keep d0 there, which is part of the contract --, while the
pass-by returns to d0 and acts on every source.  The pairs the scheme must refuse (a window across a closed path's seam, lane(+15) on the oval's 14.5 m bends) are in the
refusal test."""
import functools
import math

import numpy as np

import path_make_numpy as make_twin
import path_offset_numpy as twin

LMAX = 300
N_KNOTS = [40, 64, 64, 259, 28, 2]
CLOSED = [0, 1, 1, 1, 0, 0]
N_PATH, N_SETS = 6, 7
CIRCLE_R = 20.0
_CH_ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]


def sets():
    S = twin.offset_set
    return [S(), S(d0=3.5, d1=3.5), S(d0=-3.5, d1=-3.5), S(d0=0.0, d1=1.5, s_a=212.0, s_b=217.0), S(d0=0.0, d1=5.0, s_a=230.0, s_b=330.0),
            S(d0=0.0, d1=3.0, s_a=20.0, s_b=35.0, s_c=45.0, s_d=60.0), S(d0=2.0, d1=2.0, edge_mode=1)]


@functools.lru_cache(maxsize=None)
def _sources():
    from conftest import load_pkg
    pkg = load_pkg()
    seg = make_twin.segment
    k = 1.0 / CIRCLE_R
    turn = 2.0 * math.pi * CIRCLE_R
    made = [make_twin.make([seg(length=390.0)], 40, (3.0, -2.0, 0.4), 6.0),
            make_twin.make([seg(length=turn, kappa0=k, kappa1=k)], 64, (10.0, 5.0, 0.3), 6.0),
            make_twin.make([seg(length=turn, kappa0=-k, kappa1=-k)], 64, (10.0, 5.0, 0.3), 7.5),
            make_twin.make(pkg.vehicles.oval_segments(40.0, 14.5, 15.0), 259, (12.0, -30.0, 0.5), 6.0)]
    ch = np.zeros((N_PATH, 10, LMAX))
    for p, r in enumerate(made):
        ch[p] = make_twin.channels(r, LMAX)
    vs = pkg.load_path_fixture("variable_speed")
    assert len(vs) == 28 and np.ptp(vs.V) > 0
    ch[4, :, :28] = vs.data[_CH_ROWS]
    ch[5] = make_twin.channels(make_twin.make([seg(length=10.0)], 2, (0.0, 0.0, 0.0), 6.0), LMAX)
    ch.setflags(write=False)
    return ch


def sources():
    """channels_in [6][10][LMAX] float64 (0 at and past L); computed once, shared, never modified"""
    return _sources()


@functools.lru_cache(maxsize=None)
def _reference():
    ch = sources()
    return [[twin.offset(ch[p][:, :N_KNOTS[p]], S, bool(CLOSED[p])) for S in sets()] for p in range(N_PATH)]


def reference():
    """the twin's results [path][set]; computed once, shared, never modified"""
    return _reference()


def expected_channels():
    """[42][10][LMAX] float64 of the twin, k = path * N_SETS + set"""
    return np.stack([twin.channels(r, LMAX) for row in reference() for r in row])


def packed(which_paths=range(N_PATH), which_sets=range(N_SETS), Lmax=LMAX):
    """(L int32, closed int32, channels_in float64 [n][10][Lmax], sets: a ctypes array of pg_offset_set) of the call over the chosen paths and sets"""
    Lc = __import__("sys").modules["pigeon_jl_amd"]._lib
    which_paths, which_sets = list(which_paths), list(which_sets)
    L = np.array([N_KNOTS[p] for p in which_paths], dtype=np.int32)
    cl = np.array([CLOSED[p] for p in which_paths], dtype=np.int32)
    ch = np.ascontiguousarray(sources()[which_paths][:, :, :Lmax])
    all_sets = sets()
    arr = (Lc.pg_offset_set * len(which_sets))()
    for j, q in enumerate(which_sets):
        for name, _ in Lc.pg_offset_set._fields_:
            setattr(arr[j], name, all_sets[q][name])
    return L, cl, ch, arr
