"""The path library the path-maker tests share (tests/test_gpu_path_make.py, tests/test_path_make_host.py), one call with Lmax = 300, and the twin's result over it, computed once.

  0  a line of 2 knots, one segment: the smallest call
  1  oval_segments(40, 14.5, 15), closed, 300 knots: 299 intervals -- past 256, no multiple of the workgroup or the wavefront; the curvature of skidpadoval
  2  seven segments, 40 knots over 20 m: three segments of 0.05 m inside ONE knot interval (the piece loop), and the first segment bound exactly on knot 10 (b_j <= s_i)
  3  a line into an arc of negative curvature with no clothoid, from the pose (-286, -161, 3.0), 65 knots: a curvature jump, a right turn, a large offset, one knot past a wavefront
  4  a 30 m clothoid from 0 to 0.2 1/m, 31 knots, the edges running 3 -> 5 and -2 -> -6"""
import functools
import math

import numpy as np

import path_make_numpy as twin

LMAX = 300
N_KNOTS = [2, 300, 40, 65, 31]
POSES = [(0.0, 0.0, 0.0), (12.0, -30.0, 0.5), (5.0, 6.0, -1.0), (-286.0, -161.0, 3.0), (0.0, 0.0, 0.0)]
V_REFS = [6.0, 6.0, 4.0, 7.5, 6.0]
CLOSED = [0, 1, 0, 0, 0]


def seven_segments(veh):
    """total exactly 20 m (ds = 20 / 39); b_1 = 10 ds = s_10 exactly; the segments 2, 3, 4 of 0.05 m lie inside the knot interval 16 (8.205 .. 8.718 m)"""
    ds = 20.0 / 39
    seg = veh.path_segment
    head = [seg(length=10 * ds), seg(length=3.1, kappa1=0.1), seg(length=0.05, kappa0=0.1, kappa1=0.1), seg(length=0.05, kappa0=0.1, kappa1=-0.05),
            seg(length=0.05, kappa0=-0.05, kappa1=-0.05), seg(length=5.0, kappa0=-0.05, kappa1=0.08)]
    b = 0.0
    for g in head:
        b = b + g["length"]
    last = 20.0 - b
    for _ in range(8):                                              # (the lengths are summed in floating point: take the neighbour at which the sum is 20 exactly)
        if b + last == 20.0:
            break
        last = math.nextafter(last, math.inf if b + last < 20.0 else 0.0)
    segs = head + [seg(length=last, kappa0=0.08, kappa1=0.08)]
    bb, _ = twin.bounds(segs, 0.0)
    assert bb[-1] == 20.0 and bb[1] == 10 * ds and 16 * ds < bb[2] and bb[5] < 17 * ds, bb
    return segs


def paths(veh):
    seg = veh.path_segment
    return [veh.line_segments(10.0),
            veh.oval_segments(40.0, 14.5, 15.0),
            seven_segments(veh),
            [seg(length=20.0), seg(length=25.0, kappa0=-0.08, kappa1=-0.08)],
            [seg(length=30.0, kappa1=0.2, edge_L0=3.0, edge_L1=5.0, edge_R0=-2.0, edge_R1=-6.0)]]


@functools.lru_cache(maxsize=None)
def _reference():
    from conftest import load_pkg
    pkg = load_pkg()
    p = paths(pkg.vehicles)
    ref = [twin.make(p[k], N_KNOTS[k], POSES[k], V_REFS[k]) for k in range(len(p))]
    return p, ref


def reference():
    """(paths: the five segment lists, the twin's results); computed once, shared, never modified"""
    return _reference()


def bar(k):
    """the bound on |E, N of the library - E, N of the twin| of path k: 4 (n_knots + 64) 2^-53 total -- n_knots roundings of the twin's serial sum at a magnitude of at most
    the path's length, the 64-odd of the library's blocked sum, and a few ulp of sin / cos per node"""
    _, ref = reference()
    return 4.0 * (N_KNOTS[k] + 64) * 2.0 ** -53 * ref[k]["stats"]["length"]


def expected_channels():
    """[5][10][LMAX] float64 of the twin"""
    _, ref = reference()
    return np.stack([twin.channels(r, LMAX) for r in ref])
