"""The case the path-refine tests share (tests/test_gpu_path_refine.py, tests/test_path_refine_host.py): three sources x five refine sets in one call, Lmax = 258,
Lmax_out = 900, and the twin's result over it, computed once.  The sources are made by the existing twin (path_make_numpy), so no device is needed.

  0  an open path of line (40 m), arc (30 m, 0.05 1/m) and clothoid (58.5 m, 0.05 -> -0.02 1/m), 258 knots exactly 0.5 m apart from the pose (3, -2, 0.4): 257 intervals,
     so the blocked scan runs with c = 2 and crosses a block boundary.  Its speed is not constant: V = 6 + 2 sin(s / 20), with t and A by the Result rule of
     pg_plan_speeds, and its edges vary along the clothoid
  1  oval_segments(40, 14.5, 15), closed, 65 knots (3.14 m apart)
  2  a line of 64 m with 2 knots: the smallest path

  0  the identity
  1  ds = 0.25 alone: source 0 is cut in 2 everywhere (515 knots: a thread owns up to three), the oval in 13 (833), the line in 256 -- L_out = 257, one knot past a
     workgroup's threads
  2  one window (10.1, 10.4, 0.1) inside a single interval of every source: [10, 10.5] of source 0, [9.4, 12.6] of the oval, the line's only one
  3  two overlapping windows of different spacing, (20, 30, 0.2) and (25, 40, 0.125): the smaller spacing holds where both reach
  4  a window beyond every path's end, (500, 600, 0.1): the identity's output"""
import functools
import math

import numpy as np

import path_make_numpy as make_twin
import path_refine_numpy as twin

LMAX, LMAX_OUT = 258, 900
N_KNOTS = [258, 65, 2]
CLOSED = [0, 1, 0]
N_PATH, N_SETS = 3, 5


def sets():
    S = twin.refine_set
    return [S(), S(ds=0.25), S(windows=[(10.1, 10.4, 0.1)]), S(windows=[(20.0, 30.0, 0.2), (25.0, 40.0, 0.125)]), S(windows=[(500.0, 600.0, 0.1)])]


def with_speed(r, V):
    """the made path r with the speed V [L] at its knots: A and t by the Result rule of pg_plan_speeds, t serial from t_0 = 0"""
    s = r["s"]; L = len(s)
    A = np.zeros(L); t = np.zeros(L)
    for i in range(L - 1):
        ds = float(s[i + 1]) - float(s[i])
        A[i] = ((V[i + 1] * V[i + 1]) - (V[i] * V[i])) / (2.0 * ds)
        t[i + 1] = t[i] + (2.0 * ds) / (V[i] + V[i + 1])
    out = dict(r); out.update(V=np.array(V, dtype=np.float64), A=A, t=t)
    return out


@functools.lru_cache(maxsize=None)
def _sources():
    from conftest import load_pkg
    pkg = load_pkg()
    seg = make_twin.segment
    a = make_twin.make([seg(length=40.0), seg(length=30.0, kappa0=0.05, kappa1=0.05), seg(length=58.5, kappa0=0.05, kappa1=-0.02, edge_L1=5.0, edge_R1=-3.0)], 258, (3.0, -2.0, 0.4), 6.0)
    assert np.all(a["s"] == 0.5 * np.arange(258))
    a = with_speed(a, 6.0 + 2.0 * np.sin(a["s"] / 20.0))
    ch = np.zeros((N_PATH, 10, LMAX))
    ch[0] = make_twin.channels(a, LMAX)
    ch[1] = make_twin.channels(make_twin.make(pkg.vehicles.oval_segments(40.0, 14.5, 15.0), 65, (12.0, -30.0, 0.5), 6.0), LMAX)
    ch[2] = make_twin.channels(make_twin.make([seg(length=64.0)], 2, (0.0, 0.0, 0.0), 8.0), LMAX)
    ch.setflags(write=False)
    return ch


def sources():
    """channels_in [3][10][LMAX] float64 (0 at and past L); computed once, shared, never modified"""
    return _sources()


@functools.lru_cache(maxsize=None)
def _reference():
    ch = sources()
    return [[twin.refine(ch[p][:, :N_KNOTS[p]], S) for S in sets()] for p in range(N_PATH)]


def reference():
    """the twin's results [path][set]; computed once, shared, never modified"""
    return _reference()


def expected_channels():
    """[15][10][LMAX_OUT] float64 of the twin, k = path * N_SETS + set"""
    return np.stack([twin.channels(r, LMAX_OUT) for row in reference() for r in row])


def fill_set(rec, S):
    rec.ds = S["ds"]
    for j in range(4):
        rec.s_lo[j], rec.s_hi[j], rec.ds_w[j] = S["windows"][j]
    for j in range(3):
        rec.reserved[j] = S["reserved"][j]


def packed(which_paths=range(N_PATH), which_sets=range(N_SETS), Lmax=LMAX):
    """(L int32, closed int32, channels_in float64 [n][10][Lmax], sets: a ctypes array of pg_refine_set) of the call over the chosen paths and sets; Lmax may be larger
    than LMAX (zeros past it)"""
    Lc = __import__("sys").modules["pigeon_jl_amd"]._lib
    which_paths, which_sets = list(which_paths), list(which_sets)
    L = np.array([N_KNOTS[p] for p in which_paths], dtype=np.int32)
    cl = np.array([CLOSED[p] for p in which_paths], dtype=np.int32)
    ch = np.zeros((len(which_paths), 10, Lmax))
    w = min(Lmax, LMAX)
    ch[:, :, :w] = sources()[which_paths][:, :, :w]
    all_sets = sets()
    arr = (Lc.pg_refine_set * len(which_sets))()
    for j, q in enumerate(which_sets):
        fill_set(arr[j], all_sets[q])
    return L, cl, ch, arr


# ---- the two failures the knot-wise makers document, on the line of tests/path_offset_cases.py: 40 knots 10 m apart ----
def documented_line():
    import path_offset_cases
    return np.array(path_offset_cases.sources()[0][:, :40])


def as_twin_set(rset):
    """a vehicles.refine(...) dict as the twin's set"""
    return twin.refine_set(ds=rset["ds"], windows=rset["windows"])


def trapezoid_length(d1, a, b, total):
    """the length of lane_change(0, d1, a, b) on a straight line of `total` m: a fine trapezoid of sqrt(1 + d'^2) over the window (as tests/test_path_offset_host.py)"""
    u = np.linspace(a, b, 200001)
    tau = (u - a) / (b - a)
    g = np.sqrt(1.0 + (d1 * (30.0 * tau ** 2 * (1.0 - tau) ** 2) / (b - a)) ** 2)
    return total + float(np.sum(0.5 * (g[1:] + g[:-1]) * np.diff(u))) - (b - a)
