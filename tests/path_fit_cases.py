"""The waypoint library the path-fit tests share (tests/test_gpu_path_fit.py, tests/test_path_fit_host.py), one call with Lmax = 520, and the twin's result over it, computed
once.  Six paths; path 1 is fitted at two knot counts from ONE range of waypoints, so the call has seven entries:

  0  open, 2 waypoints, 2 knots: the minimum (no row of the tridiagonal system; a straight line)
  1  closed, 3 waypoints (a triangle), 3 knots and 40 knots: the cyclic system whose every off-diagonal place is taken
  2  closed counter-clockwise circle of R = 7 around (20, -30), 24 waypoints from the angle pi - 0.05 on, 300 knots: psi_raw crosses +pi between knots 2 and 3 (the unwrap),
     and a thread of the knot pass holds more than one knot
  3  the same circle clockwise, 64 knots: negative kappa, turn = -2 pi
  4  open S-curve N = 3 sin(E / 6), 300 waypoints 0.2 m apart in E, 37 knots: many spans without a knot; c = 2 in the span prefix (299 spans)
  5  open, 9 waypoints with the chords 0.3, 9, 1.2, 4, 0.5, 7, 2.5, 0.8 m, 513 knots: many knots per span; three knots per thread in the store passes, c = 3 in the prefix of the jumps"""
import functools
import math

import numpy as np

import path_fit_numpy as twin

LMAX = 520
N_ENTRIES = 7
PATH_OF = [0, 1, 1, 2, 3, 4, 5]                                     # the path of an entry
N_KNOTS = [2, 3, 40, 300, 64, 37, 513]
V_REFS = [6.0, 3.0, 3.0, 6.0, 7.5, 4.0, 5.0]
CLOSED = [0, 1, 1, 1, 1, 0, 0]
CIRCLE_R, CIRCLE_C, CIRCLE_TH0 = 7.0, (20.0, -30.0), math.pi - 0.05
UNEVEN_CHORDS = (0.3, 9.0, 1.2, 4.0, 0.5, 7.0, 2.5, 0.8)


def circle(n, sign, R=CIRCLE_R, centre=CIRCLE_C, th0=CIRCLE_TH0, **edges):
    """n waypoints on a circle from the angle th0 on, counter-clockwise in the (E, N) plane for sign = +1 -- a left turn under dE/ds = -sin psi, dN/ds = cos psi"""
    return [twin.waypoint(E=centre[0] + R * math.cos(th0 + sign * 2.0 * math.pi * k / n), N=centre[1] + R * math.sin(th0 + sign * 2.0 * math.pi * k / n), **edges) for k in range(n)]


def uneven():
    E, N, head = [2.0], [-1.0], 0.3
    for k, c in enumerate(UNEVEN_CHORDS):
        head += (0.25, -0.1, 0.3, 0.2, -0.35, 0.15, 0.3, -0.2)[k]
        E.append(E[-1] - c * math.sin(head)); N.append(N[-1] + c * math.cos(head))
    return [twin.waypoint(E=e, N=n, edge_L=3.0 + 0.25 * k, edge_R=-2.0 - 0.5 * (k % 3)) for k, (e, n) in enumerate(zip(E, N))]


def paths():
    """the six waypoint lists"""
    return [[twin.waypoint(E=0.0, N=0.0), twin.waypoint(E=3.0, N=4.0, edge_L=5.0, edge_R=-1.0)],
            [twin.waypoint(E=0.0, N=0.0), twin.waypoint(E=10.0, N=0.0, edge_L=3.0), twin.waypoint(E=4.0, N=8.0, edge_R=-2.0)],
            circle(24, +1, edge_L=3.0, edge_R=-2.0),
            circle(24, -1),
            [twin.waypoint(E=0.2 * k, N=3.0 * math.sin(0.2 * k / 6.0), edge_L=4.0 + 0.001 * k) for k in range(300)],
            uneven()]


def entries():
    """the seven entries as fit_paths takes them"""
    p = paths()
    return [dict(waypoints=p[PATH_OF[e]], n_knots=N_KNOTS[e], V_ref=V_REFS[e], closed=bool(CLOSED[e])) for e in range(N_ENTRIES)]


def packed(mpc_class, which=range(N_ENTRIES), Lmax=LMAX):
    """(specs, waypoints) of the call, path 1 stored ONCE: the entries 1 and 2 refer to the same range of waypoints"""
    L = __import__("sys").modules["pigeon_jl_amd"]._lib
    p = paths()
    which = list(which)
    used = sorted({PATH_OF[e] for e in which})
    start, flat = {}, []
    for k in used:
        start[k] = len(flat); flat += p[k]
    wps = (L.pg_waypoint * len(flat))()
    for i, w in enumerate(flat):
        wps[i].E, wps[i].N, wps[i].edge_L, wps[i].edge_R = w["E"], w["N"], w["edge_L"], w["edge_R"]
    specs = (L.pg_fit_spec * len(which))()
    for i, e in enumerate(which):
        k = PATH_OF[e]
        specs[i].V_ref, specs[i].wp0, specs[i].n_wp, specs[i].n_knots, specs[i].closed = V_REFS[e], start[k], len(p[k]), N_KNOTS[e], CLOSED[e]
    return specs, wps


@functools.lru_cache(maxsize=None)
def _reference():
    ref = [twin.fit(e["waypoints"], e["n_knots"], e["V_ref"], e["closed"]) for e in entries()]
    for e, r in enumerate(ref):
        # no two neighbouring raw headings differ by within 1e-9 of +-pi: a last-bit difference of atan2 cannot flip a jump of the unwrap
        d = np.abs(np.diff(r["psi_raw"]))
        assert d.size == 0 or np.min(np.abs(d - math.pi)) > 1e-9, e
    return ref


def reference():
    """the twin's results of the seven entries; computed once, shared, never modified"""
    return _reference()


def expected_channels():
    """[7][10][LMAX] float64 of the twin"""
    return np.stack([twin.channels(r, LMAX) for r in reference()])


def psi_bar(psi):
    """8 * 2^-52 * max(pi, |psi|): two ulp of the device's atan2 (the OpenCL bound), one of libm's, and the rounding of the offset add"""
    return 8.0 * 2.0 ** -52 * np.maximum(math.pi, np.abs(psi))
