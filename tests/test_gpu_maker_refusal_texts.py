"""The refusals the five makers of a trajectory library word alike (pg_plan_speeds, pg_make_paths, pg_fit_paths, pg_offset_paths, pg_clip_tubes): the WHOLE text
pg_last_error returns for each, not its prefix only -- the other maker tests check the prefix.  The texts are those of csrc/pg_api.hip, word for word; which of two
defects of one input is reported is part of the contract too (the source paths are checked one after the other, each of them completely).

The smallest input that reaches each line: two paths of 3 knots, the first open and the second closed, Lmax = 4, one set that changes nothing.  Every call is refused
before anything is launched."""
import math

import numpy as np
import pytest

from path_libs import INVALID, c_dp, c_i32p, handle, lib

pytestmark = pytest.mark.gpu

LMAX = 4
BIG = 2**31 - 1
T, S, V, E = 0, 1, 2, 4                                              # rows of a trajectory [10][Lmax]: t, s, V, A, E, N, psi, kappa, edge_L, edge_R

NULL = "null argument"
NEED = "need n_path >= 1, n_sets >= 1 and Lmax >= 2"
BITS = "n_path * n_sets must fit 31 bits"
ALLOC = "n_path * n_sets * 10 * Lmax elements are more than the allocation arithmetic holds"
LENGTH = "every path needs 2 <= L[k] <= Lmax"
CLOSED = "a closed path needs >= 3 knots"
FINITE = "a geometry value of a valid knot is not finite"
RISING = "s must increase strictly over the valid knots"


@pytest.fixture(scope="module")
def m(pkg):
    m = handle(pkg)
    yield m
    m.close()


def source():
    """L, closed, channels [2][10][4]: two straight paths of 3 knots 1 m apart at 5 m/s (the makers look at the closed flag and the knot count only)"""
    ch = np.zeros((2, 10, LMAX))
    ch[:, S, :3] = [0.0, 1.0, 2.0]; ch[:, T, :3] = ch[:, S, :3] / 5.0; ch[:, V, :3] = 5.0; ch[:, E, :3] = ch[:, S, :3]
    ch[:, 8, :3] = 4.0; ch[:, 9, :3] = -4.0
    return np.array([3, 3], dtype=np.int32), np.array([0, 1], dtype=np.int32), ch


def pair_cases(alloc, v_and_length):
    """{name: (edits of the call, the text after the prefix)} of a pair maker; alloc: it has the allocation-arithmetic refusal; v_and_length: what it says of a
    library whose path 0 has a non-finite V and whose path 1 has one knot"""
    cases = {
        "null L": (dict(null="L"), NULL), "null channels": (dict(null="ch"), NULL), "null sets": (dict(null="sets"), NULL),
        "n_path 0": (dict(n_path=0), NEED), "n_sets 0": (dict(n_sets=0), NEED), "Lmax 1": (dict(Lmax=1), NEED),
        "pairs past 31 bits": (dict(n_path=BIG, n_sets=2), BITS),
        "L 1": (dict(L=(1, 1)), LENGTH), "L above Lmax": (dict(L=(0, LMAX + 1)), LENGTH), "closed with 2 knots": (dict(L=(1, 2)), CLOSED),
        "E inf": (dict(knots=[(0, E, 1, math.inf)]), FINITE), "edge_R nan": (dict(knots=[(1, 9, 2, math.nan)]), FINITE), "s nan": (dict(knots=[(1, S, 0, math.nan)]), FINITE),
        "s equal": (dict(knots=[(0, S, 2, 1.0)]), RISING), "s decreasing": (dict(knots=[(1, S, 1, -1.0)]), RISING),
        "L 1 before a non-finite E of the same path": (dict(L=(0, 1), knots=[(0, E, 0, math.inf)]), LENGTH),
        "non-finite E before s equal of the same path": (dict(knots=[(0, E, 2, math.inf), (0, S, 1, 0.0)]), FINITE),
        "s equal of path 0 before L 1 of path 1": (dict(L=(1, 1), knots=[(0, S, 2, 1.0)]), RISING),
        "V nan of path 0 and L 1 of path 1": (dict(L=(1, 1), knots=[(0, V, 0, math.nan)]), v_and_length),
    }
    if alloc:
        cases["too many elements"] = (dict(n_path=BIG, n_sets=1, Lmax=BIG), ALLOC)
    return cases


def check(m, who, call, cases):
    for name, (kw, text) in cases.items():
        assert call(**kw) == INVALID, name
        assert m.lib.pg_last_error(m.h).decode() == who + ": " + text, name


def edited(L=None, knots=(), null=None, **sizes):
    """the source with L = (path, value) and knots = [(path, row, knot, value)] written in; the arguments of a pair maker's call, one of them null"""
    Lk, cl, ch = source()
    if L:
        Lk[L[0]] = L[1]
    for p, row, i, x in knots:
        ch[p, row, i] = x
    arg = dict(L=Lk.ctypes.data_as(c_i32p), ch=ch.ctypes.data_as(c_dp), sets=True, keep=(Lk, cl, ch), cl=cl.ctypes.data_as(c_i32p))
    if null:
        arg[null] = None
    return arg, dict(dict(n_path=2, n_sets=1, Lmax=LMAX), **sizes)


def test_pg_plan_speeds(m):
    sets = (lib().pg_speed_plan * 1)(m.lib.pg_default_speed_plan())

    def call(**kw):
        a, n = edited(**kw)
        return m.lib.pg_plan_speeds(m.h, n["n_path"], n["Lmax"], a["L"], a["cl"], a["ch"], n["n_sets"], a["sets"] and sets, None, 1, None, None)

    check(m, "pg_plan_speeds", call, pair_cases(alloc=False, v_and_length=LENGTH))      # (V is what this maker writes: it does not read the source's)


def test_pg_offset_paths(m):
    sets = (lib().pg_offset_set * 1)(m.lib.pg_default_offset_set())

    def call(**kw):
        a, n = edited(**kw)
        return m.lib.pg_offset_paths(m.h, n["n_path"], n["Lmax"], a["L"], a["cl"], a["ch"], n["n_sets"], a["sets"] and sets, 1, None, None, None, None)

    cases = pair_cases(alloc=True, v_and_length="V of a valid knot is not finite and > 0")      # (path 0 is checked completely, its V included, before path 1 is looked at)
    cases["V nan after s equal of the same path"] = (dict(knots=[(0, V, 0, math.nan), (0, S, 2, 1.0)]), RISING)
    cases["t inf of the first knot"] = (dict(knots=[(1, T, 0, math.inf)]), "t of the first knot is not finite")
    check(m, "pg_offset_paths", call, cases)


def test_pg_clip_tubes(m):
    sets = (lib().pg_obstacle_set * 1)(m.lib.pg_default_obstacle_set())

    def call(**kw):
        a, n = edited(**kw)
        return m.lib.pg_clip_tubes(m.h, n["n_path"], n["Lmax"], a["L"], a["cl"], a["ch"], n["n_sets"], a["sets"] and sets, 0, None, 1, None, None, None, None, None)

    check(m, "pg_clip_tubes", call, pair_cases(alloc=True, v_and_length=LENGTH))         # (V travels as it is: this maker does not look at it)


def spec_call(m, maker, specs, parts, n_path=2, Lmax=LMAX, null=None):
    return getattr(m.lib, maker)(m.h, n_path, None if null == "specs" else specs, len(parts), None if null == "parts" else parts, Lmax, 1, None, None, None, None)


SPEC_ALLOC = "n_path * 10 * Lmax elements are more than the allocation arithmetic holds"
SPEC_LENGTH = "every path needs 2 <= n_knots <= Lmax"


def spec_cases(call, closed_text):
    """the counterparts of a spec maker: call(field edits of the two specs {(path, field): value}, **sizes)"""
    return {
        "null specs": (lambda: call({}, null="specs"), NULL), "null parts": (lambda: call({}, null="parts"), NULL),
        "too many elements": (lambda: call({}, n_path=BIG, Lmax=BIG), SPEC_ALLOC),
        "n_knots 1": (lambda: call({(1, "n_knots"): 1}), SPEC_LENGTH), "n_knots above Lmax": (lambda: call({(0, "n_knots"): LMAX + 1}), SPEC_LENGTH),
        "closed with 2 knots": (lambda: call({(1, "n_knots"): 2}), closed_text),
        "n_knots 1 of path 0 before closed with 2 knots of path 1": (lambda: call({(0, "n_knots"): 1, (1, "n_knots"): 2}), SPEC_LENGTH),
    }


def check_spec(m, who, cases):
    for name, (run, text) in cases.items():
        assert run() == INVALID, name
        assert m.lib.pg_last_error(m.h).decode() == who + ": " + text, name


def test_pg_make_paths(m):
    def call(edits, **kw):
        segs = (lib().pg_path_segment * 2)(m.lib.pg_default_path_segment(), m.lib.pg_default_path_segment())
        specs = (lib().pg_path_spec * 2)()
        for k in range(2):                                          # one straight segment of 1 m each; the second path is called closed
            specs[k].V_ref = 5.0; specs[k].seg0 = k; specs[k].n_seg = 1; specs[k].n_knots = 3; specs[k].closed = k
        for (k, field), x in edits.items():
            setattr(specs[k], field, x)
        return spec_call(m, "pg_make_paths", specs, segs, **kw)

    check_spec(m, "pg_make_paths", spec_cases(call, CLOSED))


def test_pg_fit_paths(m):
    def call(edits, **kw):
        wps = (lib().pg_waypoint * 6)(*[m.lib.pg_default_waypoint() for _ in range(6)])
        for i, (e, n) in enumerate([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (0.0, 5.0), (1.0, 5.0), (0.0, 6.0)]):
            wps[i].E = e; wps[i].N = n
        specs = (lib().pg_fit_spec * 2)()
        for k in range(2):                                          # three waypoints each: a line, and a triangle that is closed
            specs[k].V_ref = 5.0; specs[k].wp0 = 3 * k; specs[k].n_wp = 3; specs[k].n_knots = 3; specs[k].closed = k
        for (k, field), x in edits.items():
            setattr(specs[k], field, x)
        return spec_call(m, "pg_fit_paths", specs, wps, **kw)

    # (this maker words the closed path's refusal together with the waypoint counts)
    check_spec(m, "pg_fit_paths", spec_cases(call, "an open path needs >= 2 waypoints, a closed one >= 3 waypoints and >= 3 knots"))
