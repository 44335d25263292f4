"""CPU tests of the route library (pg_set_route_sets): the numpy twin on hand-written schedules -- an event at step 0, two events, an event that never fires, relative -1
from index 0 --, the four anchors, the packer and vehicles.route, every refusal text of route_set_problem against the text in csrc/pg_api.hip, the ctypes structures
against the header as the C compiler lays it out, and the new names declared, exported and mirrored."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import route_numpy as rn
from conftest import ROOT

NEW_NAMES = ["pg_set_route_sets", "pg_set_route_index", "pg_clear_route_sets", "pg_get_route_sets", "pg_get_route_state", "pg_set_route_history_dev"]


def test_hand_written_schedules():
    sets = [rn.route(),                                                                  # 0: identity
            rn.route(rn.event(0, 2)),                                                    # 1: at step 0
            rn.route(rn.event(1, 1), rn.event(3, 0)),                                    # 2: two events
            rn.route(rn.event(7, 1)),                                                    # 3: never fires in 5 steps
            rn.route(rn.event(2, -1, relative=True)),                                    # 4: relative -1
            rn.route(rn.event(1, 2, relative=True), rn.event(2, 2, relative=True))]      # 5: relative, wrapping forward
    index = np.arange(6); home = np.array([1, 0, 2, 0, 0, 2])
    ran, fired, last = rn.schedule(sets, index, home, 3, 0, 5)
    assert ran.T.tolist() == [[1] * 5, [2] * 5, [2, 1, 1, 0, 0], [0] * 5, [0, 0, 2, 2, 2], [2, 1, 0, 0, 0]]
    assert fired.tolist() == [0, 1, 2, 0, 1, 2] and last.tolist() == [-1, 0, 3, -1, 2, 2]
    # a call that continues the clock sees the same schedule from its first step on
    late, fired2, last2 = rn.schedule(sets, index, home, 3, 2, 3)
    assert np.array_equal(late, ran[2:]) and np.array_equal(fired2, fired) and np.array_equal(last2, last)
    # one set for everyone needs no index
    one, f1, _ = rn.schedule([sets[4]], None, [0, 1, 2], 3, 0, 4)
    assert one.T.tolist() == [[0, 0, 2, 2], [1, 1, 0, 0], [2, 2, 1, 1]] and f1.tolist() == [1, 1, 1]
    assert rn.target_of(rn.event(0, -4, relative=True), 0, 3) == 2 and rn.target_of(rn.event(0, 5, relative=True), 2, 3) == 1


def test_the_four_anchors(pkg, skidpad):
    t0, toff = 12.5, 3.25
    assert rn.offset_of(rn.event(2, 1, rn.KEEP), t0, toff) == (3.25, 9.25)
    off, at = rn.offset_of(rn.event(2, 1, rn.PATH), t0, toff)
    assert np.isnan(off) and np.isnan(at)
    assert rn.offset_of(rn.event(2, 1, rn.STAMP), t0, toff) == (12.5, 0.0) and rn.offset_of(rn.event(2, 1, rn.STAMP, t_join=1.5), t0, toff) == (11.0, 1.5)
    keep_nan = rn.offset_of(rn.event(2, 1, rn.KEEP), t0, np.nan)
    assert np.isnan(keep_nan[0]) and np.isnan(keep_nan[1])
    # PROJECT: a point 0.3 m left of knot 40's segment joins the trajectory where the oracle's projection puts it
    i = 40
    E, N, psi = skidpad.E[i], skidpad.N[i], skidpad.psi[i]
    s, e, t = rn.project(skidpad.data, E - 0.3 * np.cos(psi), N - 0.3 * np.sin(psi))
    assert abs(e - 0.3) < 1e-6 and abs(s - skidpad.s[i]) < 0.05 and abs(t - skidpad.t[i]) < 0.01
    off, at = rn.offset_of(rn.event(2, 1, rn.PROJECT, t_join=0.5), t0, toff, t_proj=t)
    assert at == t and off == t0 - (t + 0.5)


def test_packer_and_vehicles_route(pkg):
    from pigeon_jl_amd import _lib
    M = pkg.BatchedTrajectoryTrackingMPC
    assert pkg.route() == rn.route() and pkg.vehicles.route is pkg.route and pkg.vehicles.route_event is pkg.route_event
    assert pkg.route_event(40, 1) == rn.event(40, 1) and pkg.route_event(3, -1, anchor="project", relative=True, cold=False, t_join=0.25) == rn.event(3, -1, rn.PROJECT, True, False, 0.25)
    for name, code in (("keep", rn.KEEP), ("path", rn.PATH), ("stamp", rn.STAMP), ("project", rn.PROJECT)):
        assert pkg.route_event(1, 0, anchor=name)["anchor"] == code == pkg.vehicles.ROUTE_ANCHORS[name]
    with pytest.raises(KeyError):
        pkg.route_event(1, 0, anchor="snap")
    with pytest.raises(ValueError):
        pkg.route_event(1.5, 0)
    with pytest.raises(ValueError):
        pkg.route(*[pkg.route_event(k, 0) for k in range(5)])
    arr = M.pack_routes([pkg.route(), pkg.route(pkg.route_event(1, 1, "keep"), pkg.route_event(3, -1, "project", relative=True, cold=False, t_join=0.5)), [pkg.route_event(2, 2)]])
    assert len(arr) == 3 and isinstance(arr[0], _lib.pg_route)
    rows = lambda r: [tuple(getattr(e, f) for f in rn.FIELDS) for e in r.ev]
    unused = (-1, 0, 0, rn.STAMP, 1, 0, 0.0)
    assert rows(arr[0]) == [unused] * 4                         # pg_default_route, field for field
    assert rows(arr[1]) == [(1, 1, 0, rn.KEEP, 1, 0, 0.0), (3, -1, 1, rn.PROJECT, 0, 0, 0.5), unused, unused]
    assert rows(arr[2]) == [(2, 2, 0, rn.STAMP, 1, 0, 0.0)] + [unused] * 3                # a shorter list is filled with unused slots
    assert bytes(M.pack_routes([arr[1]])[0]) == bytes(arr[1])
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    body = re.search(r"pg_route pg_default_route\(void\) \{(.*?)\n\}", api, flags=re.S).group(1)
    assert "memset(&r, 0, sizeof(r))" in body and "e.step = -1; e.anchor = PG_ROUTE_STAMP; e.cold = 1;" in body
    assert tuple(n for n, _ in _lib.pg_route_event._fields_) == rn.FIELDS == pkg.vehicles.ROUTE_EVENT_FIELDS


def test_every_refusal_of_route_set_problem_in_the_words_of_the_library():
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    body = re.search(r"static const char\* route_set_problem\(const pg_route& r\) \{(.*?)\n\}", api, flags=re.S).group(1)
    assert tuple(re.findall(r'return "([^"]+)";', body)) == rn.PROBLEMS      # the same texts in the same order of tests
    ev = rn.event
    cases = [(rn.route(dict(ev(1, 0), target_mode=2)), rn.BAD_TARGET_MODE), (rn.route(dict(ev(1, 0), anchor=4)), rn.BAD_ANCHOR), (rn.route(dict(ev(1, 0), anchor=-1)), rn.BAD_ANCHOR),
             (rn.route(dict(ev(1, 0), cold=2)), rn.BAD_COLD), (rn.route(dict(ev(1, 0), reserved=1)), rn.BAD_RESERVED),
             (rn.route(ev(1, 0, t_join=np.inf)), rn.BAD_T_JOIN), (rn.route(ev(1, 0, t_join=np.nan)), rn.BAD_T_JOIN),
             (rn.route(ev(1, 0, rn.KEEP, t_join=0.5)), rn.T_JOIN_UNUSED), (rn.route(ev(1, 0, rn.PATH, t_join=-0.5)), rn.T_JOIN_UNUSED),
             ([ev(-1, 0), ev(2, 1), ev(-1, 0), ev(-1, 0)], rn.USED_BEHIND_UNUSED),
             (rn.route(ev(2, 0), ev(2, 1)), rn.NOT_INCREASING), (rn.route(ev(3, 0), ev(1, 1)), rn.NOT_INCREASING),
             (rn.route(ev(1, -1)), rn.NEGATIVE_TARGET)]
    assert {why for _, why in cases} == set(rn.PROBLEMS)
    for rset, why in cases:
        assert rn.problem(rset) == why, (rset, why)
    for good in (rn.route(), rn.route(ev(0, 0)), rn.route(ev(0, 1), ev(1, -2, relative=True), ev(5, 2, rn.PROJECT, t_join=-0.5), ev(6, 0, rn.PATH, cold=False)),
                 rn.route(dict(ev(-1, -3), t_join=0.0))):      # (an unused slot's target is not looked at)
        assert rn.problem(good) is None, good
    # ... and the three things a rollout refuses, each with the word the caller needs
    ready = api[api.index("static int rollout_ready("):api.index("struct RolloutHist")]
    for phrase in ("no trajectory library of at least two trajectories", "pg_set_trajectory_index does not cover the batch", "outside the installed trajectory library of", "index_covers(h, U.lib)"):
        assert phrase in ready, phrase


def test_structure_layout_equals_the_headers(pkg, tmp_path):
    """sizeof / offsetof of pg_route_event and pg_route as the C compiler lays out include/pigeon_mpc.h, against the ctypes mirror"""
    from pigeon_jl_amd import _lib
    assert C.sizeof(_lib.pg_route_event) == 32 and C.sizeof(_lib.pg_route) == 128 and _lib.PG_ROUTE_EVENTS == rn.EVENTS == pkg.vehicles.ROUTE_EVENTS == 4
    src = tmp_path / "layout.c"
    fields = [n for n, _ in _lib.pg_route_event._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pigeon_mpc.h"\nint main(void) { printf("%zu %zu %d %d %d %d %d %d %d", sizeof(pg_route), sizeof(pg_route_event), '
                   'PG_ROUTE_EVENTS, PG_ROUTE_ABSOLUTE, PG_ROUTE_RELATIVE, PG_ROUTE_KEEP, PG_ROUTE_PATH, PG_ROUTE_STAMP, PG_ROUTE_PROJECT);\n'
                   + "".join(f'printf(" %zu", offsetof(pg_route_event, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 32, 4, rn.ABSOLUTE, rn.RELATIVE, rn.KEEP, rn.PATH, rn.STAMP, rn.PROJECT] + [getattr(_lib.pg_route_event, f).offset for f in fields]
    assert got[9:] == [0, 4, 8, 12, 16, 20, 24]
    assert (_lib.PG_ROUTE_ABSOLUTE, _lib.PG_ROUTE_RELATIVE, _lib.PG_ROUTE_KEEP, _lib.PG_ROUTE_PATH, _lib.PG_ROUTE_STAMP, _lib.PG_ROUTE_PROJECT) == (0, 1, 0, 1, 2, 3)


def test_names_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    julia = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint " + name + r"\(pg_handle\*", header), name
        assert name in pkg.SYMBOLS and ":" + name in julia and name in integration, name
    assert re.search(r"\bpg_route pg_default_route\(void\);", header) and "pg_default_route" in pkg.SYMBOLS and ":pg_default_route" in julia
    assert '"stat_route_steps"' in header and "IDENTITY: pg_default_route()" in header
    from pigeon_jl_amd import _lib
    assert sorted(_lib.ROUTE_SET_PROTOTYPES) == sorted(NEW_NAMES)
    for lib_name in ("libpigeon_hip.so", "libpigeon_hip_f32.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib_name)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NEW_NAMES + ["pg_default_route"]) <= exported, sorted(set(NEW_NAMES) - exported)
    M = pkg.BatchedTrajectoryTrackingMPC
    for meth in ("pack_routes", "set_routes", "set_route_index", "clear_routes", "routes", "route_state", "record_route"):
        assert callable(getattr(M, meth)), meth
    # the kernel is a source of the build, a file of its own, and entitled to double arithmetic for the time offset only
    make = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert "pg_route.hip" in re.search(r"^SRCS := (.*)$", make, re.M).group(1)
    assert '#include "pg_route.hip"' in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()
