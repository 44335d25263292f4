"""pg_fit_paths on the device against its float64 numpy twin (tests/path_fit_numpy.py) over the shared case of tests/path_fit_cases.py: seven entries in one call,
Lmax = 520.  Then the fp32 library (the fp64 library's output rounded to float), independence of the batch and overlapping waypoint ranges, the install path against
pg_set_trajectories, the chain into pg_plan_speeds and a rollout, every refusal, and waypoints no path refers to.

fp64 library: every operation of the scheme is rounded once in both places, so t, s, V, A, E, N, kappa and both edges are the twin's bit for bit, and so is every stat but
turn and closure_psi.  psi, turn and closure_psi carry atan2: within 8 * 2^-52 * max(pi, |psi|) (path_fit_cases.psi_bar)."""
import math

import numpy as np
import pytest

import path_fit_cases as cases
from path_libs import INVALID, OK, c_dp, c_i32p, drive, handle, install_equals_set_trajectories, lib, refusals, step_bits

pytestmark = pytest.mark.gpu

N = cases.N_ENTRIES
EXACT = ((0, "t"), (1, "s"), (2, "V"), (3, "A"), (4, "E"), (5, "N"), (7, "kappa"), (8, "edge_L"), (9, "edge_R"))
EXACT_STATS = ("length", "closure_pos", "kappa_abs_max", "ds", "chord_min", "chord_max", "s_err_max", "reserved")


def raw_fit(m, specs, wps, Lmax=cases.LMAX, install=False):
    n = len(specs)
    out = np.full((n, 10, Lmax), np.nan)
    L = np.full(n, -1, dtype=np.int32); cl = np.full(n, -1, dtype=np.int32)
    st = (lib().pg_fit_stats * n)()
    rc = m.lib.pg_fit_paths(m.h, n, specs, len(wps), wps, Lmax, int(install), L.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), out.ctypes.data_as(c_dp), st)
    assert rc == OK, m.lib.pg_last_error(m.h)
    return out, st, L, cl


@pytest.fixture(scope="module")
def fitted(pkg):
    """the shared case through the fp64 library, once: (channels_out [7][10][520], stats, L_out, closed_out)"""
    m = handle(pkg)
    out = raw_fit(m, *cases.packed(type(m)))
    m.close()
    return out


def test_fp64_library_against_the_twin(fitted):
    out, st, L, cl = fitted
    ref = cases.reference()
    exp = cases.expected_channels()
    assert list(L) == cases.N_KNOTS and list(cl) == cases.CLOSED
    for k in range(N):
        n = cases.N_KNOTS[k]
        assert np.all(out[k][:, n:] == 0.0), k
        for c, name in EXACT:
            assert out[k, c, :n].tobytes() == exp[k, c, :n].tobytes(), (k, name)
        dpsi = np.abs(out[k, 6, :n] - exp[k, 6, :n])
        s, r = st[k], ref[k]["stats"]
        print(f"entry {k}: worst |psi - twin| {dpsi.max():.3e} (bar at least {cases.psi_bar(0.0):.3e}), {int(np.count_nonzero(dpsi))} of {n} knots differ; s_err_max {s.s_err_max:.3e}, "
              f"turn - twin {s.turn - r['turn']:.3e}")
        assert np.all(dpsi <= cases.psi_bar(exp[k, 6, :n])), k
        for f in EXACT_STATS:
            assert getattr(s, f) == r[f], (k, f)
        bar = float(cases.psi_bar(exp[k, 6, n - 1]) + cases.psi_bar(exp[k, 6, 0]))
        assert abs(s.turn - r["turn"]) <= bar and abs(s.closure_psi - r["closure_psi"]) <= bar, k
        assert (s.closure_pos == 0.0) == bool(cases.CLOSED[k])
    # the circle: +1 / R counter-clockwise, -1 / R clockwise, one lap of heading each way, unwrapped
    assert np.all(out[3, 7, :300] > 0) and np.all(out[4, 7, :64] < 0) and np.all(np.diff(out[3, 6, :300]) > 0)
    assert st[3].turn == pytest.approx(2 * math.pi, abs=1e-12) and st[4].turn == pytest.approx(-2 * math.pi, abs=1e-12)


def test_fp32_library_is_the_fp64_output_rounded(pkg, fitted):
    out, st, L, cl = fitted
    m = handle(pkg, "f32")
    o32, s32, L32, cl32 = raw_fit(m, *cases.packed(type(m)))
    m.close()
    assert o32.tobytes() == out.astype(np.float32).astype(np.float64).tobytes()
    assert bytes(s32) == bytes(st) and list(L32) == list(L) and list(cl32) == list(cl)


def test_independence_of_the_batch_and_overlapping_ranges(pkg, fitted):
    out, st, L, cl = fitted
    m = handle(pkg)
    M = type(m)
    for k in range(N):                                              # each entry alone, Lmax = its own knot count
        n = cases.N_KNOTS[k]
        one, s1, L1, c1 = raw_fit(m, *cases.packed(M, [k]), Lmax=n)
        assert one[0].tobytes() == np.ascontiguousarray(out[k][:, :n]).tobytes(), k
        assert bytes(s1[0]) == bytes(st[k]) and L1[0] == n and c1[0] == cases.CLOSED[k], k
    rev, srev, _, _ = raw_fit(m, *cases.packed(M, reversed(range(N))))
    for k in range(N):
        assert rev[N - 1 - k].tobytes() == out[k].tobytes() and bytes(srev[N - 1 - k]) == bytes(st[k]), k
    # one circle fitted twice from ONE range of waypoints, at 300 and at 64 knots: each as it is alone
    specs, wps = cases.packed(M, [3])
    two = (lib().pg_fit_spec * 2)(specs[0], specs[0])
    two[1].n_knots = 64
    o2, s2, L2, _ = raw_fit(m, two, wps)
    alone, sa, _, _ = raw_fit(m, (lib().pg_fit_spec * 1)(two[1]), wps)
    assert list(L2) == [300, 64] and o2[0].tobytes() == out[3].tobytes() and o2[1].tobytes() == alone[0].tobytes() and bytes(s2[1]) == bytes(sa[0])
    assert s2[0].length == s2[1].length and np.all(o2[1][7, :64] > 0)
    # the Python method returns the same tubes, flags and stats
    tubes, closed, stats = m.fit_paths(cases.entries(), Lmax=cases.LMAX)
    for k, t in enumerate(tubes):
        n = cases.N_KNOTS[k]
        assert len(t) == n and t.E.tobytes() == out[k, 4, :n].tobytes() and t.psi.tobytes() == out[k, 6, :n].tobytes() and np.all(t.theta == 0), k
    assert list(closed) == cases.CLOSED and [float(x) for x in stats["length"]] == [s.length for s in st] and stats["s_err_max"].tobytes() == np.array([s.s_err_max for s in st]).tobytes()
    m.close()


def test_install_equals_set_trajectories_with_the_returned_channels(pkg, fitted):
    out, st, L, cl = fitted
    a, b = handle(pkg), handle(pkg)
    raw_fit(a, *cases.packed(type(a)), install=True)
    scurve = a.tubes_from_channels(out, L)[5]
    index = np.full(5, 5, dtype=np.int32)                           # the starts lie on the S-curve (63.5 m)
    install_equals_set_trajectories(pkg, a, b, out, L, cases.LMAX, index, scurve)
    a.close(); b.close()


def test_the_chain_into_plan_speeds_and_a_rollout(pkg, fitted):
    """Fit the counter-clockwise circle (entry 3), hand closed_out to pg_plan_speeds with install, and drive four instances from starts on the path for 20 steps: every
    step is solved and no instance leaves the tube.  The circle's curvature 1 / 7 = 0.143 1/m is beyond what X1 can steer (kappa_max = tan(18 deg) / L = 0.113 1/m), so
    the handle's vehicle is X1 with delta_max = 30 deg (kappa_max 0.201 1/m): a vehicle that can hold the path it is asked to track."""
    out, st, L, cl = fitted
    vehicle = pkg.X1(delta_max=30 * math.pi / 180)
    assert vehicle["kappa_max"] > 1.0 / cases.CIRCLE_R > pkg.X1()["kappa_max"]
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 4, vehicle=vehicle)
    m.set_option("tracking_summary", 1)
    tubes, closed, stats = m.fit_paths([cases.entries()[3]])
    assert list(closed) == [1] and tubes[0].kappa.tobytes() == out[3, 7, :300].tobytes()
    planned, ps = m.plan_speeds(tubes, [pkg.vehicles.speed_plan(mu_scale=0.5, V_max=12.0)], closed=closed, install=True)
    tube = planned[0]
    assert tube.E.tobytes() == tubes[0].E.tobytes() and np.all(tube.V > 0) and np.isfinite(ps["usage_max"][0])
    status, summary, first_exit = drive(m, tube, [5, 80, 150, 220], 20)
    print("fitted circle: V", tube.V[[5, 80, 150, 220]], "max |e|", summary[:, 0], "first_exit", first_exit, "statuses", np.unique(status))
    assert np.all(pkg.is_solved(status)), np.unique(status)
    assert np.all(first_exit == -1), first_exit
    m.close()


def test_every_refusal_leaves_the_installed_library_alone(pkg):
    m = handle(pkg)
    M = type(m)
    before = step_bits(m, pkg)
    Lc = lib()

    def call(n_path=N, Lmax=cases.LMAX, spec=None, wp=None, null_specs=False, null_wps=False, n_wp_total=None):
        """the shared case with one edit: spec = (entry, field, value), wp = (waypoint, field, value)"""
        specs, wps = cases.packed(M)
        if spec:
            setattr(specs[spec[0]], spec[1], spec[2])
        if wp:
            setattr(wps[wp[0]], wp[1], wp[2])
        return m.lib.pg_fit_paths(m.h, n_path, None if null_specs else specs, len(wps) if n_wp_total is None else n_wp_total, None if null_wps else wps, Lmax, 1,
                                  None, None, None, None)

    specs, wps = cases.packed(M)
    n_wps = len(wps)
    assert n_wps == 2 + 3 + 24 + 24 + 300 + 9 and [s.wp0 for s in specs] == [0, 2, 2, 5, 29, 53, 353]
    big = 2**31 - 1
    refused = {
        "null specs": dict(null_specs=True), "null waypoints": dict(null_wps=True), "n_path 0": dict(n_path=0), "n_wp_total 0": dict(n_wp_total=0), "Lmax 1": dict(Lmax=1),
        "n_knots 1": dict(spec=(0, "n_knots", 1)), "n_knots above Lmax": dict(spec=(5, "n_knots", 521)), "Lmax below n_knots": dict(Lmax=512),
        "open with 1 waypoint": dict(spec=(0, "n_wp", 1)), "n_wp 0": dict(spec=(5, "n_wp", 0)), "closed with 2 waypoints": dict(spec=(1, "n_wp", 2)),
        "closed with 2 knots": dict(spec=(1, "n_knots", 2)), "wp0 negative": dict(spec=(4, "wp0", -1)), "wp0 at n_wp_total": dict(spec=(0, "wp0", n_wps)),
        "range past the end": dict(spec=(6, "n_wp", 10)), "range past a smaller n_wp_total": dict(n_wp_total=n_wps - 1), "n_wp that overflows": dict(spec=(6, "n_wp", big)),
        "E nan": dict(wp=(3, "E", np.nan)), "N inf": dict(wp=(30, "N", np.inf)), "edge_L nan": dict(wp=(60, "edge_L", np.nan)), "edge_R -inf": dict(wp=(361, "edge_R", -np.inf)),
        "edge_L = edge_R": dict(wp=(6, "edge_L", -2.0)), "edge_L below edge_R": dict(wp=(100, "edge_L", -7.0)),
        "V_ref 0": dict(spec=(0, "V_ref", 0.0)), "V_ref negative": dict(spec=(3, "V_ref", -6.0)), "V_ref inf": dict(spec=(2, "V_ref", np.inf)), "V_ref nan": dict(spec=(2, "V_ref", np.nan)),
        "too many elements": dict(n_path=big, Lmax=big),
    }
    assert call() == OK                                             # the unedited call is accepted (and installs: put the first library back)
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    refusals(m, pkg, call, refused, "pg_fit_paths", before)

    def one(points, n_knots, closed, h=m, Lmax=None):
        w = (Lc.pg_waypoint * len(points))()
        for i, (E, Nn) in enumerate(points):
            w[i] = h.lib.pg_default_waypoint(); w[i].E = E; w[i].N = Nn
        s = (Lc.pg_fit_spec * 1)()
        s[0].V_ref = 6.0; s[0].wp0 = 0; s[0].n_wp = len(points); s[0].n_knots = n_knots; s[0].closed = closed
        return h.lib.pg_fit_paths(h.h, 1, s, len(points), w, Lmax or n_knots, 1, None, None, None, None)

    # two neighbouring waypoints at the same point: inside the path, and last-to-first on a closed one (open, the same points are accepted)
    tri = [(0.0, 0.0), (10.0, 0.0), (4.0, 8.0)]
    for points, closed in (([tri[0], tri[1], tri[1], tri[2]], 0), (tri + [tri[0]], 1)):
        assert one(points, 9, closed) == INVALID
        assert m.lib.pg_last_error(m.h).decode().startswith("pg_fit_paths") and "same point" in m.lib.pg_last_error(m.h).decode()
        assert step_bits(m, pkg) == before
    assert one(tri + [tri[0]], 9, 0, Lmax=9) == OK
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    # knots so dense that s cannot be shown to increase: chords whose sum over n_knots - 1 leaves the stated range ...
    assert one([(0.0, 0.0), (1e-29, 0.0)], 100, 0) == INVALID
    assert "dense" in m.lib.pg_last_error(m.h).decode() and m.lib.pg_last_error(m.h).decode().startswith("pg_fit_paths")
    assert step_bits(m, pkg) == before
    m.close()
    # ... and, in the fp32 library, more than 2^21 intervals (nothing is allocated: the refusal comes first)
    f = handle(pkg, "f32")
    before32 = step_bits(f, pkg)
    assert one(tri, 2**21 + 2, 1, h=f) == INVALID
    assert "dense" in f.lib.pg_last_error(f.h).decode()
    assert step_bits(f, pkg) == before32
    f.close()


def test_waypoints_no_path_refers_to_are_not_looked_at(pkg, fitted):
    out, st, L, cl = fitted
    m = handle(pkg)
    specs, wps0 = cases.packed(type(m))
    n = len(wps0)
    wps = (lib().pg_waypoint * (n + 2))()
    wps[0].E = np.nan; wps[0].N = np.inf; wps[0].edge_L = np.nan; wps[0].edge_R = np.nan
    for i in range(n):
        wps[i + 1] = wps0[i]
    wps[n + 1] = wps[0]
    for s in specs:
        s.wp0 += 1
    got, st2, _, _ = raw_fit(m, specs, wps)
    assert got.tobytes() == out.tobytes() and bytes(st2) == bytes(st)
    m.close()
