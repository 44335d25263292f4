"""pg_make_paths on the device against its float64 numpy twin (tests/path_make_numpy.py) over the shared case of tests/path_make_cases.py: five paths in one call,
Lmax = 300.  Then the fp32 library (the fp64 library's output rounded to float), determinism and independence of the batch, the install path against
pg_set_trajectories, the chain into pg_plan_speeds, every refusal, and one closed-loop condition.

fp64 library: s, psi, kappa, the edges, t, V and A are closed forms whose every operation is rounded once in both places: bit for bit.  E and N: the library sums the
interval increments in blocks, the twin serially; the bar 4 (n_knots + 64) 2^-53 total is derived (path_make_cases.bar), 3.3e-11 m for the oval of 201.1 m.
Measured on the MI355X: see EXPERIMENTS 30."""
import numpy as np
import pytest

import path_make_cases as cases
from path_libs import INVALID, OK, c_dp, c_i32p, drive, handle, install_equals_set_trajectories, lib, refusals, step_bits

pytestmark = pytest.mark.gpu

GEOMETRY = (1, 4, 5, 6, 7, 8, 9)
N_PATH = 5


def packed(m, which=range(N_PATH)):
    p, _ = cases.reference()
    which = list(which)
    return m.pack_path_specs([p[k] for k in which], [cases.N_KNOTS[k] for k in which], V_ref=[cases.V_REFS[k] for k in which], pose=[cases.POSES[k] for k in which],
                             closed=[cases.CLOSED[k] for k in which])


def raw_make(m, specs, segs, Lmax=cases.LMAX, install=False):
    n = len(specs)
    out = np.full((n, 10, Lmax), np.nan)
    L = np.full(n, -1, dtype=np.int32); cl = np.full(n, -1, dtype=np.int32)
    st = (lib().pg_path_stats * n)()
    rc = m.lib.pg_make_paths(m.h, n, specs, len(segs), segs, Lmax, int(install), L.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), out.ctypes.data_as(c_dp), st)
    assert rc == OK, m.lib.pg_last_error(m.h)
    return out, st, L, cl


@pytest.fixture(scope="module")
def made(pkg):
    """the shared case through the fp64 library, once: (channels_out [5][10][300], stats, L_out, closed_out)"""
    m = handle(pkg)
    out = raw_make(m, *packed(m))
    m.close()
    return out


def test_fp64_library_against_the_twin(made):
    out, st, L, cl = made
    _, ref = cases.reference()
    exp = cases.expected_channels()
    assert list(L) == cases.N_KNOTS and list(cl) == cases.CLOSED
    for k in range(N_PATH):
        n = cases.N_KNOTS[k]; bar = cases.bar(k)
        assert np.all(out[k][:, n:] == 0.0), k
        for c, name in ((1, "s"), (6, "psi"), (7, "kappa"), (8, "edge_L"), (9, "edge_R"), (0, "t"), (2, "V"), (3, "A")):
            assert out[k, c, :n].tobytes() == exp[k, c, :n].tobytes(), (k, name)
        worst = max(float(np.max(np.abs(out[k, 4, :n] - exp[k, 4, :n]))), float(np.max(np.abs(out[k, 5, :n] - exp[k, 5, :n]))))
        s, r = st[k], ref[k]["stats"]
        print(f"path {k}: worst |E, N - twin| {worst:.3e} m (bar {bar:.3e}); closure_pos {s.closure_pos:.3e} (twin {r['closure_pos']:.3e}), closure_psi {s.closure_psi:.3e}")
        assert worst <= bar, k
        assert out[k, 4, 0] == cases.POSES[k][0] and out[k, 5, 0] == cases.POSES[k][1]
        for f in ("length", "turn", "closure_psi", "kappa_abs_max", "ds"):
            assert getattr(s, f) == r[f], (k, f)
        assert abs(s.closure_pos - r["closure_pos"]) <= bar, k
        assert s.closure_pos == pytest.approx(float(np.hypot(out[k, 4, n - 1] - out[k, 4, 0], out[k, 5, n - 1] - out[k, 5, 0])), abs=bar)


def test_fp32_library_is_the_fp64_output_rounded(pkg, made):
    out, st, L, cl = made
    m = handle(pkg, "f32")
    o32, s32, L32, cl32 = raw_make(m, *packed(m))
    m.close()
    assert o32.tobytes() == out.astype(np.float32).astype(np.float64).tobytes()
    assert bytes(s32) == bytes(st) and list(L32) == list(L) and list(cl32) == list(cl)


def test_determinism_and_independence_of_the_batch(pkg, made):
    out, st, L, cl = made
    m = handle(pkg)
    again = raw_make(m, *packed(m))
    assert again[0].tobytes() == out.tobytes() and bytes(again[1]) == bytes(st)
    for k in range(N_PATH):                                         # each path alone, Lmax = its own knot count
        n = cases.N_KNOTS[k]
        one, s1, L1, c1 = raw_make(m, *packed(m, [k]), Lmax=n)
        assert one[0].tobytes() == np.ascontiguousarray(out[k][:, :n]).tobytes(), k
        assert bytes(s1[0]) == bytes(st[k]) and L1[0] == n and c1[0] == cases.CLOSED[k], k
    rev, srev, Lrev, crev = raw_make(m, *packed(m, reversed(range(N_PATH))))
    for k in range(N_PATH):
        assert rev[N_PATH - 1 - k].tobytes() == out[k].tobytes() and bytes(srev[N_PATH - 1 - k]) == bytes(st[k]), k
    # the Python method returns the same tubes and stats
    p, _ = cases.reference()
    tubes, stats = m.make_paths(p, n_knots=cases.N_KNOTS, V_ref=cases.V_REFS, pose=cases.POSES, closed=cases.CLOSED)
    for k, t in enumerate(tubes):
        n = cases.N_KNOTS[k]
        assert len(t) == n and t.E.tobytes() == out[k, 4, :n].tobytes() and t.edge_R.tobytes() == out[k, 9, :n].tobytes() and np.all(t.theta == 0), k
    assert stats.tobytes() == bytes(st)
    m.close()


def test_install_equals_set_trajectories_with_the_returned_channels(pkg, made):
    out, st, L, cl = made
    a, b = handle(pkg), handle(pkg)
    raw_make(a, *packed(a), install=True)
    oval = a.tubes_from_channels(out, L)[1]
    index = np.full(5, 1, dtype=np.int32)                           # the starts lie on the oval
    install_equals_set_trajectories(pkg, a, b, out, L, cases.LMAX, index, oval)
    a.close(); b.close()


def test_the_chain_into_plan_speeds(pkg, made):
    out, st, L, cl = made
    m = handle(pkg)
    pick = [1, 3]
    sets = [pkg.vehicles.speed_plan(mu_scale=0.5, V_max=12.0), pkg.vehicles.speed_plan(mu_scale=0.9, V_max=20.0, V_end=2.0)]
    arr = m.pack_speed_plans(sets)
    ch = np.ascontiguousarray(out[pick]); Lp = np.ascontiguousarray(L[pick]); clp = np.ascontiguousarray(cl[pick])
    planned = np.full((4, 10, cases.LMAX), np.nan)
    ps = (lib().pg_speed_plan_stats * 4)()
    rc = m.lib.pg_plan_speeds(m.h, 2, cases.LMAX, Lp.ctypes.data_as(c_i32p), clp.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), 2, arr, None, 0, planned.ctypes.data_as(c_dp), ps)
    assert rc == OK, m.lib.pg_last_error(m.h)
    for i, k in enumerate(pick):
        n = cases.N_KNOTS[k]
        for j in range(2):
            o = planned[i * 2 + j]; s = ps[i * 2 + j]
            assert np.isfinite(s.usage_max) and s.n_cap + s.n_accel + s.n_brake == n, (k, j)
            for c in GEOMETRY:
                assert o[c].tobytes() == out[k, c].tobytes(), (k, j, c)
            assert np.all(np.isfinite(o[:, :n])) and np.all(o[2, :n] > 0) and np.all(o[:, n:] == 0)
    m.close()


def test_every_refusal_leaves_the_installed_library_alone(pkg):
    m = handle(pkg)
    before = step_bits(m, pkg)
    L = lib()

    def call(n_path=N_PATH, Lmax=cases.LMAX, spec=None, seg=None, null_specs=False, null_segs=False, n_seg_total=None):
        """the shared case with one edit: spec = (path, field, value), seg = (segment, field, value)"""
        specs, segs = packed(m)
        if spec:
            setattr(specs[spec[0]], spec[1], spec[2])
        if seg:
            setattr(segs[seg[0]], seg[1], seg[2])
        return m.lib.pg_make_paths(m.h, n_path, None if null_specs else specs, len(segs) if n_seg_total is None else n_seg_total, None if null_segs else segs, Lmax, 1,
                                   None, None, None, None)

    n_segs = len(packed(m)[1])
    assert n_segs == 19
    big = 2**31 - 1
    refused = {
        "null specs": dict(null_specs=True), "null segments": dict(null_segs=True), "n_path 0": dict(n_path=0), "n_seg_total 0": dict(n_seg_total=0), "Lmax 1": dict(Lmax=1),
        "n_knots 1": dict(spec=(2, "n_knots", 1)), "n_knots above Lmax": dict(spec=(1, "n_knots", 301)), "Lmax below n_knots": dict(Lmax=299),
        "closed with 2 knots": dict(spec=(0, "closed", 1)), "n_seg 0": dict(spec=(3, "n_seg", 0)), "seg0 negative": dict(spec=(3, "seg0", -1)),
        "seg0 at n_seg_total": dict(spec=(0, "seg0", n_segs)), "range past the end": dict(spec=(4, "n_seg", 2)), "range past a smaller n_seg_total": dict(n_seg_total=n_segs - 1),
        "n_seg that overflows": dict(spec=(4, "n_seg", big)),
        "length 0": dict(seg=(3, "length", 0.0)), "length negative": dict(seg=(0, "length", -1.0)), "length inf": dict(seg=(3, "length", np.inf)), "length nan": dict(seg=(18, "length", np.nan)),
        "kappa0 nan": dict(seg=(5, "kappa0", np.nan)), "kappa1 inf": dict(seg=(5, "kappa1", np.inf)), "edge_L0 inf": dict(seg=(9, "edge_L0", np.inf)), "edge_R1 nan": dict(seg=(9, "edge_R1", np.nan)),
        "E0 nan": dict(spec=(1, "E0", np.nan)), "N0 inf": dict(spec=(1, "N0", np.inf)), "psi0 nan": dict(spec=(4, "psi0", np.nan)),
        "edge_L0 = edge_R0": dict(seg=(2, "edge_L0", -4.0)), "edge_L1 below edge_R1": dict(seg=(18, "edge_L1", -7.0)),
        "V_ref 0": dict(spec=(0, "V_ref", 0.0)), "V_ref negative": dict(spec=(0, "V_ref", -6.0)), "V_ref inf": dict(spec=(2, "V_ref", np.inf)), "V_ref nan": dict(spec=(2, "V_ref", np.nan)),
        "reserved 1": dict(seg=(7, "reserved", 1.0)),
        "too many elements": dict(n_path=big, Lmax=big),
    }
    assert call() == OK                                             # the unedited call is accepted (and installs: put the first library back)
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    refusals(m, pkg, call, refused, "pg_make_paths", before)
    # knots so dense that s does not increase strictly in the library's element type.  In double, i ds is at least an ulp of the total apart for any n_knots an int32
    # holds, except where ds itself is lost:
    specs = (L.pg_path_spec * 1)(); segs = (L.pg_path_segment * 1)()
    segs[0] = m.lib.pg_default_path_segment()
    segs[0].length = 5e-324                                         # the smallest subnormal: total / 2 rounds to 0, and s_1 = s_0
    specs[0].V_ref = 6.0; specs[0].seg0 = 0; specs[0].n_seg = 1; specs[0].n_knots = 3
    assert m.lib.pg_make_paths(m.h, 1, specs, 1, segs, 3, 1, None, None, None, None) == INVALID
    assert "dense" in m.lib.pg_last_error(m.h).decode() and m.lib.pg_last_error(m.h).decode().startswith("pg_make_paths")
    assert step_bits(m, pkg) == before
    m.close()
    # ... and of the fp32 library: 2^25 + 1 knots over a length of 1 are 2^-25 apart, half an ulp of a float in [0.5, 1) (nothing is allocated: the refusal comes first)
    f = handle(pkg, "f32")
    before32 = step_bits(f, pkg)
    segs[0].length = 1.0; specs[0].n_knots = 2**25 + 1
    assert f.lib.pg_make_paths(f.h, 1, specs, 1, segs, 2**25 + 1, 1, None, None, None, None) == INVALID
    assert "dense" in f.lib.pg_last_error(f.h).decode()
    assert step_bits(f, pkg) == before32
    f.close()
    # a non-finite value in a segment that no spec refers to is not looked at
    m = handle(pkg)
    specs, segs0 = packed(m)
    segs = (L.pg_path_segment * (n_segs + 1))(*segs0)
    segs[n_segs] = m.lib.pg_default_path_segment(); segs[n_segs].length = np.nan; segs[n_segs].kappa0 = np.inf
    assert m.lib.pg_make_paths(m.h, N_PATH, specs, n_segs + 1, segs, cases.LMAX, 0, None, None, None, None) == OK, m.lib.pg_last_error(m.h)
    m.close()


def test_a_made_path_is_drivable(pkg, made):
    """Closed loop, a condition: the oval of the shared case (300 knots, the curvature of skidpadoval) made alone and installed at its constant V_ref = 6; four instances
    start on the path at a straight, a clothoid entry, the arc's middle and a clothoid exit (Uy = 0, e = 0, r = V kappa) and run 100 steps of 0.01 s in trajectory mode at
    the default horizon.  Every step of every instance ends SOLVED or SOLVED_UNVERIFIED and no instance leaves the tube's edges."""
    p, ref = cases.reference()
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 4)
    m.set_option("tracking_summary", 1)
    tubes, stats = m.make_paths([p[1]], n_knots=300, V_ref=6.0, pose=cases.POSES[1], closed=True, install=True)
    tube = tubes[0]
    assert tube.E.tobytes() == made[0][1, 4].tobytes()
    b = np.cumsum([0.0] + [g["length"] for g in p[1]])             # straight [b0, b1], clothoid in [b1, b2], arc [b2, b3], clothoid out [b3, b4]
    at = [0.5 * (b[0] + b[1]), 0.5 * (b[1] + b[2]), 0.5 * (b[2] + b[3]), 0.5 * (b[3] + b[4])]
    knots = [int(np.argmin(np.abs(tube.s - s))) for s in at]
    status, summary, first_exit = drive(m, tube, knots, 100)
    print("made oval: starts at knots", knots, "kappa", tube.kappa[knots], "max |e|", summary[:, 0], "min Ux", summary[:, 4], "first_exit", first_exit, "statuses", np.unique(status))
    assert np.all(pkg.is_solved(status)), np.unique(status)
    assert np.all(first_exit == -1), first_exit
    m.close()
