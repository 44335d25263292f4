"""pg_optimize_line on the device against its twin (tests/line_opt_numpy.py) over the shared case of tests/line_opt_cases.py: six paths, both sides of the 1024 rows the
kernel keeps in LDS, under four sets each.  The scheme has only + - * / sqrt and exact comparisons, every operation rounded once in both places, so waypoints_out and
every stat are the twin's bit for bit; waypoints are doubles in both libraries, so the fp32 library returns the same bytes.  Then a batch of 3 paths x 4 sets against the
single-pair calls, every refusal with its whole text, the sign of the normal against k_project, and the chain into pg_fit_paths and pg_plan_speeds."""
import numpy as np
import pytest

import line_opt_cases as cases
import line_opt_numpy as twin
from path_libs import INVALID, OK, handle, lib, step_bits

pytestmark = pytest.mark.gpu

NAMES = [name for name, _, _ in cases.paths()]


def pack_sets(M, sets):
    return M.pack_lines([dict(s, windows=[tuple(w) for w in s["windows"]]) for s in sets])


def pack_paths(names, gap=0):
    """(specs, waypoints): the named paths of the case, `gap` waypoints no path refers to before each of them and after the last"""
    Lc = lib()
    ps = [cases.path(n) for n in names]
    total = sum(len(w) for _, w in ps) + gap * (len(ps) + 1)
    wps = (Lc.pg_waypoint * total)()
    specs = (Lc.pg_fit_spec * len(ps))()
    for i in range(total):                                          # (a stray waypoint: values the path side would refuse)
        wps[i].E, wps[i].N, wps[i].edge_L, wps[i].edge_R = np.nan, 1e300 + i, -1.0, 1.0
    at = gap
    for k, (closed, w) in enumerate(ps):
        specs[k].V_ref, specs[k].wp0, specs[k].n_wp, specs[k].n_knots, specs[k].closed = 6.0, at, len(w), 2, int(closed)
        for i, p in enumerate(w):
            wps[at + i].E, wps[at + i].N, wps[at + i].edge_L, wps[at + i].edge_R = p["E"], p["N"], p["edge_L"], p["edge_R"]
        at += len(w) + gap
    return specs, wps


def raw(m, specs, wps, sets, want_out=True, want_stats=True):
    Lc = lib()
    n, ns, nw = len(specs), len(sets), len(wps)
    out = (Lc.pg_waypoint * (ns * nw))() if want_out else None
    st = (Lc.pg_line_stats * (n * ns))() if want_stats else None
    rc = m.lib.pg_optimize_line(m.h, n, specs, nw, wps, ns, sets, out, st)
    assert rc == OK, m.lib.pg_last_error(m.h)
    o = None if out is None else np.frombuffer(out, dtype=np.float64).reshape(ns, nw, 4).copy()
    s = None if st is None else np.frombuffer(st, dtype=np.float64).reshape(n, ns, 12).copy()
    return o, s


@pytest.fixture(scope="module")
def m64(pkg):
    m = handle(pkg)
    yield m
    m.close()


@pytest.fixture(scope="module")
def results(m64):
    """every path of the case under its four sets through the fp64 library, one call per path, computed as first asked for"""
    got = {}

    def run(name):
        if name not in got:
            got[name] = raw(m64, *pack_paths([name]), pack_sets(type(m64), cases.sets_for(name)))
        return got[name]
    return run


@pytest.mark.parametrize("name", NAMES)
def test_fp64_library_is_the_twin_bit_for_bit(results, name):
    out, st = results(name)
    ref = cases.reference(name)
    for k, r in enumerate(ref):
        a, b = out[k], cases.as_bits(r)
        print(f"{name} set {cases.SET_NAMES[k]}: {int(np.count_nonzero(a != b))} of {a.size} output values differ from the twin; stats {[float('%.4g' % v) for v in st[0, k]]}")
        assert a.tobytes() == b.tobytes(), (name, k)
        for f, x in zip(twin.STATS, st[0, k]):
            assert x.tobytes() == np.float64(r["stats"][f]).tobytes(), (name, k, f, x, r["stats"][f])
    # the set with tol stops early, where the twin stops
    assert st[0, 2, twin.STATS.index("iters_done")] == ref[2]["stats"]["iters_done"] < cases.sets_for(name)[2]["iters"]
    # the pinning window returns input bits
    closed, w = cases.path(name)
    given = np.array([[q["E"], q["N"], q["edge_L"], q["edge_R"]] for q in w])
    pinned = (ref[1]["U"] >= 10.0) & (ref[1]["U"] <= 20.0)
    assert pinned.any() and out[1][pinned].tobytes() == given[pinned].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_fp32_library_returns_the_same_bytes(pkg, results, name):
    m = handle(pkg, "f32")
    o32, s32 = raw(m, *pack_paths([name]), pack_sets(type(m), cases.sets_for(name)))
    m.close()
    assert o32.tobytes() == results(name)[0].tobytes() and s32.tobytes() == results(name)[1].tobytes()


def test_a_batch_of_three_paths_and_four_sets_equals_the_single_pair_calls(m64, results):
    m = m64
    M = type(m)
    names = list(cases.BATCH_PATHS)
    sets = cases.sets_for(names[0])
    assert all(cases.sets_for(n) == sets for n in names)
    # both libraries reversed, three stray waypoints before every path and after the last: the strays are copied as given into every block
    specs, wps = pack_paths(list(reversed(names)), gap=3)
    out, st = raw(m, specs, wps, pack_sets(M, list(reversed(sets))))
    given = np.frombuffer(wps, dtype=np.float64).reshape(len(wps), 4)
    touched = np.zeros(len(wps), dtype=bool)
    for i, name in enumerate(reversed(names)):
        a = specs[i].wp0
        touched[a:a + specs[i].n_wp] = True
        one_out, one_st = results(name)
        for k in range(4):
            assert out[3 - k, a:a + specs[i].n_wp].tobytes() == one_out[k].tobytes() and st[i, 3 - k].tobytes() == one_st[0, k].tobytes(), (name, k)
            pair_out, pair_st = raw(m, *pack_paths([name]), pack_sets(M, [sets[k]]))            # the pair alone
            assert pair_out[0].tobytes() == one_out[k].tobytes() and pair_st[0, 0].tobytes() == one_st[0, k].tobytes(), (name, k)
    assert np.count_nonzero(~touched) == 3 * 4
    for k in range(4):
        assert out[k, ~touched].tobytes() == given[~touched].tobytes(), k
    # the NULL outputs
    specs, wps = pack_paths(names)
    full = raw(m, specs, wps, pack_sets(M, sets))
    only_stats = raw(m, specs, wps, pack_sets(M, sets), want_out=False)
    only_out = raw(m, specs, wps, pack_sets(M, sets), want_stats=False)
    assert only_stats[0] is None and only_stats[1].tobytes() == full[1].tobytes() and only_out[1] is None and only_out[0].tobytes() == full[0].tobytes()
    # the Python method: the same waypoints and stats
    lines, stats = m.optimize_line(cases.fit_paths_list(names), [dict(s, windows=list(s["windows"])) for s in sets])
    assert stats.shape == (3, 4) and stats.tobytes() == full[1].tobytes()
    starts = np.concatenate([[0], np.cumsum([len(cases.path(n)[1]) for n in names])])
    for k in range(4):
        for p in range(3):
            mine = np.array([[q["E"], q["N"], q["edge_L"], q["edge_R"]] for q in lines[k][p]])
            assert mine.tobytes() == full[0][k, starts[p]:starts[p + 1]].tobytes(), (p, k)


def test_every_refusal_with_its_whole_text_leaves_the_handle_alone(pkg, m64):
    m = m64
    M = type(m)
    before = step_bits(m, pkg)
    names = ["open5", "closed5"]                                    # waypoints 0-4 and 5-9
    big = 2**31 - 1
    sets3 = cases.sets_for("open5")[:3]

    def call(n_path=None, n_sets=None, n_wp_total=None, spec=None, wp=None, sset=None, null=None):
        specs, wps = pack_paths(names)
        sets = pack_sets(M, sets3)
        if spec:
            setattr(specs[spec[0]], spec[1], spec[2])
        if wp:
            setattr(wps[wp[0]], wp[1], wp[2])
        if sset:
            if len(sset) == 4:
                getattr(sets[sset[0]], sset[1])[sset[2]] = sset[3]
            else:
                setattr(sets[sset[0]], sset[1], sset[2])
        return m.lib.pg_optimize_line(m.h, len(specs) if n_path is None else n_path, None if null == "specs" else specs, len(wps) if n_wp_total is None else n_wp_total,
                                      None if null == "waypoints" else wps, len(sets) if n_sets is None else n_sets, None if null == "sets" else sets, None, None)
    assert call() == OK and step_bits(m, pkg) == before
    nul = "null argument"
    cnt = "need n_path >= 1, n_sets >= 1 and n_wp_total >= 1"
    few = "an open path needs >= 2 waypoints, a closed one >= 5"
    rng = "the waypoints of a path must lie inside [0, n_wp_total)"
    fin = "a field of a waypoint is not finite"
    edg = "a waypoint needs edge_L > edge_R"
    same = "two neighbouring waypoints of a path lie at the same point (a chord must be finite and > 0)"
    win = "a window of a set needs u_lo <= u_hi"
    wmg = "the margin of a window is finite and >= 0"
    its = "iters of a set lies in [1, 4096]"
    res = "reserved of a set must be 0"
    refused = [
        (dict(null="specs"), nul), (dict(null="waypoints"), nul), (dict(null="sets"), nul), (dict(n_path=0), cnt), (dict(n_sets=0), cnt), (dict(n_wp_total=0), cnt),
        (dict(n_path=-1), cnt), (dict(n_path=big, n_sets=big), "n_path * n_sets must fit 31 bits"),
        (dict(spec=(0, "n_wp", 1)), few), (dict(spec=(1, "n_wp", 4)), few), (dict(spec=(1, "n_wp", 0)), few),
        (dict(spec=(0, "wp0", -1)), rng), (dict(spec=(0, "wp0", 10)), rng), (dict(spec=(1, "n_wp", 6)), rng), (dict(n_wp_total=9), rng), (dict(spec=(1, "n_wp", big)), rng),
        (dict(wp=(3, "E", np.nan)), fin), (dict(wp=(6, "N", np.inf)), fin), (dict(wp=(0, "edge_L", np.nan)), fin), (dict(wp=(9, "edge_R", -np.inf)), fin),
        (dict(wp=(7, "edge_L", -4.0)), edg), (dict(wp=(2, "edge_R", 9.0)), edg), (dict(wp=(6, "edge_L", -5.0)), edg),
        (dict(spec=(1, "wp0", 4)), "the waypoint ranges of path 0 and path 1 overlap"),
        (dict(sset=(1, "mu", 0.0)), "mu of a set is finite and > 0"), (dict(sset=(1, "mu", np.nan)), "mu of a set is finite and > 0"),
        (dict(sset=(0, "rho", -1.0)), "rho of a set is finite and > 0"), (dict(sset=(0, "rho", np.inf)), "rho of a set is finite and > 0"),
        (dict(sset=(2, "margin", -0.1)), "margin of a set is finite and >= 0"), (dict(sset=(2, "margin", np.nan)), "margin of a set is finite and >= 0"),
        (dict(sset=(0, "alpha_max", 0.0)), "alpha_max of a set is finite and > 0"), (dict(sset=(0, "alpha_max", np.inf)), "alpha_max of a set is finite and > 0"),
        (dict(sset=(2, "tol", -1e-9)), "tol of a set is finite and >= 0"), (dict(sset=(2, "tol", np.inf)), "tol of a set is finite and >= 0"),
        (dict(sset=(0, "iters", 0)), its), (dict(sset=(0, "iters", 4097)), its), (dict(sset=(0, "iters", -3)), its),
        (dict(sset=(1, "u_lo", 0, 13.0)), win), (dict(sset=(1, "u_hi", 1, np.nan)), win),
        (dict(sset=(1, "win_margin", 0, -1.0)), wmg), (dict(sset=(1, "win_margin", 1, np.inf)), wmg),
        (dict(sset=(0, "n_win", 5)), "n_win of a set lies in [0, 4]"), (dict(sset=(0, "n_win", -1)), "n_win of a set lies in [0, 4]"),
        (dict(sset=(1, "reserved", 0, 1)), res), (dict(sset=(2, "reserved", 1, -1)), res),
        # the box: open5's waypoint 0 has the edges 3 and -2; a margin of 2.6 leaves lo = 0.6 > hi = 0.4 there (set 2, the first pair the host reaches with it)
        (dict(sset=(2, "margin", 2.6)), "path 0, set 2, waypoint 0: the margins leave no room between the edges (lo > hi)"),
        # ... and a window with that margin over U in [5, 12] empties waypoint 2 of open5 (edges 3.5 and -3: 3.5 - 3.3 < -3 + 3.3)
        (dict(sset=(1, "win_margin", 0, 3.3)), "path 0, set 1, waypoint 2: the margins leave no room between the edges (lo > hi)"),
    ]
    for kw, text in refused:
        assert call(**kw) == INVALID, kw
        assert m.lib.pg_last_error(m.h).decode() == "pg_optimize_line: " + text, (kw, m.lib.pg_last_error(m.h))
        assert step_bits(m, pkg) == before, kw
    # two neighbouring waypoints at the same point: inside a path, and last-to-first on a closed one
    for a, b in ((3, 2), (9, 5)):
        specs, wps = pack_paths(names)
        wps[a].E, wps[a].N = wps[b].E, wps[b].N
        assert m.lib.pg_optimize_line(m.h, 2, specs, len(wps), wps, 1, pack_sets(M, sets3[:1]), None, None) == INVALID
        assert m.lib.pg_last_error(m.h).decode() == "pg_optimize_line: " + same
        assert step_bits(m, pkg) == before
    # n_win = 0: the window slots are not looked at; a pinned waypoint has no margin to fail
    assert call(sset=(0, "u_lo", 0, np.nan)) == OK and call(sset=(0, "win_margin", 3, -1.0)) == OK and call(sset=(1, "win_margin", 1, 100.0)) == OK

    # ---- after the launch: the message names path, set and waypoint, and nothing is copied out ----
    def one(points, closed, s, first_set=sets3[0]):
        ps = [(False, cases.path("open5")[1]), (closed, points)]
        Lc = lib()
        total = sum(len(w) for _, w in ps)
        wps = (Lc.pg_waypoint * total)(); specs = (Lc.pg_fit_spec * len(ps))()
        at = 0
        for k, (cl, w) in enumerate(ps):
            specs[k].V_ref, specs[k].wp0, specs[k].n_wp, specs[k].n_knots, specs[k].closed = 6.0, at, len(w), 2, int(cl)
            for i, q in enumerate(w):
                wps[at + i].E, wps[at + i].N, wps[at + i].edge_L, wps[at + i].edge_R = q["E"], q["N"], q["edge_L"], q["edge_R"]
            at += len(w)
        out = (Lc.pg_waypoint * (2 * total))()
        before_out = bytes(out)
        rc = m.lib.pg_optimize_line(m.h, len(ps), specs, total, wps, 2, pack_sets(M, [first_set, s]), out, None)
        return rc, m.lib.pg_last_error(m.h).decode(), bytes(out) == before_out
    wp = cases.shapes.wp
    # chords of 1e-160 m: 1 / h^3 overflows and the Hessian's places are Inf and NaN; the twin says which pivot is the first that is not > 0.  The plain set (set 0 of
    # the call) meets the same pivots, and it is the first pair of path 1 the host looks at
    tiny = [wp(k * 1e-160, 0.0) for k in range(5)]
    piv = twin.optimize(tiny, False, sets3[0])["pivots"]
    assert not np.all(piv > 0)
    rc, text, untouched = one(tiny, False, sets3[2])
    assert rc == INVALID and text == f"pg_optimize_line: path 1, set 0, waypoint {int(np.argmax(~(piv > 0)))}: a pivot of the factorisation is not > 0" and untouched, text
    assert step_bits(m, pkg) == before
    # a path that runs out and straight back, (0, 0), (1, 0), (0, 0): the chord from waypoint 0 to waypoint 2 is 0, the middle normal 0 / 0; row 0 holds it only in the
    # place (0, 1), so its own pivot is sound and the first that is not > 0 is row 1's
    cusp = [wp(0.0, 0.0), wp(1.0, 0.0), wp(0.0, 0.0)]
    with pytest.raises(ZeroDivisionError):                          # (the twin divides by that zero)
        twin.optimize(cusp, False, sets3[0])
    rc, text, untouched = one(cusp, False, sets3[0])
    assert rc == INVALID and text == "pg_optimize_line: path 1, set 0, waypoint 1: a pivot of the factorisation is not > 0" and untouched, text
    assert step_bits(m, pkg) == before
    # coordinates at 2^53 + 1000, where a double's step is 2 m: a left corner with legs of 2 m steps whose two waypoints before the turn have tubes that lie wholly to
    # the left of them (edge_R > 0), so their boxes force alpha into [1.5, 1.7] and [2.5, 3.1]; moved by that much along their normals both round onto (B - 2, B - 2).
    # Every pivot is > 0 and every output finite (the twin), so this is the same-point refusal and no other
    B = 2.0 ** 53 + 1000.0
    far = [wp(B, B - 4.0), wp(B, B - 2.0, 2.2, 1.0), wp(B, B, 3.6, 2.0), wp(B - 2.0, B), wp(B - 4.0, B)]
    s_far = twin.line_set(mu=1e-6, rho=0.1, margin=0.5, alpha_max=4.0, iters=50)
    r = twin.optimize(far, False, s_far)
    assert (r["E"][1], r["N"][1]) == (r["E"][2], r["N"][2]) == (B - 2.0, B - 2.0) and r["stats"]["chord_min"] == 0.0 and np.all(r["pivots"] > 0) and np.all(np.isfinite(cases.as_bits(r)))
    first = int(np.argmax(np.hypot(np.diff(r["E"]), np.diff(r["N"])) == 0.0))
    rc, text, untouched = one(far, False, s_far, first_set=dict(s_far, iters=49))      # (under the plain set, alpha_max 2, waypoint 2 of this path has lo = 2.5 > hi = 2)
    r49 = twin.optimize(far, False, dict(s_far, iters=49))      # (set 0 of the call: the same set one iteration short, the first pair of path 1 the host looks at)
    assert r49["stats"]["chord_min"] == 0.0 and np.all(r49["pivots"] > 0) and int(np.argmax(np.hypot(np.diff(r49["E"]), np.diff(r49["N"])) == 0.0)) == first
    assert rc == INVALID and text == f"pg_optimize_line: path 1, set 0, waypoint {first}: this output waypoint and the next lie at the same point" and untouched, text
    assert step_bits(m, pkg) == before
    # not pinned here: "the output is not finite" needs a finite input whose move overflows, which alpha_max times a unit normal cannot do below 1e308 m, and "the scratch
    # of all pairs is more than the allocation arithmetic holds" needs hundreds of gigabytes of input; every other text is above


def test_the_sign_of_the_normal_against_k_project(pkg):
    """A path that runs north and then turns left, 3 m between waypoints.  The least-bend line goes out, in, out: on the northward leg it moves to the outside, alpha = -2
    at waypoint 4 (east: E = +2 exactly, the normal there is (-1, 0)), and cuts the corner to the inside, alpha > 0 at waypoint 10 (south-west).  keep_walls shifts both
    edges by -alpha.  k_project, looking from the SURVEYED path, calls the car at the moved waypoint 4 e = -2, right, and the one at the moved corner e > 0, left: a
    positive alpha gives a positive e."""
    V = pkg.vehicles
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 1)
    w = [V.waypoint(E=0.0, N=3.0 * i) for i in range(11)] + [V.waypoint(E=-3.0 * i, N=30.0) for i in range(1, 11)]
    lines, stats = m.optimize_line([dict(waypoints=w)], [V.line(h_mean=3.0, keep_walls=True, iters=300)])
    out, apex = lines[0][0][4], lines[0][0][10]
    assert (out["E"], out["N"], out["edge_L"], out["edge_R"]) == (2.0, 12.0, 6.0, -2.0)
    a = 4.0 - apex["edge_L"]
    assert a > 0.5 and apex["E"] < 0.0 and apex["N"] < 30.0 and apex["edge_R"] == pytest.approx(-4.0 - a, abs=1e-12)
    assert stats["bend_out"][0, 0] < stats["bend_in"][0, 0]
    m.fit_paths([dict(waypoints=w, n_knots=240, V_ref=6.0)], install=True)
    e = []
    for q, t0 in ((out, 2.0), (apex, 5.0)):
        m.step_(np.array([[q["E"], q["N"], 0.0, 6.0, 0.0, 0.0]]), np.zeros((1, 3)), np.array([t0]), time_offset=np.zeros(1))
        e.append(float(m.path_coordinates()[0, 1]))
    print(f"seen from the surveyed path: the car at waypoint 4 moved by alpha = -2 has e = {e[0]:.3f}, the one at the corner moved by alpha = {a:.3f} has e = {e[1]:.3f}")
    assert e[0] == pytest.approx(-2.0, abs=0.05) and e[1] > 0.5
    m.close()


def test_the_chain_into_fit_paths_and_plan_speeds(pkg):
    """closed63: the surveyed line and the optimised one, each fitted by pg_fit_paths at 400 knots and planned by pg_plan_speeds under the default plan.  The lap time (t of
    the last knot) of the optimised line is below that of the input line: a strict comparison, both numbers come from the same existing makers."""
    V = pkg.vehicles
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 1)
    closed, w = cases.path("closed63")
    paths = [dict(waypoints=w, closed=True, n_knots=400, V_ref=6.0)]
    lines, stats = m.optimize_line(paths, [V.line(h_mean=3.74)])
    ref = twin.optimize(w, True, twin.line_set(**{k: v for k, v in V.line(h_mean=3.74).items()}))
    assert stats["bend_out"][0, 0] == ref["stats"]["bend_out"] and stats["r_prim"][0, 0] == ref["stats"]["r_prim"]
    tubes, cl, fs = m.fit_paths(paths + m.smoothed_fit_paths(paths, lines, 0))
    planned, ps = m.plan_speeds(tubes, [V.speed_plan()], closed=cl)
    t_in, t_out = float(planned[0].t[-1]), float(planned[1].t[-1])
    print(f"closed63: bend {stats['bend_in'][0, 0]:.4f} -> {stats['bend_out'][0, 0]:.4f}, {int(stats['n_active'][0, 0])} active, r_prim {stats['r_prim'][0, 0]:.2e}; "
          f"length {float(tubes[0].s[-1]):.2f} -> {float(tubes[1].s[-1]):.2f} m, max |kappa| {float(np.max(np.abs(tubes[0].kappa))):.4f} -> {float(np.max(np.abs(tubes[1].kappa))):.4f} 1/m, "
          f"planned lap {t_in:.3f} -> {t_out:.3f} s")
    assert t_out < t_in
    m.close()
