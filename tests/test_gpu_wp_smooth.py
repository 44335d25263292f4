"""pg_smooth_waypoints on the device against its twin (tests/wp_smooth_numpy.py) over the shared case of tests/wp_smooth_cases.py: 15 paths x 5 sets in one call.  The
scheme has only + - * / sqrt, every operation rounded once in both places, so waypoints_out and every stat are the twin's bit for bit; waypoints are doubles in both
libraries, so the fp32 library returns the same bytes.  Then independence of the batch, the NULL outputs, every refusal with its whole text, and the chain into
pg_fit_paths, pg_make_starts and a rollout."""
import os

import numpy as np
import pytest

import path_fit_numpy as fit_twin
import wp_smooth_cases as cases
import wp_smooth_numpy as twin
from conftest import ROOT
from path_libs import INVALID, OK, handle, lib, step_bits

pytestmark = pytest.mark.gpu

P, S = len(cases.paths()), len(cases.SETS)


def pack_sets(M, sets=cases.SETS):
    return M.pack_smooths([dict(s) for s in sets])


def pack_paths(order=range(P), gap=0):
    """(specs, waypoints): the paths of the case in `order`, `gap` waypoints no path refers to before each of them and after the last"""
    Lc = lib()
    ps = [cases.paths()[k] for k in order]
    total = sum(len(w) for _, _, w in ps) + gap * (len(ps) + 1)
    wps = (Lc.pg_waypoint * total)()
    specs = (Lc.pg_fit_spec * len(ps))()
    for i in range(total):                                          # (a stray waypoint: values the path side would refuse)
        wps[i].E, wps[i].N, wps[i].edge_L, wps[i].edge_R = np.nan, 1e300 + i, -1.0, 1.0
    at = gap
    for k, (_, closed, w) in enumerate(ps):
        specs[k].V_ref, specs[k].wp0, specs[k].n_wp, specs[k].n_knots, specs[k].closed = 6.0, at, len(w), 2, int(closed)
        for i, p in enumerate(w):
            wps[at + i].E, wps[at + i].N, wps[at + i].edge_L, wps[at + i].edge_R = p["E"], p["N"], p["edge_L"], p["edge_R"]
        at += len(w) + gap
    return specs, wps


def raw(m, specs, wps, sets, want_out=True, want_stats=True):
    Lc = lib()
    n, ns, nw = len(specs), len(sets), len(wps)
    out = (Lc.pg_waypoint * (ns * nw))() if want_out else None
    st = (Lc.pg_smooth_stats * (n * ns))() if want_stats else None
    rc = m.lib.pg_smooth_waypoints(m.h, n, specs, nw, wps, ns, sets, out, st)
    assert rc == OK, m.lib.pg_last_error(m.h)
    o = None if out is None else np.frombuffer(out, dtype=np.float64).reshape(ns, nw, 4).copy()
    s = None if st is None else np.frombuffer(st, dtype=np.float64).reshape(n, ns, 9).copy()
    return o, s


def expected():
    """(waypoints_out [S][n_wp_total][4], stats [P][S][9]) from the twin, for the paths packed in order without a gap"""
    ref = cases.reference()
    out = np.stack([np.concatenate([cases.as_bits(ref[p][k]) for p in range(P)]) for k in range(S)])
    st = np.array([[[ref[p][k]["stats"][f] for f in twin.STATS] for k in range(S)] for p in range(P)])
    return out, st


@pytest.fixture(scope="module")
def smoothed(pkg):
    """the shared case through the fp64 library, once"""
    m = handle(pkg)
    got = raw(m, *pack_paths(), pack_sets(type(m)))
    m.close()
    return got


def test_fp64_library_is_the_twin_bit_for_bit(smoothed):
    out, st = smoothed
    eo, es = expected()
    at = 0
    for p, (name, closed, w) in enumerate(cases.paths()):
        for k in range(S):
            a, b = out[k, at:at + len(w)], eo[k, at:at + len(w)]
            print(f"{name} set {k}: {int(np.count_nonzero(a != b))} of {a.size} output values differ from the twin; stats {[float('%.4g' % v) for v in st[p, k]]}")
            assert a.tobytes() == b.tobytes(), (name, k)
            for f, x, y in zip(twin.STATS, st[p, k], es[p, k]):
                assert x.tobytes() == y.tobytes(), (name, k, f, x, y)
        at += len(w)
    # lambda = 0 reproduces the input bit for bit, on the device as in the twin
    given = np.concatenate([[[q["E"], q["N"], q["edge_L"], q["edge_R"]] for q in w] for _, _, w in cases.paths()])
    assert out[0].tobytes() == given.tobytes()


def test_fp32_library_returns_the_same_bytes(pkg, smoothed):
    m = handle(pkg, "f32")
    o32, s32 = raw(m, *pack_paths(), pack_sets(type(m)))
    m.close()
    assert o32.tobytes() == smoothed[0].tobytes() and s32.tobytes() == smoothed[1].tobytes()


def test_a_pair_depends_on_its_own_path_and_set_alone(pkg, smoothed):
    out, st = smoothed
    m = handle(pkg)
    M = type(m)
    starts = np.concatenate([[0], np.cumsum([len(w) for _, _, w in cases.paths()])])
    for p in range(P):                                              # each pair alone
        specs, wps = pack_paths([p])
        for k in range(S):
            o1, s1 = raw(m, specs, wps, pack_sets(M, [cases.SETS[k]]))
            assert o1[0].tobytes() == out[k, starts[p]:starts[p + 1]].tobytes() and s1[0, 0].tobytes() == st[p, k].tobytes(), (p, k)
    # both libraries reversed, three stray waypoints before every path and after the last: the strays are copied as given into every block
    order = list(reversed(range(P)))
    specs, wps = pack_paths(order, gap=3)
    orev, srev = raw(m, specs, wps, pack_sets(M, list(reversed(cases.SETS))))
    given = np.frombuffer(wps, dtype=np.float64).reshape(len(wps), 4)
    touched = np.zeros(len(wps), dtype=bool)
    for i, p in enumerate(order):
        a = specs[i].wp0
        touched[a:a + specs[i].n_wp] = True
        for k in range(S):
            assert orev[S - 1 - k, a:a + specs[i].n_wp].tobytes() == out[k, starts[p]:starts[p + 1]].tobytes() and srev[i, S - 1 - k].tobytes() == st[p, k].tobytes(), (p, k)
    assert np.count_nonzero(~touched) == 3 * (P + 1)
    for k in range(S):
        assert orev[k, ~touched].tobytes() == given[~touched].tobytes(), k
    # the NULL outputs
    specs, wps = pack_paths()
    only_stats = raw(m, specs, wps, pack_sets(M), want_out=False)
    only_out = raw(m, specs, wps, pack_sets(M), want_stats=False)
    assert only_stats[0] is None and only_stats[1].tobytes() == st.tobytes() and only_out[1] is None and only_out[0].tobytes() == out.tobytes()
    # the Python method: the same waypoints and stats
    sm, stats = m.smooth_waypoints(cases.fit_paths_list(), [dict(s) for s in cases.SETS])
    assert stats.shape == (P, S) and stats.tobytes() == st.tobytes()
    for k in range(S):
        for p in range(P):
            mine = np.array([[q["E"], q["N"], q["edge_L"], q["edge_R"]] for q in sm[k][p]])
            assert mine.tobytes() == out[k, starts[p]:starts[p + 1]].tobytes(), (p, k)
    m.close()


def test_every_refusal_with_its_whole_text_leaves_the_handle_alone(pkg):
    m = handle(pkg)
    M = type(m)
    before = step_bits(m, pkg)
    small = [0, 1, 4, 5]                                            # open2 (waypoints 0-1), open3 (2-4), closed5 (5-9), closed6 (10-15)
    big = 2**31 - 1

    def call(n_path=None, n_sets=None, n_wp_total=None, spec=None, wp=None, sset=None, null=None):
        specs, wps = pack_paths(small)
        sets = pack_sets(M, cases.SETS[:2] + [cases.SETS[3]])
        if spec:
            setattr(specs[spec[0]], spec[1], spec[2])
        if wp:
            setattr(wps[wp[0]], wp[1], wp[2])
        if sset:
            f = getattr(sets[sset[0]], sset[1])
            if len(sset) == 4:
                f[sset[2]] = sset[3]
            else:
                setattr(sets[sset[0]], sset[1], sset[2])
        return m.lib.pg_smooth_waypoints(m.h, len(specs) if n_path is None else n_path, None if null == "specs" else specs, len(wps) if n_wp_total is None else n_wp_total,
                                         None if null == "waypoints" else wps, len(sets) if n_sets is None else n_sets, None if null == "sets" else sets, None, None)
    assert call() == OK and step_bits(m, pkg) == before
    nul = "null argument"
    cnt = "need n_path >= 1, n_sets >= 1 and n_wp_total >= 1"
    few = "an open path needs >= 2 waypoints, a closed one >= 5"
    rng = "the waypoints of a path must lie inside [0, n_wp_total)"
    fin = "a field of a waypoint is not finite"
    edg = "a waypoint needs edge_L > edge_R"
    same = "two neighbouring waypoints of a path lie at the same point (a chord must be finite and > 0)"
    lam = "lambda of a set is finite and >= 0"
    fac = "factor of a window is finite and >= 0"
    win = "a window of a set needs u_lo <= u_hi"
    refused = [
        (dict(null="specs"), nul), (dict(null="waypoints"), nul), (dict(null="sets"), nul), (dict(n_path=0), cnt), (dict(n_sets=0), cnt), (dict(n_wp_total=0), cnt),
        (dict(n_path=-1), cnt), (dict(n_path=big, n_sets=big), "n_path * n_sets must fit 31 bits"),
        (dict(spec=(0, "n_wp", 1)), few), (dict(spec=(2, "n_wp", 4)), few), (dict(spec=(1, "closed", 1)), few), (dict(spec=(3, "n_wp", 0)), few),
        (dict(spec=(0, "wp0", -1)), rng), (dict(spec=(0, "wp0", 16)), rng), (dict(spec=(3, "n_wp", 7)), rng), (dict(n_wp_total=15), rng), (dict(spec=(3, "n_wp", big)), rng),
        (dict(wp=(3, "E", np.nan)), fin), (dict(wp=(6, "N", np.inf)), fin), (dict(wp=(0, "edge_L", np.nan)), fin), (dict(wp=(15, "edge_R", -np.inf)), fin),
        (dict(wp=(7, "edge_L", -4.0)), edg), (dict(wp=(12, "edge_R", 9.0)), edg),
        (dict(spec=(1, "wp0", 1)), "the waypoint ranges of path 0 and path 1 overlap"), (dict(spec=(1, "n_wp", 4)), "the waypoint ranges of path 1 and path 2 overlap"),
        (dict(spec=(2, "wp0", 0)), "the waypoint ranges of path 0 and path 2 overlap"),
        (dict(sset=(1, "lam", -0.1)), lam), (dict(sset=(1, "lam", np.nan)), lam), (dict(sset=(0, "lam", np.inf)), lam),
        (dict(sset=(2, "factor", 0, -1.0)), fac), (dict(sset=(2, "factor", 1, np.inf)), fac), (dict(sset=(2, "factor", 1, np.nan)), fac),
        (dict(sset=(2, "u_lo", 0, 7.0)), win), (dict(sset=(2, "u_hi", 1, np.nan)), win),
        (dict(sset=(0, "n_win", 5)), "n_win of a set lies in [0, 4]"), (dict(sset=(0, "n_win", -1)), "n_win of a set lies in [0, 4]"),
        (dict(sset=(1, "reserved", 1)), "reserved of a set must be 0"),
    ]
    for kw, text in refused:
        assert call(**kw) == INVALID, kw
        assert m.lib.pg_last_error(m.h).decode() == "pg_smooth_waypoints: " + text, (kw, m.lib.pg_last_error(m.h))
        assert step_bits(m, pkg) == before, kw
    # two neighbouring waypoints at the same point: inside a path, and last-to-first on a closed one
    specs, wps = pack_paths(small)
    for a, b in ((3, 2), (9, 5)):
        assert call(wp=(a, "E", wps[b].E)) == OK                    # (only E equal: still apart)
    for a, b in ((3, 2), (9, 5)):
        specs, wps = pack_paths(small)
        wps[a].E, wps[a].N = wps[b].E, wps[b].N
        assert m.lib.pg_smooth_waypoints(m.h, 4, specs, len(wps), wps, 1, pack_sets(M, cases.SETS[:1]), None, None) == INVALID
        assert m.lib.pg_last_error(m.h).decode() == "pg_smooth_waypoints: " + same
        assert step_bits(m, pkg) == before
    # n_win = 0: the window slots are not looked at
    assert call(sset=(0, "u_lo", 0, np.nan)) == OK and call(sset=(0, "factor", 3, -1.0)) == OK

    # ---- after the launch: the message names path, set and waypoint ----
    def one(points, closed, s, path_before=True, first_set=cases.SETS[0]):
        ps = ([("pad", False, cases.paths()[1][2])] if path_before else []) + [("bad", closed, points)]
        Lc = lib()
        total = sum(len(w) for _, _, w in ps)
        wps = (Lc.pg_waypoint * total)(); specs = (Lc.pg_fit_spec * len(ps))()
        at = 0
        for k, (_, cl, w) in enumerate(ps):
            specs[k].V_ref, specs[k].wp0, specs[k].n_wp, specs[k].n_knots, specs[k].closed = 6.0, at, len(w), 2, int(cl)
            for i, q in enumerate(w):
                wps[at + i].E, wps[at + i].N, wps[at + i].edge_L, wps[at + i].edge_R = q["E"], q["N"], q["edge_L"], q["edge_R"]
            at += len(w)
        out = (Lc.pg_waypoint * (2 * total))()
        before_out = bytes(out)
        rc = m.lib.pg_smooth_waypoints(m.h, len(ps), specs, total, wps, 2, pack_sets(M, [first_set, s]), out, None)
        return rc, m.lib.pg_last_error(m.h).decode(), bytes(out) == before_out
    # chords of 1e-160 m: 1 / h^2 overflows, the first pivot is +Inf and the second Inf - Inf (the twin: [inf, nan, nan]) -- row 1 is waypoint 2
    # (under the identity, set 0 of the call, lambda a0 is 0 * Inf: that pair's first pivot is NaN already, and it is the first pair the host looks at)
    tiny = [cases.wp(k * 1e-160, 0.0) for k in range(5)]
    piv = twin.smooth(tiny, False, twin.smooth_set(lam=1.0))["pivots"]
    assert piv[0] == np.inf and np.isnan(piv[1]) and np.isnan(twin.smooth(tiny, False, twin.smooth_set())["pivots"][0])
    rc, text, untouched = one(tiny, False, twin.smooth_set(lam=1.0))
    assert rc == INVALID and text == "pg_smooth_waypoints: path 1, set 0, waypoint 1: a pivot of the factorisation is not > 0" and untouched, text
    rc, text, untouched = one(tiny, False, twin.smooth_set(lam=1.0), first_set=twin.smooth_set(lam=0.5))
    assert twin.smooth(tiny, False, twin.smooth_set(lam=0.5))["pivots"][0] == np.inf and np.isnan(twin.smooth(tiny, False, twin.smooth_set(lam=0.5))["pivots"][1])
    assert rc == INVALID and text == "pg_smooth_waypoints: path 1, set 0, waypoint 2: a pivot of the factorisation is not > 0" and untouched, text
    assert step_bits(m, pkg) == before
    # a tube 2e-19 m wide: the shift by c rounds both edges onto one double wherever the waypoint moved
    thin = [dict(q, edge_L=1e-19, edge_R=-1e-19) for q in cases.paths()[5][2]]
    r = twin.smooth(thin, True, twin.smooth_set(lam=1.0, keep_walls=True))
    first = int(np.argmax(~(r["edge_L"] > r["edge_R"])))
    assert not r["edge_L"][first] > r["edge_R"][first]
    rc, text, untouched = one(thin, True, twin.smooth_set(lam=1.0, keep_walls=True))
    assert rc == INVALID and text == f"pg_smooth_waypoints: path 1, set 1, waypoint {first}: edge_L <= edge_R after keep_walls" and untouched, text
    assert step_bits(m, pkg) == before
    rc, text, _ = one(thin, True, twin.smooth_set(lam=1.0))         # (without keep_walls the same tube is copied)
    assert rc == OK, text
    # coordinates at 2^53 + 1000, where a double's step is 2 m: the middle waypoint pinned by a window, lambda = 1e3 pulls waypoint 0 towards the line and it rounds
    # onto waypoint 1.  Every pivot is > 0 and every output finite (the twin), so this is the same-point refusal and no other
    B = 2.0 ** 53 + 1000.0
    far = [cases.wp(B, B), cases.wp(B + 2.0, B), cases.wp(B, B + 2.0)]
    fold = twin.smooth_set(lam=1e3, windows=[(1.5, 2.5, 0.0)])
    r = twin.smooth(far, False, fold)
    assert (r["E"][0], r["N"][0]) == (r["E"][1], r["N"][1]) and r["stats"]["chord_min"] == 0.0 and r["stats"]["pivot_min"] > 300 and np.all(np.isfinite(cases.as_bits(r)))
    rc, text, untouched = one(far, False, fold)
    assert rc == INVALID and text == "pg_smooth_waypoints: path 1, set 1, waypoint 0: this output waypoint and the next lie at the same point" and untouched, text
    assert step_bits(m, pkg) == before
    # a path that runs out and straight back, (0, 0), (1, 0), (0, 0): the natural spline through it has gamma_1 = -2 / (2 / 3) = -3 exactly, so its tangent at the
    # middle waypoint is -1 - ((1 (2 (-3) + 0)) / 6) = 0 exactly in E and 0 in N: no normal, 0 / 0, and keep_walls would store NaN edges (the twin divides by zero there).
    # lambda = 0: the only pivot is 2 / 3 and E, N are the input
    cusp = [cases.wp(0.0, 0.0), cases.wp(1.0, 0.0), cases.wp(0.0, 0.0)]
    S0 = twin.system([0.0, 1.0, 0.0], [0.0, 0.0, 0.0], False, twin.smooth_set())
    assert twin.gammas(S0, 3, False)[0] == [0.0, -3.0, 0.0]
    with pytest.raises(ZeroDivisionError):
        twin.smooth(cusp, False, twin.smooth_set(keep_walls=True))
    rc, text, untouched = one(cusp, False, twin.smooth_set(keep_walls=True))
    assert rc == INVALID and text == "pg_smooth_waypoints: path 1, set 1, waypoint 1: the output is not finite" and untouched, text
    assert step_bits(m, pkg) == before
    rc, text, _ = one(cusp, False, twin.smooth_set())               # (without keep_walls no normal is needed for the output: accepted)
    assert rc == OK, text
    # not pinned here: "the scratch of all pairs is more than the allocation arithmetic holds" needs n_sets * n_wp_total * 18 * 8 >= 2^62 with every set and waypoint
    # valid, that is, hundreds of gigabytes of input; every other text before the launch is above
    m.close()


def test_the_chain_into_fit_paths_starts_and_a_rollout(pkg):
    """skidpadoval under {identity, lambda = 0.1}, then ONE pg_fit_paths call over both blocks with install (set k's paths start k * n_wp_total further on), compared with
    the file's k_1pm at equal s / total as tests/test_wp_smooth_host.py does: the smoothed survey's max |kappa - file| is below a tenth of the interpolated one's.  Four
    instances placed by pg_make_starts on the smoothed path run 10 steps: every step solved, nobody leaves the tube.  Then the sign of keep_walls against k_project."""
    from test_path_fit_host import at_equal_fraction
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", "skidpadoval.npz")))
    V = pkg.vehicles
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 4)
    m.set_option("tracking_summary", 1)
    paths = [dict(waypoints=cases.golden("skidpadoval", True), closed=True, n_knots=1000, V_ref=6.0)]
    sm, stats = m.smooth_waypoints(paths, [V.smooth(), V.smooth(lam=0.1)])
    both = m.smoothed_fit_paths(paths, sm, 0) + m.smoothed_fit_paths(paths, sm, 1)
    tubes, closed, fs = m.fit_paths(both, install=True)
    err = []
    for t in tubes:
        r = dict(s=t.s, stats=dict(length=float(t.s[-1])))
        err.append(float(np.max(np.abs(t.kappa - at_equal_fraction(r, d["s_m"], d["k_1pm"])))))
    print(f"oval on the device: max |kappa - file| {err[0]:.3e} interpolated, {err[1]:.3e} smoothed at lambda = 0.1; dev_max {stats['dev_max'][0, 1]:.3e} m, "
          f"dev_rms {stats['dev_rms'][0, 1]:.3e} m, pivot_min {stats['pivot_min'][0, 1]:.3f}")
    assert err[1] < 0.1 * err[0] and stats["dev_max"][0, 1] < 1e-3 and stats["dev_max"][0, 0] == 0.0
    state, control, t0, toff = pkg.synthetic.config2_inputs(tubes[1], 4, seed=4)
    m.set_inputs(state, control, t0, time_offset=toff)
    m.set_trajectory_index(np.ones(4, dtype=np.int32))
    m.make_starts([V.start(s=(20.0, 150.0))], seed=3, B=4, install=True)
    status = np.zeros((10, 4), dtype=np.int32)
    for k in range(10):
        m.simulate_(1, dt=0.01)
        status[k] = m.solve_info()[0]
    summary, _, first_exit = m.tracking_summary()
    print("rollout on the smoothed oval: max |e|", summary[:, 0], "first_exit", first_exit, "statuses", np.unique(status))
    assert np.all(pkg.is_solved(status)), np.unique(status)
    assert np.all(first_exit == -1), first_exit
    m.close()
    # the sign: a path that runs north with one waypoint 0.5 m to the east.  Smoothing moves it west; k_project calls a car to the west of the path e > 0, left;
    # keep_walls brings both edges of a waypoint that moved left DOWN by what it moved, so the walls stay where they were
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 1)
    line = [V.waypoint(E=0.5 if i == 30 else 0.0, N=2.0 * i) for i in range(60)]
    sm, stats = m.smooth_waypoints([dict(waypoints=line)], [V.smooth(lam=1.0, keep_walls=True)])
    q = sm[0][0][30]
    assert q["E"] < 0.5 and q["edge_L"] < 4.0 and q["edge_R"] < -4.0 and q["edge_L"] - q["edge_R"] == pytest.approx(8.0, abs=1e-12)
    tubes, _, _ = m.fit_paths([dict(waypoints=sm[0][0], n_knots=120, V_ref=6.0)], install=True)
    m.step_(np.array([[-0.5, 30.0, 0.0, 6.0, 0.0, 0.0]]), np.zeros((1, 3)), np.array([5.0]), time_offset=np.zeros(1))
    sep = m.path_coordinates()
    print("a car 0.5 m west of a path that runs north: (s, e, dpsi) =", sep[0])
    assert 0.3 < sep[0, 1] < 0.7
    m.close()
