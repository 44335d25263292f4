"""pg_tune_smoothing on the device against its twin (tests/wp_tune_numpy.py) over the shared case of tests/wp_tune_cases.py: 8 paths x 8 sets in one call.  The scheme
has only + - * / sqrt and exact comparisons, so every field of tune, stats and waypoints_out is the twin's bit for bit, in both libraries; the final solve is
pg_smooth_waypoints' own under the chosen weight, on the same handle.  Then independence of the batch, repeated calls, the NULL outputs, every refusal with its whole
text, the refusal after the launch, and the oval's bracket."""
import numpy as np
import pytest

import wp_smooth_cases as smooth_cases
import wp_smooth_numpy as smooth_twin
import wp_tune_cases as cases
import wp_tune_numpy as twin
from path_libs import INVALID, OK, handle, lib, step_bits

pytestmark = pytest.mark.gpu

P, S = len(cases.paths()), len(cases.SETS)


def pack_sets(M, sets=cases.SETS):
    return M.pack_tunes([cases.as_vehicle_set(t) for t in sets])


def pack_paths(order=range(P), gap=0, paths=None):
    """(specs, waypoints): the paths of the case in `order`, `gap` waypoints no path refers to before each of them and after the last"""
    Lc = lib()
    ps = [cases.paths()[k] for k in order] if paths is None else paths
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


def raw(m, specs, wps, sets, want=(True, True, True)):
    Lc = lib()
    n, ns, nw = len(specs), len(sets), len(wps)
    out = (Lc.pg_waypoint * (ns * nw))() if want[0] else None
    st = (Lc.pg_smooth_stats * (n * ns))() if want[1] else None
    tn = (Lc.pg_tune_stats * (n * ns))() if want[2] else None
    rc = m.lib.pg_tune_smoothing(m.h, n, specs, nw, wps, ns, sets, out, st, tn)
    assert rc == OK, m.lib.pg_last_error(m.h)
    o = None if out is None else np.frombuffer(out, dtype=np.float64).reshape(ns, nw, 4).copy()
    s = None if st is None else np.frombuffer(st, dtype=np.float64).reshape(n, ns, 9).copy()
    t = None if tn is None else np.frombuffer(tn, dtype=np.float64).reshape(n, ns, 9).copy()
    return o, s, t


def expected():
    """(waypoints_out [S][n_wp_total][4], stats [P][S][9], tune [P][S][9]) from the twin, for the paths packed in order without a gap"""
    ref = cases.reference()
    out = np.stack([np.concatenate([smooth_cases.as_bits(ref[p][k]["solve"]) for p in range(P)]) for k in range(S)])
    st = np.array([[[ref[p][k]["solve"]["stats"][f] for f in smooth_twin.STATS] for k in range(S)] for p in range(P)])
    tn = np.array([[[ref[p][k]["stats"][f] for f in twin.TUNE_STATS] for k in range(S)] for p in range(P)])
    return out, st, tn


STARTS = np.concatenate([[0], np.cumsum([len(w) for _, _, w in cases.paths()])])


@pytest.fixture(scope="module")
def tuned(pkg):
    """the shared case through the fp64 library, once"""
    m = handle(pkg)
    got = raw(m, *pack_paths(), pack_sets(type(m)))
    m.close()
    return got


def test_fp64_library_is_the_twin_bit_for_bit(tuned):
    out, st, tn = tuned
    eo, es, et = expected()
    for p, (name, closed, w) in enumerate(cases.paths()):
        for k in range(S):
            a, b = out[k, STARTS[p]:STARTS[p + 1]], eo[k, STARTS[p]:STARTS[p + 1]]
            print(f"{name} set {k}: {int(np.count_nonzero(a != b))} of {a.size} output values differ from the twin; tune {[float('%.6g' % v) for v in tn[p, k]]} "
                  f"(twin {[float('%.6g' % v) for v in et[p, k]]})")
            for f, x, y in zip(twin.TUNE_STATS, tn[p, k], et[p, k]):
                assert x.tobytes() == y.tobytes(), (name, k, f, x, y)
            assert a.tobytes() == b.tobytes(), (name, k)
            for f, x, y in zip(smooth_twin.STATS, st[p, k], es[p, k]):
                assert x.tobytes() == y.tobytes(), (name, k, f, x, y)
            # Result: rms_lo is the dev_rms of the final solve, and it keeps the target wherever the verdict is >= 0
            assert tn[p, k, 3] == st[p, k, 1] and tn[p, k, 0] == tn[p, k, 1]
            if tn[p, k, 5] >= 0:
                assert st[p, k, 1] <= cases.SETS[k]["target"], (name, k)
    assert tn[2, 2, 5] == 0.0 and tn[2, 2, 6] == 7.0                # closed5 under the narrow set: stopped early, after 7 of 8 rounds
    assert np.all(tn[0, :, 5] == 1.0) and np.all(tn[0, :, 6] == 1.0) and np.all(st[0, :, 1] == 0.0)      # two waypoints: verdict +1 in round 0


def test_fp32_library_returns_the_same_bytes(pkg, tuned):
    m = handle(pkg, "f32")
    got = raw(m, *pack_paths(), pack_sets(type(m)))
    m.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, tuned))


def test_the_final_solve_is_pg_smooth_waypoints_under_the_chosen_weight(pkg, tuned):
    m = handle(pkg)
    M = type(m)
    Lc = lib()
    specs, wps = pack_paths()
    out, st, tn = raw(m, specs, wps, pack_sets(M))                  # on this handle, the one pg_smooth_waypoints is called on below
    assert all(a.tobytes() == b.tobytes() for a, b in zip((out, st, tn), tuned))
    for k in range(S):                                              # one pg_smooth_waypoints call per tune set: a smoothing set per path, its weight the chosen one
        b = cases.SETS[k]["base"]
        sets = M.pack_smooths([dict(b, windows=list(b["windows"]), lam=float(tn[p, k, 0])) for p in range(P)])
        o = (Lc.pg_waypoint * (P * len(wps)))(); s = (Lc.pg_smooth_stats * (P * P))()
        assert m.lib.pg_smooth_waypoints(m.h, P, specs, len(wps), wps, P, sets, o, s) == OK, m.lib.pg_last_error(m.h)
        o = np.frombuffer(o, dtype=np.float64).reshape(P, len(wps), 4); s = np.frombuffer(s, dtype=np.float64).reshape(P, P, 9)
        for p in range(P):
            assert o[p, STARTS[p]:STARTS[p + 1]].tobytes() == out[k, STARTS[p]:STARTS[p + 1]].tobytes() and s[p, p].tobytes() == st[p, k].tobytes(), (p, k)
    m.close()


def test_a_pair_depends_on_its_own_path_and_set_alone_and_calls_repeat(pkg, tuned):
    out, st, tn = tuned
    m = handle(pkg)
    M = type(m)
    again = raw(m, *pack_paths(), pack_sets(M))                     # a repeated call on another handle: the same bits
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, tuned))
    for p in range(P):                                              # each pair alone
        specs, wps = pack_paths([p])
        for k in range(S):
            o1, s1, t1 = raw(m, specs, wps, pack_sets(M, [cases.SETS[k]]))
            assert o1[0].tobytes() == out[k, STARTS[p]:STARTS[p + 1]].tobytes() and s1[0, 0].tobytes() == st[p, k].tobytes() and t1[0, 0].tobytes() == tn[p, k].tobytes(), (p, k)
    # both libraries reversed, three stray waypoints before every path and after the last: the strays are copied as given into every block
    order = list(reversed(range(P)))
    specs, wps = pack_paths(order, gap=3)
    orev, srev, trev = raw(m, specs, wps, pack_sets(M, list(reversed(cases.SETS))))
    given = np.frombuffer(wps, dtype=np.float64).reshape(len(wps), 4)
    touched = np.zeros(len(wps), dtype=bool)
    for i, p in enumerate(order):
        a = specs[i].wp0
        touched[a:a + specs[i].n_wp] = True
        for k in range(S):
            assert orev[S - 1 - k, a:a + specs[i].n_wp].tobytes() == out[k, STARTS[p]:STARTS[p + 1]].tobytes(), (p, k)
            assert srev[i, S - 1 - k].tobytes() == st[p, k].tobytes() and trev[i, S - 1 - k].tobytes() == tn[p, k].tobytes(), (p, k)
    assert np.count_nonzero(~touched) == 3 * (P + 1)
    for k in range(S):
        assert orev[k, ~touched].tobytes() == given[~touched].tobytes(), k
    # the NULL outputs
    specs, wps = pack_paths()
    for j in range(3):
        want = tuple(i == j for i in range(3))
        got = raw(m, specs, wps, pack_sets(M), want)
        assert [g is None for g in got] == [not w for w in want] and got[j].tobytes() == tuned[j].tobytes()
    # the Python method: the same waypoints, stats and tune stats
    sm, stats, tune = m.tune_smoothing(cases.fit_paths_list(), [cases.as_vehicle_set(t) for t in cases.SETS])
    assert stats.shape == (P, S) and stats.tobytes() == st.tobytes() and tune.shape == (P, S) and tune.tobytes() == tn.tobytes()
    assert tune.dtype.names == twin.TUNE_STATS
    for k in range(S):
        for p in range(P):
            mine = np.array([[q["E"], q["N"], q["edge_L"], q["edge_R"]] for q in sm[k][p]])
            assert mine.tobytes() == out[k, STARTS[p]:STARTS[p + 1]].tobytes(), (p, k)
    m.close()


def test_the_ovals_bracket_is_the_twins(pkg):
    """skidpadoval to 1.6e-5 m rms between 1e-4 and 1e2 in two rounds: on the build container the twin ends on [0.09474635256553755, 0.1], consistent with EXPERIMENTS
    41 (lambda = 0.1 gives rms 1.6e-5 m).  The assertion is against the twin."""
    ref = cases.oval_reference()
    m = handle(pkg)
    name, closed, w = cases.paths()[-1]
    sm, stats, tune = m.tune_smoothing([dict(waypoints=w, closed=closed)], [cases.as_vehicle_set(cases.OVAL)])
    m.close()
    print(f"oval: bracket [{tune['lo'][0, 0]!r}, {tune['hi'][0, 0]!r}], dev_rms {stats['dev_rms'][0, 0]:.4e} m; the twin [{ref['stats']['lo']!r}, {ref['stats']['hi']!r}]")
    for f in twin.TUNE_STATS:
        assert tune[f][0, 0].tobytes() == np.float64(ref["stats"][f]).tobytes(), f
    assert tune["verdict"][0, 0] == 0.0 and stats["dev_rms"][0, 0] <= 1.6e-5 < tune["rms_hi"][0, 0]


def test_every_refusal_with_its_whole_text_leaves_the_handle_alone(pkg):
    m = handle(pkg)
    M = type(m)
    before = step_bits(m, pkg)
    small = [0, 1, 2]                                               # open2 (waypoints 0-1), open3 (2-4), closed5 (5-9)
    big = 2**31 - 1

    def call(n_path=None, n_sets=None, n_wp_total=None, spec=None, wp=None, sset=None, base=None, null=None):
        specs, wps = pack_paths(small)
        sets = pack_sets(M, [cases.SETS[0], cases.SETS[3]])
        if spec:
            setattr(specs[spec[0]], spec[1], spec[2])
        if wp:
            setattr(wps[wp[0]], wp[1], wp[2])
        if sset:
            setattr(sets[sset[0]], sset[1], sset[2])
        if base:
            if len(base) == 4:
                getattr(sets[base[0]].base, base[1])[base[2]] = base[3]
            else:
                setattr(sets[base[0]].base, base[1], base[2])
        return m.lib.pg_tune_smoothing(m.h, len(specs) if n_path is None else n_path, None if null == "specs" else specs, len(wps) if n_wp_total is None else n_wp_total,
                                       None if null == "waypoints" else wps, len(sets) if n_sets is None else n_sets, None if null == "sets" else sets, None, None, None)
    assert call() == OK and step_bits(m, pkg) == before
    nul = "null argument"
    cnt = "need n_path >= 1, n_sets >= 1 and n_wp_total >= 1"
    few = "an open path needs >= 2 waypoints, a closed one >= 5"
    rng = "the waypoints of a path must lie inside [0, n_wp_total)"
    fin = "a field of a waypoint is not finite"
    edg = "a waypoint needs edge_L > edge_R"
    lam = "lambda of a set is finite and >= 0"
    fac = "factor of a window is finite and >= 0"
    win = "a window of a set needs u_lo <= u_hi"
    tgt = "target of a set is finite and > 0"
    bnd = "the bounds of a set are finite with 0 < lambda_lo < lambda_hi"
    rnd = "rounds of a set lies in [1, 8]"
    refused = [
        (dict(null="specs"), nul), (dict(null="waypoints"), nul), (dict(null="sets"), nul), (dict(n_path=0), cnt), (dict(n_sets=0), cnt), (dict(n_wp_total=0), cnt),
        (dict(n_path=-1), cnt), (dict(n_path=big, n_sets=big), "n_path * n_sets must fit 31 bits"),
        (dict(spec=(0, "n_wp", 1)), few), (dict(spec=(2, "n_wp", 4)), few), (dict(spec=(1, "closed", 1)), few),
        (dict(spec=(0, "wp0", -1)), rng), (dict(spec=(0, "wp0", 10)), rng), (dict(spec=(2, "n_wp", 6)), rng), (dict(n_wp_total=9), rng), (dict(spec=(2, "n_wp", big)), rng),
        (dict(wp=(3, "E", np.nan)), fin), (dict(wp=(6, "N", np.inf)), fin), (dict(wp=(0, "edge_L", np.nan)), fin), (dict(wp=(9, "edge_R", -np.inf)), fin),
        (dict(wp=(7, "edge_L", -4.0)), edg),
        (dict(spec=(1, "wp0", 1)), "the waypoint ranges of path 0 and path 1 overlap"), (dict(spec=(1, "n_wp", 4)), "the waypoint ranges of path 1 and path 2 overlap"),
        (dict(base=(1, "lam", -0.1)), lam), (dict(base=(1, "lam", np.nan)), lam),
        (dict(base=(1, "factor", 0, -1.0)), fac), (dict(base=(1, "u_lo", 0, 7.0)), win), (dict(base=(0, "n_win", 5)), "n_win of a set lies in [0, 4]"),
        (dict(base=(0, "reserved", 1)), "reserved of a set must be 0"),
        (dict(base=(0, "lam", 0.1)), "base.lambda of a set must be 0 (the weight is what the call chooses)"),
        (dict(sset=(0, "target", 0.0)), tgt), (dict(sset=(1, "target", -1.0)), tgt), (dict(sset=(0, "target", np.nan)), tgt), (dict(sset=(0, "target", np.inf)), tgt),
        (dict(sset=(0, "lambda_lo", 0.0)), bnd), (dict(sset=(0, "lambda_lo", -1.0)), bnd), (dict(sset=(0, "lambda_lo", 1e2)), bnd), (dict(sset=(0, "lambda_lo", 1e3)), bnd),
        (dict(sset=(1, "lambda_hi", np.inf)), bnd), (dict(sset=(1, "lambda_hi", np.nan)), bnd), (dict(sset=(1, "lambda_lo", np.nan)), bnd),
        (dict(sset=(0, "rounds", 0)), rnd), (dict(sset=(1, "rounds", 9)), rnd), (dict(sset=(1, "rounds", -1)), rnd),
        (dict(sset=(1, "reserved", 1)), "reserved of a set must be 0"),
    ]
    for kw, text in refused:
        assert call(**kw) == INVALID, kw
        assert m.lib.pg_last_error(m.h).decode() == "pg_tune_smoothing: " + text, (kw, m.lib.pg_last_error(m.h))
        assert step_bits(m, pkg) == before, kw
    specs, wps = pack_paths(small)                                  # two neighbouring waypoints at the same point
    wps[3].E, wps[3].N = wps[2].E, wps[2].N
    assert m.lib.pg_tune_smoothing(m.h, 3, specs, len(wps), wps, 1, pack_sets(M, cases.SETS[:1]), None, None, None) == INVALID
    assert m.lib.pg_last_error(m.h).decode() == "pg_tune_smoothing: two neighbouring waypoints of a path lie at the same point (a chord must be finite and > 0)"
    assert step_bits(m, pkg) == before

    # ---- after the launch: a pivot that is not > 0 at a candidate; the message names path, set and round, and nothing is copied out.  The input is the one
    # tests/test_gpu_wp_smooth.py builds: chords of 1e-160 m, 1 / h^2 overflows, the first pivot is +Inf and the second Inf - Inf at every lambda > 0 ----
    tiny = [smooth_cases.wp(k * 1e-160, 0.0) for k in range(5)]
    piv = smooth_twin.smooth(tiny, False, smooth_twin.smooth_set(lam=1e-4))["pivots"]
    assert piv[0] == np.inf and np.isnan(piv[1])
    with pytest.raises(ArithmeticError):
        twin.tune(tiny, False, cases.SETS[0])
    specs, wps = pack_paths(paths=[cases.paths()[1], ("bad", False, tiny)])
    Lc = lib()
    out = (Lc.pg_waypoint * (2 * len(wps)))(); st = (Lc.pg_smooth_stats * 4)(); tn = (Lc.pg_tune_stats * 4)()
    blank = (bytes(out), bytes(st), bytes(tn))
    rc = m.lib.pg_tune_smoothing(m.h, 2, specs, len(wps), wps, 2, pack_sets(M, [cases.SETS[1], cases.SETS[0]]), out, st, tn)
    text = m.lib.pg_last_error(m.h).decode()
    assert rc == INVALID and text == "pg_tune_smoothing: path 1, set 0, round 0: a pivot of the factorisation is not > 0 at a candidate", text
    assert (bytes(out), bytes(st), bytes(tn)) == blank and step_bits(m, pkg) == before
    # not pinned here: "the scratch of all pairs is more than the allocation arithmetic holds" needs hundreds of gigabytes of valid input
    m.close()
