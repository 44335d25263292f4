"""The path refiner without a device: the numpy twin (tests/path_refine_numpy.py) on the shared case (tests/path_refine_cases.py) -- the identity, a refined
line-clothoid-arc-clothoid path against the path maker's twin asked for the denser knots directly, the two failures the knot-wise makers document
before and after refining, the Result rule of pg_plan_speeds on the sub-intervals --, and the Python mirror of pg_refine_paths (struct layouts, the default set, the
packer, the header's statement, the symbols, refine_parts against the twin on the edge values).  The measured values in the comments are those of this scheme in float64
(EXPERIMENTS 40)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import path_make_numpy as maker
import path_offset_numpy as offset_twin
import path_refine_cases as cases
import path_refine_numpy as twin
import speed_plan_numpy as speed_twin
import tube_clip_cases
import tube_clip_numpy as clip_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_identity_returns_the_source_and_every_set_keeps_the_source_knots():
    ch = cases.sources()
    for p in range(cases.N_PATH):
        n = cases.N_KNOTS[p]
        src = np.ascontiguousarray(ch[p][:, :n])
        for q in (0, 4):                                            # the identity, and a window beyond the path's end
            r = cases.reference()[p][q]
            assert twin.channels(r, n).tobytes() == src.tobytes(), (p, q)
            st = r["stats"]
            assert st["n_added"] == 0 and st["m_max"] == 1 and st["length"] == src[1, n - 1] - src[1, 0], (p, q)
        for q in (1, 2, 3):
            r = cases.reference()[p][q]
            at = np.array(r["o"])
            assert len(at) == n and at[0] == 0 and at[-1] == len(r["s"]) - 1 and r["stats"]["n_added"] == len(r["s"]) - n > 0
            assert np.ascontiguousarray(twin.channels(r, len(r["s"]))[:, at]).tobytes() == src.tobytes(), (p, q)
            assert np.all(np.diff(r["s"]) > 0) and np.all(np.diff(r["t"]) > 0), (p, q)


# measured on the CPU, max |refined - dense| over both paths below: psi 4.441e-16 rad, E 9.948e-14 m, N 5.684e-14 m.  The bars are 4 x these, for other libm builds
PSI_BAR, E_BAR, N_BAR = 4 * 4.441e-16, 4 * 9.948e-14, 4 * 5.684e-14


def test_refined_geometry_against_the_path_maker_asked_for_the_denser_knots():
    """Line, clothoid in, arc, clothoid out with every segment end on a source knot (2 m apart), refined by ds = 0.5 m (4 equal parts), against path_make_numpy asked for
    the 0.5 m knots directly -- the reference is the path maker's twin, never the refiner.  s is bit for bit in both paths: i ds and s_i + tau are exact multiples of 0.5.
    kappa and the edges: bit for bit on the dyadic path (curvatures k / 32, lengths 32 m: neither the maker's kappa0 + ((kappa1 - kappa0) u) / length nor the refiner's
    kappa_i + ((kappa_{i+1} - kappa_i) tau) / diff rounds); on the decimal path the two forms round differently and agree within 1 ulp -- of the value for the edges, of
    the path's largest |kappa| for kappa, which crosses zero."""
    seg = maker.segment
    paths = {"decimal": [seg(length=40.0), seg(length=30.0, kappa1=0.05), seg(length=30.0, kappa0=0.05, kappa1=0.05), seg(length=30.0, kappa0=0.05, kappa1=-0.02, edge_L1=5.1, edge_R1=-3.3)],
             "dyadic": [seg(length=40.0), seg(length=32.0, kappa1=0.0625), seg(length=32.0, kappa0=0.0625, kappa1=0.0625),
                        seg(length=32.0, kappa0=0.0625, kappa1=-0.03125, edge_L1=5.0, edge_R1=-3.0)]}
    for name, segs in paths.items():
        total = sum(g["length"] for g in segs)
        n, nd = int(total / 2.0) + 1, int(total / 0.5) + 1
        src = maker.make(segs, n, (3.0, -2.0, 0.4), 6.0)
        dense = maker.make(segs, nd, (3.0, -2.0, 0.4), 6.0)
        assert np.all(np.diff(src["s"]) == 2.0) and np.all(np.diff(dense["s"]) == 0.5)
        r = twin.refine(maker.channels(src, n), twin.refine_set(ds=0.5))
        assert len(r["s"]) == nd and r["stats"]["m_max"] == 4 and r["stats"]["ds_min"] == r["stats"]["ds_max"] == 0.5
        assert r["s"].tobytes() == dense["s"].tobytes(), name
        if name == "dyadic":
            assert all(r[c].tobytes() == dense[c].tobytes() for c in ("kappa", "edge_L", "edge_R")), name
        else:
            assert np.max(np.abs(r["kappa"] - dense["kappa"])) <= np.spacing(np.max(np.abs(dense["kappa"])))
            assert all(np.all(np.abs(r[c] - dense[c]) <= np.spacing(np.abs(dense[c]))) for c in ("edge_L", "edge_R"))
        d = {c: float(np.max(np.abs(r[c] - dense[c]))) for c in ("psi", "E", "N")}
        print(f"{name}: max |refined - dense| psi {d['psi']:.3e} rad, E {d['E']:.3e} m, N {d['N']:.3e} m; closure_pos_max {r['stats']['closure_pos_max']:.3e} m, "
              f"closure_psi_max {r['stats']['closure_psi_max']:.3e} rad")
        assert d["psi"] <= PSI_BAR and d["E"] <= E_BAR and d["N"] <= N_BAR, (name, d)
        # the source's E and N are its own psi and kappa integrated: the closures are rounding
        assert r["stats"]["closure_pos_max"] <= 1e-13 and r["stats"]["closure_psi_max"] <= 1e-14


# |length - trapezoid| of lane_change(0, 1.5, 212, 217) on the line with knots 10 m apart, measured (m): on the source, after refine_for(set, knots=10) and (knots=20)
LANE_CHANGE_ERROR = {"source": 1.272e-1, 10: 8.254e-11, 20: 2.274e-13}


def test_the_short_lane_change_is_no_longer_short(pkg):
    """DESIGN 4.21, "What the quadrature sees": the 1.5 m change over 5 m inside one 10 m interval of the shared straight line comes out 0.127 m short.  After
    refine_for(set, knots=10) -- the window (212, 217, 0.5): the interval 210 .. 220 m is cut into 20 parts and both window ends fall on knots -- the error is 8.3e-11 m.
    That is NOT below the 3e-11 m tests/test_path_offset_host.py pins for ten knots: that figure (2.6e-11 m) belongs to a 5 m change over 100 m, slope d' <= 0.094, and this
    manoeuvre has d' <= 0.56; in the window's own coordinate both are ten pieces of the same 4-point rule on sqrt(1 + d'^2), whose error grows with the slope (w (d1 / w)^2
    alone gives a factor 1.8, the higher orders the rest).  Twenty knots bring it to 2.3e-13 m.  A knot count whose spacing does not put the window's ends on knots does
    worse than ten (knots=12: 2.2e-9 m, the C2 joints of the window fall inside an interval)."""
    V = pkg.vehicles
    line = cases.documented_line()
    lane = V.lane_change(0.0, 1.5, 212.0, 217.0)
    S = offset_twin.offset_set(**lane)
    exact = cases.trapezoid_length(1.5, 212.0, 217.0, 390.0)
    err = {"source": abs(offset_twin.offset(line, S)["stats"]["length"] - exact)}
    for knots in (10, 20):
        rset = V.refine_for(lane, knots=knots)
        assert rset == V.refine(windows=[(212.0, 217.0, 5.0 / knots)])
        r = twin.refine(line, cases.as_twin_set(rset))
        assert len(r["s"]) == 40 + 2 * knots - 1 and r["stats"]["m_max"] == 2 * knots
        fine = offset_twin.offset(twin.channels(r, len(r["s"])), S)
        err[knots] = abs(fine["stats"]["length"] - exact)
        inside = (r["s"] >= 212.0) & (r["s"] <= 217.0)
        assert np.count_nonzero(inside) == knots + 1 and np.count_nonzero((fine["d"] > 0.0) & (fine["d"] < 1.5)) == knots - 1
    print("length error (m):", {k: f"{v:.3e}" for k, v in err.items()})
    assert abs(err["source"] - 0.127) < 1e-3                        # what tests/test_path_offset_host.py pins
    for k, v in err.items():
        assert v <= 2 * LANE_CHANGE_ERROR[k], (k, v)
    assert err[20] < 3e-11 < err[10] < 1e-9


def test_the_disc_between_two_knots_is_seen(pkg):
    """DESIGN 4.22, "What the knots see": the disc of R = 1.5 m between the line's knots at 210 and 220 m -- the one of tests/tube_clip_cases.py (set 11, at 214 m) and the
    one at 215 m the header names -- comes back side = 0.  refine_around turns the report row (or the obstacle itself) into a window; on the refined path the disc is
    seen, a side is decided, and the pass-by pass_by_around proposes clears it."""
    V = pkg.vehicles
    line = cases.documented_line()
    case_disc = tuple(float(v) for v in tube_clip_cases.obstacles()[8])
    o215 = V.obstacle_at(line, 215.0, 0.0, 1.5)
    for disc in (case_disc, (o215["E"], o215["N"], o215["radius"])):
        S = clip_twin.obstacle_set(first=0, count=1)
        row = clip_twin.clip(line, S, [disc])["report"][0]
        assert row["side"] == 0 and row["k_at"] in (21, 22)
        for rset in (V.refine_around(row, line, 0.5, 2.0, radius=1.5), V.refine_around(V.obstacle(*disc), line, 0.5, 2.0)):
            r = twin.refine(line, cases.as_twin_set(rset))
            fine = twin.channels(r, len(r["s"]))
            assert r["stats"]["m_max"] == 20 and len(r["s"]) in (59, 78)      # one interval cut, or the two a window round a knot reaches into
            c = clip_twin.clip(fine, S, [disc])
            seen = c["report"][0]
            assert seen["side"] != 0 and seen["k_last"] - seen["k_first"] >= 4 and c["stats"]["n_seen"] == 1 and c["stats"]["n_clip_L"] + c["stats"]["n_clip_R"] >= 5
            assert abs(seen["dist_at"]) <= 0.25 + 1e-9                  # a knot within half a spacing of the disc's centre
            by = V.pass_by_around(seen, fine, 10.0)
            assert by["d1"] != 0.0 and abs(by["d1"] - seen["a_at"]) > 1.5 and -4.0 < by["d1"] < 4.0      # the plateau clears the disc, inside the road
            # ... and the windows of the proposed pass-by are in the source's arc length: the refined path kept it
            assert 210.0 < by["s_b"] <= by["s_c"] < 220.0
    with pytest.raises(ValueError):
        V.refine_around(row, line, 0.5, 2.0)                        # a record with side = 0 does not carry the radius
    # a record with side != 0: from reach before the first to reach after the last seeing knot
    assert V.refine_around(seen, fine, 0.1, 1.0)["windows"] == [(float(fine[1, seen["k_first"]]) - 1.0, float(fine[1, seen["k_last"]]) + 1.0, 0.1)]


# measured on the planned oval below, over the sub-intervals: the largest |dt - (2 ds) / (V_j + V_{j+1})| (s) and |A_j - (W_{j+1} - W_j) / (2 ds)| (m/s^2)
RESULT_RULE_DT, RESULT_RULE_A = 5.065e-15, 2.336e-13


def test_the_result_rule_of_the_speed_planner_holds_on_the_sub_intervals(pkg):
    oval = maker.make(pkg.vehicles.oval_segments(40.0, 14.5, 15.0), 65, (12.0, -30.0, 0.5), 6.0)
    plan = speed_twin.plan(oval["s"], oval["kappa"], speed_twin.speed_plan(mu_scale=0.5, V_max=14.0, V_start=3.0), pkg.X1())
    print("planned V", float(plan["V"].min()), float(plan["V"].max()), "limiters", sorted(set(int(v) for v in plan["limiter"])))
    assert np.ptp(plan["V"]) > 3.0
    src = dict(oval); src.update(V=plan["V"], A=plan["A"], t=plan["t"])
    r = twin.refine(maker.channels(src, 65), twin.refine_set(ds=0.5))
    at = np.array(r["o"])
    assert r["t"][at].tobytes() == plan["t"].tobytes() and r["V"][at].tobytes() == plan["V"].tobytes()      # the source knots keep their time
    ds = np.diff(r["s"]); W = r["V"] * r["V"]
    e_dt = float(np.max(np.abs(np.diff(r["t"]) - (2.0 * ds) / (r["V"][:-1] + r["V"][1:]))))
    e_A = float(np.max(np.abs(r["A"][:-1] - (W[1:] - W[:-1]) / (2.0 * ds))))
    print(f"Result rule on {len(ds)} sub-intervals: max |dt - 2 ds / (V_j + V_j+1)| {e_dt:.3e} s, max |A_j - dW / (2 ds)| {e_A:.3e} m/s^2")
    assert e_dt <= 4 * RESULT_RULE_DT and e_A <= 4 * RESULT_RULE_A


def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_struct_layouts_and_the_default_set(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_refine_set) == 128 and C.sizeof(L.pg_refine_stats) == 64
    assert [getattr(L.pg_refine_set, n).offset for n, _ in L.pg_refine_set._fields_] == [0, 8, 40, 72, 104]
    assert [getattr(L.pg_refine_stats, n).offset for n, _ in L.pg_refine_stats._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56]
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.REFINE_STATS_DTYPE.itemsize == 64 and mpc_mod.REFINE_STATS_DTYPE.names == tuple(n for n, _ in L.pg_refine_stats._fields_)
    V = pkg.vehicles
    inf = math.inf
    assert V.refine() == dict(ds=inf, windows=[]) and V.refine(2.0, [(1, 2, 0.5)]) == dict(ds=2.0, windows=[(1.0, 2.0, 0.5)])
    with pytest.raises(ValueError):
        V.refine(windows=[(0, 1, 0.1)] * 5)
    assert V.refine_for(V.pass_by(3, 120, 135, 145, 160), knots=5) == V.refine(windows=[(120.0, 135.0, 3.0), (145.0, 160.0, 3.0)]) and V.refine_for(V.lane(3.5)) == V.refine()
    M = pkg.BatchedTrajectoryTrackingMPC
    arr = M.pack_refines([V.refine(), V.refine(0.5, [(1, 2, 0.25), (5, 9, 0.125)])])
    assert arr[0].ds == inf and list(arr[0].s_lo) == [inf] * 4 and list(arr[0].ds_w) == [inf] * 4 and list(arr[0].reserved) == [0.0] * 3
    assert arr[1].ds == 0.5 and list(arr[1].s_lo) == [1.0, 5.0, inf, inf] and list(arr[1].s_hi) == [2.0, 9.0, inf, inf] and list(arr[1].ds_w) == [0.25, 0.125, inf, inf]
    nan = math.nan
    for bad in (dict(ds=0.0), dict(ds=-1.0), dict(ds=nan), dict(windows=[(nan, 2, 1)]), dict(windows=[(-inf, 2, 1)]), dict(windows=[(2, 2, 1)]), dict(windows=[(2, inf, 1)]),
                dict(windows=[(1, 2, 0)]), dict(windows=[(1, 2, inf)]), dict(windows=[(1, 2, nan)]), dict(windows=[(inf, nan, 1)])):
        with pytest.raises(ValueError):
            M.pack_refines([V.refine(), V.refine(**bad)])
    with pytest.raises(ValueError):
        M.pack_refines([])
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_refine_set
        f.restype = L.pg_refine_set; f.argtypes = []
        assert bytes(f()) == bytes(arr[0])


def test_header_symbols_and_lists_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_refine_set;              /* 128 bytes */" in hdr and "} pg_refine_stats;            /* 64 bytes */" in hdr
    assert "pg_refine_set pg_default_refine_set(void);" in hdr
    for line_ in ("int pg_refine_paths(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,",
                  "int32_t n_sets, const pg_refine_set* sets, int32_t Lmax_out, int32_t install,",
                  "int32_t* L_out, int32_t* closed_out, double* channels_out, pg_refine_stats* stats);"):
        assert line_ in hdr, line_
    for phrase in ("Parts ", "Offsets ", "Sub-knot ", "Heading ", "Position ", "Speed ", "Stats ", "m_i = ceil(q), refused unless q <= 4096", "psi(v) = psi_i + (v (a + (v b)))",
                   "((tau / diff) cE)", "Left out: coarsening", "tests/path_refine_numpy.py"):
        assert phrase in hdr, phrase
    assert {"pg_refine_paths", "pg_default_refine_set"} <= set(pkg.SYMBOLS)
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_refine_set) == 128 && sizeof(pg_refine_stats) == 64" in api
    for doc in ("README.md", "DESIGN.md", "EXPERIMENTS.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "refine_paths" in open(os.path.join(ROOT, doc)).read(), doc
    assert "### 4.23" in open(os.path.join(ROOT, "DESIGN.md")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_path_refine" in check_f32_purity.TIME_KERNELS and "k_path_refine" in check_f32_purity.__doc__
    assert "pg_path_refine.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert "pg_path_refine.hip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read() and "k_path_refine" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()
    assert '#include "pg_path_refine.hip"' in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()


def test_refine_parts_in_python_against_the_twin_on_the_edge_values(pkg):
    V = pkg.vehicles
    up = lambda x: math.nextafter(x, math.inf)
    inf = math.inf

    def both(rset, diff, u_lo, u_hi):
        m = V.refine_parts(rset, diff, u_lo, u_hi)
        try:
            assert twin.parts(cases.as_twin_set(rset), diff, u_lo, u_hi) == m
        except ValueError:
            assert m == V.REFINE_M_MAX + 1 == 4097
        return m

    assert both(V.refine(), 10.0, 0.0, 10.0) == 1
    assert both(V.refine(ds=2.0), 2.0, 4.0, 6.0) == 1               # diff == w
    assert both(V.refine(ds=2.0), up(2.0), 4.0, up(6.0)) == 2       # a hair above
    assert both(V.refine(ds=0.3), 2.0, 0.0, 2.0) == 7
    # a window that touches an interval's end without entering it: [10, 20] against the intervals [0, 10] and [20, 30]; one ulp inside cuts
    w = V.refine(windows=[(10.0, 20.0, 1.0)])
    assert both(w, 10.0, 0.0, 10.0) == 1 and both(w, 10.0, 20.0, 30.0) == 1 and both(w, 10.0, 10.0, 20.0) == 10
    assert both(w, up(10.0), 0.0, up(10.0)) == 11 and both(V.refine(windows=[(10.0, up(20.0), 1.0)]), 10.0, 20.0, 30.0) == 10
    # overlapping windows: the smallest spacing; an unused slot and a window beyond the end do nothing
    assert both(V.refine(ds=5.0, windows=[(0.0, 50.0, 2.0), (5.0, 8.0, 0.5)]), 10.0, 0.0, 10.0) == 20
    assert both(V.refine(windows=[(inf, inf, 0.01), (500.0, 600.0, 0.01)]), 10.0, 0.0, 10.0) == 1
    # m_i = 4096 is the most; 4097 is refused (the count stands for every larger one)
    assert both(V.refine(ds=1.0), 4096.0, 0.0, 4096.0) == 4096 and both(V.refine(ds=1.0), up(4096.0), 0.0, up(4096.0)) == 4097
    assert both(V.refine(ds=1.0), 4097.0, 0.0, 4097.0) == 4097 and both(V.refine(ds=1e-9), 1.0, 0.0, 1.0) == 4097
    M = pkg.BatchedTrajectoryTrackingMPC
    ch = np.zeros((1, 10, 3)); ch[0, 1] = [0.0, 4096.0, 8193.0]
    L = np.array([3], dtype=np.int32)
    assert list(M.refined_lengths(L, ch, M.pack_refines([V.refine(), V.refine(ds=4096.0), V.refine(windows=[(0.0, 1.0, 1.0)])]))) == [3, 4, 4098]
    with pytest.raises(ValueError, match="path 0, set 0, interval 1"):
        M.refined_lengths(L, ch, M.pack_refines(V.refine(ds=1.0)))


def test_the_shared_case_is_what_its_docstring_says():
    ch = cases.sources()
    ref = cases.reference()
    assert ch.shape == (3, 10, 258) and (cases.N_KNOTS[0] - 1 + 255) // 256 == 2
    assert [[len(r["s"]) for r in row] for row in ref] == [[258, 515, 262, 368, 258], [65, 833, 96, 230, 65], [2, 257, 641, 513, 2]]
    assert max(len(r["s"]) for row in ref for r in row) <= cases.LMAX_OUT
    assert np.ptp(ch[0, 2, :258]) > 3.0 and np.ptp(ch[0, 8, :258]) > 0.5 and ref[0][0]["stats"]["closure_pos_max"] > 1e-4      # the kappa step at the line's end
    assert [m for m in ref[0][2]["m"] if m > 1] == [5] and sorted(set(ref[0][3]["m"])) == [1, 3, 4]
