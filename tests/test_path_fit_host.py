"""The path fitter without a device: the numpy twin (tests/path_fit_numpy.py) against scipy's cubic splines, against circles (sign and order of convergence), against the
project's own generator and against the recorded paths; and the Python mirror of pg_fit_paths (struct layouts, defaults, every ValueError of the packer, the header's
statement, the symbols, the purity list).  The measured values in the comments are those of this scheme in float64 (EXPERIMENTS 32)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import path_fit_cases as cases
import path_fit_numpy as twin
import path_make_numpy as maker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin ----
def test_second_derivatives_against_scipy():
    interpolate = pytest.importorskip("scipy.interpolate")
    p = cases.paths()
    for k, closed in ((0, False), (1, True), (2, True), (3, True), (4, False), (5, False)):
        r = twin.fit(p[k], 5, 6.0, closed)
        E = np.array([w["E"] for w in p[k]]); N = np.array([w["N"] for w in p[k]])
        x = np.concatenate([[0.0], np.cumsum(r["h"])])              # the cumulative chord parameter
        if closed:
            cs = interpolate.CubicSpline(x, np.stack([np.append(E, E[0]), np.append(N, N[0])], axis=1), bc_type="periodic")
            M = cs(x[:-1], 2)
        else:
            cs = interpolate.CubicSpline(x, np.stack([E, N], axis=1), bc_type="natural")
            M = cs(x, 2)
        scale = float(np.max(np.abs(M)))
        worst = max(float(np.max(np.abs(M[:, 0] - r["M_E"]))), float(np.max(np.abs(M[:, 1] - r["M_N"]))))
        print(f"path {k}: largest |M - scipy| {worst:.3e}, max |M| {scale:.3e}")      # measured: at most 4.2e-12 of max |M| (path 4)
        assert worst <= 1e-9 * scale, k


def test_circle_sign_and_convergence():
    pos, kap = {}, {}
    for n in (16, 32, 64):
        for sign in (+1, -1):
            r = twin.fit(cases.circle(n, sign), 200, 6.0, True)
            assert np.all(r["kappa"] > 0) if sign > 0 else np.all(r["kappa"] < 0), (n, sign)      # counter-clockwise: a left turn, +1 / R
            assert r["stats"]["turn"] == pytest.approx(sign * twin.TWO_PI, abs=1e-12) and r["stats"]["closure_pos"] == 0.0
            radius = np.hypot(r["E"] - cases.CIRCLE_C[0], r["N"] - cases.CIRCLE_C[1])
            pos[n, sign] = float(np.max(np.abs(radius - cases.CIRCLE_R))); kap[n, sign] = float(np.max(np.abs(r["kappa"] - sign / cases.CIRCLE_R)))
    for sign in (+1, -1):
        for a, b in ((16, 32), (32, 64)):
            print(f"circle {a} -> {b} waypoints (sign {sign:+d}): position error {pos[a, sign]:.3e} -> {pos[b, sign]:.3e} (x {pos[a, sign] / pos[b, sign]:.2f}), "
                  f"curvature error {kap[a, sign]:.3e} -> {kap[b, sign]:.3e} (x {kap[a, sign] / kap[b, sign]:.2f})")      # measured x 16.47, 16.12 and x 4.08, 4.02
            assert pos[a, sign] >= 10.0 * pos[b, sign] and kap[a, sign] >= 3.0 * kap[b, sign], (a, b, sign)


def at_equal_fraction(r, s_ref, y_ref):
    """y_ref (given at s_ref) at the knots of r, at equal s / total"""
    return np.interp(r["s"] / r["s"][-1] * s_ref[-1], s_ref, y_ref)


def test_against_the_projects_own_generator(pkg):
    m = maker.make(pkg.vehicles.oval_segments(40.0, 14.5, 15.0), 300)
    wps = [twin.waypoint(E=m["E"][i], N=m["N"][i]) for i in range(0, 299, 4)]      # every 4th knot; knot 299 is knot 0 again
    r = twin.fit(wps, 300, 6.0, True)
    length = abs(r["stats"]["length"] - m["stats"]["length"]) / m["stats"]["length"]
    kappa = float(np.max(np.abs(r["kappa"] - m["kappa"])))
    position = float(np.max(np.hypot(r["E"] - m["E"], r["N"] - m["N"])))
    print(f"oval from every 4th of 300 knots: relative length error {length:.3e}, largest |kappa| difference {kappa:.3e} 1/m, largest position difference {position:.3e} m")
    assert length <= 2 * 1.091e-6                                   # measured 1.091e-06
    assert kappa <= 2 * 1.900e-3                                    # measured 1.900e-03 (the curvature of the clothoid oval has corners; 1 / 14.5 = 6.9e-2)
    assert position <= 2 * 1.024e-3                                 # measured 1.024e-03 m
    assert r["stats"]["closure_pos"] == 0.0 and abs(r["stats"]["closure_psi"]) < 1e-12


# (path, closed): measured largest |psi - file| (rad), |kappa - file| (1/m)
RECORDED = {("skidpadoval", True): (1.221e-3, 1.781e-2), ("flidpadoval", True): (1.246e-3, 1.817e-2), ("newskidpadoval", True): (3.140e-4, 5.030e-3),
            ("vail", False): (5.072e-6, 1.876e-4), ("variable_speed", False): (1.593e-2, 1.942e-2)}      # (variable_speed: 28 knots about 2 m apart)


@pytest.mark.parametrize("name,closed", list(RECORDED))
def test_against_the_recorded_files(pkg, name, closed):
    """Every knot of the file as a waypoint (a closed file's repeated last knot dropped), fitted at the file's own knot count, against the file's psi_rad and k_1pm at equal
    s / total.  The files hold rounded positions 0.1-0.24 m apart: an interpolating spline differentiates that rounding twice, which is what the curvature figures show."""
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", name + ".npz")))
    n = len(d["s_m"])
    r = twin.fit(pkg.vehicles.waypoints_from_tube(d, 1, closed), n, 6.0, closed)
    dpsi = r["psi"] - at_equal_fraction(r, d["s_m"], d["psi_rad"])
    dpsi = dpsi - round(float(dpsi[0]) / twin.TWO_PI) * twin.TWO_PI  # (the file's heading may start on another turn)
    psi = float(np.max(np.abs(dpsi))); kappa = float(np.max(np.abs(r["kappa"] - at_equal_fraction(r, d["s_m"], d["k_1pm"]))))
    print(f"{name}: {n} knots, length {r['stats']['length']:.5f} m (file {d['s_m'][-1]:.5f}), largest |psi - file| {psi:.3e} rad, |kappa - file| {kappa:.3e} 1/m "
          f"(file max |kappa| {np.max(np.abs(d['k_1pm'])):.3e}), s_err_max {r['stats']['s_err_max']:.1e}")
    assert psi <= 2 * RECORDED[name, closed][0] and kappa <= 2 * RECORDED[name, closed][1]


def test_the_shared_case_is_what_its_docstring_says():
    ref = cases.reference()
    assert [len(r["s"]) for r in ref] == cases.N_KNOTS and max(cases.N_KNOTS) <= cases.LMAX and len(ref) == cases.N_ENTRIES
    assert [len(p) for p in cases.paths()] == [2, 3, 24, 24, 300, 9]
    assert np.all(ref[0]["kappa"] == 0.0) and ref[0]["stats"]["length"] == pytest.approx(5.0, rel=1e-14) and np.all(ref[0]["M_E"] == 0.0)
    raw = ref[3]["psi_raw"]
    assert raw[2] > 3.1 and raw[3] < -3.1 and np.all(np.diff(ref[3]["psi"]) > 0)      # the jump lies between knots 2 and 3, and the unwrap removes it
    assert ref[3]["stats"]["turn"] == pytest.approx(twin.TWO_PI, abs=1e-12) and ref[4]["stats"]["turn"] == pytest.approx(-twin.TWO_PI, abs=1e-12)
    assert np.all(ref[3]["kappa"] > 0) and np.all(ref[4]["kappa"] < 0)
    assert len(ref[5]["l"]) == 299 and len(ref[6]["l"]) == 8
    assert ref[6]["stats"]["chord_min"] == pytest.approx(0.3) and ref[6]["stats"]["chord_max"] == pytest.approx(9.0)
    for r, closed in zip(ref, cases.CLOSED):
        assert (r["stats"]["closure_pos"] == 0.0) == bool(closed)
        assert r["stats"]["s_err_max"] <= 1e-11 * r["stats"]["length"]      # measured: at most 1.3e-12 m (entry 2, 40 knots over three spans of 10 m)
        assert np.all(np.diff(r["s"]) > 0) and np.all(r["edge_L"] > r["edge_R"])


# ---- the mirror ----
def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_struct_layouts_and_defaults(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_waypoint) == 32 and C.sizeof(L.pg_fit_spec) == 24 and C.sizeof(L.pg_fit_stats) == 80
    assert [getattr(L.pg_waypoint, n).offset for n, _ in L.pg_waypoint._fields_] == [0, 8, 16, 24]
    assert [getattr(L.pg_fit_spec, n).offset for n, _ in L.pg_fit_spec._fields_] == [0, 8, 12, 16, 20]
    assert [n for n, _ in L.pg_fit_stats._fields_][:6] == [n for n, _ in L.pg_path_stats._fields_]
    assert [getattr(L.pg_fit_stats, n).offset for n, _ in L.pg_fit_stats._fields_] == list(range(0, 80, 8))
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.FIT_STATS_DTYPE.itemsize == 80 and mpc_mod.FIT_STATS_DTYPE.names[6:] == ("chord_min", "chord_max", "s_err_max", "reserved")
    assert pkg.vehicles.waypoint() == dict(E=0.0, N=0.0, edge_L=4.0, edge_R=-4.0) == twin.waypoint()
    assert pkg.vehicles.waypoint(E=3, edge_R=-1)["edge_R"] == -1.0
    with pytest.raises(KeyError):
        pkg.vehicles.waypoint(psi=0.1)
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_waypoint
        f.restype = L.pg_waypoint; f.argtypes = []
        r = f()
        assert [getattr(r, n) for n, _ in L.pg_waypoint._fields_] == [0.0, 0.0, 4.0, -4.0]


def test_header_symbols_and_purity_list_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_waypoint;              /* 32 bytes */" in hdr and "} pg_fit_spec;              /* 24 bytes */" in hdr and "} pg_fit_stats;             /* 80 bytes */" in hdr
    assert "/* { 0, 0, 4, -4 }" in hdr and "pg_waypoint pg_default_waypoint(void);" in hdr
    assert "int pg_fit_paths(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints, int32_t Lmax," in hdr
    assert "                 int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_fit_stats* stats);" in hdr
    for phrase in ("Spans ", "Spline ", "Cubic ", "Lengths ", "Knots ", "Channels ", "Unwrap ", "Sherman-Morrison", "gamma = -b_0", "exactly three Newton steps", "ceil(n_span / 256)",
                   "atan2(-E', N')", "6.283185307179586", "tests/path_fit_numpy.py"):
        assert phrase in hdr, phrase
    assert "pg_*" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_exports.map")).read()
    assert {"pg_fit_paths", "pg_default_waypoint"} <= set(pkg.SYMBOLS)
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_waypoint) == 32 && sizeof(pg_fit_spec) == 24 && sizeof(pg_fit_stats) == 80" in api
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "fit_paths" in open(os.path.join(ROOT, doc)).read(), doc
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_path_fit" in check_f32_purity.TIME_KERNELS and "k_path_fit" in check_f32_purity.__doc__
    assert "pg_path_fit.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert "pg_path_fit.hip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()


def test_waypoints_from_tube(pkg):
    V = pkg.vehicles
    tube = pkg.load_path_fixture("skidpadoval")
    n = len(tube)
    w = V.waypoints_from_tube(tube, closed=True)
    assert len(w) == n - 1 and w[0] == V.waypoint(E=tube.E[0], N=tube.N[0], edge_L=tube.edge_L[0], edge_R=tube.edge_R[0]) and w[-1]["E"] == tube.E[n - 2]
    w16 = V.waypoints_from_tube(tube, every=16, closed=True)
    assert len(w16) == math.ceil((n - 1) / 16) and w16[1]["N"] == tube.N[16]
    open_ = V.waypoints_from_tube(tube, every=16)
    assert open_[-1]["E"] == tube.E[-1] and len(open_) == math.ceil(n / 16) + ((n - 1) % 16 != 0)
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", "vail.npz")))
    assert V.waypoints_from_tube(d, 4)[1] == V.waypoint(E=d["posE_m"][4], N=d["posN_m"][4], edge_L=d["edgeL_m"][4], edge_R=d["edgeR_m"][4])
    for bad in (0, 1.5, -2):
        with pytest.raises(ValueError):
            V.waypoints_from_tube(tube, every=bad)


def test_the_packer_refuses_what_the_library_refuses(pkg):
    M = pkg.BatchedTrajectoryTrackingMPC
    wp = pkg.vehicles.waypoint
    tri = [wp(E=0, N=0), wp(E=10, N=0), wp(E=4, N=8)]
    good = [dict(waypoints=tri[:2], n_knots=2), dict(waypoints=tri, n_knots=40, V_ref=3.0, closed=True)]
    specs, wps, Lmax = M.pack_fit_specs(good)
    assert Lmax == 40 and len(wps) == 5
    assert [(s.V_ref, s.wp0, s.n_wp, s.n_knots, s.closed) for s in specs] == [(6.0, 0, 2, 2, 0), (3.0, 2, 3, 40, 1)]
    assert M.pack_fit_specs(good, Lmax=64)[2] == 64
    L = lib_mod()
    assert len(M.pack_fit_specs([dict(waypoints=[L.pg_waypoint(0, 0, 4, -4), L.pg_waypoint(1, 0, 4, -4)], n_knots=2)])[1]) == 2
    for bad in (dict(E=math.nan), dict(N=math.inf), dict(edge_L=math.nan), dict(edge_R=-math.inf), dict(edge_L=-4.0), dict(edge_L=-5.0), dict(E=4.0, N=8.0), dict(E=0.0, N=0.0)):
        with pytest.raises(ValueError):                             # (the last two: the point of waypoint 2 before it, of waypoint 0 -- last-to-first on the closed path)
            M.pack_fit_specs([good[0], dict(waypoints=tri + [wp(**{**dict(E=2.0, N=3.0), **bad})], n_knots=9, closed=True)])
    for path in (dict(waypoints=tri, n_knots=1), dict(waypoints=tri, n_knots=2.5), dict(waypoints=tri[:1], n_knots=5), dict(waypoints=tri[:2], n_knots=5, closed=True),
                 dict(waypoints=tri, n_knots=2, closed=True), dict(waypoints=tri, n_knots=5, V_ref=0.0), dict(waypoints=tri, n_knots=5, V_ref=-1.0),
                 dict(waypoints=tri, n_knots=5, V_ref=math.inf), dict(waypoints=tri, n_knots=5, V_ref=math.nan), dict(waypoints=tri), dict(n_knots=5),
                 dict(waypoints=tri, n_knots=5, pose=(0, 0, 0)), dict(waypoints=[wp(), wp(E=1e-170)], n_knots=2), dict(waypoints=[wp(), wp(E=1e-29)], n_knots=100),
                 dict(waypoints=[wp(), wp(E=1e31)], n_knots=5)):
        with pytest.raises(ValueError):
            M.pack_fit_specs([path])
    with pytest.raises(ValueError, match="dense"):
        M.pack_fit_specs([dict(waypoints=tri, n_knots=2**21 + 2)], precision="f32")
    M.pack_fit_specs([dict(waypoints=tri, n_knots=2**21 + 1)], precision="f32"); M.pack_fit_specs([dict(waypoints=tri, n_knots=2**21 + 2)])
    for kw in (dict(Lmax=39), dict(Lmax=40.5), dict(Lmax=2**31)):
        with pytest.raises(ValueError):
            M.pack_fit_specs(good, **kw)
    with pytest.raises(ValueError):
        M.pack_fit_specs([])
    with pytest.raises(KeyError):
        M.pack_fit_specs([dict(waypoints=[dict(x=1.0), wp(E=1)], n_knots=2)])
