"""The path maker without a device: the numpy twin (tests/path_make_numpy.py) against closed forms -- circle, clothoid (Fresnel integrals), the closure of ovals, the
dE/ds = -sin psi, dN/ds = cos psi convention, the lane change --, and the Python mirror of pg_make_paths (struct layouts, defaults, builders, every ValueError of the
packers, the header's statement, the export map, the purity list).  The measured values in the comments are those of this scheme in float64."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import path_make_cases as cases
import path_make_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def knots_for(segs, ds):
    return max(2, math.ceil(sum(g["length"] for g in segs) / ds) + 1)


# ---- the twin against closed forms ----
def test_circle_against_cos_and_sin(pkg):
    segs = pkg.vehicles.circle_segments(7.0)
    r = twin.make(segs, knots_for(segs, 0.5))
    th = r["s"] / 7.0                                               # psi0 = 0: the path leaves (0, 0) towards +N and turns left, around (-7, 0)
    err = float(np.max(np.hypot(r["E"] - 7.0 * (np.cos(th) - 1.0), r["N"] - 7.0 * np.sin(th))))
    print("circle of radius 7 at ds 0.5: largest distance to the closed form", err)      # measured 7.6e-15
    assert err < 1e-12
    assert np.all(r["kappa"] == 1.0 / 7.0) and r["stats"]["closure_pos"] < 1e-12


def test_clothoid_against_the_fresnel_integrals(pkg):
    from scipy.special import fresnel
    L, k1 = 20.0, 0.2
    a = math.sqrt(math.pi * L / k1)                                 # psi = k1 s^2 / (2 L) = (pi / 2) (s / a)^2
    for ds, bound in ((0.25, 1e-12), (1.0, 1e-12), (2.0, 1e-9)):    # measured 7.5e-15, 4.5e-14, 1.2e-11: the quadrature error shows at the spacing of variable_speed
        r = twin.make([pkg.vehicles.path_segment(length=L, kappa1=k1)], knots_for([dict(length=L)], ds))
        S, Cf = fresnel(r["s"] / a)
        err = float(np.max(np.hypot(r["E"] + a * S, r["N"] - a * Cf)))
        print(f"20 m clothoid to 0.2 1/m at ds {ds}: largest distance to the Fresnel integrals {err:.3e}")
        assert err < bound, ds
        assert r["psi"][-1] == pytest.approx(0.5 * k1 * L, rel=1e-15) and r["kappa"][-1] == k1


def test_ovals_close(pkg):
    worst = 0.0
    for straight, radius, clothoid in ((30.0, 8.0, 6.0), (50.0, 20.0, 15.0), (10.0, 5.0, 0.0)):
        segs = pkg.vehicles.oval_segments(straight, radius, clothoid)
        assert len(segs) == (8 if clothoid else 4)
        for ds in (0.25, 1.0, 2.0):
            st = twin.make(segs, knots_for(segs, ds))["stats"]
            worst = max(worst, st["closure_pos"])
            assert st["closure_pos"] <= 1e-12, (straight, radius, clothoid, ds)
            assert st["closure_psi"] == 0, (straight, radius, clothoid, ds)
            assert st["kappa_abs_max"] == pytest.approx(1.0 / radius, rel=1e-15)
    print("ovals: largest closure_pos", worst)                      # measured 5.0e-14


def test_positions_follow_minus_sin_and_cos_of_psi(pkg):
    p, ref = cases.reference()
    for k in (1, 2, 3, 4):
        r = ref[k]
        ds = np.diff(r["s"])
        mid = 0.5 * (r["psi"][1:] + r["psi"][:-1])
        # (E, N)' / ds of an interval is the mean of (-sin psi, cos psi) over it, and every heading of the interval lies within var = max |kappa| ds of every other
        # and of their mean `mid`: each component is within var of its value at mid, and the chord is shorter than the arc by at most var^2 / 2
        var = max(max(abs(g["kappa0"]), abs(g["kappa1"])) for g in p[k]) * ds
        dE = np.diff(r["E"]) / ds; dN = np.diff(r["N"]) / ds
        assert np.all(np.abs(dE + np.sin(mid)) <= var + 1e-12), k
        assert np.all(np.abs(dN - np.cos(mid)) <= var + 1e-12), k
        assert np.all(np.abs(np.hypot(dE, dN) - 1.0) <= 0.5 * var * var + 1e-12), k
        assert np.max(np.abs(np.sin(mid))) > 2 * var.max()         # (the sign of the sine is visible: -sin and +sin are further apart than the bound)
    # the line leaves its pose along (-sin psi0, cos psi0)
    r = twin.make(pkg.vehicles.line_segments(10.0), 11, pose=(3.0, 4.0, 0.7))
    assert np.max(np.abs(r["E"] - (3.0 - r["s"] * math.sin(0.7)))) < 1e-14 and np.max(np.abs(r["N"] - (4.0 + r["s"] * math.cos(0.7)))) < 1e-14
    assert np.all(r["psi"] == 0.7) and np.all(r["t"] == r["s"] / 6.0) and np.all(r["V"] == 6.0) and np.all(r["A"] == 0.0)


def test_lane_change_reaches_the_offset_and_keeps_the_heading(pkg):
    V = pkg.vehicles
    assert V.LANE_CHANGE_TOL == 1e-11
    for offset, length in ((3.5, 20.0), (3.5, 60.0), (-3.5, 40.0), (0.5, 8.0)):
        segs = V.lane_change_segments(offset, length)
        assert len(segs) == 4 and all(g["length"] == length / 4 for g in segs)
        k = segs[0]["kappa1"]
        assert [(g["kappa0"], g["kappa1"]) for g in segs] == [(0.0, k), (k, 0.0), (0.0, -k), (-k, 0.0)] and k * offset > 0
        r = twin.make(segs, knots_for(segs, 0.25))
        shift = -(r["E"][-1])                                       # psi0 = 0: left is -E
        print(f"lane change of {offset} m in {length} m: peak curvature {k:.6f}, shift - offset {shift - offset:.3e}, turn {r['stats']['turn']:.3e}")
        assert abs(shift - offset) <= V.LANE_CHANGE_TOL
        # the four heading changes cancel exactly in the bounds (a + a - a - a from psi0 = 0); the last knot adds the roundings of its own closed form: a few ulp of the peak heading
        assert abs(r["stats"]["turn"]) <= 4 * 2.0 ** -52 * abs(k) * length / 4
    with pytest.raises(ValueError):
        V.lane_change_segments(30.0, 20.0)
    assert all(g["kappa1"] == 0 for g in V.lane_change_segments(0.0, 20.0))


def test_the_shared_case_is_what_its_docstring_says(pkg):
    p, ref = cases.reference()
    assert [len(r["s"]) for r in ref] == cases.N_KNOTS and max(cases.N_KNOTS) == cases.LMAX
    assert [len(s) for s in p] == [1, 8, 7, 2, 1]
    b, _ = twin.bounds(p[2], 0.0)
    assert ref[2]["s"][10] == b[1] and ref[2]["kappa"][10] == 0.0 and ref[2]["kappa"][11] > 0      # the bound that falls on knot 10 belongs to the segment that starts there
    assert ref[2]["s"][16] < b[2] < b[5] < ref[2]["s"][17]
    assert ref[1]["stats"]["kappa_abs_max"] == pytest.approx(1 / 14.5) and ref[1]["stats"]["closure_pos"] < 1e-12 
    # (from psi0 = 0.5 the eight heading sums are rounded at a magnitude below 8: 8 roundings of at most 2^-53 x 8; from psi0 = 0 they are exact, test_ovals_close)
    assert abs(ref[1]["stats"]["closure_psi"]) <= 8 * 2.0 ** -53 * 8
    assert ref[3]["kappa"].min() == -0.08 and ref[3]["stats"]["turn"] == pytest.approx(-2.0)
    assert ref[4]["edge_L"][0] == 3 and ref[4]["edge_L"][-1] == 5 and ref[4]["edge_R"][0] == -2 and ref[4]["edge_R"][-1] == -6
    assert cases.bar(1) == pytest.approx(3.25e-11, rel=0.01)      # 4 x 364 x 2^-53 x 201.1 m


# ---- the mirror ----
def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_struct_layouts_and_defaults(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_path_segment) == 64 and C.sizeof(L.pg_path_spec) == 48 and C.sizeof(L.pg_path_stats) == 48
    assert [getattr(L.pg_path_segment, n).offset for n, _ in L.pg_path_segment._fields_] == list(range(0, 64, 8))
    assert [getattr(L.pg_path_spec, n).offset for n, _ in L.pg_path_spec._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert [getattr(L.pg_path_stats, n).offset for n, _ in L.pg_path_stats._fields_] == list(range(0, 48, 8))
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.PATH_STATS_DTYPE.itemsize == 48 and mpc_mod.PATH_STATS_DTYPE.names == ("length", "turn", "closure_pos", "closure_psi", "kappa_abs_max", "ds")
    d = pkg.vehicles.path_segment()
    assert d == dict(length=1.0, kappa0=0.0, kappa1=0.0, edge_L0=4.0, edge_L1=4.0, edge_R0=-4.0, edge_R1=-4.0, reserved=0.0) == twin.segment()
    assert pkg.vehicles.path_segment(edge_L=3.0, edge_R1=-1.0)["edge_L1"] == 3.0
    with pytest.raises(KeyError):
        pkg.vehicles.path_segment(kappa=0.1)
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_path_segment
        f.restype = L.pg_path_segment; f.argtypes = []
        r = f()
        assert [getattr(r, n) for n, _ in L.pg_path_segment._fields_] == [1.0, 0.0, 0.0, 4.0, 4.0, -4.0, -4.0, 0.0]


def test_header_export_map_and_purity_list_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_path_segment;          /* 64 bytes */" in hdr and "} pg_path_spec;             /* 48 bytes */" in hdr and "} pg_path_stats;            /* 48 bytes */" in hdr
    assert "/* { 1, 0, 0, 4, 4, -4, -4, 0 }" in hdr and "pg_path_segment pg_default_path_segment(void);" in hdr
    assert "int pg_make_paths(pg_handle* h, int32_t n_path, const pg_path_spec* specs, int32_t n_seg_total, const pg_path_segment* segments, int32_t Lmax," in hdr
    for phrase in ("Bounds ", "Knots ", "Position ", "Prefix ", "0.8611363115940526", "0.3478548451374538", "0.3399810435848563", "0.6521451548625461",
                   "dE/ds = -sin psi, dN/ds = cos psi", "ceil((n_knots - 1) / 256)", "tests/path_make_numpy.py"):
        assert phrase in hdr, phrase
    assert "pg_*" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_exports.map")).read()
    assert {"pg_make_paths", "pg_default_path_segment"} <= set(pkg.SYMBOLS)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "make_paths" in open(os.path.join(ROOT, doc)).read(), doc
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_path_make" in check_f32_purity.TIME_KERNELS and "k_path_make" in check_f32_purity.__doc__
    assert "pg_path_make.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert "pg_path_make.hip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()


def test_builders(pkg):
    V = pkg.vehicles
    assert V.line_segments(12.0, edge_L=2.0) == [V.path_segment(length=12.0, edge_L0=2.0, edge_L1=2.0)]
    c = V.circle_segments(-5.0, turns=2, edge_R=-1.0)
    assert len(c) == 1 and c[0]["kappa0"] == c[0]["kappa1"] == -0.2 and c[0]["length"] == 2 * math.pi * 5 * 2 and c[0]["edge_R1"] == -1.0
    o = V.oval_segments(40.0, 14.5, 15.0, edge_L=5.0)
    assert [g["length"] for g in o[:4]] == [g["length"] for g in o[4:]] and all(g["edge_L0"] == 5.0 for g in o)
    assert [(g["kappa0"], g["kappa1"]) for g in o[:4]] == [(0, 0), (0, 1 / 14.5), (1 / 14.5, 1 / 14.5), (1 / 14.5, 0)]
    assert o[2]["length"] == pytest.approx((math.pi - 15 / 14.5) * 14.5, rel=1e-15)
    assert V.oval_segments(10.0, -5.0, 0.0)[1]["kappa0"] == -0.2
    for bad in ((40.0, 4.0, 13.0), (0.0, 5.0, 1.0), (10.0, 0.0, 1.0), (10.0, 5.0, -1.0)):
        with pytest.raises(ValueError):
            V.oval_segments(*bad)
    with pytest.raises(ValueError):
        V.circle_segments(0.0)


def test_packers_refuse_what_the_library_refuses(pkg):
    M = pkg.BatchedTrajectoryTrackingMPC
    seg = pkg.vehicles.path_segment
    good = [pkg.vehicles.line_segments(10.0), pkg.vehicles.oval_segments(10.0, 5.0, 2.0)]
    specs, segs = M.pack_path_specs(good, [2, 50], V_ref=[5.0, 6.0], pose=(1.0, 2.0, 3.0), closed=[False, True])
    assert len(specs) == 2 and len(segs) == 9
    assert [(s.seg0, s.n_seg, s.n_knots, s.closed, s.V_ref, s.E0, s.N0, s.psi0) for s in specs] == [(0, 1, 2, 0, 5.0, 1.0, 2.0, 3.0), (1, 8, 50, 1, 6.0, 1.0, 2.0, 3.0)]
    specs, _ = M.pack_path_specs(good, 7, pose=[(0, 0, 0), (1, 1, 1)])
    assert [s.n_knots for s in specs] == [7, 7] and specs[1].psi0 == 1.0 and specs[0].V_ref == 6.0
    for bad in (dict(length=0.0), dict(length=-1.0), dict(length=math.inf), dict(length=math.nan), dict(kappa0=math.nan), dict(kappa1=math.inf), dict(edge_L0=math.inf),
                dict(edge_R1=math.nan), dict(edge_L0=-4.0), dict(edge_L1=-5.0), dict(edge_R0=4.0), dict(reserved=1.0)):
        with pytest.raises(ValueError):
            M.pack_path_specs([good[0], [seg(**bad)]], 5)
    for kw in (dict(n_knots=1), dict(n_knots=2.5), dict(n_knots=2, closed=True), dict(n_knots=5, V_ref=0.0), dict(n_knots=5, V_ref=math.inf), dict(n_knots=5, V_ref=math.nan),
               dict(n_knots=5, pose=(0.0, math.nan, 0.0)), dict(n_knots=5, pose=(0.0, 0.0, math.inf)), dict(n_knots=[5, 5, 5]), dict(n_knots=5, closed=[True]),
               dict(n_knots=5, pose=(0.0, 0.0))):
        with pytest.raises(ValueError):
            M.pack_path_specs(good, **kw)
    with pytest.raises(ValueError):
        M.pack_path_specs([], 5)
    with pytest.raises(ValueError):
        M.pack_path_specs([good[0], []], 5)
    with pytest.raises(KeyError):
        M.pack_path_specs([[dict(radius=3.0)]], 5)
    # make_paths: ds or n_knots, one of them; both are checked before the library is reached (no handle is needed for these)
    class NoHandle(M):
        def __init__(self):
            pass
    for kw in (dict(), dict(ds=0.5, n_knots=10), dict(ds=0.0), dict(ds=-1.0), dict(ds=math.nan)):
        with pytest.raises(ValueError):
            NoHandle().make_paths(good, **kw)
