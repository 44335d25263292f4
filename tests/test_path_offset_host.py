"""The path offsetter without a device: the numpy twin (tests/path_offset_numpy.py) on the shared case (tests/path_offset_cases.py) -- the identity set, the circles (which
fix the sign), a lane change on a straight line against its closed forms, vehicles.lane_change_segments against lane_change --, and the Python mirror of pg_offset_paths
(struct layouts, the default set, every ValueError of the packer, the header's statement, the symbols, the purity and doc_numbers lists).  The measured values in the
comments are those of this scheme in float64 (EXPERIMENTS 37)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import path_make_numpy as maker
import path_offset_cases as cases
import path_offset_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_identity_set_returns_the_source_bit_for_bit():
    ch = cases.sources()
    for p in range(cases.N_PATH):
        n = cases.N_KNOTS[p]
        r = cases.reference()[p][0]
        for c, name in ((1, "s"), (2, "V"), (4, "E"), (5, "N"), (6, "psi"), (7, "kappa"), (8, "edge_L"), (9, "edge_R")):
            assert r[name].tobytes() == np.ascontiguousarray(ch[p, c, :n]).tobytes(), (p, name)
        st = r["stats"]
        assert st["x_min"] == 1.0 and st["d_abs_max"] == 0.0 and st["n_outside"] == 0 and st["length"] == ch[p, 1, n - 1] - ch[p, 1, 0]
        assert r["t"][0] == ch[p, 0, 0] and np.all(np.diff(r["t"]) > 0)
    # ... and a set whose windows lie beyond a path's end leaves that path on d0: the two lane changes on every source but the line
    for p in range(1, cases.N_PATH):
        for q in (3, 4):
            a, b = cases.reference()[p][q], cases.reference()[p][0]
            assert all(a[name].tobytes() == b[name].tobytes() for name in twin.CHANNELS), (p, q)


def test_lanes_of_the_circles_fix_the_sign():
    ch = cases.sources()
    R = cases.CIRCLE_R
    E0, N0, psi0 = 10.0, 5.0, 0.3
    for p, sign in ((1, +1.0), (2, -1.0)):
        centre = (E0 - sign * R * math.cos(psi0), N0 - sign * R * math.sin(psi0))      # R to the left of the start on the counter-clockwise circle, to the right on the other
        src_dist = np.hypot(ch[p, 4, :64] - centre[0], ch[p, 5, :64] - centre[1])
        assert np.max(np.abs(src_dist - R)) < 1e-11
        for q, d in ((1, 3.5), (2, -3.5), (6, 2.0)):
            r = cases.reference()[p][q]
            kappa = sign / R
            x = 1.0 - kappa * d
            assert np.max(np.abs(r["kappa"] - kappa / x)) <= 1e-12 * abs(kappa / x), (p, q)
            assert abs(r["stats"]["length"] - x * (2.0 * math.pi * R)) <= 1e-12 * x * 2.0 * math.pi * R, (p, q)
            dist = np.hypot(r["E"] - centre[0], r["N"] - centre[1])
            # the centre distance is R - d counter-clockwise and R + d clockwise: knot by knot the source's own distance moved by d
            assert np.max(np.abs(dist - (src_dist - sign * d))) <= 1e-12 * R, (p, q)
            assert np.max(np.abs(dist - (R - sign * d))) < 1e-11
            assert r["psi"].tobytes() == np.ascontiguousarray(ch[p, 6, :64]).tobytes() and r["stats"]["x_min"] == pytest.approx(x, rel=1e-15)
            assert r["stats"]["closure_pos"] < 1e-11 and r["stats"]["d_abs_max"] == abs(d)


def sigma(tau):
    tau = np.clip(tau, 0.0, 1.0)
    return tau ** 3 * (10.0 - 15.0 * tau + 6.0 * tau ** 2), 30.0 * tau ** 2 * (1.0 - tau) ** 2, 60.0 * tau * (1.0 - tau) * (1.0 - 2.0 * tau)


def test_lane_change_on_the_straight_line_against_its_closed_forms():
    ch = cases.sources()
    E0, N0, psi0 = 3.0, -2.0, 0.4
    s = ch[0, 1, :40]
    for q, (d1, a, b) in ((3, (1.5, 212.0, 217.0)), (4, (5.0, 230.0, 330.0))):
        r = cases.reference()[0][q]
        f, f1, f2 = sigma((s - a) / (b - a))
        d, dp, dpp = d1 * f, d1 * f1 / (b - a), d1 * f2 / (b - a) ** 2
        # the line: E = E0 - s sin psi0, N = N0 + s cos psi0; the left normal is (-cos psi0, -sin psi0)
        assert np.max(np.abs(r["E"] - (E0 - s * math.sin(psi0) - d * math.cos(psi0)))) <= 1e-12
        assert np.max(np.abs(r["N"] - (N0 + s * math.cos(psi0) - d * math.sin(psi0)))) <= 1e-12
        assert np.max(np.abs(r["psi"] - (psi0 + np.arctan(dp)))) <= 1e-12
        assert np.max(np.abs(r["kappa"] - dpp / (1.0 + dp ** 2) ** 1.5)) <= 1e-12
        # the length against a fine trapezoid of sqrt(1 + d'^2) over the window
        u = np.linspace(a, b, 200001)
        g = np.sqrt(1.0 + (d1 * sigma((u - a) / (b - a))[1] / (b - a)) ** 2)
        exact = 390.0 + float(np.sum(0.5 * (g[1:] + g[:-1]) * np.diff(u))) - (b - a)
        err = abs(r["stats"]["length"] - exact)
        print(f"set {q}: length {r['stats']['length']:.12f} m against the trapezoid {exact:.12f} m: error {err:.3e} m; n_outside {r['stats']['n_outside']}")
        assert err <= 2 * MEASURED_LENGTH_ERROR[q]
        assert np.all(np.diff(r["s"]) > 0) and r["s"][0] == s[0]
    # d1 = 5 m takes the road's left edge (4 m) past the path from where d >= 4 on; the short window lies inside one interval: no knot moves, the length does
    assert cases.reference()[0][4]["stats"]["n_outside"] == int(np.count_nonzero(5.0 * sigma((s - 230.0) / 100.0)[0] >= 4.0)) > 0
    inside = cases.reference()[0][3]
    assert np.all(inside["d"][:22] == 0.0) and np.all(inside["d"][22:] == 1.5) and inside["stats"]["length"] > 390.0 + 0.1


# measured |length - trapezoid| (m): the window inside one knot interval is seen by four nodes of ONE 10 m interval -- the 4-point rule on a C2 bump 5 m wide -- and that is
# what the scheme gives for a window narrower than the knot spacing (the header says the scheme is knot-wise: choose the knots to the manoeuvre); the window over ten knots
MEASURED_LENGTH_ERROR = {3: 1.272e-1, 4: 2.615e-11}


def test_lane_change_segments_against_lane_change(pkg):
    """Two constructions of one manoeuvre: four clothoids (vehicles.lane_change_segments, through the path maker's twin) and the quintic offset of a straight line.  The
    clothoid path of arc length 30 m advances F < 30 m along the road; the straight line is F long with the window over all of it, so both end one lane over, F ahead,
    heading as they started: the end pose agrees.  In between they differ, and the differences are printed, not bounded."""
    offset, length, n = 3.5, 30.0, 61
    a = maker.make(pkg.vehicles.lane_change_segments(offset, length), n, (0.0, 0.0, 0.0), 6.0)
    F = float(a["N"][-1])                                           # psi0 = 0: North is forward, and left is -E
    line = maker.make([maker.segment(length=F)], n, (0.0, 0.0, 0.0), 6.0)
    b = twin.offset(maker.channels(line, n), twin.offset_set(d0=0.0, d1=offset, s_a=0.0, s_b=F))
    print(f"lane change of {offset} m: clothoids advance {F:.6f} m over {length} m of arc, the offset line is {b['stats']['length']:.6f} m long; "
          f"peak |kappa| {np.max(np.abs(a['kappa'])):.4f} (clothoids) / {b['stats']['kappa_abs_max']:.4f} (quintic) 1/m; "
          f"peak heading {np.max(np.abs(a['psi'])):.4f} / {np.max(np.abs(b['psi'])):.4f} rad")
    assert abs(a["E"][-1] - b["E"][-1]) <= 1e-9 and abs(a["N"][-1] - b["N"][-1]) <= 1e-9 and abs(a["psi"][-1] - b["psi"][-1]) <= 1e-9
    assert b["E"][-1] == -offset and b["kappa"][0] == 0.0 and b["kappa"][-1] == 0.0


def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_struct_layouts_and_the_default_set(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_offset_set) == 64 and C.sizeof(L.pg_offset_stats) == 64
    assert [getattr(L.pg_offset_set, n).offset for n, _ in L.pg_offset_set._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert [getattr(L.pg_offset_stats, n).offset for n, _ in L.pg_offset_stats._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60]
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.OFFSET_STATS_DTYPE.itemsize == 64 and mpc_mod.OFFSET_STATS_DTYPE.names == tuple(n for n, _ in L.pg_offset_stats._fields_)
    V = pkg.vehicles
    inf = math.inf
    assert V.offset() == dict(d0=0.0, d1=0.0, s_a=inf, s_b=inf, s_c=inf, s_d=inf, x_min=0.1, edge_mode=0, reserved=0) == twin.offset_set()
    assert V.lane(3.5) == V.offset(d0=3.5, d1=3.5) and V.lane(-2, edge_mode=1)["edge_mode"] == 1
    assert V.lane_change(0, 3.5, 40, 70) == V.offset(d1=3.5, s_a=40, s_b=70)
    assert V.pass_by(3, 120, 135, 145, 160) == V.offset(d1=3.0, s_a=120, s_b=135, s_c=145, s_d=160)
    with pytest.raises(KeyError):
        V.offset(width=3.0)
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_offset_set
        f.restype = L.pg_offset_set; f.argtypes = []
        r = f()
        assert [getattr(r, n) for n, _ in L.pg_offset_set._fields_] == [0.0, 0.0, inf, inf, inf, inf, 0.1, 0, 0]


def test_header_symbols_and_lists_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_offset_set;              /* 64 bytes */" in hdr and "} pg_offset_stats;            /* 64 bytes */" in hdr
    assert "/* { 0, 0, +Inf, +Inf, +Inf, +Inf, 0.1, 0, 0 }: the identity */" in hdr and "pg_offset_set pg_default_offset_set(void);" in hdr
    assert "int pg_offset_paths(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in," in hdr
    assert "int32_t n_sets, const pg_offset_set* sets, int32_t install, int32_t* L_out, int32_t* closed_out, double* channels_out, pg_offset_stats* stats);" in hdr
    for phrase in ("Window ", "Offset ", "Arclength ", "Frame ", "Speed ", "Edges ", "Stats ", "a parenthesis is one rounded operation", "tau^3 (10 - 15 tau + 6 tau^2)",
                   "(w_k (g - 1))", "1.9999999999999996", "ceil((L - 1) / 256)", "atan2(y, x)", "(-cos psi, -sin psi)", "pg_plan_speeds' job", "tests/path_offset_numpy.py"):
        assert phrase in hdr, phrase
    assert {"pg_offset_paths", "pg_default_offset_set"} <= set(pkg.SYMBOLS)
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_offset_set) == 64 && sizeof(pg_offset_stats) == 64" in api
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "EXPERIMENTS.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "offset_paths" in open(os.path.join(ROOT, doc)).read(), doc
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_path_offset" in check_f32_purity.TIME_KERNELS and "k_path_offset" in check_f32_purity.__doc__
    assert "pg_path_offset.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert "pg_path_offset.hip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read() and "k_path_offset" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()
    # tools/isa_mix.py hashes what bench.kernel_source_sha16() hashes (tests/test_abi_and_host.py compares the two): the makers' own files are in neither list, and
    # pg_kernels.hip, which includes this one, is in both
    import bench
    import isa_mix
    assert isa_mix.source_hash() == bench.kernel_source_sha16()
    assert '#include "pg_path_offset.hip"' in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()


def test_the_shared_case_is_what_its_docstring_says():
    ch = cases.sources()
    ref = cases.reference()
    assert ch.shape == (6, 10, 300) and all(np.all(ch[p][:, cases.N_KNOTS[p]:] == 0.0) for p in range(6))
    assert (cases.N_KNOTS[3] - 1 + 255) // 256 == 2
    s0 = ch[0, 1, :40]
    assert s0[21] == 210.0 and s0[22] == 220.0 and np.ptp(ch[4, 2, :28]) > 0
    lengths = [float(ch[p, 1, cases.N_KNOTS[p] - 1] - ch[p, 1, 0]) for p in range(6)]
    assert max(lengths[1:]) < 212.0 < lengths[0]                    # the lane changes act on the line alone
    oval = ref[3][5]
    assert oval["stats"]["d_abs_max"] == 3.0 and oval["stats"]["kappa_abs_max"] > 1.0 / 14.5 and oval["stats"]["closure_pos"] < 1e-9
    for p in range(6):
        for q in range(7):
            st = ref[p][q]["stats"]
            assert st["x_min"] >= 0.1 and st["ds_min"] > 0 and np.all(np.isfinite(twin.channels(ref[p][q], 300))), (p, q)
    assert ref[1][6]["edge_L"].tobytes() == np.ascontiguousarray(ch[1, 8, :64]).tobytes() and np.all(ref[1][1]["edge_L"] == ch[1, 8, :64] - 3.5)


def test_the_packer_refuses_what_the_library_refuses(pkg):
    M = pkg.BatchedTrajectoryTrackingMPC
    V = pkg.vehicles
    arr = M.pack_offsets([V.offset(), V.lane(3.5), V.lane_change(0, 3.5, 40, 70), V.pass_by(3, 20, 35, 35, 60, edge_mode=1)])
    assert len(arr) == 4 and arr[2].s_a == 40.0 and arr[3].edge_mode == 1 and arr[0].x_min == 0.1 and math.isinf(arr[1].s_c)
    assert len(M.pack_offsets(V.lane(1.0))) == 1 and len(M.pack_offsets(arr[1])) == 1
    nan, inf = math.nan, math.inf
    refused = [dict(d0=nan), dict(d1=inf), dict(s_a=nan), dict(s_a=-inf, s_b=3.0), dict(s_a=10.0, s_b=10.0), dict(s_a=10.0, s_b=5.0), dict(s_a=10.0, s_b=inf),
               dict(s_a=10.0, s_b=nan), dict(s_b=nan), dict(s_d=nan), dict(s_a=10.0, s_b=20.0, s_c=30.0, s_d=30.0), dict(s_a=10.0, s_b=20.0, s_c=30.0, s_d=nan),
               dict(s_a=10.0, s_b=20.0, s_c=15.0, s_d=40.0), dict(s_c=30.0, s_d=40.0), dict(s_a=10.0, s_b=20.0, s_c=nan), dict(x_min=0.0), dict(x_min=1.5), dict(x_min=nan),
               dict(edge_mode=2), dict(edge_mode=-1), dict(reserved=1)]
    for kw in refused:
        with pytest.raises(ValueError):
            M.pack_offsets([V.offset(), V.offset(**kw)])
    with pytest.raises(ValueError):
        M.pack_offsets([])
