"""The tube clipper without a device: the numpy twin (tests/tube_clip_numpy.py) against closed forms on a straight line, its invariance under a rigid motion, the shared
case (tests/tube_clip_cases.py) and how far its decisions are from a tie, vehicles.pass_by_around, and the Python mirror of pg_clip_tubes (struct layouts, the default set,
every ValueError of the packer, the header's statement, the symbols, the purity and doc_numbers lists)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import path_make_numpy as maker
import tube_clip_cases as cases
import tube_clip_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E0, N0, PSI0 = 3.0, -2.0, 0.4


def line(n=201, length=200.0, pose=(E0, N0, PSI0)):
    return maker.channels(maker.make([maker.segment(length=length)], n, pose, 10.0), n)


def beside(pose, u, e):
    """the point u along and e to the left of a line from `pose`"""
    E, N, psi = pose
    return E - u * math.sin(psi) - e * math.cos(psi), N + u * math.cos(psi) - e * math.sin(psi)


def test_hard_clip_on_a_straight_line_is_the_chord():
    ch = line()
    s = ch[1]
    e0, R = 0.3, 1.5
    oE, oN = beside((E0, N0, PSI0), 100.4, e0)
    r = twin.clip(ch, twin.obstacle_set(first=0, count=1), [(oE, oN, R)])
    b = 100.4 - s                                                   # the disc lies b ahead of knot i
    inside = np.abs(b) < R
    assert list(np.flatnonzero(inside)) == [99, 100, 101]
    want = np.where(inside, e0 - np.sqrt(np.maximum(R * R - b * b, 0.0)), 4.0)
    assert np.max(np.abs(r["edge_L"] - want)) <= 1e-12 and r["edge_R"].tobytes() == ch[9].tobytes()
    rep = r["report"][0]
    assert (rep["side"], rep["k_at"], rep["k_first"], rep["k_last"]) == (1, 100, 99, 101) and rep["u_at"] == 100.0
    assert abs(rep["a_at"] - e0) <= 1e-12 and abs(rep["dist_at"] - math.hypot(0.4, e0)) <= 1e-12
    assert abs(rep["free_right"] - ((e0 - rep["h_at"]) + 4.0)) <= 1e-12 and abs(rep["free_left"] - (4.0 - (e0 + rep["h_at"]))) <= 1e-12
    st = r["stats"]
    assert (st["n_clip_L"], st["n_clip_R"], st["n_seen"], st["n_ignored"], st["n_blocked"]) == (3, 0, 1, 0, 0) and st["n_centre_out"] == 3 and st["u_width_min"] == 100.0
    # the same disc on the right of the centre line clips the right edge, mirrored
    oE, oN = beside((E0, N0, PSI0), 100.4, -e0)
    m = twin.clip(ch, twin.obstacle_set(first=0, count=1), [(oE, oN, R)])
    assert np.max(np.abs(m["edge_R"] + want)) <= 1e-12 and m["edge_L"].tobytes() == ch[8].tobytes() and m["report"][0]["side"] == -1


def test_taper_bounds_and_monotony():
    ch = line()
    s = ch[1]
    obs = [beside((E0, N0, PSI0), 100.4, 0.3) + (1.5,), beside((E0, N0, PSI0), 140.2, -2.0) + (1.0,), beside((E0, N0, PSI0), 60.0, 9.0) + (1.0,)]
    hard = twin.clip(ch, twin.obstacle_set(first=0, count=3), obs)
    for m in (0.25, 2.0):
        r = twin.clip(ch, twin.obstacle_set(first=0, count=3, taper=m), obs)
        assert np.all(r["edge_L"] <= ch[8]) and np.all(r["edge_R"] >= ch[9]) and np.all(r["edge_L"] <= hard["edge_L"]) and np.all(r["edge_R"] >= hard["edge_R"])
        for k in np.flatnonzero(hard["edge_L"] < ch[8]):
            assert np.all(r["edge_L"] <= hard["edge_L"][k] + m * np.abs(s - s[k]))
        for k in np.flatnonzero(hard["edge_R"] > ch[9]):
            assert np.all(r["edge_R"] >= hard["edge_R"][k] - m * np.abs(s - s[k]))
        assert r["stats"]["n_clip_L"] > hard["stats"]["n_clip_L"] and [x["side"] for x in r["report"]] == [1, -1, 0] and r["stats"]["n_ignored"] == 1
    # the slope between neighbours is at most m where the taper holds the edge
    r = twin.clip(ch, twin.obstacle_set(first=0, count=3, taper=0.25), obs)
    assert np.max(np.abs(np.diff(r["edge_L"])[:95])) <= 0.25 * 1.0 + 1e-12


def test_identity_in_identity_out_and_the_unseen_disc():
    ch = cases.sources()
    ref = cases.reference()
    for p in range(cases.N_PATH):
        n = cases.N_KNOTS[p]
        for q in (0, 4, 11):                                        # the identity, the disc outside the tube, the disc between two knots
            r = ref[p][q]
            for c, name in enumerate(twin.CHANNELS):
                assert r[name].tobytes() == np.ascontiguousarray(ch[p, c, :n]).tobytes(), (p, q, name)
            assert r["stats"]["n_seen"] == 0 and r["stats"]["n_clip_L"] == 0 and r["stats"]["n_clip_R"] == 0 and r["stats"]["width_min"] == 8.0
            assert all(x["side"] == 0 and x["k_first"] == -1 and x["k_last"] == -1 for x in r["report"])
    # what the knots see: on the line with knots 10 m apart a disc of R = 1.5 m at 215 m lies between two knots farther apart than its chord
    at215 = beside((3.0, -2.0, 0.4), 215.0, 0.0) + (1.5,)
    r = twin.clip(ch[0][:, :40], twin.obstacle_set(first=0, count=1), [at215])
    assert r["report"][0]["side"] == 0 and r["stats"]["n_ignored"] == 1 and r["report"][0]["k_at"] in (21, 22) and abs(r["report"][0]["dist_at"] - 5.0) <= 1e-9
    assert r["edge_L"].tobytes() == np.ascontiguousarray(ch[0, 8, :40]).tobytes()
    # ... and 201 knots over the same stretch see it
    fine = line(n=391, length=390.0, pose=(3.0, -2.0, 0.4))
    assert twin.clip(fine, twin.obstacle_set(first=0, count=1), [at215])["stats"]["n_clip_L"] + twin.clip(fine, twin.obstacle_set(first=0, count=1), [at215])["stats"]["n_clip_R"] == 3


def test_the_shared_case_is_what_its_docstring_says():
    ref = cases.reference()
    ch = cases.sources()
    sets = cases.sets()
    assert len(sets) == cases.N_SETS and max(s["count"] for s in sets) == cases.MAX_COUNT == 64 and len(cases.obstacles()) == cases.N_OBS
    assert np.all(ch[:, 8, 0] == 4.0) and np.all(ch[:, 9, 0] == -4.0)
    L = ref[0]
    assert L[1]["stats"]["n_centre_out"] > 0 and L[1]["stats"]["n_clip_L"] == 1 and L[2]["stats"]["n_clip_L"] == 3 and L[2]["stats"]["n_centre_out"] == L[1]["stats"]["n_centre_out"]
    assert L[3]["stats"]["n_clip_L"] >= 1 and L[3]["stats"]["n_centre_out"] == 0 and L[3]["report"][0]["a_at"] + L[3]["report"][0]["h_at"] > 4.0
    assert L[4]["stats"]["n_ignored"] == 1 and L[5]["stats"]["n_blocked"] > 0 and L[5]["stats"]["width_min"] < 3.0 and [x["side"] for x in L[5]["report"]] == [1, -1]
    assert [L[q]["report"][0]["side"] for q in (6, 7, 8, 9)] == [-1, -1, -1, 1]      # right of the centre: CENTRE and WIDER pass left, LEFT too, RIGHT clips the left edge
    assert L[12]["stats"]["n_seen"] > 0 and L[12]["stats"]["n_ignored"] > 0 and L[12]["stats"]["n_seen"] + L[12]["stats"]["n_ignored"] == 64
    assert L[12]["report"][0] == L[11]["report"][0]                 # the two ranges overlap in the shared array
    for p in (1, 2):                                                # the circles: the taper wraps the seam, and knot L-1 is knot 0 again
        r = ref[p][10]
        touched = np.flatnonzero(r["edge_L"] != 4.0)
        assert touched[0] == 0 and touched[-1] == 63 and 30 not in touched and r["edge_L"][63] == r["edge_L"][0] and r["stats"]["n_clip_L"] == len(touched) - 1
    oval = ref[3][10]
    assert oval["report"][1]["k_first"] <= 256 <= oval["report"][1]["k_last"] and oval["edge_R"][257] != -4.0 and oval["edge_R"][1] != -4.0 and oval["edge_R"][258] == oval["edge_R"][0]
    for p in (1, 2, 3, 4, 5):                                       # the discs on the line are far from every other source
        assert all(ref[p][q]["stats"]["n_seen"] == 0 for q in range(cases.N_SETS) if q != 10), p


def test_decision_margin():
    assert cases.decision_margin() >= 1e-6


def test_invariance_under_a_rigid_motion():
    """path and obstacles turned by 0.7 rad and moved by (-250, 410): the same clip within the bar of tests/test_gpu_tube_clip.py -- the moved copy carries other sines
    and cosines, nothing else differs -- and the same integers"""
    ch = cases.sources()
    th, dE, dN = 0.7, -250.0, 410.0
    c, s = math.cos(th), math.sin(th)
    # psi is measured from North, counter-clockwise positive: the tangent (-sin psi, cos psi) turns with the points when psi grows by th
    turn = lambda E, N: (c * E - s * N + dE, s * E + c * N + dN)
    obs = np.array(cases.obstacles())
    mE, mN = turn(obs[:, 0], obs[:, 1])
    moved_obs = np.stack([mE, mN, obs[:, 2]], axis=1)
    worst = 0.0
    for p, q in ((0, 2), (0, 5), (0, 12), (1, 10), (3, 10)):
        n = cases.N_KNOTS[p]
        a = cases.reference()[p][q]
        src = np.array(ch[p][:, :n])
        src[4], src[5] = turn(ch[p, 4, :n], ch[p, 5, :n])
        src[6] = ch[p, 6, :n] + th
        b = twin.clip(src, cases.sets()[q], moved_obs, bool(cases.CLOSED[p]))
        assert [tuple(x[f] for f in ("k_at", "k_first", "k_last", "side")) for x in a["report"]] == [tuple(x[f] for f in ("k_at", "k_first", "k_last", "side")) for x in b["report"]]
        assert all(a["stats"][f] == b["stats"][f] for f in twin.STATS_INTS)
        # the moved points carry the rounding of the motion itself: 2^-52 of coordinates of some 500 m, through the same (1 + |b| / h)
        motion = 4.0 * 2.0 ** -52 * 500.0 / (twin.EPS8 * 1.0)
        for name, bar in (("edge_L", a["bar_L"]), ("edge_R", a["bar_R"])):
            d = np.abs(a[name] - b[name])
            assert np.all(d[bar == 0.0] == 0.0) and np.all(d <= bar * (1.0 + motion)), (p, q, name, float(d.max()))
            worst = max(worst, float(d.max()))
    print(f"worst |edge - moved edge| {worst:.3e} m")


def test_pass_by_around(pkg):
    V = pkg.vehicles
    ch = line()
    for e0, side in ((0.3, 1), (-0.3, -1)):
        disc = V.obstacle_at(ch, 100.0, e0, 1.5)
        assert abs(disc["E"] - beside((E0, N0, PSI0), 100.0, e0)[0]) <= 1e-12 and abs(disc["N"] - beside((E0, N0, PSI0), 100.0, e0)[1]) <= 1e-12 and disc["radius"] == 1.5
        r = twin.clip(ch, twin.obstacle_set(first=0, count=1, taper=0.25), [(disc["E"], disc["N"], 1.5)])
        row = r["report"][0]
        assert row["side"] == side
        pb = V.pass_by_around(row, ch, 30.0)
        want = 0.5 * ((e0 - 1.5) - 4.0) if side > 0 else 0.5 * ((e0 + 1.5) + 4.0)
        assert abs(pb["d1"] - want) <= 1e-12 and pb["d0"] == 0.0 and (pb["s_a"], pb["s_b"], pb["s_c"], pb["s_d"]) == (69.0, 99.0, 101.0, 131.0) and pb["x_min"] == 0.1
        assert pb["edge_mode"] == 0 and V.pass_by_around(row, ch, 10.0, x_min=0.2)["x_min"] == 0.2
    unseen = dict(row, side=0, k_first=-1, k_last=-1)
    assert V.pass_by_around(unseen, ch, 30.0) == V.offset()
    # a disc that leaves nothing on the side it is passed on: R = 3 m, 2 m left of the centre under PG_PASS_LEFT (3 m of chord beyond the 4 m edge)
    disc = V.obstacle_at(ch, 100.0, 2.0, 3.0)
    r = twin.clip(ch, twin.obstacle_set(first=0, count=1, policy=twin.LEFT), [(disc["E"], disc["N"], 3.0)])
    assert r["report"][0]["side"] == -1 and r["report"][0]["free_left"] < 0
    with pytest.raises(ValueError):
        V.pass_by_around(r["report"][0], ch, 30.0)
    assert V.pass_by_around(twin.clip(ch, twin.obstacle_set(first=0, count=1), [(disc["E"], disc["N"], 3.0)])["report"][0], ch, 30.0)["d1"] == pytest.approx(0.5 * (-1.0 - 4.0))


def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_struct_layouts_and_the_default_set(pkg):
    L = lib_mod()
    offs = lambda T: [getattr(T, n).offset for n, _ in T._fields_]
    assert [C.sizeof(T) for T in (L.pg_obstacle, L.pg_obstacle_set, L.pg_clip_stats, L.pg_obstacle_report)] == [32, 64, 64, 64]
    assert offs(L.pg_obstacle) == [0, 8, 16, 24]
    assert [n for n, _ in L.pg_obstacle_set._fields_] == ["first", "count", "margin", "taper", "min_width", "policy", "reserved", "pad"] and offs(L.pg_obstacle_set) == [0, 4, 8, 16, 24, 32, 36, 40]
    assert [n for n, _ in L.pg_clip_stats._fields_] == ["width_min", "u_width_min", "reserved_d", "n_clip_L", "n_clip_R", "n_blocked", "n_centre_out", "n_seen", "n_ignored", "reserved"]
    assert offs(L.pg_clip_stats) == [0, 8, 16, 32, 36, 40, 44, 48, 52, 56]
    assert [n for n, _ in L.pg_obstacle_report._fields_] == list(twin.REPORT_FIELDS) and offs(L.pg_obstacle_report) == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.CLIP_STATS_DTYPE.itemsize == 64 and mpc_mod.OBSTACLE_REPORT_DTYPE.itemsize == 64
    assert [mpc_mod.CLIP_STATS_DTYPE.fields[n][1] for n, _ in L.pg_clip_stats._fields_] == offs(L.pg_clip_stats)
    assert mpc_mod.OBSTACLE_REPORT_DTYPE.names == twin.REPORT_FIELDS
    V = pkg.vehicles
    assert V.obstacle_set() == dict(obstacles=[], margin=0.0, taper=math.inf, min_width=0.0, policy=0)
    assert V.obstacle(1, 2, 3) == dict(E=1.0, N=2.0, radius=3.0, reserved=0.0) and V.obstacle_set([V.obstacle(1, 2, 3)], policy="wider")["policy"] == 1
    assert V.PASS_POLICIES == dict(centre=twin.CENTRE, wider=twin.WIDER, left=twin.LEFT, right=twin.RIGHT)
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_obstacle_set
        f.restype = L.pg_obstacle_set; f.argtypes = []
        r = f()
        assert [r.first, r.count, r.margin, r.taper, r.min_width, r.policy, r.reserved, list(r.pad)] == [0, 0, 0.0, math.inf, 0.0, 0, 0, [0.0, 0.0, 0.0]]


def test_header_symbols_and_lists_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    for line_ in ("} pg_obstacle;                /* 32 bytes */", "} pg_obstacle_set;            /* 64 bytes */", "} pg_clip_stats;              /* 64 bytes */",
                  "} pg_obstacle_report;         /* 64 bytes */", "/* { 0, 0, 0.0, +Inf, 0.0, 0, 0, {0, 0, 0} }: the identity */", "pg_obstacle_set pg_default_obstacle_set(void);",
                  "enum pg_pass_policy { PG_PASS_CENTRE = 0, PG_PASS_WIDER = 1, PG_PASS_LEFT = 2, PG_PASS_RIGHT = 3 };",
                  "int pg_clip_tubes(pg_handle* h, int32_t n_path, int32_t Lmax, const int32_t* L, const int32_t* closed, const double* channels_in,",
                  "int32_t n_sets, const pg_obstacle_set* sets, int32_t n_obs, const pg_obstacle* obstacles, int32_t install,",
                  "int32_t* L_out, int32_t* closed_out, double* channels_out, pg_clip_stats* stats, pg_obstacle_report* report);"):
        assert line_ in hdr, line_
    for phrase in ("Frame ", "Sight ", "Closest ", "Side ", "Hard clip ", "Taper ", "Stats ", "Output ", "a parenthesis is one rounded operation", "src/trajectories.jl:8-44",
                   "h = sqrt((R R) - (b b))", "(cL_k + (m dist(i, k)))", "(cR_k - (m dist(i, k)))", "((s_{L-1} - s_0) - |s_i - s_k|)", "the lowest index on ties",
                   "What the knots see", "215 m", "tests/tube_clip_numpy.py", "(1 + |b| / h)"):
        assert phrase in hdr, phrase
    assert {"pg_clip_tubes", "pg_default_obstacle_set"} <= set(pkg.SYMBOLS)
    assert "global: pg_*;" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_exports.map")).read()
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_obstacle) == 32 && sizeof(pg_obstacle_set) == 64 && sizeof(pg_clip_stats) == 64 && sizeof(pg_obstacle_report) == 64" in api
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "EXPERIMENTS.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "clip_tubes" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.22" in design and "obstacle sets and tube clipping" not in design[design.index("### 4.21"):design.index("### 4.22")]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_tube_clip" in check_f32_purity.TIME_KERNELS and "k_tube_clip" in check_f32_purity.__doc__
    assert "pg_tube_clip.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert "pg_tube_clip.hip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read() and "k_tube_clip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()
    # tools/isa_mix.py hashes what bench.kernel_source_sha16() hashes (tests/test_abi_and_host.py compares the two): the makers' own files are in neither list, and
    # pg_kernels.hip, which includes this one, is in both
    import bench
    import isa_mix
    assert isa_mix.source_hash() == bench.kernel_source_sha16()
    assert '#include "pg_tube_clip.hip"' in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_clip_tubes.py"))


def test_the_packer_refuses_what_the_library_refuses(pkg):
    M = pkg.BatchedTrajectoryTrackingMPC
    V = pkg.vehicles
    o = V.obstacle(1.0, 2.0, 0.5)
    arr, obs, n_obs = M.pack_obstacle_sets([V.obstacle_set(), V.obstacle_set([o, V.obstacle(3, 4, 0)], margin=0.9, taper=0.25, min_width=2.5, policy="right"), V.obstacle_set([o])])
    assert n_obs == 3 and [(s.first, s.count) for s in arr] == [(0, 0), (0, 2), (2, 1)] and arr[1].policy == 3 and arr[1].taper == 0.25 and math.isinf(arr[0].taper)
    assert (obs[1].E, obs[1].N, obs[1].radius, obs[2].radius) == (3.0, 4.0, 0.0, 0.5) and arr[1].min_width == 2.5 and list(arr[1].pad) == [0.0, 0.0, 0.0]
    assert len(M.pack_obstacle_sets(V.obstacle_set([o]))[0]) == 1
    nan, inf = math.nan, math.inf
    refused = [dict(margin=-1.0), dict(margin=nan), dict(margin=inf), dict(taper=0.0), dict(taper=-1.0), dict(taper=nan), dict(min_width=-0.1), dict(min_width=nan),
               dict(min_width=inf), dict(policy=4), dict(policy=-1), dict(obstacles=[V.obstacle(nan, 0, 1)]), dict(obstacles=[V.obstacle(0, inf, 1)]),
               dict(obstacles=[V.obstacle(0, 0, nan)]), dict(obstacles=[V.obstacle(0, 0, -1.0)]), dict(obstacles=[V.obstacle(0, 0, 0.0)]), dict(obstacles=[o] * 65),
               dict(obstacles=[dict(o, reserved=1.0)])]
    for kw in refused:
        with pytest.raises(ValueError):
            M.pack_obstacle_sets([V.obstacle_set(), V.obstacle_set(**kw)])
    with pytest.raises(ValueError):
        M.pack_obstacle_sets([])
    with pytest.raises(ValueError):
        M.pack_obstacle_sets([dict(V.obstacle_set(), width=3.0)])
    with pytest.raises(KeyError):
        V.obstacle_set(policy="over")
