"""pg_smooth_waypoints on the host: the twin (tests/wp_smooth_numpy.py, written from the scheme in include/pigeon_mpc.h) against a dense solve of the system it claims to
solve, the properties that need no tolerance, the recorded oval, the walls, the layouts, and the recurrence helpers of the kernel as a stand-alone host program."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import path_fit_numpy as fit_twin
import wp_smooth_cases as cases
import wp_smooth_numpy as twin
from conftest import ROOT

# EXPERIMENTS 41, measured on the build container over the case list (75 pairs): the largest |gamma - dense| / max |dense gamma| is 6.649e-11 and the largest
# |g - dense| 4.547e-13 m (coordinates up to 320 m).  Both sides are double; the gap is rounding times the conditioning.  The bars are 16 x those figures.
GAMMA_BAR = 16 * 6.649e-11
G_BAR = 16 * 4.547e-13


def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_the_twin_against_a_dense_solve_of_the_same_system():
    worst_gamma = worst_g = 0.0
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        n = len(w)
        for s, r in zip(cases.SETS, row):
            gamma, g = twin.dense(w, closed, s)
            rows = slice(0, n) if closed else slice(1, n - 1)
            mine = np.stack([r["gamma_E"][rows], r["gamma_N"][rows]], axis=1)
            eg = float(np.max(np.abs(mine - gamma)) / np.max(np.abs(gamma))) if gamma.size and np.max(np.abs(gamma)) > 0 else 0.0
            ey = float(np.max(np.abs(np.stack([r["E"], r["N"]], axis=1) - g)))
            worst_gamma = max(worst_gamma, eg); worst_g = max(worst_g, ey)
            assert eg <= GAMMA_BAR and ey <= G_BAR, (name, s, eg, ey)
            assert r["stats"]["pivot_min"] > 0
    print(f"twin against numpy.linalg.solve over {len(cases.paths()) * len(cases.SETS)} pairs: worst relative |gamma - dense| {worst_gamma:.3e} (bar {GAMMA_BAR:.3e}), "
          f"worst |g - dense| {worst_g:.3e} m (bar {G_BAR:.3e})")


def test_properties_that_need_no_tolerance():
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        given = np.array([[p["E"], p["N"], p["edge_L"], p["edge_R"]] for p in w])
        # lambda = 0: the input bit for bit, and nothing moved
        assert cases.as_bits(row[0]).tobytes() == given.tobytes(), name
        assert row[0]["stats"]["dev_max"] == 0.0 and row[0]["stats"]["dev_rms"] == 0.0 and row[0]["stats"]["n_outside"] == 0.0
        # pinned ends of an open path; on a closed one the flag is not looked at
        r = row[2]
        if not closed:
            assert (r["E"][0], r["N"][0], r["E"][-1], r["N"][-1]) == (w[0]["E"], w[0]["N"], w[-1]["E"], w[-1]["N"]), name
        else:
            assert cases.as_bits(r).tobytes() == cases.as_bits(twin.smooth(w, True, twin.smooth_set(lam=10.0))).tobytes(), name
        # the window of factor 0 pins what only it holds; where the later window of factor 4 holds a waypoint too, that one wins
        r = row[3]
        U = r["U"]
        pinned = (U >= 2.0) & (U < 5.0)
        assert np.all(r["winv"][pinned] == 0.0) and np.all(r["winv"][(U >= 5.0) & (U <= 40.0)] == 4.0) and np.all(r["winv"][(U < 2.0) | (U > 40.0)] == 1.0), name
        assert np.all(r["E"][pinned] == given[pinned, 0]) and np.all(r["N"][pinned] == given[pinned, 1]), name
        # without keep_walls the edges are copied
        for k in (1, 2, 3):
            assert row[k]["edge_L"].tobytes() == given[:, 2].tobytes() and row[k]["edge_R"].tobytes() == given[:, 3].tobytes(), (name, k)
        if len(w) == 2:
            for r in row:
                assert cases.as_bits(r)[:, :2].tobytes() == given[:, :2].tobytes() and r["stats"]["pivot_min"] == math.inf
    # collinear waypoints with dyadic coordinates and chords: every slope is exact and equal, the right-hand side is 0 and so is gamma
    steps = [1, 2, 1, 4, 8, 1, 2]
    u = np.concatenate([[0.0], np.cumsum(steps)]) * 0.5
    line = [cases.wp(3.0 * a - 7.0, 4.0 * a + 2.0) for a in u]
    for lam in (0.0, 0.1, 10.0, 1e6):
        for s in (twin.smooth_set(lam=lam), twin.smooth_set(lam=lam, keep_walls=True, windows=[(3.0, 9.0, 4.0)])):
            r = twin.smooth(line, False, s)
            assert cases.as_bits(r).tobytes() == np.array([[p["E"], p["N"], 4.0, -4.0] for p in line]).tobytes(), lam
            assert r["stats"]["bend"] == 0.0 and r["stats"]["dev_max"] == 0.0


def test_chords_prefix_and_windows_by_hand():
    """What the dense check takes from the twin itself -- h, U, winv -- on a case worked by hand: the 3-4-5 triangle walked open from (0, 0) by (3, 0) and (3, 4) back
    to (0, 0).  Chords 3, 4, 5 and U = 0, 3, 7, 12 are exact.  Windows [3, 7] with factor 0 and then [7, 20] with factor 2.5: waypoint 0 is in neither (1), waypoint 1
    (U = 3, on the first window's closed end) is pinned, waypoint 2 (U = 7) is in both and the later one wins, waypoint 3 is in the second."""
    w = [cases.wp(0, 0), cases.wp(3, 0), cases.wp(3, 4), cases.wp(0, 0)]
    s = twin.smooth_set(lam=1.0, windows=[(3.0, 7.0, 0.0), (7.0, 20.0, 2.5)])
    r = twin.smooth(w, False, s)
    assert list(r["h"]) == [3.0, 4.0, 5.0] and list(r["U"]) == [0.0, 3.0, 7.0, 12.0] and list(r["winv"]) == [1.0, 0.0, 2.5, 2.5]
    assert (r["E"][1], r["N"][1]) == (3.0, 0.0) and (r["E"][2], r["N"][2]) != (3.0, 4.0)
    assert list(twin.smooth(w, False, dict(s, pin_ends=True))["winv"]) == [0.0, 0.0, 2.5, 0.0]
    # the same windows listed the other way round: now [3, 7] is the later one and takes waypoint 2 as well
    assert list(twin.smooth(w, False, twin.smooth_set(lam=1.0, windows=[(7.0, 20.0, 2.5), (3.0, 7.0, 0.0)]))["winv"]) == [1.0, 0.0, 0.0, 2.5]
    # the blocked prefix past one block: 300 chords of 0.5 m, c = 2 -- every partial sum is exact, so U_i = i / 2 whatever the order
    line = [cases.wp(0.0, 0.5 * i) for i in range(301)]
    assert list(twin.smooth(line, False, twin.smooth_set())["U"]) == [0.5 * i for i in range(301)]


def test_the_recorded_oval(pkg):
    """skidpadoval, 999 waypoints 0.24 m apart holding rounded positions, smoothed by the twin and then fitted by path_fit_numpy at 1000 knots, against the file's k_1pm at
    equal s / total.  Measured on the build container (EXPERIMENTS 41): max |kappa - file| 1.781e-2 1/m interpolated, 7.088e-4 at lambda = 0.1 (25-fold less); dev_max
    2.348e-4 m, dev_rms 1.605e-5 m.  dev_max over the ladder 0, 1e-3 .. 10: 0, 8.020e-5, 1.486e-4, 2.348e-4, 5.486e-4, 2.844e-3 m."""
    from test_path_fit_host import at_equal_fraction
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "paths", "skidpadoval.npz")))
    w = cases.golden("skidpadoval", True)
    assert len(w) == 999

    def kappa_err(r):
        out = [dict(E=r["E"][i], N=r["N"][i], edge_L=r["edge_L"][i], edge_R=r["edge_R"][i]) for i in range(len(w))]
        f = fit_twin.fit(out, 1000, 6.0, True)
        return float(np.max(np.abs(f["kappa"] - at_equal_fraction(f, d["s_m"], d["k_1pm"]))))
    ladder = [twin.smooth(w, True, twin.smooth_set(lam=lam)) for lam in cases.LADDER]
    dev = [r["stats"]["dev_max"] for r in ladder]
    k0, k1 = kappa_err(ladder[0]), kappa_err(ladder[3])
    print(f"oval: max |kappa - file| {k0:.3e} interpolated, {k1:.3e} at lambda = 0.1; dev_max over the ladder {['%.3e' % v for v in dev]}, dev_rms {ladder[3]['stats']['dev_rms']:.3e}")
    assert k0 == pytest.approx(1.781e-2, rel=1e-3)
    assert k1 < 0.1 * 1.781e-2 and k1 == pytest.approx(7.088e-4, rel=1e-3)
    assert dev[3] < 1e-3 and dev[3] == pytest.approx(2.348e-4, rel=1e-3)
    assert all(a <= b for a, b in zip(dev, dev[1:])), dev
    assert ladder[3]["stats"]["n_outside"] == 0.0 and ladder[3]["stats"]["width_min"] == 8.0


def test_keep_walls_leaves_the_walls_where_they_were_surveyed():
    """The wall's world position is centre + edge * n (n the left normal at the smoothed waypoint); its component along n is (centre . n) + edge.  edge' = edge - c with
    c = (g - y) . n, so (g . n) + edge' and (y . n) + edge differ by the rounding of: the two products and the sum of c (each within 2^-53 of |c| <= |dev|), the
    subtraction edge - c (2^-53 |edge|), and, in this check's own arithmetic, the two dot products of coordinates up to |y| (4 products and 2 sums, 2^-53 |y| each) and
    the sum with the edge.  With |edge| <= 5 m and |y| <= 320 m (vail) that is below (|edge| + |y|) * 2^-50 for every case: the bar, from the magnitudes alone."""
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        r = row[4]
        n = len(w)
        if n == 2:
            continue
        worst = 0.0
        for i in range(n):
            # the left normal restated here from the convention dE/ds = -sin psi, dN/ds = cos psi: tangent (tE, tN), left normal (-tN, tE) / |t|
            if closed or i < n - 1:
                ip = (i + 1) % n
                h = r["h"][i]
                t = [(o[ip] - o[i]) / h - h * (2.0 * g[i] + g[ip]) / 6.0 for o, g in ((r["E"], r["gamma_E"]), (r["N"], r["gamma_N"]))]
            else:
                h = r["h"][i - 1]
                t = [(o[i] - o[i - 1]) / h + h * (2.0 * g[i] + g[i - 1]) / 6.0 for o, g in ((r["E"], r["gamma_E"]), (r["N"], r["gamma_N"]))]
            v = math.hypot(t[0], t[1])
            nE, nN = -t[1] / v, t[0] / v
            for new, old in ((r["edge_L"][i], w[i]["edge_L"]), (r["edge_R"][i], w[i]["edge_R"])):
                after = (r["E"][i] * nE + r["N"][i] * nN) + new
                before = (w[i]["E"] * nE + w[i]["N"] * nN) + old
                bar = (abs(old) + max(abs(w[i]["E"]), abs(w[i]["N"]))) * 2.0 ** -50
                worst = max(worst, abs(after - before) / bar)
                assert abs(after - before) <= bar, (name, i)
        moved = np.abs(r["edge_L"] - np.array([p["edge_L"] for p in w]))
        print(f"{name}: walls kept within {worst:.2f} of the bar; the largest edge shift {moved.max():.3e} m")
        assert moved.max() > 0 or r["stats"]["dev_max"] == 0.0
        assert np.array_equal(r["edge_L"] - r["edge_R"] > 0, np.ones(n, dtype=bool))
    # the sign: a waypoint pushed to the LEFT of a path that runs north (psi = 0: left is -E) brings both edges down
    w = [cases.wp(0.0, 0.0), cases.wp(0.0, 1.0), cases.wp(0.5, 2.0), cases.wp(0.0, 3.0), cases.wp(0.0, 4.0)]
    r = twin.smooth(w, False, twin.smooth_set(lam=1.0, keep_walls=True))
    assert r["E"][2] < 0.5 and r["edge_L"][2] < 4.0 and r["edge_R"][2] < -4.0


def test_struct_layouts_and_the_default_set(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_smooth_set) == 120 and C.sizeof(L.pg_smooth_stats) == 72
    assert [getattr(L.pg_smooth_set, n).offset for n, _ in L.pg_smooth_set._fields_] == [0, 8, 40, 72, 104, 108, 112, 116]
    assert [getattr(L.pg_smooth_stats, n).offset for n, _ in L.pg_smooth_stats._fields_] == list(range(0, 72, 8))
    assert tuple(n for n, _ in L.pg_smooth_stats._fields_) == twin.STATS
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.SMOOTH_STATS_DTYPE.itemsize == 72 and mpc_mod.SMOOTH_STATS_DTYPE.names == twin.STATS
    V = pkg.vehicles
    assert V.smooth() == dict(lam=0.0, pin_ends=False, keep_walls=False, windows=[])
    assert V.smooth(lam=0.1, windows=[V.smooth_window(2, 6), V.smooth_window(5, 40, 4)]) == dict(lam=0.1, pin_ends=False, keep_walls=False, windows=[(2.0, 6.0, 0.0), (5.0, 40.0, 4.0)])
    with pytest.raises(KeyError):
        V.smooth(mu=1.0)
    with pytest.raises(ValueError):
        V.smooth(windows=[(0, 1, 0)] * 5)
    M = pkg.BatchedTrajectoryTrackingMPC
    arr = M.pack_smooths([V.smooth(), V.smooth(**cases.SETS[3]), V.smooth(lam=0.5, keep_walls=True, pin_ends=True)])
    assert (arr[0].lam, arr[0].n_win, arr[0].pin_ends, arr[0].keep_walls, arr[0].reserved) == (0.0, 0, 0, 0, 0) and list(arr[0].factor) == [1.0] * 4 and list(arr[0].u_hi) == [0.0] * 4
    assert arr[1].n_win == 2 and list(arr[1].u_lo) == [2.0, 5.0, 0.0, 0.0] and list(arr[1].u_hi) == [6.0, 40.0, 0.0, 0.0] and list(arr[1].factor) == [0.0, 4.0, 1.0, 1.0]
    assert (arr[2].lam, arr[2].pin_ends, arr[2].keep_walls) == (0.5, 1, 1)
    nan, inf = math.nan, math.inf
    for bad in (dict(lam=-1.0), dict(lam=nan), dict(lam=inf), dict(windows=[(2, 1, 0)]), dict(windows=[(nan, 1, 0)]), dict(windows=[(0, 1, -1)]), dict(windows=[(0, 1, inf)]),
                dict(windows=[(0, 1, nan)])):
        with pytest.raises(ValueError):
            M.pack_smooths([V.smooth(), V.smooth(**bad)])
    with pytest.raises(ValueError):
        M.pack_smooths([])
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_smooth_set
        f.restype = L.pg_smooth_set; f.argtypes = []
        assert bytes(f()) == bytes(arr[0])


def test_header_symbols_and_lists_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_smooth_set;              /* 120 bytes */" in hdr and "} pg_smooth_stats;            /* 72 bytes */" in hdr
    assert "pg_smooth_set pg_default_smooth_set(void);" in hdr
    for line_ in ("int pg_smooth_waypoints(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,",
                  "int32_t n_sets, const pg_smooth_set* sets, pg_waypoint* waypoints_out, pg_smooth_stats* stats);"):
        assert line_ in hdr, line_
    for phrase in ("Chords ", "U  ", "winv ", "System ", "Band ", "Open ", "Closed ", "Result ", "Walls ", "Stats ", "Sum ", "d_r = (D_r - (e2 l2_r)) - (c1 l1_r)", "y - (0 x)",
                   "tests/wp_smooth_numpy.py", "go through pg_smooth_waypoints below first"):
        assert phrase in hdr, phrase
    assert "the curvature of\n * noisy waypoints is the caller's to judge" not in hdr
    assert {"pg_smooth_waypoints", "pg_default_smooth_set"} <= set(pkg.SYMBOLS)
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_smooth_set) == 120 && sizeof(pg_smooth_stats) == 72" in api
    for doc in ("README.md", "DESIGN.md", "EXPERIMENTS.md", "INTEGRATION.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "smooth_waypoints" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.24" in design and "the curvature of noisy waypoints is the caller's to judge" not in design
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_wp_smooth" in check_f32_purity.TIME_KERNELS and "k_wp_smooth" in check_f32_purity.__doc__
    assert "pg_waypoint_smooth.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert '#include "pg_waypoint_smooth.hip"' in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()


def test_the_case_list_is_what_its_docstring_says():
    got = [(name, closed, len(w)) for name, closed, w in cases.paths()]
    assert got == [("open2", False, 2), ("open3", False, 3), ("open4", False, 4), ("open5", False, 5), ("closed5", True, 5), ("closed6", True, 6), ("closed7", True, 7),
                   ("open257", False, 257), ("open300", False, 300), ("closed257", True, 257), ("closed300", True, 300), ("open1100", False, 1100), ("closed1030", True, 1030),
                   ("skidpadoval", True, 999), ("vail", False, 1000)]
    assert len(cases.SETS) == 5 and [s["lam"] for s in cases.SETS] == [0.0, 0.1, 10.0, 1.0, 0.5]
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        h = row[0]["h"]
        assert h.min() > 0 and (len(w) < 4 or name in ("skidpadoval", "vail") or h.max() / h.min() > 1.2), name      # unequal chords (the recorded files are near equal)
        for r in row:
            assert np.all(np.isfinite(cases.as_bits(r))) and r["stats"]["chord_min"] > 0 and r["stats"]["width_min"] > 0, name
    # every set moves something on every path of three waypoints or more
    assert all(row[k]["stats"]["dev_max"] > 0 for (name, _, w), row in zip(cases.paths(), cases.reference()) if len(w) > 2 for k in (1, 2, 4))


def test_the_recurrence_helpers_as_a_stand_alone_host_program(tmp_path):
    """tests/wp_smooth_host_main.cpp calls the kernel's own __host__ __device__ helpers on the closed path of 5 and the open path of 3 waypoints; built with
    AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded and nothing is loaded into Python), it prints gamma, which the twin reproduces bit for bit."""
    exe = str(tmp_path / "wp_smooth_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pigeon.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wp_smooth_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    by_name = {name: (closed, w) for name, closed, w in cases.paths()}
    for name in ("closed5", "open3"):
        closed, w = by_name[name]
        ref = twin.smooth(w, closed, twin.smooth_set(lam=0.1))
        rows = [l for l in lines if l[0] == name and l[1] != "pivot_min"]
        assert len(rows) == len(w)
        for i, l in enumerate(rows):
            assert int(l[1]) == i and float.fromhex(l[2]) == ref["gamma_E"][i] and float.fromhex(l[3]) == ref["gamma_N"][i], (name, i, l)
        piv = [l for l in lines if l[0] == name and l[1] == "pivot_min"][0]
        assert float.fromhex(piv[2]) == ref["stats"]["pivot_min"] and piv[4] == piv[6]      # no bad row
