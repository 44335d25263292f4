"""pg_optimize_line on the host: the twin (tests/line_opt_numpy.py, written from the scheme in include/pigeon_mpc.h) against a dense numpy.linalg restatement of the problem
it claims to solve, the properties that need no tolerance, the layouts and the lists, and the helpers of the kernel as a stand-alone host program under the sanitizers."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import line_opt_cases as cases
import line_opt_numpy as twin
from conftest import ROOT

SMALL = ("open5", "open64", "closed5", "closed63")


def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_the_twin_against_a_dense_restatement():
    """H and g rebuilt densely from A and W, the same ADMM with numpy.linalg.solve.  Both solves are backward stable, so one iterate of each is within
    c n 2^-53 cond(H + rho I) max|x| of the exact one; clip is non-expansive and so is an ADMM step in (z, u), so after k iterations the two alphas differ by at most
    k times the gap of one step.  The bar: 2 (two solves) * k * n * cond * 2^-53 * max|x|, with cond and max|x| taken from the dense side.  Measured (EXPERIMENTS 43): the
    worst ratio to the bar over the 16 pairs is 1.8e-2."""
    worst = 0.0
    for name in SMALL:
        closed, w = cases.path(name)
        n = len(w)
        for k, (s, r) in enumerate(zip(cases.sets_for(name), cases.reference(name))):
            d = twin.dense(w, closed, s)
            gap = float(np.max(np.abs(d["alpha"] - r["alpha"])))
            bar = 2.0 * d["iters_done"] * n * d["cond"] * 2.0 ** -53 * d["xmax"]
            print(f"{name} set {cases.SET_NAMES[k]}: cond(H + rho I) {d['cond']:.4g}, max |x| {d['xmax']:.3f}, {d['iters_done']} iterations, |alpha - dense| {gap:.3e} m, bar {bar:.3e} m")
            assert gap <= bar, (name, k, gap, bar)
            assert d["iters_done"] == r["stats"]["iters_done"]
            # the closed-form band is the dense H: the same entries within rounding of their size
            S = twin.system([q["E"] for q in w], [q["N"] for q in w], [q["edge_L"] for q in w], [q["edge_R"] for q in w], closed, s)
            Hb = np.zeros((n, n))
            for i in range(n):
                Hb[i, i] += S["D"][i]
                for off, band in ((1, S["E1"]), (2, S["E2"])):
                    j = (i + off) % n
                    if closed or i + off < n:
                        Hb[i, j] += band[i]; Hb[j, i] += band[i]
            assert np.max(np.abs(Hb - d["H"])) <= 64 * 2.0 ** -53 * np.max(np.abs(d["H"])), name
            assert np.max(np.abs(np.array(S["g"]) - d["g"])) <= 64 * 2.0 ** -53 * max(np.max(np.abs(d["g"])), 1e-300), name
            assert r["stats"]["bend_in"] == pytest.approx(d["bend_in"], rel=1e-12) and r["stats"]["bend_out"] == pytest.approx(d["bend_out"], rel=1e-9)
            worst = max(worst, gap / bar)
    print(f"worst |alpha - dense| / bar over {len(SMALL) * 4} pairs: {worst:.3e}")


def test_properties_that_need_no_tolerance():
    for name, closed, w in cases.paths():
        given = np.array([[p["E"], p["N"], p["edge_L"], p["edge_R"]] for p in w])
        row = cases.reference(name)
        for k, r in enumerate(row):
            st = r["stats"]
            # inside the box always, whatever the iteration count
            assert np.all(r["alpha"] >= r["lo"]) and np.all(r["alpha"] <= r["hi"]), (name, k)
            assert st["pivot_min"] > 0 and st["chord_min"] > 0 and st["width_min"] > 0 and np.all(np.isfinite(cases.as_bits(r))), (name, k)
            assert st["n_active"] == np.count_nonzero((r["alpha"] == r["lo"]) | (r["alpha"] == r["hi"]))
            # a waypoint that did not move returns its input bits
            still = r["alpha"] == 0.0
            assert cases.as_bits(r)[still, :2].tobytes() == given[still, :2].tobytes(), (name, k)
            # bend_out <= bend_in on every converged case
            if st["r_prim"] <= 1e-3 and st["r_dual"] <= 1e-3:
                assert st["bend_out"] <= st["bend_in"], (name, k)
        assert all(row[k]["stats"]["r_prim"] <= 1e-3 for k in (0, 2)) or name in cases.BIG, name
        # the pinning window: what only the first window holds keeps its margin of 0.25, what the later one holds is pinned
        r = row[1]
        U = r["U"]
        pinned = (U >= 10.0) & (U <= 20.0)
        assert np.all(r["alpha"][pinned] == 0.0) and np.all(r["lo"][pinned] == 0.0) and np.all(r["hi"][pinned] == 0.0), name
        assert cases.as_bits(r)[pinned].tobytes() == given[pinned].tobytes(), name
        first = (U >= 5.0) & (U < 10.0)
        assert np.all(r["hi"][first] == np.minimum(given[first, 2] - 0.25, 2.0)), name
        assert pinned.sum() >= 2 and first.sum() >= 1, name
        # keep_walls keeps edge - alpha ... + alpha invariant: the shifted edges plus the move are the surveyed ones, within one rounding of the edge
        for k in (1, 3):
            r = row[k]
            for col, out in ((2, r["edge_L"]), (3, r["edge_R"])):
                assert np.all(out == given[:, col] - r["alpha"]), (name, k)
                assert np.max(np.abs((out + r["alpha"]) - given[:, col])) <= 2.0 ** -52 * 8.0, (name, k)
        # without keep_walls the edges are copied
        for k in (0, 2):
            assert cases.as_bits(row[k])[:, 2:].tobytes() == given[:, 2:].tobytes(), (name, k)
        # pin_ends of an open path returns the ends' input bits; on a closed one the flag is not looked at
        r = row[3]
        if not closed:
            assert r["alpha"][0] == 0.0 and r["alpha"][-1] == 0.0 and cases.as_bits(r)[[0, -1]].tobytes() == given[[0, -1]].tobytes(), name
        else:
            s = dict(cases.sets_for(name)[3], pin_ends=False)
            assert cases.as_bits(twin.optimize(w, True, s)).tobytes() == cases.as_bits(r).tobytes(), name
        # the stop: the tol set ends early with both residuals within tol, and one iteration earlier at least one was not
        st = row[2]["stats"]
        s = cases.sets_for(name)[2]
        assert st["iters_done"] < s["iters"] and st["r_prim"] <= s["tol"] and st["r_dual"] <= s["tol"], name
        if st["iters_done"] > 1:
            before = twin.optimize(w, closed, dict(s, tol=0.0, iters=int(st["iters_done"]) - 1))["stats"]
            assert before["r_prim"] > s["tol"] or before["r_dual"] > s["tol"], name


def test_a_second_call_moves_less_than_the_first():
    """closed63 under keep_walls (the walls stay where they were surveyed), converged; the second call re-linearises about the first result"""
    closed, w = cases.path("closed63")
    s = twin.line_set(iters=1000, keep_walls=True, **cases.BASE)
    a = twin.optimize(w, closed, s)
    again = [dict(E=a["E"][i], N=a["N"][i], edge_L=a["edge_L"][i], edge_R=a["edge_R"][i]) for i in range(len(w))]
    b = twin.optimize(again, closed, s)
    print(f"closed63: first call moves by at most {a['stats']['alpha_abs_max']:.3f} m (r_prim {a['stats']['r_prim']:.2e}), the second by {b['stats']['alpha_abs_max']:.3f} m; "
          f"bend {a['stats']['bend_in']:.4f} -> {a['stats']['bend_out']:.4f} -> {b['stats']['bend_out']:.4f} (the second call's own bend_in {b['stats']['bend_in']:.4f})")
    assert a["stats"]["r_prim"] <= 1e-5 and b["stats"]["alpha_abs_max"] < a["stats"]["alpha_abs_max"]
    assert float(np.sqrt(np.mean(b["alpha"] ** 2))) < float(np.sqrt(np.mean(a["alpha"] ** 2)))


def test_the_normal_points_left_and_the_line_cuts_the_corner():
    """A path that runs north and turns left (west): the left normal at a waypoint of the northward leg is -E, and the least-bend line moves the corner's waypoints to the
    inside of the turn, alpha > 0"""
    w = [cases.shapes.wp(0.0, 3.0 * i) for i in range(6)] + [cases.shapes.wp(-3.0 * i, 15.0) for i in range(1, 6)]
    r = twin.optimize(w, False, twin.line_set(iters=300, **cases.BASE))
    assert (r["nE"][2], r["nN"][2]) == (-1.0, 0.0)
    assert r["alpha"][5] > 0.5 and r["E"][5] < 0.0 and r["N"][5] < 15.0 and r["stats"]["bend_out"] < r["stats"]["bend_in"]


def test_struct_layouts_defaults_and_packing(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_line_set) == 176 and C.sizeof(L.pg_line_stats) == 96
    assert [getattr(L.pg_line_set, n).offset for n, _ in L.pg_line_set._fields_] == [0, 8, 16, 24, 32, 40, 72, 104, 136, 152, 156, 160, 164, 168]
    assert tuple(n for n, _ in L.pg_line_stats._fields_) == twin.STATS
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.LINE_STATS_DTYPE.itemsize == 96 and mpc_mod.LINE_STATS_DTYPE.names == twin.STATS
    V = pkg.vehicles
    assert V.line() == dict(mu=1e-6, rho=0.1, margin=0.5, alpha_max=2.0, tol=0.0, iters=1000, pin_ends=False, keep_walls=False, windows=[])
    s = V.line(h_mean=2.0, margin=0.25, windows=[V.line_window(5, 12, 0.25), V.line_window(10, 20, pin=True)])
    assert s["mu"] == 1e-6 / 8.0 and s["rho"] == 0.1 / 8.0 and s["windows"] == [(5.0, 12.0, 0.25, 0), (10.0, 20.0, 0.5, 1)]
    with pytest.raises(KeyError):
        V.line(lam=1.0)
    with pytest.raises(ValueError):
        V.line(windows=[(0, 1, 0, 0)] * 5)
    with pytest.raises(ValueError):
        V.line(h_mean=0.0)
    M = pkg.BatchedTrajectoryTrackingMPC
    arr = M.pack_lines([V.line(), s, V.line(pin_ends=True, keep_walls=True, tol=1e-4, iters=7)])
    assert (arr[0].mu, arr[0].rho, arr[0].margin, arr[0].alpha_max, arr[0].tol, arr[0].iters, arr[0].n_win, arr[0].pin_ends, arr[0].keep_walls) == (1e-6, 0.1, 0.5, 2.0, 0.0, 1000, 0, 0, 0)
    assert arr[1].n_win == 2 and list(arr[1].u_lo) == [5.0, 10.0, 0.0, 0.0] and list(arr[1].win_margin) == [0.25, 0.5, 0.0, 0.0] and list(arr[1].win_pin) == [0, 1, 0, 0]
    assert (arr[2].pin_ends, arr[2].keep_walls, arr[2].tol, arr[2].iters) == (1, 1, 1e-4, 7)
    nan, inf = math.nan, math.inf
    for bad in (dict(mu=0.0), dict(mu=nan), dict(rho=-1.0), dict(rho=inf), dict(margin=-0.1), dict(alpha_max=0.0), dict(tol=-1.0), dict(tol=nan), dict(iters=0), dict(iters=4097),
                dict(windows=[(2, 1, 0, 0)]), dict(windows=[(nan, 1, 0, 0)]), dict(windows=[(0, 1, -1, 0)]), dict(windows=[(0, 1, inf, 0)])):
        with pytest.raises(ValueError):
            M.pack_lines([V.line(), V.line(**bad)])
    with pytest.raises(ValueError):
        M.pack_lines([])
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_line_set
        f.restype = L.pg_line_set; f.argtypes = []
        assert bytes(f()) == bytes(arr[0])


def test_header_symbols_and_lists_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_line_set;                /* 176 bytes */" in hdr and "} pg_line_stats;              /* 96 bytes */" in hdr
    assert "pg_line_set pg_default_line_set(void);" in hdr
    for line_ in ("int pg_optimize_line(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,",
                  "int32_t n_sets, const pg_line_set* sets, pg_waypoint* waypoints_out, pg_line_stats* stats);"):
        assert line_ in hdr, line_
    for phrase in ("Chords ", "Normal ", "Bend rows ", "Hessian ", "Box ", "Solve ", "Result ", "Stats ", "tests/line_opt_numpy.py", "waypoints_from_tube(every=)"):
        assert phrase in hdr[hdr.index("The line inside the tube"):], phrase
    assert {"pg_optimize_line", "pg_default_line_set"} <= set(pkg.SYMBOLS)
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_line_set) == 176 && sizeof(pg_line_stats) == 96" in api
    for doc in ("README.md", "DESIGN.md", "EXPERIMENTS.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "optimize_line" in open(os.path.join(ROOT, doc)).read(), doc
    assert "### 4.26" in open(os.path.join(ROOT, "DESIGN.md")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    assert "k_line_opt" in check_f32_purity.TIME_KERNELS and "k_line_opt" in check_f32_purity.__doc__
    assert "pg_line_opt.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    assert '#include "pg_line_opt.hip"' in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()
    assert "pg_line_opt.hip" in open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()


def test_the_case_list_is_what_its_docstring_says():
    got = [(name, closed, len(w)) for name, closed, w in cases.paths()]
    assert got == [("open5", False, 5), ("open64", False, 64), ("closed5", True, 5), ("closed63", True, 63), ("open1100", False, 1100), ("closed1030", True, 1030)]
    for name, closed, w in cases.paths():
        sets = cases.sets_for(name)
        assert len(sets) == 4 and all(s["iters"] == (8 if name in cases.BIG else sets[0]["iters"]) for s in sets)
        assert (len(w) if not closed else len(w) - 2) > 1024 or name not in cases.BIG      # both sides of the 1024 rows the kernel keeps in LDS
    assert all(cases.reference(n)[0]["stats"]["alpha_abs_max"] > 0 for n, _, _ in cases.paths())
    # the issue's converging case: the bend goes from 0.3601 to 0.2416 with 20 waypoints active
    st = cases.reference("closed63")[0]["stats"]
    assert round(st["bend_in"], 4) == 0.3601 and round(st["bend_out"], 4) == 0.2416 and st["n_active"] == 20 and st["r_prim"] < 1e-6


def test_the_helpers_as_a_stand_alone_host_program(tmp_path):
    """tests/line_opt_host_main.cpp calls the kernel's own __host__ __device__ helpers on the closed and the open path of 5 waypoints; built with AddressSanitizer and
    UBSan (a stand-alone program: nothing is preloaded and nothing is loaded into Python), it prints alpha, the box and U, which the twin reproduces bit for bit."""
    exe = str(tmp_path / "line_opt_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pigeon.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "line_opt_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    scale = 1.0 / (3.74 * 3.74 * 3.74)
    for name in ("closed5", "open5"):
        closed, w = cases.path(name)
        ref = twin.optimize(w, closed, twin.line_set(mu=1e-6 * scale, rho=0.1 * scale, margin=0.5, alpha_max=2.0, iters=40))
        rows = [l for l in lines if l[0] == name and l[1] != "stats"]
        assert len(rows) == len(w)
        for i, l in enumerate(rows):
            assert int(l[1]) == i and [float.fromhex(v) for v in l[2:6]] == [ref["alpha"][i], ref["lo"][i], ref["hi"][i], ref["U"][i]], (name, i, l)
        st = [l for l in lines if l[0] == name and l[1] == "stats"][0]
        assert (float.fromhex(st[2]), float.fromhex(st[3]), int(st[4]), float.fromhex(st[5])) == (ref["stats"]["r_prim"], ref["stats"]["r_dual"], int(ref["stats"]["iters_done"]),
                                                                                                   ref["stats"]["pivot_min"]) and st[7] == st[9]      # no bad row
