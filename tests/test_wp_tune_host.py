"""pg_tune_smoothing on the host: the twin (tests/wp_tune_numpy.py, written from the scheme in include/pigeon_mpc.h) over the shared case -- the bracket it ends on, a
plain bisection inside it, monotone, the verdicts --, the layouts and the packer, the names the lists carry, and the search helpers of the kernel as a stand-alone host
program under the host sanitizers."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import wp_smooth_numpy as smooth_twin
import wp_tune_cases as cases
import wp_tune_numpy as twin
from conftest import ROOT


def lib_mod():
    return sys.modules["pigeon_jl_amd._lib"]


def test_the_bracket_the_twin_ends_on():
    """On every pair with verdict 0: F(lo) <= target < F(hi), lambda == lo, and hi / lo is the first ratio raised to 1 / 16^rounds_done.  The bar on the last: a
    ladder's step is four nested square roots of a product, each operation within 2^-53 relative, so a level moves the logarithm of a step by at most 2 * 2^-53 and a
    round by 8 * 2^-53 (a few ulp per level, as the issue puts it); narrowing to one step divides the ratio's logarithm by 16 and carries that error on.  After r rounds
    |log(hi / lo) - log(ratio) / 16^r| <= r * 16 * 2^-53, taken generously as 4 ulp per level and round."""
    seen = 0
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        for k, (t, r) in enumerate(zip(cases.SETS, row)):
            s = r["stats"]
            assert s["lam"] == s["lo"] and s["reserved"] == 0.0 and s["rms_lo"] == r["solve"]["stats"]["dev_rms"], (name, k)
            assert 1.0 <= s["rounds_done"] <= t["rounds"] and s["rounds_done"] == len(r["rounds"])
            if s["verdict"] >= 0:
                assert r["solve"]["stats"]["dev_rms"] <= t["target"], (name, k)
            if s["verdict"] != 0.0:
                assert s["lo"] == s["hi"] == (t["lambda_lo"] if s["verdict"] < 0 else t["lambda_hi"]) and s["rounds_done"] == 1.0 and s["rms_lo"] == s["rms_hi"], (name, k)
                assert (s["rms_lo"] > t["target"]) if s["verdict"] < 0 else (s["rms_hi"] <= t["target"]), (name, k)
                continue
            seen += 1
            base = dict(t["base"])
            F = lambda lam: smooth_twin.smooth(w, closed, dict(base, lam=lam))["stats"]["dev_rms"]
            assert F(s["lo"]) == s["rms_lo"] <= t["target"] < s["rms_hi"] == F(s["hi"]), (name, k)
            assert t["lambda_lo"] <= s["lo"] < s["hi"] <= t["lambda_hi"], (name, k)
            want = math.log(t["lambda_hi"] / t["lambda_lo"]) / 16.0 ** s["rounds_done"]
            got = math.log(s["hi"] / s["lo"]) if s["hi"] / s["lo"] > 1.0 + 2.0 ** -20 else math.log1p((s["hi"] - s["lo"]) / s["lo"])
            bar = s["rounds_done"] * 16.0 * 2.0 ** -53 + 2.0 ** -52      # (+ one ulp: the spacing of the doubles lo and hi themselves)
            print(f"{name} set {k}: bracket [{s['lo']!r}, {s['hi']!r}], log ratio {got:.6e} against {want:.6e}, rounds_done {s['rounds_done']:.0f}, monotone {s['monotone']:.0f}")
            assert abs(got - want) <= bar + 2.0 ** -52 * abs(want) * 4, (name, k, got, want)
    assert seen >= 20


def test_a_plain_bisection_lands_inside_the_bracket_where_monotone():
    """64 steps of bisection on dev_rms with math.sqrt midpoints from the set's own bounds: its last bracket lies inside the reported one wherever monotone is 1.  Every
    pair of the list with verdict 0, and the oval's own case."""
    seen = 0
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        for k, (t, r) in enumerate(zip(cases.SETS, row)):
            s = r["stats"]
            if s["verdict"] != 0.0 or s["monotone"] != 1.0:
                continue
            lo, hi = twin.bisect(w, closed, t, steps=64)
            seen += 1
            assert s["lo"] <= lo and hi <= s["hi"], (name, k, lo, hi, s["lo"], s["hi"])
    assert seen >= 25
    name, closed, w = cases.paths()[-1]
    s = cases.oval_reference()["stats"]
    lo, hi = twin.bisect(w, closed, cases.OVAL, steps=64)
    print(f"oval: the twin's bracket [{s['lo']!r}, {s['hi']!r}], dev_rms {s['rms_lo']:.4e} .. {s['rms_hi']:.4e}; 64 steps of bisection end on [{lo!r}, {hi!r}]")
    assert s["monotone"] == 1.0 and s["verdict"] == 0.0 and s["rounds_done"] == 2.0 and s["lo"] <= lo and hi <= s["hi"]
    assert s["hi"] == 0.1 and s["lo"] == pytest.approx(0.0947463525655, rel=1e-9)      # (the build container's figures; the device is compared with the twin)


def test_monotone_the_verdicts_and_the_two_waypoint_path():
    for (name, closed, w), row in zip(cases.paths(), cases.reference()):
        for k, r in enumerate(row):
            if k not in cases.WINDOWED:
                assert r["stats"]["monotone"] == 1.0, (name, k)
            for c, f in r["rounds"]:
                assert (r["stats"]["monotone"] == 0.0) or all(a <= b for a, b in zip(f, f[1:]))
        if len(w) > 2:
            assert row[5]["stats"]["verdict"] == -1.0 and row[5]["stats"]["lam"] == cases.LO, name
        assert row[6]["stats"]["verdict"] == 1.0 and row[6]["stats"]["lam"] == cases.HI, name
    two = cases.reference()[0]
    for r in two:                                                   # two waypoints have no row: F = 0 everywhere, verdict +1 in round 0, the waypoints come back
        assert r["stats"]["verdict"] == 1.0 and r["stats"]["rounds_done"] == 1.0 and r["stats"]["rms_hi"] == 0.0 and r["rounds"][0][1] == [0.0] * 17
        assert r["solve"]["stats"]["dev_max"] == 0.0
    # the early stop: closed5 under the narrow set ends after 7 of its 8 rounds, and the ladder of its last bracket repeats a candidate
    s = cases.reference()[2][2]["stats"]
    assert s["verdict"] == 0.0 and s["rounds_done"] == 7.0 and cases.SETS[2]["rounds"] == 8
    c = twin.ladder(s["lo"], s["hi"])
    assert any(a == b for a, b in zip(c, c[1:])) and s["lo"] < s["hi"]
    # every code path of the list is taken: a verdict 0 on either side of both LDS limits, 1, 2, 3 and 7 rounds done
    done = {r["stats"]["rounds_done"] for row in cases.reference() for r in row}
    assert {1.0, 2.0, 3.0, 7.0} <= done
    assert all(any(r["stats"]["verdict"] == 0.0 for r in cases.reference()[p]) for p in range(1, len(cases.paths())))


def test_the_ladder_by_hand():
    c = twin.ladder(1.0, 65536.0)                                   # 2^16: every product and root is exact
    assert c == [2.0 ** j for j in range(17)]
    c = twin.ladder(1e-4, 1e2)
    assert c[8] == math.sqrt(1e-4 * 1e2) and c[4] == math.sqrt(c[0] * c[8]) and c[12] == math.sqrt(c[8] * c[16]) and c[6] == math.sqrt(c[4] * c[8])
    assert c[7] == math.sqrt(c[6] * c[8]) and c[15] == math.sqrt(c[14] * c[16]) and all(a < b for a, b in zip(c, c[1:]))


def test_struct_layouts_the_default_set_and_the_packer(pkg):
    L = lib_mod()
    assert C.sizeof(L.pg_tune_set) == 152 and C.sizeof(L.pg_tune_stats) == 72
    assert [getattr(L.pg_tune_set, n).offset for n, _ in L.pg_tune_set._fields_] == [0, 120, 128, 136, 144, 148]
    assert [getattr(L.pg_tune_stats, n).offset for n, _ in L.pg_tune_stats._fields_] == list(range(0, 72, 8))
    assert tuple(n for n, _ in L.pg_tune_stats._fields_) == twin.TUNE_STATS
    mpc_mod = sys.modules["pigeon_jl_amd.mpc"]
    assert mpc_mod.TUNE_STATS_DTYPE.itemsize == 72 and mpc_mod.TUNE_STATS_DTYPE.names == twin.TUNE_STATS
    V = pkg.vehicles
    assert V.tune() == dict(base=V.smooth(), target=1e-3, lambda_lo=1e-6, lambda_hi=1e3, rounds=3)
    assert V.tune(target=2e-3, rounds=2, keep_walls=True, windows=[V.smooth_window(2, 6)]) == dict(base=V.smooth(keep_walls=True, windows=[(2.0, 6.0, 0.0)]), target=2e-3,
                                                                                                    lambda_lo=1e-6, lambda_hi=1e3, rounds=2)
    with pytest.raises(KeyError):
        V.tune(lam=0.1)
    with pytest.raises(KeyError):
        V.tune(mu=1.0)
    M = pkg.BatchedTrajectoryTrackingMPC
    arr = M.pack_tunes([V.tune(), cases.as_vehicle_set(cases.SETS[3])])
    assert (arr[0].target, arr[0].lambda_lo, arr[0].lambda_hi, arr[0].rounds, arr[0].reserved) == (1e-3, 1e-6, 1e3, 3, 0)
    assert bytes(arr[0].base) == bytes(M.pack_smooths([V.smooth()])[0])
    assert (arr[1].base.n_win, arr[1].base.pin_ends, arr[1].base.lam, arr[1].rounds, arr[1].target) == (1, 1, 0.0, 2, 1e-3)
    assert len(M.pack_tunes(V.tune())) == 1 and len(M.pack_tunes(arr[1])) == 1
    nan, inf = math.nan, math.inf
    for bad in (dict(target=0.0), dict(target=-1.0), dict(target=nan), dict(target=inf), dict(lambda_lo=0.0), dict(lambda_lo=-1.0), dict(lambda_lo=nan), dict(lambda_hi=inf),
                dict(lambda_lo=2.0, lambda_hi=2.0), dict(lambda_lo=3.0, lambda_hi=2.0), dict(rounds=0), dict(rounds=9), dict(windows=[(2, 1, 0)]), dict(windows=[(0, 1, -1)])):
        with pytest.raises(ValueError):
            M.pack_tunes([V.tune(), V.tune(**bad)])
    with pytest.raises(ValueError):
        M.pack_tunes([dict(V.tune(), base=V.smooth(lam=0.1))])       # the weight is what the call chooses
    with pytest.raises(ValueError):
        M.pack_tunes([dict(V.tune(), goal=1.0)])
    with pytest.raises(ValueError):
        M.pack_tunes([])
    rec = L.pg_tune_set(); C.memmove(C.byref(rec), C.byref(arr[0]), 152); rec.reserved = 1
    with pytest.raises(ValueError):
        M.pack_tunes([rec])
    lib = os.path.join(ROOT, "pigeon.jl_amd", "csrc", "libpigeon_hip.so")
    if os.path.exists(lib):                                         # (loading needs no device)
        f = C.CDLL(lib).pg_default_tune_set
        f.restype = L.pg_tune_set; f.argtypes = []
        assert bytes(f()) == bytes(arr[0])


def test_header_symbols_and_lists_carry_the_new_names(pkg):
    hdr = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    assert "} pg_tune_set;                     /* 152 bytes */" in hdr and "} pg_tune_stats;                   /* 72 bytes */" in hdr
    assert "pg_tune_set pg_default_tune_set(void);" in hdr
    for line_ in ("int pg_tune_smoothing(pg_handle* h, int32_t n_path, const pg_fit_spec* specs, int32_t n_wp_total, const pg_waypoint* waypoints,",
                  "int32_t n_sets, const pg_tune_set* sets, pg_waypoint* waypoints_out, pg_smooth_stats* stats, pg_tune_stats* tune);",
                  "pg_smooth_set base;            /* windows, pin_ends, keep_walls as pg_smooth_waypoints reads them; base.lambda must be 0 */"):
        assert line_ in hdr, line_
    for phrase in ("F  ", "Ladder ", "Round 0 ", "Narrowing ", "Rounds ", "monotone ", "Result ", "c_8 = sqrt((c_0 c_16))", "tests/wp_tune_numpy.py",
                   "Choosing lambda is pg_tune_smoothing below"):
        assert phrase in hdr, phrase
    assert "Left out: choosing lambda" not in hdr
    assert {"pg_tune_smoothing", "pg_default_tune_set"} <= set(pkg.SYMBOLS)
    api = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_api.hip")).read()
    assert "static_assert(sizeof(pg_tune_set) == 152 && sizeof(pg_tune_stats) == 72" in api
    for doc in ("README.md", "DESIGN.md", "EXPERIMENTS.md", "INTEGRATION.md", os.path.join("julia", "PigeonMI355X.jl"), os.path.join("tools", "README.md")):
        assert "tune_smoothing" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.25" in design and "Choosing `lambda` automatically (Reinsch's discrepancy criterion needs a search)" not in design
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_f32_purity
    import doc_numbers
    assert "k_wp_tune" in check_f32_purity.TIME_KERNELS and "k_wp_tune" in check_f32_purity.__doc__
    src = open(os.path.join(ROOT, "tools", "doc_numbers.py")).read()
    assert '"pg_waypoint_tune.hip"' in src and '"pg_waypoint_tune.hpp"' in src and "k_wp_tune" in doc_numbers.QUOTED
    assert "pg_waypoint_tune.hip" in open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "Makefile")).read()
    kernels = open(os.path.join(ROOT, "pigeon.jl_amd", "csrc", "pg_kernels.hip")).read()
    assert kernels.index('#include "pg_waypoint_smooth.hip"') < kernels.index('#include "pg_waypoint_tune.hip"')


def test_the_case_list_is_what_its_docstring_says():
    got = [(name, closed, len(w)) for name, closed, w in cases.paths()]
    assert got == [("open2", False, 2), ("open3", False, 3), ("closed5", True, 5), ("open256", False, 256), ("closed257", True, 257), ("open1100", False, 1100),
                   ("closed1030", True, 1030), ("skidpadoval", True, 999)]
    assert len(cases.SETS) == 8 and [t["rounds"] for t in cases.SETS] == [3, 1, 8, 2, 2, 3, 3, 3]
    assert cases.SETS[7] == twin.tune_set() == dict(base=smooth_twin.smooth_set(), target=1e-3, lambda_lo=1e-6, lambda_hi=1e3, rounds=3)      # pg_default_tune_set
    assert cases.SETS[3]["base"]["pin_ends"] and cases.SETS[3]["base"]["windows"][0][2] == 0.0 and cases.SETS[4]["base"]["keep_walls"]
    assert all(t["base"]["lam"] == 0.0 for t in cases.SETS)


def test_the_search_helpers_as_a_stand_alone_host_program(tmp_path):
    """tests/wp_tune_host_main.cpp calls the kernel's own __host__ __device__ helpers on the closed path of 5 and the open path of 3 waypoints with the candidates a row
    apart, as the kernel lays them out; built with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded and nothing is loaded into Python), it prints
    the ladder and F at every candidate, which the twin reproduces bit for bit, and the narrowing."""
    exe = str(tmp_path / "wp_tune_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pigeon.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wp_tune_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    for p, name in ((2, "closed5"), (1, "open3")):
        c, f = cases.reference()[p][0]["rounds"][0]
        rows = [l for l in lines if l[0] == name and l[1] not in ("narrow", "bad")]
        assert len(rows) == 17, r.stdout
        for j, l in enumerate(rows):
            assert int(l[1]) == j and float.fromhex(l[2]) == c[j] and float.fromhex(l[3]) == f[j], (name, j, l, c[j], f[j])
        nar = [l for l in lines if l[0] == name and l[1] == "narrow"][0]
        assert int(nar[2]) == min(k for k in range(1, 17) if f[k] > 2e-3) and nar[4] == "1" and nar[6] == "0"
    assert ["narrowest", "repeats", "1"] in lines
