"""pg_offset_paths on the device against its float64 numpy twin (tests/path_offset_numpy.py) over the shared case of tests/path_offset_cases.py: six sources x seven offset
sets in one call, Lmax = 300.  Then the fp32 library (the fp64 library's output rounded to float), independence of the batch, the install path against
pg_set_trajectories, the chain pg_make_paths -> pg_offset_paths -> pg_plan_speeds and a rollout on the inner lane, a route event onto a lane change, every refusal, and
sets whose windows no path reaches.

fp64 library: every operation of the scheme is rounded once in both places, so t, s, V, A, kappa and both edges are the twin's bit for bit (they carry no libm call but
sqrt), and so is every stat but closure_pos.  psi carries atan2: within 8 * 2^-52 * max(pi, |psi|) (path_fit_cases.psi_bar).  E and N carry cos and sin of psi times d:
within 8 * 2^-52 * (|d| + |E or N|)."""
import math

import numpy as np
import pytest

import path_make_numpy as maker
import path_offset_cases as cases
from path_fit_cases import psi_bar
from path_libs import INVALID, OK, c_dp, c_i32p, drive, handle, install_equals_set_trajectories, lib, refusals, step_bits

pytestmark = pytest.mark.gpu

NP, NS = cases.N_PATH, cases.N_SETS
EXACT = ((0, "t"), (1, "s"), (2, "V"), (3, "A"), (7, "kappa"), (8, "edge_L"), (9, "edge_R"))
EXACT_STATS = ("length", "ds_min", "ds_max", "kappa_abs_max", "x_min", "d_abs_max", "n_outside", "reserved")


def raw_offset(m, L, cl, ch, sets, install=False):
    n = len(L) * len(sets)
    Lmax = ch.shape[2]
    out = np.full((n, 10, Lmax), np.nan)
    Lo = np.full(n, -1, dtype=np.int32); co = np.full(n, -1, dtype=np.int32)
    st = (lib().pg_offset_stats * n)()
    rc = m.lib.pg_offset_paths(m.h, len(L), Lmax, L.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), len(sets), sets, int(install),
                               Lo.ctypes.data_as(c_i32p), co.ctypes.data_as(c_i32p), out.ctypes.data_as(c_dp), st)
    assert rc == OK, m.lib.pg_last_error(m.h)
    return out, st, Lo, co


@pytest.fixture(scope="module")
def made(pkg):
    """the shared case through the fp64 library, once: (channels_out [42][10][300], stats, L_out, closed_out)"""
    m = handle(pkg)
    out = raw_offset(m, *cases.packed())
    m.close()
    return out


def test_fp64_library_against_the_twin(made):
    out, st, Lo, co = made
    ref = cases.reference()
    exp = cases.expected_channels()
    assert list(Lo) == [cases.N_KNOTS[k // NS] for k in range(NP * NS)] and list(co) == [cases.CLOSED[k // NS] for k in range(NP * NS)]
    worst = dict(psi=0.0, E=0.0, N=0.0); differ = dict(psi=0, E=0, N=0)
    for k in range(NP * NS):
        p, q = divmod(k, NS)
        n = cases.N_KNOTS[p]
        r = ref[p][q]
        assert np.all(out[k][:, n:] == 0.0), k
        for c, name in EXACT:
            assert out[k, c, :n].tobytes() == exp[k, c, :n].tobytes(), (p, q, name)
        dpsi = np.abs(out[k, 6, :n] - exp[k, 6, :n])
        dE = np.abs(out[k, 4, :n] - exp[k, 4, :n]); dN = np.abs(out[k, 5, :n] - exp[k, 5, :n])
        for name, d in (("psi", dpsi), ("E", dE), ("N", dN)):
            worst[name] = max(worst[name], float(d.max())); differ[name] += int(np.count_nonzero(d))
        assert np.all(dpsi <= psi_bar(exp[k, 6, :n])), (p, q)
        assert np.all(dE <= 8.0 * 2.0 ** -52 * (np.abs(r["d"]) + np.abs(exp[k, 4, :n]))), (p, q)
        assert np.all(dN <= 8.0 * 2.0 ** -52 * (np.abs(r["d"]) + np.abs(exp[k, 5, :n]))), (p, q)
        for f in EXACT_STATS:
            assert getattr(st[k], f) == r["stats"][f], (p, q, f)
        # closure_pos carries E and N of two knots
        assert abs(st[k].closure_pos - r["stats"]["closure_pos"]) <= 4 * 8.0 * 2.0 ** -52 * (abs(r["d"][0]) + float(np.max(np.abs(exp[k, 4:6, :n])))), (p, q)
    total = sum(cases.N_KNOTS) * NS
    print(f"worst |psi - twin| {worst['psi']:.3e} rad ({differ['psi']} of {total} knots differ), |E - twin| {worst['E']:.3e} m ({differ['E']}), |N - twin| {worst['N']:.3e} m ({differ['N']})")


def test_fp32_library_is_the_fp64_output_rounded(pkg, made):
    out, st, Lo, co = made
    m = handle(pkg, "f32")
    o32, s32, L32, c32 = raw_offset(m, *cases.packed())
    m.close()
    assert o32.tobytes() == out.astype(np.float32).astype(np.float64).tobytes()
    assert bytes(s32) == bytes(st) and L32.tobytes() == Lo.tobytes() and c32.tobytes() == co.tobytes()


def test_independence_of_the_batch(pkg, made):
    out, st, Lo, co = made
    m = handle(pkg)
    for p in range(NP):                                             # each pair alone, Lmax = the path's own knot count
        n = cases.N_KNOTS[p]
        for q in range(NS):
            one, s1, L1, c1 = raw_offset(m, *cases.packed([p], [q], Lmax=n))
            k = p * NS + q
            assert one[0].tobytes() == np.ascontiguousarray(out[k][:, :n]).tobytes(), (p, q)
            assert bytes(s1[0]) == bytes(st[k]) and L1[0] == n and c1[0] == cases.CLOSED[p], (p, q)
    rev, srev, _, _ = raw_offset(m, *cases.packed(reversed(range(NP))))
    for p in range(NP):
        for q in range(NS):
            a, b = (NP - 1 - p) * NS + q, p * NS + q
            assert rev[a].tobytes() == out[b].tobytes() and bytes(srev[a]) == bytes(st[b]), (p, q)
    rev, srev, _, _ = raw_offset(m, *cases.packed(which_sets=reversed(range(NS))))
    for p in range(NP):
        for q in range(NS):
            a, b = p * NS + (NS - 1 - q), p * NS + q
            assert rev[a].tobytes() == out[b].tobytes() and bytes(srev[a]) == bytes(st[b]), (p, q)
    two, s2, L2, _ = raw_offset(m, *cases.packed([3, 0, 3]))       # one source given twice
    for q in range(NS):
        assert two[q].tobytes() == two[2 * NS + q].tobytes() == out[3 * NS + q].tobytes() and bytes(s2[q]) == bytes(s2[2 * NS + q]) == bytes(st[3 * NS + q]), q
    # the Python method returns the same tubes and stats
    V = pkg.vehicles
    sets = [V.offset(), V.lane(3.5), V.lane(-3.5), V.lane_change(0, 1.5, 212, 217), V.lane_change(0, 5, 230, 330), V.pass_by(3, 20, 35, 45, 60), V.lane(2, edge_mode=1)]
    src = m.tubes_from_channels(np.array(cases.sources()), cases.N_KNOTS)
    tubes, stats = m.offset_paths(src, sets, closed=cases.CLOSED)
    for k, t in enumerate(tubes):
        n = cases.N_KNOTS[k // NS]
        assert len(t) == n and t.E.tobytes() == out[k, 4, :n].tobytes() and t.kappa.tobytes() == out[k, 7, :n].tobytes() and t.t.tobytes() == out[k, 0, :n].tobytes(), k
    assert stats["length"].tobytes() == np.array([s.length for s in st]).tobytes() and list(stats["n_outside"]) == [s.n_outside for s in st]
    m.close()


def test_install_equals_set_trajectories_with_the_returned_channels(pkg, made):
    out, st, Lo, co = made
    a, b = handle(pkg), handle(pkg)
    raw_offset(a, *cases.packed(), install=True)
    k = 3 * NS + 5                                                  # the starts lie on the oval's pass-by (2 .. 20 m: before the rise)
    tube = a.tubes_from_channels(out, cases.N_KNOTS, NS)[k]
    install_equals_set_trajectories(pkg, a, b, out, Lo, cases.LMAX, np.full(5, k, dtype=np.int32), tube)
    a.close(); b.close()


def test_the_chain_make_offset_plan_and_a_rollout_on_the_inner_lane(pkg):
    """pg_make_paths(oval) -> pg_offset_paths (lanes 0 and +3.5 m, the same road) -> pg_plan_speeds(install) with the closed flags: four instances from knots of the inner
    lane for 50 steps.  The oval turns left, so +3.5 m is the inner lane: radius 11 m in the bends, 0.091 1/m, which X1 steers (kappa_max = tan(18 deg) / L = 0.113 1/m).
    The plan uses mu_scale 0.3: `drive` starts an instance with zero steering wherever its knot lies, and at mu_scale 0.5 the one that starts on the clothoid into the bend
    (knot 80) returns statuses 2 and 3 on the source oval itself (lane 0) as on the inner lane, with X1 and with delta_max = 30 deg alike (EXPERIMENTS 37) -- the
    controller at that start, not the offset."""
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 4)
    vehicle = m.vehicle
    m.set_option("tracking_summary", 1)
    V = pkg.vehicles
    src, _ = m.make_paths([V.oval_segments(40.0, 14.5, 15.0)], n_knots=300, closed=True)
    lanes, ost = m.offset_paths(src, [V.lane(0.0), V.lane(3.5)], closed=[1])
    assert lanes[0].E.tobytes() == src[0].E.tobytes() and ost["kappa_abs_max"][1] == pytest.approx(1.0 / 11.0, rel=1e-12) and ost["length"][1] < ost["length"][0]
    assert vehicle["kappa_max"] > ost["kappa_abs_max"][1] and list(ost["n_outside"]) == [0, 0] and np.all(lanes[1].edge_L == src[0].edge_L - 3.5)
    planned, ps = m.plan_speeds(lanes, [V.speed_plan(mu_scale=0.3)], closed=[1, 1], install=True)
    print("inner / outer lane: length", ost["length"], "planned v_min", ps["v_min"], "v_max", ps["v_max"], "t_end", ps["t_end"])
    assert ps["v_max"][1] < ps["v_max"][0] and ps["v_min"][1] < ps["v_min"][0]      # the inner lane of the bend needs the slower profile
    m.set_trajectory_index(np.ones(4, dtype=np.int32))
    status, summary, first_exit = drive(m, planned[1], [5, 80, 150, 220], 50)
    print("inner lane: V", planned[1].V[[5, 80, 150, 220]], "max |e|", summary[:, 0], "first_exit", first_exit, "statuses", np.unique(status))
    assert np.all(pkg.is_solved(status)), np.unique(status)
    assert np.all(first_exit == -1), first_exit
    m.close()


def test_a_route_event_hands_over_the_lane_change(pkg):
    """A straight line of 100 m at 10 m/s, the sets identity and lane_change(0, 3.5, 30, 60), installed from the device buffer.  Eight instances start on the line between 2
    and 9 m; the odd ones carry a PROJECT event at step 5 onto trajectory 1.  After 640 steps of 0.01 s every instance is past s = 60 m (9 + 64 m at the most: the line is
    100 m long): the switched ones are within 0.3 m -- a tenth of the manoeuvre -- of the +3.5 m lane, the others of the line."""
    E0, N0, psi0, Vr = 3.0, -2.0, 0.4, 10.0
    line = maker.make([maker.segment(length=100.0)], 201, (E0, N0, psi0), Vr)
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 8)
    V = pkg.vehicles
    src = m.tubes_from_channels(maker.channels(line, 201)[None], [201])
    tubes, st = m.offset_paths(src, [V.offset(), V.lane_change(0.0, 3.5, 30.0, 60.0)], install=True)
    assert st["d_abs_max"][1] == 3.5 and tubes[1].kappa[60] == 0.0 and np.max(tubes[1].kappa) > 0.02
    m.set_trajectory_index(np.zeros(8, dtype=np.int32))
    m.set_routes([V.route(), V.route(V.route_event(5, 1, "project"))], np.arange(8) % 2)
    at = 4 + 2 * np.arange(8)                                       # knots 4 .. 18: s = 2 .. 9 m
    t = tubes[0]
    state = np.stack([t.E[at], t.N[at], t.psi[at], t.V[at], np.zeros(8), np.zeros(8)], axis=1)
    m.set_inputs(state, np.zeros((8, 3)), t.t[at], time_offset=np.zeros(8))
    final = m.simulate_(640, dt=0.01)[0]
    along = -(final[:, 0] - E0) * math.sin(psi0) + (final[:, 1] - N0) * math.cos(psi0)
    left = -(final[:, 0] - E0) * math.cos(psi0) - (final[:, 1] - N0) * math.sin(psi0)
    rs = m.route_state()
    print("along", along, "left of the line", left, "on trajectory", rs["traj"])
    assert list(rs["traj"]) == [0, 1] * 4 and np.all(along > 60.0) and np.all(along < 100.0)
    assert np.all(np.abs(left[1::2] - 3.5) <= 0.3) and np.all(np.abs(left[0::2]) <= 0.3)
    m.close()


def test_every_refusal_leaves_the_installed_library_alone(pkg):
    m = handle(pkg)
    before = step_bits(m, pkg)
    nan, inf = math.nan, math.inf

    def call(n_path=NP, n_sets=NS, Lmax=cases.LMAX, L=None, closed=None, knot=None, sset=None, null=None, paths=range(NP)):
        """the shared case with one edit: L = (path, value), closed = (path, value), knot = (path, channel, knot, value), sset = (set, field, value), null = an argument"""
        Lk, cl, ch, sets = cases.packed(paths)
        if L:
            Lk[L[0]] = L[1]
        if closed:
            cl[closed[0]] = closed[1]
        if knot:
            ch[knot[0], knot[1], knot[2]] = knot[3]
        for e in ([sset] if isinstance(sset, tuple) else sset or []):
            setattr(sets[e[0]], e[1], e[2])
        arg = dict(L=Lk.ctypes.data_as(c_i32p), ch=ch.ctypes.data_as(c_dp), sets=sets)
        if null:
            arg[null] = None
        return m.lib.pg_offset_paths(m.h, n_path, Lmax, arg["L"], cl.ctypes.data_as(c_i32p), arg["ch"], n_sets, arg["sets"], 1, None, None, None, None)

    big = 2**31 - 1
    refused = {
        "null L": dict(null="L"), "null channels": dict(null="ch"), "null sets": dict(null="sets"), "n_path 0": dict(n_path=0), "n_sets 0": dict(n_sets=0), "Lmax 1": dict(Lmax=1),
        "L 1": dict(L=(5, 1)), "L above Lmax": dict(L=(0, 301)), "closed with 2 knots": dict(closed=(5, 1)),
        "s equal": dict(knot=(4, 1, 7, float(cases.sources()[4, 1, 6]))), "s decreasing": dict(knot=(0, 1, 3, 5.0)),
        "s nan": dict(knot=(0, 1, 3, nan)), "E inf": dict(knot=(1, 4, 0, inf)), "N nan": dict(knot=(2, 5, 63, nan)), "psi nan": dict(knot=(3, 6, 100, nan)),
        "kappa inf": dict(knot=(3, 7, 258, -inf)), "edge_L nan": dict(knot=(4, 8, 27, nan)), "edge_R inf": dict(knot=(5, 9, 1, inf)),
        "V zero": dict(knot=(0, 2, 39, 0.0)), "V nan": dict(knot=(4, 2, 0, nan)), "t_0 inf": dict(knot=(1, 0, 0, inf)),
        "d0 nan": dict(sset=(0, "d0", nan)), "d1 inf": dict(sset=(1, "d1", inf)),
        "s_b = s_a": dict(sset=(3, "s_b", 212.0)), "s_b < s_a": dict(sset=(4, "s_b", 100.0)), "s_b inf": dict(sset=(4, "s_b", inf)), "s_a nan": dict(sset=(4, "s_a", nan)),
        "s_a -inf": dict(sset=(4, "s_a", -inf)), "s_b nan without a rise": dict(sset=(1, "s_b", nan)), "s_d nan without a fall": dict(sset=(3, "s_d", nan)),
        "s_d = s_c": dict(sset=(5, "s_d", 45.0)), "s_d nan": dict(sset=(5, "s_d", nan)), "s_c nan": dict(sset=(5, "s_c", nan)), "s_c < s_b": dict(sset=(5, "s_c", 34.0)),
        "a fall without a rise": dict(sset=[(1, "s_c", 30.0), (1, "s_d", 40.0)]),
        "x_min 0": dict(sset=(0, "x_min", 0.0)), "x_min above 1": dict(sset=(2, "x_min", 1.5)), "x_min nan": dict(sset=(6, "x_min", nan)),
        "edge_mode 2": dict(sset=(6, "edge_mode", 2)), "edge_mode -1": dict(sset=(0, "edge_mode", -1)), "reserved 1": dict(sset=(5, "reserved", 1)),
        # the pairs: lane(+15) on the oval's 14.5 m bends reaches the centre of curvature; the same lane with x_min above what the circle leaves
        "lane(+15) on the oval": dict(sset=[(1, "d0", 15.0), (1, "d1", 15.0)]), "x_min above 1 - d / R": dict(sset=(1, "x_min", 0.9)),
        # a closed path does not close: a window across the seam (the oval is 201.1 m long), the seam inside a window, the ends on different plateaus
        "rise across the seam": dict(sset=[(3, "s_a", 195.0), (3, "s_b", 205.0)]), "first knot inside a window": dict(sset=[(5, "s_a", -5.0)]),
        "ends on different plateaus": dict(sset=[(4, "s_a", 100.0), (4, "s_b", 110.0)]),
        "too many elements": dict(n_path=big, n_sets=1, Lmax=big), "n_path * n_sets past 31 bits": dict(n_path=big, n_sets=big),
    }
    assert call() == OK                                             # the unedited call is accepted (and installs: put the first library back)
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    refusals(m, pkg, call, refused, "pg_offset_paths", before)
    assert call(sset=[(1, "d0", 15.0), (1, "d1", 15.0)]) == INVALID
    msg = m.lib.pg_last_error(m.h).decode()
    assert "path 3, set 1, knot " in msg and "x_min" in msg, msg   # (the circles leave 1 - 15 / 20 = 0.25: the oval is the first pair below 0.1)
    # the same windows on the open sources alone are accepted
    assert call(n_path=3, paths=[0, 4, 5], sset=[(3, "s_a", 195.0), (3, "s_b", 205.0)]) == OK
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    m.close()
    # after the launch: knots that the offset brings so close that s' does not increase as a float holds it.  The circle with its s counted from 2^20 m (a float carries
    # 0.0625 m there; the source's own 2 m spacing survives) and a lane at x = 1 - kappa d = 2^-10, which shrinks ds to 2 mm; the fp64 library accepts the same call
    f = handle(pkg, "f32")
    before32 = step_bits(f, pkg)
    d = cases.CIRCLE_R * (1.0 - 2.0 ** -10)
    for h, want in ((f, INVALID), (handle(pkg), OK)):
        Lk, cl, ch, sets = cases.packed([1], [1])
        ch[0, 1, :64] += 2.0 ** 20
        sets[0].d0 = sets[0].d1 = d; sets[0].x_min = 2.0 ** -11
        rc = h.lib.pg_offset_paths(h.h, 1, cases.LMAX, Lk.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), 1, sets, 1, None, None, None, None)
        assert rc == want, h.lib.pg_last_error(h.h)
        if h is not f:
            h.close()
    assert f.lib.pg_last_error(f.h).decode().startswith("pg_offset_paths") and "dense" in f.lib.pg_last_error(f.h).decode()
    assert step_bits(f, pkg) == before32
    f.close()


def test_windows_no_path_reaches_are_not_looked_at_beyond_their_own_ranges(pkg, made):
    """A set is judged on its own ranges and on the knots of the paths it meets, nothing else: windows far beyond every path, and a plateau that would reach the centre of
    curvature if a path got there, are accepted and leave every path on d0 -- the identity's output."""
    out, st, Lo, co = made
    m = handle(pkg)
    Lk, cl, ch, _ = cases.packed()
    sets = (lib().pg_offset_set * 2)()
    for j, (a, b, c, d) in enumerate(((1e6, 1e6 + 1.0, math.inf, math.inf), (1e9, 2e9, 3e9, 4e9))):
        sets[j] = m.lib.pg_default_offset_set()
        sets[j].d1 = 1e4; sets[j].s_a = a; sets[j].s_b = b; sets[j].s_c = c; sets[j].s_d = d
    got, st2, _, _ = raw_offset(m, Lk, cl, ch, sets)
    for p in range(NP):
        for j in range(2):
            assert got[2 * p + j].tobytes() == out[p * NS].tobytes() and bytes(st2[2 * p + j]) == bytes(st[p * NS]), (p, j)
    m.close()
