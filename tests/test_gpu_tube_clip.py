"""pg_clip_tubes on the device against its float64 numpy twin (tests/tube_clip_numpy.py) over the shared case of tests/tube_clip_cases.py: six sources x thirteen obstacle
sets in one call, Lmax = 300.  Then the fp32 library (the fp64 library's output rounded to float), independence of the batch, the install path against
pg_set_trajectories, every refusal, the geometric chain make_paths -> clip_tubes -> pass_by_around -> offset_paths, and one rollout through and round the obstacle.

fp64 library: the eight copied channels, L_out, closed_out, every integer of the stats and the reports and every edge of a knot no obstacle touches are the twin's bit for
bit.  A touched edge and the report's doubles carry sin and cos of psi: within 8 * 2^-52 * (|wE| + |wN| + R) * (1 + |b| / h) of the twin, evaluated per knot with the
twin's own b and h (h -> R where the knot's |b| >= R).  The factor 8 is the one pg_offset_paths carries for the same sincos and a two-term product sum, (1 + |b| / h) is
the condition number of sqrt(R^2 - b^2).  The bar is derived, not measured; the measured maximum is printed (EXPERIMENTS 38)."""
import ctypes as C
import math

import numpy as np
import pytest

import tube_clip_cases as cases
import tube_clip_numpy as twin
from path_libs import OK, c_dp, c_i32p, handle, install_equals_set_trajectories, lib, refusals, step_bits

pytestmark = pytest.mark.gpu

NP, NS, MC = cases.N_PATH, cases.N_SETS, cases.MAX_COUNT
REPORT_DOUBLES = ("u_at", "a_at", "h_at", "dist_at", "free_left", "free_right")
REPORT_INTS = ("k_at", "k_first", "k_last", "side")


def raw_clip(m, L, cl, ch, sets, obs, install=False):
    n = len(L) * len(sets)
    Lmax = ch.shape[2]
    mc = max(s.count for s in sets)
    out = np.full((n, 10, Lmax), np.nan)
    Lo = np.full(n, -1, dtype=np.int32); co = np.full(n, -1, dtype=np.int32)
    st = (lib().pg_clip_stats * n)()
    rp = (lib().pg_obstacle_report * max(n * mc, 1))()
    C.memset(rp, 0xff, C.sizeof(rp))
    rc = m.lib.pg_clip_tubes(m.h, len(L), Lmax, L.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), len(sets), sets, len(obs), obs, int(install),
                             Lo.ctypes.data_as(c_i32p), co.ctypes.data_as(c_i32p), out.ctypes.data_as(c_dp), st, rp)
    assert rc == OK, m.lib.pg_last_error(m.h)
    return out, st, rp, Lo, co


def slots(rp, k, mc, count):
    """the bytes of the used report slots of pair k"""
    return bytes(rp)[k * mc * 64:(k * mc + count) * 64]


@pytest.fixture(scope="module")
def made(pkg):
    """the shared case through the fp64 library, once: (channels_out [78][10][300], stats, reports [78][64], L_out, closed_out)"""
    m = handle(pkg)
    out = raw_clip(m, *cases.packed())
    m.close()
    return out


def test_fp64_library_against_the_twin(made):
    out, st, rp, Lo, co = made
    ref = cases.reference()
    exp = cases.expected_channels()
    sets = cases.sets()
    assert list(Lo) == [cases.N_KNOTS[k // NS] for k in range(NP * NS)] and list(co) == [cases.CLOSED[k // NS] for k in range(NP * NS)]
    worst_edge = worst_rep = worst_ratio = 0.0
    touched = differ = 0
    for k in range(NP * NS):
        p, q = divmod(k, NS)
        n = cases.N_KNOTS[p]
        r = ref[p][q]
        assert np.all(out[k][:, n:] == 0.0), k
        for c in range(8):
            assert out[k, c, :n].tobytes() == exp[k, c, :n].tobytes(), (p, q, c)
        for c, bar in ((8, r["bar_L"]), (9, r["bar_R"])):
            d = np.abs(out[k, c, :n] - exp[k, c, :n])
            free = bar == 0.0
            assert out[k, c, :n][free].tobytes() == exp[k, c, :n][free].tobytes(), (p, q, c)
            assert np.all(d <= bar), (p, q, c, float(d.max()))
            worst_edge = max(worst_edge, float(d.max())); touched += int(np.count_nonzero(~free)); differ += int(np.count_nonzero(d))
            if (~free).any():
                worst_ratio = max(worst_ratio, float(np.max(d[~free] / bar[~free])))
        for f in twin.STATS_INTS:
            assert getattr(st[k], f) == r["stats"][f], (p, q, f)
        assert list(st[k].reserved) == [0, 0] and list(st[k].reserved_d) == [0.0, 0.0]
        assert st[k].u_width_min == r["stats"]["u_width_min"], (p, q)
        wbar = float(max(r["bar_L"].max(), r["bar_R"].max()))
        assert abs(st[k].width_min - r["stats"]["width_min"]) <= 2.0 * wbar, (p, q)
        for j in range(MC):
            got = rp[k * MC + j]
            if j >= sets[q]["count"]:
                assert bytes(got) == bytes(6 * 8) + np.array([-1, -1, -1, 0], dtype=np.int32).tobytes(), (p, q, j)
                continue
            want = r["report"][j]
            for f in REPORT_INTS:
                assert getattr(got, f) == want[f], (p, q, j, f)
            assert got.u_at == want["u_at"] and got.dist_at == want["dist_at"], (p, q, j)      # (no sincos in either)
            for f in REPORT_DOUBLES:
                d = abs(getattr(got, f) - want[f])
                assert d <= r["report_bar"][j], (p, q, j, f, d)
                worst_rep = max(worst_rep, d); worst_ratio = max(worst_ratio, d / r["report_bar"][j])
    print(f"worst |edge - twin| {worst_edge:.3e} m ({differ} of {touched} touched edges differ), worst |report double - twin| {worst_rep:.3e} m, worst difference / bar {worst_ratio:.3f}")


def test_fp32_library_is_the_fp64_output_rounded(pkg, made):
    out, st, rp, Lo, co = made
    m = handle(pkg, "f32")
    o32, s32, r32, L32, c32 = raw_clip(m, *cases.packed())
    m.close()
    assert o32.tobytes() == out.astype(np.float32).astype(np.float64).tobytes()
    assert bytes(s32) == bytes(st) and bytes(r32) == bytes(rp) and L32.tobytes() == Lo.tobytes() and c32.tobytes() == co.tobytes()


def test_independence_of_the_batch(pkg, made):
    out, st, rp, Lo, co = made
    sets = cases.sets()
    m = handle(pkg)
    for p in range(NP):                                             # each pair alone, Lmax = the path's own knot count
        n = cases.N_KNOTS[p]
        for q in range(NS):
            one, s1, r1, L1, c1 = raw_clip(m, *cases.packed([p], [q], Lmax=n))
            k = p * NS + q
            cnt = sets[q]["count"]
            assert one[0].tobytes() == np.ascontiguousarray(out[k][:, :n]).tobytes(), (p, q)
            assert bytes(s1[0]) == bytes(st[k]) and L1[0] == n and c1[0] == cases.CLOSED[p], (p, q)
            assert slots(r1, 0, cnt, cnt) == slots(rp, k, MC, cnt), (p, q)
    rev, srev, rrev, _, _ = raw_clip(m, *cases.packed(reversed(range(NP)), reversed(range(NS))))
    for p in range(NP):
        for q in range(NS):
            a, b = (NP - 1 - p) * NS + (NS - 1 - q), p * NS + q
            assert rev[a].tobytes() == out[b].tobytes() and bytes(srev[a]) == bytes(st[b]) and slots(rrev, a, MC, MC) == slots(rp, b, MC, MC), (p, q)
    big, sbig, rbig, _, _ = raw_clip(m, *_wider(cases.packed([3, 0, 3]), 777))      # a larger Lmax, one source given twice
    for q in range(NS):
        for a in (q, 2 * NS + q):
            assert np.ascontiguousarray(big[a][:, :cases.LMAX]).tobytes() == out[3 * NS + q].tobytes() and np.all(big[a][:, cases.LMAX:] == 0.0), q
            assert bytes(sbig[a]) == bytes(st[3 * NS + q]) and slots(rbig, a, MC, MC) == slots(rp, 3 * NS + q, MC, MC), q
    # the Python method returns the same tubes, stats and reports
    V = pkg.vehicles
    ob = [V.obstacle(*o) for o in cases.obstacles()]
    pol = {0: "centre", 1: "wider", 2: "left", 3: "right"}
    dsets = [V.obstacle_set(ob[s["first"]:s["first"] + s["count"]], margin=s["margin"], taper=s["taper"], min_width=s["min_width"], policy=pol[s["policy"]]) for s in sets]
    src = m.tubes_from_channels(np.array(cases.sources()), cases.N_KNOTS)
    tubes, stats, reports = m.clip_tubes(src, dsets, closed=cases.CLOSED)
    assert reports.shape == (NP * NS, MC)
    for k, t in enumerate(tubes):
        n = cases.N_KNOTS[k // NS]
        assert len(t) == n and t.edge_L.tobytes() == out[k, 8, :n].tobytes() and t.edge_R.tobytes() == out[k, 9, :n].tobytes() and t.E.tobytes() == out[k, 4, :n].tobytes(), k
    assert stats.tobytes() == bytes(st) and reports.tobytes() == bytes(rp)
    m.close()


def _wider(packed, Lmax):
    L, cl, ch, sets, obs = packed
    big = np.zeros((ch.shape[0], 10, Lmax))
    big[:, :, :ch.shape[2]] = ch
    return L, cl, big, sets, obs


def test_install_equals_set_trajectories_with_the_returned_channels(pkg, made):
    out, st, rp, Lo, co = made
    a, b = handle(pkg), handle(pkg)
    raw_clip(a, *cases.packed(), install=True)
    k = 3 * NS + 10                                                 # the starts lie on the oval under set 10 (2 .. 20 m: inside the taper that wraps the seam)
    tube = a.tubes_from_channels(out, cases.N_KNOTS, NS)[k]
    install_equals_set_trajectories(pkg, a, b, out, Lo, cases.LMAX, np.full(5, k, dtype=np.int32), tube)
    a.close(); b.close()


def test_every_refusal_leaves_the_installed_library_alone(pkg):
    m = handle(pkg)
    before = step_bits(m, pkg)
    nan, inf = math.nan, math.inf

    def call(n_path=NP, n_sets=NS, Lmax=cases.LMAX, n_obs=cases.N_OBS, L=None, closed=None, knot=None, sset=None, ob=None, null=None):
        """the shared case with one edit: L = (path, value), closed = (path, value), knot = (path, channel, knot, value), sset = (set, field, value), ob = (obstacle,
        field, value), null = an argument"""
        Lk, cl, ch, sets, obs = cases.packed()
        if L:
            Lk[L[0]] = L[1]
        if closed:
            cl[closed[0]] = closed[1]
        if knot:
            ch[knot[0], knot[1], knot[2]] = knot[3]
        for e in ([sset] if isinstance(sset, tuple) else sset or []):
            if e[1] == "pad":
                sets[e[0]].pad[1] = e[2]
            else:
                setattr(sets[e[0]], e[1], e[2])
        if ob:
            setattr(obs[ob[0]], ob[1], ob[2])
        arg = dict(L=Lk.ctypes.data_as(c_i32p), ch=ch.ctypes.data_as(c_dp), sets=sets, obs=obs)
        if null:
            arg[null] = None
        return m.lib.pg_clip_tubes(m.h, n_path, Lmax, arg["L"], cl.ctypes.data_as(c_i32p), arg["ch"], n_sets, arg["sets"], n_obs, arg["obs"], 1, None, None, None, None, None)

    big = 2**31 - 1
    refused = {
        "null L": dict(null="L"), "null channels": dict(null="ch"), "null sets": dict(null="sets"), "null obstacles": dict(null="obs"), "n_path 0": dict(n_path=0),
        "n_sets 0": dict(n_sets=0), "Lmax 1": dict(Lmax=1), "n_obs -1": dict(n_obs=-1), "n_obs too small": dict(n_obs=71),
        "L 1": dict(L=(5, 1)), "L above Lmax": dict(L=(0, 301)), "closed with 2 knots": dict(closed=(5, 1)),
        "s equal": dict(knot=(4, 1, 7, float(cases.sources()[4, 1, 6]))), "s decreasing": dict(knot=(0, 1, 3, 5.0)),
        "s nan": dict(knot=(0, 1, 3, nan)), "E inf": dict(knot=(1, 4, 0, inf)), "N nan": dict(knot=(2, 5, 63, nan)), "psi nan": dict(knot=(3, 6, 100, nan)),
        "kappa inf": dict(knot=(3, 7, 258, -inf)), "edge_L nan": dict(knot=(4, 8, 27, nan)), "edge_R inf": dict(knot=(5, 9, 1, inf)),
        "first -1": dict(sset=(1, "first", -1)), "first + count past the array": dict(sset=(12, "first", 9)), "count 65": dict(sset=[(12, "first", 0), (12, "count", 65)]),
        "count -1": dict(sset=(3, "count", -1)),
        "obstacle E nan": dict(ob=(0, "E", nan)), "obstacle N inf": dict(ob=(3, "N", inf)), "radius nan": dict(ob=(5, "radius", nan)), "radius inf": dict(ob=(70, "radius", inf)),
        "radius < 0": dict(ob=(5, "radius", -0.1)), "radius + margin 0": dict(ob=(1, "radius", 0.0)), "obstacle reserved": dict(ob=(2, "reserved", 1.0)),
        "margin -1": dict(sset=(6, "margin", -1.0)), "margin nan": dict(sset=(6, "margin", nan)), "margin inf": dict(sset=(0, "margin", inf)),
        "min_width -1": dict(sset=(5, "min_width", -1.0)), "min_width nan": dict(sset=(5, "min_width", nan)), "min_width inf": dict(sset=(0, "min_width", inf)),
        "taper 0": dict(sset=(2, "taper", 0.0)), "taper -1": dict(sset=(2, "taper", -1.0)), "taper nan": dict(sset=(0, "taper", nan)),
        "policy 4": dict(sset=(7, "policy", 4)), "policy -1": dict(sset=(0, "policy", -1)), "reserved 1": dict(sset=(5, "reserved", 1)), "pad": dict(sset=(4, "pad", 1.0)),
        "too many elements": dict(n_path=big, n_sets=1, Lmax=big), "n_path * n_sets past 31 bits": dict(n_path=big, n_sets=big),
    }
    assert call() == OK                                             # the unedited call is accepted (and installs: put the first library back)
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    refusals(m, pkg, call, refused, "pg_clip_tubes", before)
    # an obstacle no set uses is not looked at, and a call whose sets are all empty needs no obstacle array
    Lk, cl, ch, sets, obs = cases.packed(which_sets=[0, 1])
    obs[40].E = nan
    assert m.lib.pg_clip_tubes(m.h, NP, cases.LMAX, Lk.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), 2, sets, cases.N_OBS, obs, 0,
                               None, None, None, None, None) == OK
    Lk, cl, ch, sets, obs = cases.packed(which_sets=[0])
    out = np.full((NP, 10, cases.LMAX), nan)
    assert m.lib.pg_clip_tubes(m.h, NP, cases.LMAX, Lk.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), 1, sets, 0, None, 0,
                               None, None, out.ctypes.data_as(c_dp), None, None) == OK
    src = cases.sources()
    for p in range(NP):                                             # the identity: every channel of an open path bit for bit; a closed path's last edges are knot 0's
        n = cases.N_KNOTS[p]
        assert out[p][:, :n].tobytes() == np.ascontiguousarray(src[p][:, :n]).tobytes() and np.all(out[p][:, n:] == 0.0), p
    assert step_bits(m, pkg) == before
    m.close()


def straight(pkg, m):
    """a line of 200 m, 201 knots, tube +-4 m, at 10 m/s, and the same line clipped round one disc at 100 m, 0.3 m left of the centre, R = 1.5, taper 0.25"""
    V = pkg.vehicles
    src, _ = m.make_paths([V.line_segments(200.0)], n_knots=201, V_ref=10.0)
    disc = V.obstacle_at(src[0], 100.0, 0.3, 1.5)
    clipped, st, rep = m.clip_tubes(src, [V.obstacle_set([disc], taper=0.25)])
    return src, clipped, st, rep


def test_the_geometric_chain_make_clip_propose_offset(pkg):
    m = handle(pkg)
    V = pkg.vehicles
    src, clipped, st, rep = straight(pkg, m)
    assert np.all(src[0].edge_L == 4.0) and np.all(src[0].edge_R == -4.0)
    r = rep[0, 0]
    print("stats", st[0], "report", r)
    assert r["side"] == 1 and r["k_at"] == 100 and (r["k_first"], r["k_last"]) == (99, 101) and st["n_centre_out"][0] > 0 and st["n_clip_R"][0] == 0
    assert abs(clipped[0].edge_L[100] - (0.3 - 1.5)) <= 1e-12 and clipped[0].edge_R.tobytes() == src[0].edge_R.tobytes()
    proposed = V.pass_by_around(r, src[0], 30.0)
    assert abs(proposed["d1"] - 0.5 * ((0.3 - 1.5) - 4.0)) <= 1e-12 and (proposed["s_b"], proposed["s_c"]) == (99.0, 101.0)
    lanes, ost = m.offset_paths(clipped, [V.offset(), proposed])    # edge_mode 0: the same (clipped) road
    print("n_outside", ost["n_outside"])
    assert ost["n_outside"][1] == 0 and ost["n_outside"][0] > 0
    m.close()


def test_one_rollout_through_and_round_the_obstacle(pkg):
    """The clipped straight with [identity, proposed pass-by] installed as two trajectories, one instance on each, from 40 m on the line at 10 m/s (speed and ramp length
    of the lane-change rollout of tests/test_gpu_path_offset.py); 950 steps of 0.01 s take both past the obstacle at 100 m and past the end of the fall at 131 m.  The
    one that drives through leaves the clipped tube (first_exit >= 0), the one that goes round does not (-1); every step is solved."""
    m = pkg.BatchedTrajectoryTrackingMPC(pkg.load_path_fixture("skidpadoval"), 2)
    m.set_option("tracking_summary", 1)
    V = pkg.vehicles
    src, clipped, st, rep = straight(pkg, m)
    tubes, ost = m.offset_paths(clipped, [V.offset(), V.pass_by_around(rep[0, 0], src[0], 30.0)], install=True)
    m.set_trajectory_index(np.array([0, 1], dtype=np.int32))
    state = np.stack([np.array([t.E[40], t.N[40], t.psi[40], t.V[40], 0.0, 0.0]) for t in tubes])
    m.set_inputs(state, np.zeros((2, 3)), np.array([t.t[40] for t in tubes]), time_offset=np.zeros(2))
    steps = 950
    status = np.zeros((steps, 2), dtype=np.int32)
    for k in range(steps):                                          # (one step per call, as path_libs.drive: the step's statuses can be read)
        m.simulate_(1, dt=0.01)
        status[k] = m.solve_info()[0]
    summary, n_steps, first_exit = m.tracking_summary()
    print("first_exit", first_exit, "max |e|", summary[:, 0], "s of the last step", summary[:, 5], "statuses", np.unique(status))
    assert np.all(pkg.is_solved(status)), np.unique(status)
    assert first_exit[0] >= 0 and first_exit[1] == -1, first_exit
    m.close()
