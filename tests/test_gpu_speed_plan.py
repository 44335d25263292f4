"""pg_plan_speeds on the device against its float64 numpy twin (tests/speed_plan_numpy.py) over the shared case of tests/speed_plan_cases.py: three paths (open 130
knots, open 28 knots with non-uniform ds, closed 65 knots starting away from i0), Lmax = 130, 65 sets -- one set past a wavefront (lane = set), a
ragged library, both closures in one call.  Then determinism, the install path against pg_set_trajectories, every refusal, and one closed-loop condition.

fp64 library: every operation of the scheme is correctly rounded in both places, so the expected difference is zero: MEASURED_F64 = 0 on the MI355X, asserted as 8 x 0.
fp32 library against the float64 twin: MEASURED_F32 (largest relative difference of V over the valid knots, and of t_end), asserted at 8 x measured -- the factor of the
HJI solve's fp32 bound: it covers the change of rounding order between batch shapes, not more."""
import numpy as np
import pytest

import speed_plan_cases as cases
import speed_plan_numpy as twin
from path_libs import OK, c_dp, c_i32p, drive, handle, install_equals_set_trajectories, lib, refusals, step_bits

pytestmark = pytest.mark.gpu

MEASURED_F64 = {"V": 0.0, "A": 0.0, "t": 0.0, "stats": 0.0}
MEASURED_F32 = {"V": 7.72e-5, "t_end": 1.04e-5}                 # measured on the MI355X (EXPERIMENTS 27); the loss sits in along = sqrt(a_lim^2 - (W kappa)^2) near the cap


@pytest.fixture(scope="module")
def planned(pkg):
    """the shared case through the fp64 library, once: (channels_out [195][10][130], stats)"""
    p, closed, sets, vehs, _ = cases.reference()
    m = handle(pkg)
    out = raw_plan(m, p, closed, sets, vehs)
    m.close()
    return out


def raw_plan(m, paths, closed, sets, vehs=None, install=False):
    L, ch, cl = m.pack_paths(paths, closed)
    arr = m.pack_speed_plans(sets)
    veh = None if vehs is None else m.pack_vehicles(vehs)
    n = len(L) * len(arr)
    out = np.full((n, 10, ch.shape[2]), np.nan)
    st = (lib().pg_speed_plan_stats * n)()
    rc = m.lib.pg_plan_speeds(m.h, len(L), ch.shape[2], L.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), len(arr), arr, veh, int(install),
                              out.ctypes.data_as(c_dp), st)
    assert rc == OK, m.lib.pg_last_error(m.h)
    return out, st


def compare(out, st, single=np.float64):
    """largest differences of the library's result to the twin's over the shared case: {V, A, t: relative to the channel's scale; t_end, stats: relative}; also checks the
    copied channels and the zero tails bit for bit (against the input as the library's element type holds it)"""
    p, closed, sets, vehs, ref = cases.reference()
    ch_in = cases.channels_of(p, cases.LMAX).astype(single).astype(np.float64)
    worst = {"V": 0.0, "A": 0.0, "t": 0.0, "t_end": 0.0, "stats": 0.0}
    counts_equal = True
    for i, t in enumerate(p):
        n = len(t)
        for j in range(cases.N_SETS):
            k = i * cases.N_SETS + j; r = ref[i][j]; o = out[k]
            assert np.all(o[:, n:] == 0.0), (i, j)
            for c in (1, 4, 5, 6, 7, 8, 9):
                assert o[c, :n].tobytes() == ch_in[i, c, :n].tobytes(), (i, j, c)
            worst["V"] = max(worst["V"], float(np.max(np.abs(o[2, :n] - r["V"]) / r["V"])))
            worst["A"] = max(worst["A"], float(np.max(np.abs(o[3, :n] - r["A"])) / max(1.0, float(np.max(np.abs(r["A"]))))))
            worst["t"] = max(worst["t"], float(np.max(np.abs(o[0, :n] - r["t"])) / r["t"][-1]))
            s = st[k]; rs = r["stats"]
            worst["t_end"] = max(worst["t_end"], abs(s.t_end - rs["t_end"]) / rs["t_end"])
            for f in ("t_end", "v_min", "v_max", "usage_max"):
                worst["stats"] = max(worst["stats"], abs(getattr(s, f) - rs[f]) / max(abs(rs[f]), 1e-300))
            counts_equal &= (s.n_cap, s.n_accel, s.n_brake) == (rs["n_cap"], rs["n_accel"], rs["n_brake"])
            assert s.n_cap + s.n_accel + s.n_brake == n and s.reserved == 0, (i, j)
    return worst, counts_equal


def test_fp64_library_reproduces_the_twin(planned):
    out, st = planned
    worst, counts_equal = compare(out, st)
    print("fp64 library against the twin:", worst)
    for f in ("V", "A", "t", "stats"):
        assert worst[f] <= 8 * MEASURED_F64[f], (f, worst)
    assert counts_equal


def test_two_knots_one_set(pkg):
    t = pkg.straight_trajectory(12.0, 4.0)
    m = handle(pkg)
    sp = pkg.vehicles.speed_plan(V_max=9.0, V_start=1.0)
    out, st = raw_plan(m, [t], None, [sp])
    r = twin.plan(t.s, t.kappa, sp, pkg.X1())
    assert out[0, 2].tobytes() == r["V"].tobytes() and out[0, 3].tobytes() == r["A"].tobytes() and out[0, 0].tobytes() == r["t"].tobytes()
    assert (st[0].n_cap, st[0].n_accel, st[0].n_brake) == (r["stats"]["n_cap"], r["stats"]["n_accel"], r["stats"]["n_brake"])
    tubes, stats = m.plan_speeds(t, sp)
    assert len(tubes) == 1 and tubes[0].V.tobytes() == r["V"].tobytes() and stats["t_end"][0] == r["t"][-1] and np.all(tubes[0].theta == 0)
    m.close()


def test_fp32_library_against_the_float64_twin(pkg):
    p, closed, sets, vehs, _ = cases.reference()
    m = handle(pkg, "f32")
    out, st = raw_plan(m, p, closed, sets, vehs)
    m.close()
    worst, _ = compare(out, st, np.float32)                        # (limiter counts are not compared: ties fall differently in float)
    print("fp32 library against the float64 twin:", worst)
    assert worst["V"] <= 8 * MEASURED_F32["V"], worst
    assert worst["t_end"] <= 8 * MEASURED_F32["t_end"], worst


def test_determinism_and_independence_of_the_batch(pkg, planned):
    p, closed, sets, vehs, _ = cases.reference()
    out, st = planned
    m = handle(pkg)
    again, st2 = raw_plan(m, p, closed, sets, vehs)
    assert again.tobytes() == out.tobytes() and bytes(st2) == bytes(st)
    for lanes in (64, 32, 16):                                      # the sets per wavefront (chosen by the size of the call otherwise) do not show in the result
        m.set_option("speed_plan_lanes", lanes)
        again, st2 = raw_plan(m, p, closed, sets, vehs)
        assert again.tobytes() == out.tobytes() and bytes(st2) == bytes(st), lanes
    m.set_option("speed_plan_lanes", 0)
    for j in (0, 19, 64):
        one, s1 = raw_plan(m, p, closed, [sets[j]], [vehs[j]])
        for i in range(3):
            assert one[i].tobytes() == out[i * cases.N_SETS + j].tobytes(), (i, j)
            assert bytes(s1[i]) == bytes(st[i * cases.N_SETS + j]), (i, j)
    m.close()


def test_install_equals_set_trajectories_with_the_returned_channels(pkg, planned):
    p, closed, sets, vehs, _ = cases.reference()
    out, st = planned
    a, b = handle(pkg), handle(pkg)
    a.plan_speeds(p, sets, vehicles=vehs, closed=closed, install=True)
    # handle B: pg_set_trajectories with A's channels_out, L repeated
    L = np.repeat(np.array([len(t) for t in p], dtype=np.int32), cases.N_SETS)
    index = np.array([0, 7, 64, 3, 40], dtype=np.int32)              # path 0 (the starts lie on it) under five sets
    install_equals_set_trajectories(pkg, a, b, out, L, cases.LMAX, index, p[0])
    a.close(); b.close()


def test_every_refusal_leaves_the_installed_library_alone(pkg):
    p, closed, sets, vehs, _ = cases.reference()
    m = handle(pkg)
    before = step_bits(m, pkg)
    L, ch, cl = m.pack_paths(p, closed)
    arr = m.pack_speed_plans(sets[:2])
    veh = m.pack_vehicles([pkg.X1(), pkg.X1()])

    def call(n_path=3, Lmax=cases.LMAX, L_=L, cl_=cl, ch_=ch, n_sets=2, arr_=arr, veh_=None):
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return m.lib.pg_plan_speeds(m.h, n_path, Lmax, ptr(L_, c_i32p), ptr(cl_, c_i32p), ptr(ch_, c_dp), n_sets, arr_, veh_, 1, None, None)

    def edited(f):
        c = ch.copy(); f(c); return c

    def bad_set(**kw):
        a = m.pack_speed_plans(sets[:2])
        for k, v in kw.items():
            setattr(a[1], k, v)
        return a

    def bad_vehicle(**kw):
        v = m.pack_vehicles([pkg.X1(), pkg.X1()])
        for k, x in kw.items():
            setattr(v[1], k, x)
        return v

    refused = {
        "null L": dict(L_=None), "null channels": dict(ch_=None), "null sets": dict(arr_=None),
        "n_path 0": dict(n_path=0), "n_sets 0": dict(n_sets=0), "Lmax 1": dict(Lmax=1),
        "L below 2": dict(L_=np.array([130, 1, 65], dtype=np.int32)), "L above Lmax": dict(L_=np.array([131, 28, 65], dtype=np.int32)),
        "closed with 2 knots": dict(L_=np.array([130, 28, 2], dtype=np.int32)),
        "s not increasing": dict(ch_=edited(lambda c: c[1, 1].__setitem__(5, c[1, 1, 4]))),
        "non-finite geometry": dict(ch_=edited(lambda c: c[0, 8].__setitem__(129, np.inf))),
        "mu_scale 0": dict(arr_=bad_set(mu_scale=0.0)), "mu_scale inf": dict(arr_=bad_set(mu_scale=np.inf)), "V_max nan": dict(arr_=bad_set(V_max=np.nan)),
        "V_floor above V_max": dict(arr_=bad_set(V_floor=100.0)), "V_floor 0": dict(arr_=bad_set(V_floor=0.0)), "V_start negative": dict(arr_=bad_set(V_start=-1.0)),
        "V_end inf": dict(arr_=bad_set(V_end=np.inf)), "ax_max negative": dict(arr_=bad_set(ax_max=-0.1)), "ax_min positive": dict(arr_=bad_set(ax_min=0.1)),
        "ax_min nan": dict(arr_=bad_set(ax_min=np.nan)), "ay_max 0": dict(arr_=bad_set(ay_max=0.0)),
        "vehicle mu 0": dict(veh_=bad_vehicle(mu=0.0)), "vehicle Fx_min 0": dict(veh_=bad_vehicle(Fx_min=0.0)),
    }
    assert call(veh_=veh) == OK                                     # the unedited call is accepted (and installs: put the first library back)
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    refusals(m, pkg, call, refused, "pg_plan_speeds", before)
    # a geometry value past L[k] is not looked at
    assert call(ch_=edited(lambda c: c[1, 8].__setitem__(28, np.nan))) == OK
    m.close()


def test_the_plan_is_drivable(pkg):
    """Closed loop, a condition: skidpadoval (closed, all 1000 knots) planned at mu_scale = 0.5, V_max = 10 and installed; four instances start on the path at a straight,
    a corner entry, an apex and a corner exit at their knot's planned speed (Uy = 0, e = 0, r = V kappa) and run 200 steps of 0.01 s in trajectory mode at the default
    horizon.  Every step of every instance ends SOLVED or SOLVED_UNVERIFIED and no instance leaves the tube's edges; the file's own 6 m/s profile from the same starts
    meets the same two conditions."""
    path = pkg.load_path_fixture("skidpadoval")
    assert len(path) == 1000 and path.s[-1] - path.s[-2] > 0 and np.hypot(path.E[-1] - path.E[0], path.N[-1] - path.N[0]) < 1e-3
    ak = np.abs(path.kappa)
    corner = np.where(ak > 0.9 * ak.max())[0]
    runs = np.split(corner, np.where(np.diff(corner) > 1)[0] + 1)
    arc = max(runs, key=len)                                        # the longest run of knots at (nearly) the largest curvature
    straight = int(np.where(ak < 1e-6)[0][len(np.where(ak < 1e-6)[0]) // 2])
    entry = int(np.where(ak[:arc[0]] < 0.5 * ak.max())[0][-1]) if arc[0] > 0 else 0
    exit_ = int(arc[-1] + np.where(ak[arc[-1]:] < 0.5 * ak.max())[0][0])
    knots = [straight, entry, int(arc[len(arc) // 2]), exit_]
    m = pkg.BatchedTrajectoryTrackingMPC(path, 4)
    m.set_option("tracking_summary", 1)
    tubes, stats = m.plan_speeds(path, pkg.vehicles.speed_plan(mu_scale=0.5, V_max=10.0), closed=True, install=True)
    print("planned: ", {n: float(stats[n][0]) for n in stats.dtype.names}, "starts at knots", knots)
    for name, tube in (("file", path), ("planned", tubes[0])):
        if name == "file":
            m.set_trajectory(path)
        else:
            m.plan_speeds(path, pkg.vehicles.speed_plan(mu_scale=0.5, V_max=10.0), closed=True, install=True)
        status, summary, first_exit = drive(m, tube, knots, 200)
        print(name, "profile: max |e|", summary[:, 0], "min Ux", summary[:, 4], "first_exit", first_exit, "statuses", np.unique(status))
        assert np.all(pkg.is_solved(status)), (name, np.unique(status))
        assert np.all(first_exit == -1), (name, first_exit)
    m.close()
