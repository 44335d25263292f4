"""pg_make_starts on the device against its float64 numpy twin (tests/start_make_numpy.py) over the shared case of tests/start_make_cases.py: three tubes (2, 1000 and
28 knots), eight sets, B = 64 (one lane past a wavefront would be B = 65: test_batch_independence runs B = 1 and a permuted 64, the refusals B = 4).

Everything outside sincos and steady_state is correctly rounded in both places: the expected difference is zero and zero is asserted.  E and N of the ego and of the other
car stay within start_make_cases.sincos_bars.  Measured on the MI355X (EXPERIMENTS 34): both libraries 0 of 64 instances differ in any channel outside steady 1 (bars
3.2e-13 m / 6.5e-13 m in fp64, 4.3e-5 m in fp32); steady 1: fp64 1.0e-16 of the largest entry (bar 1e-9), fp32 states 1.3e-7 per entry (bar 2e-5) and controls
3.0e-8 normalised (bar 1e-4)."""
import ctypes as C

import numpy as np
import pytest

import start_make_cases as cases
import start_make_numpy as twin
from path_libs import INVALID, OK, STATE, c_dp, c_i32p, get_state, handle, lib, step_bits

pytestmark = pytest.mark.gpu
c_u64p = C.POINTER(C.c_uint64)
KEYS = ("state", "control", "t0", "other", "time_offset", "placed")
SHAPES = dict(state=(6,), control=(3,), t0=(), other=(4,), time_offset=(), placed=(4,))
STEADY0 = cases.INDEX != cases.STEADY_SET


def library_handle(pkg, precision="f64", formulation="coupled", cap=cases.B, index=cases.TUBE_INDEX, **kw):
    m = pkg.BatchedTrajectoryTrackingMPC(list(cases.tubes()), cap, N_short=1, N_long=0, precision=precision, formulation=formulation, **kw)
    if index is not None:
        m.set_trajectory_index(index)
    return m


def raw(m, B, sets, n_sets=None, index=None, seed=cases.SEED, streams=None, install=0, null_sets=False):
    """the C call itself: (rc, the six arrays)"""
    arr = sets if isinstance(sets, C.Array) else m.pack_starts(sets)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint64)
    out = {k: np.full((max(B, 1),) + SHAPES[k], 7.0) for k in KEYS}
    rc = m.lib.pg_make_starts(m.h, B, len(arr) if n_sets is None else n_sets, None if null_sets else arr, None if idx is None else idx.ctypes.data_as(c_i32p),
                              C.c_uint64(seed), None if st is None else st.ctypes.data_as(c_u64p), install, *(out[k].ctypes.data_as(c_dp) for k in KEYS))
    return rc, out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def made(pkg):
    """the shared case through both libraries, once: {precision: the six arrays}"""
    out = {}
    for precision in ("f64", "f32"):
        m = library_handle(pkg, precision)
        rc, out[precision] = raw(m, cases.B, cases.sets(), index=cases.INDEX, streams=cases.STREAMS)
        assert rc == OK, m.lib.pg_last_error(m.h)
        m.close()
    return out


def against_twin(got, single, label):
    """the comparison of tests 1 and 3: bit for bit outside sincos and steady_state, the bars of the case module on E and N; prints the worst differences"""
    ref = cases.reference(single)
    for k in ("placed", "t0", "time_offset"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    s0 = STEADY0
    assert np.array_equal(bits(got["state"][s0, 3:]), bits(ref["state"][s0, 3:])) and np.array_equal(bits(got["control"][s0]), bits(ref["control"][s0]))
    assert np.array_equal(bits(got["state"][:, 2]), bits(ref["state"][:, 2])) and np.array_equal(bits(got["other"][:, 2:]), bits(ref["other"][:, 2:]))      # both headings and V_o: sums of exact terms
    ego, other = cases.sincos_bars(ref, single)
    d_ego = np.max(np.abs(got["state"][:, :2] - ref["state"][:, :2]), axis=1)
    d_oth = np.max(np.abs(got["other"][:, :2] - ref["other"][:, :2]), axis=1)
    print(f"{label} against the twin: ego E, N worst {d_ego.max():.3e} m ({np.count_nonzero(d_ego)} of {cases.B} instances differ; bar {ego.max():.3e}); "
          f"other car E, N worst {d_oth.max():.3e} m ({np.count_nonzero(d_oth)} differ; bar {other.max():.3e}); everything else identical bits")
    assert np.all(d_ego <= ego) and np.all(d_oth <= other), (d_ego.max(), d_oth.max())


def test_fp64_library_reproduces_the_twin(made):
    against_twin(made["f64"], np.float64, "fp64 library")


def test_steady_start_is_steady_state_estimates(made, pkg):
    """steady 1 against spec_numpy.steady_state_estimates (through the twin).  fp64: the bar tests/test_gpu_parity.py puts on the nodes of a cold step, 1e-9 relative to
    max(1, largest entry) -- the same device function seeds them.  fp32: the bars of tests/test_gpu_f32.py on the nodes, states 2e-5 relative per entry and the seeded
    controls 1e-4 of the control normalisation (delta_max, -Fx_min)."""
    veh = pkg.X1()
    un = np.array([veh["delta_max"], -veh["Fx_min"], -veh["Fx_min"]])
    s1 = ~STEADY0
    assert s1.sum() == 8
    for precision, single in (("f64", np.float64), ("f32", np.float32)):
        got, ref = made[precision], cases.reference(single)
        q, qr, u, ur = got["state"][s1, 3:], ref["state"][s1, 3:], got["control"][s1], ref["control"][s1]
        e_q = float(np.max(np.abs(q - qr) / np.maximum(1.0, np.abs(qr))))
        e_u = float(np.max(np.abs(u - ur) / un))
        rel_q = float(np.max(np.abs(q - qr)) / max(1.0, float(np.max(np.abs(qr)))))
        rel_u = float(np.max(np.abs(u - ur)) / max(1.0, float(np.max(np.abs(ur)))))
        print(f"steady 1, {precision}: (Ux, Uy, r) {e_q:.3e} relative per entry, {rel_q:.3e} of the largest; control {e_u:.3e} normalised, {rel_u:.3e} of the largest")
        if precision == "f64":
            assert rel_q < 1e-9 and rel_u < 1e-9
        else:
            assert e_q <= 2e-5 and e_u <= 1e-4
        assert np.all(u[:, 1] * u[:, 2] >= 0.0)                     # (Fxf, Fxr) is one total force split


def test_fp32_library_is_the_double_scheme_on_float_channels(made):
    got = made["f32"]
    for k in ("state", "control", "other"):
        assert np.array_equal(got[k], got[k].astype(np.float32).astype(np.float64)), k      # stored as float, widened
    against_twin(got, np.float32, "fp32 library")


@pytest.mark.parametrize("formulation", ["coupled", "decoupled"])
def test_install_equals_set_inputs_with_the_returned_arrays(pkg, formulation):
    a, b = library_handle(pkg, formulation=formulation), library_handle(pkg, formulation=formulation)
    rc, out = raw(a, cases.B, cases.sets(), index=cases.INDEX, streams=cases.STREAMS, install=1)
    assert rc == OK, a.lib.pg_last_error(a.h)
    a.B = cases.B
    b.set_inputs(out["state"], out["control"], out["t0"], other_car_state=out["other"], time_offset=out["time_offset"])
    res = []
    for m in (a, b):
        q0, u0 = get_state(m, cases.B)
        rc = m.lib.pg_simulate_dev(m.h, 6, C.c_double(0.01), None, None)
        assert rc == OK, m.lib.pg_last_error(m.h)
        res.append((q0, u0) + get_state(m, cases.B))
    for x, y in zip(*res):
        assert x.tobytes() == y.tobytes()                             # state, control and clock (t0 rides in the state array), before and after the run
    assert np.array_equal(res[0][0][:, :6], out["state"]) and np.array_equal(res[0][1], out["control"]) and np.array_equal(res[0][0][:, 6], out["t0"])
    ca, cb = a.simulate_clock(5, out["t0"], dt=0.01), b.simulate_clock(5, out["t0"], dt=0.01)
    assert ca.tobytes() == cb.tobytes()
    a.close(); b.close()


def test_batch_independence(pkg, made):
    ref = made["f64"]
    perm = np.random.default_rng(3).permutation(cases.B)
    m = library_handle(pkg, index=cases.TUBE_INDEX[perm])
    rc, out = raw(m, cases.B, cases.sets(), index=cases.INDEX[perm], streams=cases.STREAMS[perm])
    assert rc == OK
    for k in KEYS:
        assert out[k].tobytes() == ref[k][perm].tobytes(), k
    for b in (6, 23, 47, 63):                                         # alone: B = 1, the same (seed, stream, set, tube)
        m.set_trajectory_index(cases.TUBE_INDEX[b:b + 1])
        rc, one = raw(m, 1, cases.sets(), index=cases.INDEX[b:b + 1], streams=cases.STREAMS[b:b + 1])
        assert rc == OK
        for k in KEYS:
            assert one[k].tobytes() == ref[k][b:b + 1].tobytes(), (b, k)
        _, other_seed = raw(m, 1, cases.sets(), index=cases.INDEX[b:b + 1], streams=cases.STREAMS[b:b + 1], seed=cases.SEED + 1)
        _, other_stream = raw(m, 1, cases.sets(), index=cases.INDEX[b:b + 1], streams=cases.STREAMS[b:b + 1] + np.uint64(1))
        for o in (other_seed, other_stream):
            assert not np.array_equal(o["state"], one["state"]) and not np.array_equal(o["placed"][:, 1:3], one["placed"][:, 1:3]), b
    # streams = NULL is stream[b] = b, index = NULL is set 0
    m.set_trajectory_index(cases.TUBE_INDEX)
    _, x = raw(m, cases.B, cases.sets()[6:7])
    _, y = raw(m, cases.B, cases.sets()[6:7], index=np.zeros(cases.B, dtype=np.int32), streams=np.arange(cases.B))
    assert all(x[k].tobytes() == y[k].tobytes() for k in KEYS)
    m.close()


def test_geometry_against_the_projection(pkg, made):
    m = library_handle(pkg)
    out = m.make_starts(cases.sets(), index=cases.INDEX, seed=cases.SEED, streams=cases.STREAMS)
    assert all(out[k].tobytes() == made["f64"][k].tobytes() for k in KEYS) and m.B == cases.B
    m.compute_time_steps_(); m.compute_linearization_nodes_()
    sep = m.path_coordinates(); qs, _, _ = m.nodes()
    s, e, dpsi = out["placed"][:, 0], out["placed"][:, 1], out["placed"][:, 2]
    line = cases.TUBE_INDEX == 0
    d = np.abs(np.stack([sep[line, 0] - s[line], sep[line, 1] - e[line], qs[line, 0, 4] - dpsi[line]]))
    print(f"straight line: projection against placed (s, e, dpsi): worst {d.max(axis=1)}")
    assert d.max() <= 1e-9                                            # (the arithmetic error is of order 1e-13 at these magnitudes)
    t = cases.tubes()[1]
    sag = np.diff(t.s) ** 2 * np.maximum(np.abs(t.kappa[1:]), np.abs(t.kappa[:-1])) / 8.0      # chord sag of every interval of the fixture
    # The oval is closed: its first and last interval lie on top of each other, 0.52 mm apart in the fixture (the gap between knot 0 and the last knot).  A start within
    # one interval of either end may project onto the chord of the other end, so there the gap joins the sag (the case pins instances to both end knots)
    gap = float(np.hypot(t.E[0] - t.E[-1], t.N[0] - t.N[-1]))
    assert 5.2e-4 < gap < 5.3e-4
    worst = 0.0
    for b in np.flatnonzero(cases.TUBE_INDEX == 1):
        j = cases.reference()["look"][b]["j"]
        local = float(sag[max(j - 1, 0):j + 2].max())                 # the interval and its neighbours: the nearest chord may be the next one
        if s[b] <= t.s[1] or s[b] >= t.s[-2]:
            local += gap
        worst = max(worst, abs(sep[b, 1] - e[b]) - local)
        assert abs(sep[b, 1] - e[b]) <= local + 1e-9, (b, sep[b, 1], e[b], local)
    print(f"skidpadoval: |e projected - e placed| exceeds the local chord sag by at most {worst:.3e} m (largest sag {sag.max():.3e} m)")
    # e_mode 1: f = +1 / -1 lands on edge_L / edge_R as traj_edges_at_s gives them
    _, edge = raw(m, cases.B, [twin.start(s=(3.0, 30.0), e=1.0, e_mode=1), twin.start(s=(0.1, 0.9), s_mode=1, e=-1.0, e_mode=1)], index=cases.INDEX % 2, streams=cases.STREAMS)
    for b in range(cases.B):
        K = twin.lookup(twin.held(cases.tubes()[cases.TUBE_INDEX[b]]), edge["placed"][b, 0])
        want = K["edge_L"] if cases.INDEX[b] % 2 == 0 else K["edge_R"]
        assert abs(edge["placed"][b, 1] - want) <= 2.0 ** -52 * (abs(K["edge_L"]) + abs(K["edge_R"])), b      # (mid + half: two roundings of sums of the edges)
    m.close()


def test_every_refusal_leaves_inputs_and_clock_alone(pkg):
    m = handle(pkg, cap=8)                                            # one tube (skidpadoval)
    before = step_bits(m, pkg)
    S = lib().pg_start_set
    good = pkg.start(s=(3.0, 30.0), e=(-0.5, 0.5))

    def broken(**kw):
        arr = m.pack_starts([good, good])
        for k, v in kw.items():
            if k == "reserved":
                arr[1].reserved[2] = v
            else:
                setattr(arr[1], k, v)
        return arr
    two = m.pack_starts([good, good])
    calls = {"null sets": dict(B=4, sets=two, null_sets=True), "n_sets = 0": dict(B=4, sets=two, n_sets=0), "n_sets < 0": dict(B=4, sets=two, n_sets=-1),
             "B = 0": dict(B=0, sets=two), "B > capacity": dict(B=9, sets=two), "index < 0": dict(B=4, sets=two, index=[0, 1, -1, 0]),
             "index = n_sets": dict(B=4, sets=two, index=[0, 1, 2, 0]), "NaN": dict(B=4, sets=broken(e_lo=np.nan)), "Inf": dict(B=4, sets=broken(fx_hi=np.inf)),
             "lo > hi": dict(B=4, sets=broken(s_lo=31.0)), "v_lo = 0": dict(B=4, sets=broken(v_lo=0.0)), "v_lo < 0": dict(B=4, sets=broken(v_lo=-1.0)),
             "s_mode": dict(B=4, sets=broken(s_mode=2)), "e_mode": dict(B=4, sets=broken(e_mode=-1)), "steady": dict(B=4, sets=broken(steady=3)),
             "time_mode": dict(B=4, sets=broken(time_mode=2)), "other_mode": dict(B=4, sets=broken(other_mode=7)), "reserved": dict(B=4, sets=broken(reserved=1))}
    state, control, t0, toff = pkg.synthetic.config2_inputs(m.trajectories[0], 3, seed=8)
    for install in (0, 1):
        for name, kw in calls.items():
            m.set_inputs(state, control, t0, time_offset=toff)
            clock = m.simulate_clock(3, t0, dt=0.01)
            rc, out = raw(m, install=install, **kw)
            assert rc == INVALID and m.lib.pg_last_error(m.h).decode().startswith("pg_make_starts"), (name, rc)
            assert all(np.all(v == 7.0) for v in out.values()), name      # nothing was written
            q, u = get_state(m, 3)
            assert np.array_equal(q[:, :6], state) and np.array_equal(u, control) and np.array_equal(q[:, 6], t0) and m.B == 3, name
            assert m.simulate_clock(3, t0, dt=0.01).tobytes() == clock.tobytes(), name
            assert step_bits(m, pkg) == before, name
    m.close()
    # PG_ERR_STATE: several tubes and no trajectory index that covers B
    m = library_handle(pkg, cap=8, index=None)
    m.set_inputs(state, control, t0, time_offset=toff)
    assert raw(m, 4, [good], install=1)[0] == STATE
    m.set_trajectory_index([0, 1, 2])
    assert raw(m, 4, [good], install=1)[0] == STATE                   # (covers 3 of 4)
    q, u = get_state(m, 3)
    assert np.array_equal(q[:, :6], state) and np.array_equal(u, control) and np.array_equal(q[:, 6], t0)
    assert raw(m, 3, [good], install=0)[0] == OK
    m.close()


def test_other_car_reaches_the_safety_rollout(pkg, made):
    m = library_handle(pkg)
    out = m.make_starts(cases.sets(), index=cases.INDEX, seed=cases.SEED, streams=cases.STREAMS)
    res = m.simulate_safety_(3, dt=0.01, use_HJI_policy=False, record=True)
    hist = res[4]
    on = out["other"][:, 3] != 0.0
    assert on.sum() == 24 and np.array_equal(hist["other"][0], out["other"]) and np.array_equal(hist["state"][0], out["state"])
    for k in ("state", "control", "other", "human"):
        assert np.all(np.isfinite(hist[k])), k
    assert np.all(hist["V"] == np.inf)                                # (no grid: no value was looked up, which the record states as +Inf)
    assert np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[3]))
    m.close()
