"""GPU tests of the control-parameter library (pg_set_control_param_sets / pg_set_control_param_index): one handle carries K sets of control_params and a per-instance
selection; every instance must compute what a controller created with ITS set computes -- against the oracle (one per set) and, bit for bit, against handles created with
one set in pg_config.control and no library.

The sets (relative to pg_default_config) were checked on the CPU with the oracle on `skidpadoval`, synthetic.config2_inputs(traj, 96, seed=7): status 1 for 96 of 96 under
every set; the applied control differs from the default set's by 2e-4 .. 2e-2 (median) and 3e-3 .. 6e-2 (largest), set 2 moves the seeded nodes by up to 1.2, and Ux of the
batch (5.4 .. 6.6 m/s) lies inside set 4's bounds: a library that is silently ignored misses every comparison below by orders of magnitude."""
import numpy as np
import pytest

from conftest import make_oracle

pytestmark = pytest.mark.gpu

B = 160


def rel_inf(a, b, floor=1.0):
    a = np.asarray(a); b = np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(floor, float(np.max(np.abs(b)))))


def scaled(base, **factors):
    d = dict(base)
    for k, f in factors.items():
        d[k] = base[k] * f
    return d


def coupled_sets(pkg, n=5):
    d = dict(pkg.CoupledControlParams())
    sets = [dict(d),
            scaled(d, Q_e=4, Q_dpsi=0.25, R_ddelta=3),
            scaled(d, k_V=0.5, k_s=2, deltadot_max=0.6),
            scaled(d, W_beta=0.1, W_r=10, R_dFx=0.2, Q_ds=3),
            dict(d, V_min=3.0, V_max=8.0, R_delta=0.5, R_Fx=0.05),
            # three more, built the same way (test 4: their instances of the 256-instance sample are held against solve_exact like the others)
            scaled(d, Q_e=2, W_r=3, R_ddelta=0.5),
            scaled(d, k_V=2, Q_dpsi=3, R_dFx=4, deltadot_max=0.8),
            dict(scaled(d, W_beta=3, Q_ds=0.3), V_min=2.0, V_max=10.0, R_delta=0.1)]
    return sets[:n]


def lateral_sets(pkg):
    """the lateral subset of the fields in sets 0, 1, 2 and 4"""
    d = dict(pkg.DecoupledControlParams())
    return [dict(d), scaled(d, Q_e=4, Q_dpsi=0.25, R_ddelta=3), scaled(d, k_V=0.5, k_s=2, deltadot_max=0.6), dict(d, V_min=3.0, V_max=8.0, R_delta=0.5)]


@pytest.fixture(scope="module")
def batch(pkg, skidpad):
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=7)
    idx = ((7 * np.arange(B) + 3) % 5).astype(np.int32)
    return state, control, t0, toff, idx


def snapshot(m):
    qs, us, ps = m.nodes()
    st, it = m.solve_info()[:2]
    return dict(qs=qs, us=us, ps=ps, qp=m.qp_data(), st=st, it=it)


def assert_same_bits(mixed, uni, sel, what, skip=()):
    for k in mixed:
        if k not in skip:
            assert np.array_equal(mixed[k][sel], uni[k][sel]), (what, k)


def test_mixed_batch_against_the_oracle(pkg, oracle_mod, skidpad, batch):
    state, control, t0, toff, idx = batch
    sets = coupled_sets(pkg)
    orcs = []
    for cp in sets:
        o = make_oracle(oracle_mod, skidpad)
        o.set_control_params(**{k: cp[k] for k in o.CP_FIELDS})          # (by name: N_HJI sits at position 11 of the oracle's field order)
        orcs.append(o)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    mpc.set_control_params(sets, idx)
    u, status, _ = mpc.step_(state, control, t0, time_offset=toff)
    assert np.all(status == pkg.SOLVED), status
    qs, us, ps = mpc.nodes(); qp = mpc.qp_data(); x, _ = mpc.solution()
    worst = 0.0
    for b in range(B):
        orc = orcs[idx[b]]
        ts, dt = orc.time_steps(t0[b])
        oq, ou, op = orc.nodes(state[b], control[b], ts, dt, time_offset=toff[b])
        assert rel_inf(qs[b], oq) < 1e-9 and rel_inf(us[b], ou) < 1e-9 and rel_inf(ps[b], op) < 1e-9, b
        sd = orc.update_qp(oq, ou, op, dt, state[b], control[b], (0, 0, 0, 0))
        G = orc.unpack_sd(qp[b]); O = orc.unpack_sd(sd)
        for k in O:
            assert rel_inf(G[k], O[k]) < 1e-8, (b, k)
        xe, ye, info = orc.solve_exact(qp[b])
        assert info["status"] == 1, b
        err = rel_inf(x[b, 1, 6:], orc.split_x(xe)["u"][1]); worst = max(worst, err)
        assert err < 1e-6, (b, idx[b], err)
    print(f"mixed batch: max |u - u_exact| (normalised) = {worst:.2e}")
    got, gidx = mpc.control_param_sets()
    assert len(got) == 5 and np.array_equal(gidx, idx) and all(got[k][f] == sets[k][f] for k in range(5) for f in sets[k])
    mpc.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_mixed_coupled_batch_equals_uniform_handles_bit_for_bit(pkg, skidpad, batch, precision):
    state, control, t0, toff, idx = batch
    sets = coupled_sets(pkg)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, precision=precision)
    mpc.set_control_params(sets, idx)
    u, status, _ = mpc.step_(state, control, t0, time_offset=toff)
    mixed = dict(snapshot(mpc), u=u)
    ref_default = None
    for k, cp in enumerate(sets):
        one = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, control_params=cp, precision=precision)
        u1, _, _ = one.step_(state, control, t0, time_offset=toff)
        uni = dict(snapshot(one), u=u1)
        if k == 0:
            ref_default = u1
        else:            # the sets are not cosmetic: the uniform handles themselves differ
            assert np.max(np.abs(u1 - ref_default)) > 1e-5, k
        assert_same_bits(mixed, uni, idx == k, f"{precision} set {k}")
        one.close()
    mpc.close()


@pytest.mark.parametrize("N_short,N_long,walls", [(10, 20, False), (10, 40, True)])
def test_mixed_decoupled_batch_equals_uniform_handles_bit_for_bit(pkg, skidpad, batch, N_short, N_long, walls):
    """The only check of the lateral path (the oracle's decoupled handle has no parameter setter).  B = 160 runs one instance per wavefront (lat_single_max) in the
    mixed handle and in the uniform ones: the arrangement does not depend on the library."""
    state, control, t0, toff, _ = batch
    sets = lateral_sets(pkg)
    idx = ((7 * np.arange(B) + 3) % len(sets)).astype(np.int32)
    kw = dict(formulation="decoupled", N_short=N_short, N_long=N_long, walls=walls)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, **kw)
    mpc.set_control_params(sets, idx)
    u, status, _ = mpc.step_(state, control, t0, time_offset=toff)
    mixed = dict(snapshot(mpc), u=u)
    for k, cp in enumerate(sets):
        one = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, control_params=cp, **kw)
        u1, _, _ = one.step_(state, control, t0, time_offset=toff)
        assert_same_bits(mixed, dict(snapshot(one), u=u1), idx == k, f"decoupled N={N_short + N_long} set {k}")
        one.close()
    mpc.close()


def test_closed_loop_equals_uniform_handles_bit_for_bit(pkg, skidpad, batch):
    """simulate_ and simulate_node_ (with a pre_flag pattern that gates instances out) for 60 steps: the warm node branch and the warm solver start under a library."""
    state, control, t0, toff, idx = batch
    sets = coupled_sets(pkg)
    steps = 60
    rng = np.random.default_rng(11)
    pre = (rng.random((steps, B)) > 0.15).astype(np.uint8)

    def run(m):
        m.set_inputs(state, control, t0, time_offset=toff)
        s, c, t, qh, uh = m.simulate_(steps, record=True)
        m.reset(); m.set_inputs(state, control, t0, time_offset=toff)
        s2, c2, t2, o2, a2, H = m.simulate_node_(steps, pre_flag=pre, record=True)
        return dict(qh=np.moveaxis(qh, 1, 0), uh=np.moveaxis(uh, 1, 0), ns=np.moveaxis(H["state"], 1, 0), na=np.moveaxis(H["applied"], 1, 0), ne=np.moveaxis(H["event"], 1, 0))

    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    mpc.set_control_params(sets, idx)
    mixed = run(mpc)
    assert np.any(mixed["ne"] == 4)                     # PG_NODE_PRE_FLAG_OFF: some instances were gated out
    for k, cp in enumerate(sets):
        one = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, control_params=cp)
        assert_same_bits(mixed, run(one), idx == k, f"closed loop set {k}")
        one.close()
    mpc.close()


def test_large_coupled_batch_pipelined_and_split_paths(pkg, oracle_mod, skidpad):
    """B = 4096, 8 sets: the pipelined nodes + update_QP launch and the split solve read the library; same results as the launch-per-phase path and the single solve kernel."""
    Bl = 4096
    sets = coupled_sets(pkg, 8)
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, Bl, seed=7)
    idx = ((7 * np.arange(Bl) + 3) % 8).astype(np.int32)
    out = {}
    for piped in (True, False):
        mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, Bl, options={"solve_split": int(piped)})
        mpc.set_pipeline(int(piped))
        mpc.set_control_params(sets, idx)
        p0, s0 = mpc.get_option("stat_pipelined_launches"), mpc.get_option("stat_split_solve_launches")
        u, status, iters = mpc.step_(state, control, t0, time_offset=toff)
        if piped:
            assert mpc.get_option("stat_pipelined_launches") > p0 and mpc.get_option("stat_split_solve_launches") > s0 and mpc.pipeline_fallbacks() == 0
        else:
            assert mpc.get_option("stat_pipelined_launches") == p0 and mpc.get_option("stat_split_solve_launches") == s0
        assert np.all(status == pkg.SOLVED)
        out[piped] = dict(snapshot(mpc), u=u, x=mpc.solution()[0], iters=iters, pol=mpc.polish_info().copy())
        mpc.close()
    a, b = out[True], out[False]
    for k in ("qs", "us", "ps", "qp"):                                   # nodes and QP data: bit-identical across the launch shapes (fp64)
        assert np.array_equal(a[k], b[k]), k
    # split / single solve, as tests/test_gpu_full_size.py::test_split_solve_launch_gives_the_same_answers compares them: same status and iteration counts, controls of
    # two verified KKT points within 1e-8 per component (normalised), the same bits for the instances served by their active-set rounds in both launch shapes
    un = np.array([0.314159, 16793.7, 16793.7])
    assert np.array_equal(a["st"], b["st"]) and np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["it"], b["it"])
    both = (a["pol"] >= 1) & (b["pol"] >= 1)
    assert np.max(np.abs(a["u"][both] - b["u"][both]) / un) < 1e-8
    rounds_only = (a["iters"] == 0) & (b["iters"] == 0)
    assert (a["iters"] > 0).sum() >= 1                                   # (sets 2, 5 and 6 leave instances to the interior point: the list-mode launch had work to do)
    assert np.array_equal(a["u"][rounds_only], b["u"][rounds_only])
    orcs = []
    for cp in sets:
        o = make_oracle(oracle_mod, skidpad); o.set_control_params(**{k: cp[k] for k in o.CP_FIELDS}); orcs.append(o)
    for b in range(0, Bl, 16):                                           # 256-instance sample, every set 32 times
        xe, ye, info = orcs[idx[b]].solve_exact(out[True]["qp"][b])
        assert info["status"] == 1, b
        assert rel_inf(out[True]["x"][b, 1, 6:], orcs[idx[b]].split_x(xe)["u"][1]) < 1e-6, (b, idx[b])
    # against a default handle without a library on the same batch: the instances of set 0 (the defaults) have its nodes, QP data, status and iteration counts bit for
    # bit and -- served by their active-set rounds on both sides, whatever launch shape their batch-mates caused -- its controls; the instances of set 3 do not
    ref = pkg.BatchedTrajectoryTrackingMPC(skidpad, Bl)
    u0, st0, it0 = ref.step_(state, control, t0, time_offset=toff)
    r = snapshot(ref); s0 = idx == 0
    for k in ("qs", "us", "ps", "qp", "st", "it"):
        assert np.array_equal(a[k][s0], r[k][s0]), k
    assert np.all(it0[s0] == 0) and np.array_equal(a["u"][s0], u0[s0])
    assert np.max(np.abs(u0[idx == 3] - a["u"][idx == 3]) / un) > 1e-4
    ref.close()


def test_large_decoupled_batch_with_walls(pkg, skidpad):
    """Decoupled N = 50 + walls, B = 4096, 3 sets, against uniform handles stepping the same full batch: within 3e-7, the bound documented for two verified KKT points of one
    lateral QP across arrangements.  Which case holds: the library does not change the arrangement -- four instances per wavefront and the
    straggler hand-over in both handles (asserted through stat_lat_handover_solves), whose trip rule depends on each wavefront's own data only -- so the controls, the seeded
    nodes (k_V, k_s of set 2 reach Fx through k_nodes_dec) and the status are the uniform handles' bit for bit, which is asserted on top of the bound."""
    Bl = 4096
    sets = lateral_sets(pkg)[:3]
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, Bl, seed=7)
    idx = ((7 * np.arange(Bl) + 3) % 3).astype(np.int32)
    kw = dict(formulation="decoupled", N_short=10, N_long=40, walls=True)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, Bl, **kw)
    mpc.set_control_params(sets, idx)
    h0 = mpc.get_option("stat_lat_handover_solves")
    u, status, iters = mpc.step_(state, control, t0, time_offset=toff)
    assert mpc.get_option("stat_lat_handover_solves") > h0
    nodes = mpc.nodes()
    for k, cp in enumerate(sets):
        one = pkg.BatchedTrajectoryTrackingMPC(skidpad, Bl, control_params=cp, **kw)
        h1 = one.get_option("stat_lat_handover_solves")
        u1, st1, it1 = one.step_(state, control, t0, time_offset=toff)
        assert one.get_option("stat_lat_handover_solves") > h1
        sel = idx == k
        d = float(np.max(np.abs(u[sel, 0] - u1[sel, 0])))
        print(f"decoupled N=50 + walls, set {k}: max |delta - delta_uniform| = {d:.2e}, bit-exact: {np.array_equal(u[sel], u1[sel])}")
        assert np.array_equal(status[sel], st1[sel]), k
        assert d <= 3e-7, (k, d)
        assert np.array_equal(u[sel], u1[sel]) and np.array_equal(iters[sel], it1[sel]), k
        for x, y in zip(nodes, one.nodes()):
            assert np.array_equal(x[sel], y[sel]), k
        one.close()
    mpc.close()


def test_contract(pkg, skidpad, batch):
    state, control, t0, toff, idx = batch
    sets = coupled_sets(pkg)
    fresh = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    u_def, _, _ = fresh.step_(state, control, t0, time_offset=toff)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    mpc.set_control_params(sets)                                        # n_sets > 1, no index
    mpc.set_inputs(state, control, t0, time_offset=toff)
    with pytest.raises(pkg.PigeonError):
        mpc.compute_time_steps_()
    with pytest.raises(pkg.PigeonError):
        mpc.step_dev()
    mpc.set_control_param_index(idx)
    u_mix, _, _ = mpc.step_(state, control, t0, time_offset=toff)
    # rejected calls leave the handle as it was
    with pytest.raises(pkg.PigeonError):
        mpc.set_control_param_index(np.full(B, 5, dtype=np.int32))
    with pytest.raises(pkg.PigeonError):
        mpc.set_control_params([sets[0], dict(sets[1], N_HJI=sets[1]["N_HJI"] + 1)])
    with pytest.raises(pkg.PigeonError):
        mpc.set_control_params([sets[0], dict(sets[1], V_min=9.0, V_max=9.0)])
    with pytest.raises(pkg.PigeonError):
        mpc.set_control_params([dict(sets[0], R_ddelta=0.0)])
    with pytest.raises(pkg.PigeonError):
        mpc.set_control_params([dict(sets[0], Q_e=float("nan"))])
    mpc.reset()
    u_again, _, _ = mpc.step_(state, control, t0, time_offset=toff)
    assert np.array_equal(u_again, u_mix)
    # a library of one set == a handle created with that set
    mpc.set_control_params(sets[3])
    mpc.reset()                                                         # (the instances that already ran under set 3 kept their warm start: the comparison is of cold steps)
    u_one, _, _ = mpc.step_(state, control, t0, time_offset=toff)
    one = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, control_params=sets[3])
    u_ref, _, _ = one.step_(state, control, t0, time_offset=toff)
    assert np.array_equal(u_one, u_ref) and not np.array_equal(u_one, u_def)
    one.close()
    # cleared: the bits of a fresh default handle
    mpc.clear_control_params()
    assert mpc.control_param_sets()[0] == []
    mpc.reset()
    u_clr, _, _ = mpc.step_(state, control, t0, time_offset=toff)
    assert np.array_equal(u_clr, u_def)
    assert np.array_equal(snapshot(mpc)["qp"], snapshot(fresh)["qp"])
    mpc.close(); fresh.close()


def test_reindexing_resets_exactly_the_instances_whose_set_changed(pkg, skidpad, batch):
    """Two warm steps, then some instances move to another set: they must start cold (as an explicit reset(mask) on a handle that is driven alike), the others stay warm."""
    state, control, t0, toff, idx = batch
    sets = coupled_sets(pkg)
    idx2 = idx.copy(); moved = np.zeros(B, dtype=bool); moved[::3] = True
    idx2[moved] = (idx[moved] + 1) % 5
    a = pkg.BatchedTrajectoryTrackingMPC(skidpad, B); b = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    for m in (a, b):
        m.set_control_params(sets, idx)
        m.step_(state, control, t0, time_offset=toff)
        m.step_(state, control, t0 + 0.01, time_offset=toff)
    a.set_control_param_index(idx2)                                    # resets `moved` on its own
    b.reset(np.ones(B, dtype=np.uint8))                                # reference: everything cold under the new index ...
    b.set_control_param_index(idx2)
    c = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)                   # ... and: nothing moved, nothing reset
    c.set_control_params(sets, idx)
    c.step_(state, control, t0, time_offset=toff); c.step_(state, control, t0 + 0.01, time_offset=toff)
    c.set_control_param_index(idx)
    outs = []
    for m in (a, b, c):
        u, _, _ = m.step_(state, control, t0 + 0.02, time_offset=toff)
        outs.append(dict(snapshot(m), u=u))
    A, Bc, Cw = outs
    # moved instances: the cold node branch (seeded nodes) -- the bits of the handle that was reset as a whole
    assert_same_bits(A, Bc, moved, "moved instances start cold")
    # the others: the warm node branch (interpolated previous solution) -- the bits of the handle in which nothing changed
    assert_same_bits(A, Cw, ~moved, "unmoved instances stay warm")
    assert not np.array_equal(A["qs"][~moved], Bc["qs"][~moved])       # (warm and cold nodes do differ: the comparison above means something)
    for m in (a, b, c):
        m.close()


def test_fused_step_with_a_library(pkg, skidpad, batch):
    """pg_set_fusion(1): the wavefront that solves an instance linearises it first (linearize_pair inside k_solve reads the instance's steering-rate limit per lane)."""
    state, control, t0, toff, idx = batch
    sets = coupled_sets(pkg)
    outs = []
    for fuse in (0, 1):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
        m.set_fusion(fuse)
        m.set_control_params(sets, idx)
        u1, _, _ = m.step_(state, control, t0, time_offset=toff)
        cold = dict(snapshot(m), u=u1)
        u2, _, _ = m.step_(state, control, t0 + 0.01, time_offset=toff)
        outs.append((cold, dict(snapshot(m), u=u2))); m.close()
    every = np.ones(B, dtype=bool)
    assert_same_bits(outs[0][0], outs[1][0], every, "fused cold step")
    assert_same_bits(outs[0][1], outs[1][1], every, "fused warm step")


def test_graph_option_with_a_library(pkg, skidpad):
    """(a replayed step records no phase events: phase_ms() raising after a step is how a replay shows)"""
    n = 64
    sets = coupled_sets(pkg)
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, n, seed=7)
    idx = ((7 * np.arange(n) + 3) % 5).astype(np.int32)
    outs = []
    for graph in (0, 1):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, n, options={"graph": graph})
        m.set_control_params(sets, idx)
        us = [m.step_(state, control, t0 + 0.01 * k, time_offset=toff)[0] for k in range(4)]
        if graph:
            with pytest.raises(pkg.PigeonError):
                m.phase_ms()
        else:
            m.phase_ms()
        m.set_control_param_index(((idx + 1) % 5).astype(np.int32))    # a new index: the captured step must be re-captured
        us += [m.step_(state, control, t0 + 0.01 * (4 + k), time_offset=toff)[0] for k in range(4)]
        if graph:                                                      # (re-captured behind the cold step the new index caused, and replayed again)
            with pytest.raises(pkg.PigeonError):
                m.phase_ms()
        outs.append(np.array(us)); m.close()
    assert np.array_equal(outs[0], outs[1])
