"""GPU parity for (x0, reference-trajectory) instances: one handle carries a LIBRARY of TrajectoryTubes (the reference's test paths, ragged lengths)
and a per-instance selection; every instance must reproduce what a single-trajectory controller on ITS tube computes (oracle, one per tube).
Also covers the un-staged nodes kernel (a tube longer than the LDS staging limit of 2048 nodes)."""
import numpy as np
import pytest

import hji_live_cases as lc
import hji_solve_cases as solve_cases
import path_make_cases as cases
from conftest import make_oracle
from path_libs import handle, install_equals_set_trajectories, step_bits

pytestmark = pytest.mark.gpu

PATHS = ["skidpadoval", "vail", "EastPaddock", "variable_speed"]
B = 160


def rel_inf(a, b, floor=1.0):
    a = np.asarray(a); b = np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(floor, float(np.max(np.abs(b)))))


@pytest.fixture(scope="module")
def library(pkg, oracle_mod):
    tubes = [pkg.load_path_fixture(p) for p in PATHS]
    assert len({len(t) for t in tubes}) > 1                      # ragged on purpose
    idx = (np.arange(B) * 7 + 3) % len(tubes)
    state = np.zeros((B, 6)); control = np.zeros((B, 3)); t0 = np.zeros(B); toff = np.zeros(B)
    for k, t in enumerate(tubes):
        sel = np.where(idx == k)[0]
        s_, c_, t_, o_ = pkg.synthetic.config2_inputs(t, len(sel), seed=100 + k, s_range=None if t.s[-1] > 90 else (2.0, 0.4 * t.s[-1]))
        state[sel], control[sel], t0[sel], toff[sel] = s_, c_, t_, o_
    orcs = [make_oracle(oracle_mod, t) for t in tubes]
    return tubes, idx.astype(np.int32), state, control, t0, toff, orcs


def test_index_is_required(pkg, library):
    tubes, idx, state, control, t0, toff, _ = library
    mpc = pkg.BatchedTrajectoryTrackingMPC(tubes, B)
    mpc.set_inputs(state, control, t0, time_offset=toff)
    with pytest.raises(pkg.PigeonError):
        mpc.compute_time_steps_()
    with pytest.raises(pkg.PigeonError):
        mpc.set_trajectory_index(np.full(B, len(tubes), dtype=np.int32))     # out of range
    mpc.close()


def test_library_step_matches_single_trajectory_oracles(pkg, oracle_mod, library):
    tubes, idx, state, control, t0, toff, orcs = library
    mpc = pkg.BatchedTrajectoryTrackingMPC(tubes, B)
    mpc.set_trajectory_index(idx)
    u, status, _ = mpc.step_(state, control, t0, time_offset=toff)
    assert np.all(status == pkg.SOLVED), status
    sep = mpc.path_coordinates(); qs, us, ps = mpc.nodes(); qp = mpc.qp_data(); x, _ = mpc.solution()
    for b in range(B):
        orc = orcs[idx[b]]
        s, e, t, _ = orc.path_coordinates(state[b, 0], state[b, 1])
        assert abs(sep[b, 0] - s) <= 1e-9 * max(1, abs(s)) and abs(sep[b, 1] - e) <= 1e-9 and abs(sep[b, 2] - t) <= 1e-9 * max(1, abs(t)), b
        ts, dt = orc.time_steps(t0[b])
        oq, ou, op = orc.nodes(state[b], control[b], ts, dt, time_offset=toff[b])
        assert rel_inf(qs[b], oq) < 1e-9 and rel_inf(us[b], ou) < 1e-9 and rel_inf(ps[b], op) < 1e-9, b
        sd = orc.update_qp(oq, ou, op, dt, state[b], control[b], (0, 0, 0, 0))
        G = orc.unpack_sd(qp[b]); O = orc.unpack_sd(sd)
        for k in O:
            assert rel_inf(G[k], O[k]) < 1e-8, (b, k)
        if b % 4 == 0:
            xe, ye, info = orc.solve_exact(qp[b])
            assert info["status"] == 1
            assert rel_inf(x[b, 1, 6:], orc.split_x(xe)["u"][1]) < 1e-6, b
    # the same instances through four single-trajectory handles give bit-identical controls
    for k, t in enumerate(tubes):
        sel = np.where(idx == k)[0]
        one = pkg.BatchedTrajectoryTrackingMPC(t, len(sel))
        u1, st1, _ = one.step_(state[sel], control[sel], t0[sel], time_offset=toff[sel])
        assert np.array_equal(u1, u[sel]), k
        one.close()
    mpc.close()


def test_the_ways_a_library_arrives_replace_each_other(pkg, skidpad):
    """One handle, the three ways its trajectory library arrives in turn: pg_set_trajectory, pg_make_paths with install, pg_plan_speeds with install, pg_set_trajectories,
    pg_set_trajectory again.  After each library of several the handle computes, bit for bit, what a fresh handle computes that was given the same channels by
    pg_set_trajectories (and wants an index first: the previous one is dropped); the single trajectory it ends with gives the step it began with."""
    p, _ = cases.reference()
    m = handle(pkg)
    m.set_trajectory(skidpad)
    first = step_bits(m, pkg)

    def check(tubes, index, start_tube):
        L, ch, _ = m.pack_paths(tubes)                              # the channels the tubes were cut from, as pg_set_trajectories takes them
        b = handle(pkg)
        install_equals_set_trajectories(pkg, m, b, ch, L, ch.shape[2], np.array(index, dtype=np.int32), start_tube)
        b.close()

    made, _ = m.make_paths(p, n_knots=cases.N_KNOTS, V_ref=cases.V_REFS, pose=cases.POSES, closed=cases.CLOSED, install=True)
    assert len(made) == 5 and max(len(t) for t in made) == cases.LMAX
    check(made, [1, 1, 1, 1, 1], made[1])                           # the starts lie on the oval
    sets = [pkg.vehicles.speed_plan(mu_scale=0.5, V_max=12.0), pkg.vehicles.speed_plan(mu_scale=0.9, V_max=20.0, V_end=2.0)]
    planned, _ = m.plan_speeds([made[1], made[3]], sets, closed=[cases.CLOSED[1], cases.CLOSED[3]], install=True)
    assert len(planned) == 4
    check(planned, [0, 1, 0, 1, 1], planned[0])                     # the oval under both sets
    m.set_trajectories(planned)
    check(planned, [1, 0, 1, 0, 0], planned[0])
    m.set_trajectory(skidpad)
    assert step_bits(m, pkg) == first
    m.close()


@pytest.mark.parametrize("cell_dims", [3, 7])
def test_the_ways_an_hji_grid_arrives_replace_each_other(pkg, skidpad, cell_dims):
    """One coupled handle, its HJI table in turn: pg_set_hji_grid (the live grid), pg_hji_solve with install (the smallest grid of the solve tests), pg_clear_hji_grid,
    pg_set_hji_grid again.  After each the handle answers, bit for bit, as a fresh handle that received only that grid: the lookup at lookup_queries of the grid's knots,
    and the safety row after one cold step.  After the clear the lookup refuses and the row is the one of a handle that never had a grid."""
    live = lc.live_grid()
    knots_a, l0 = solve_cases.grid("A", False)
    solve = dict(install=True, fixed_dt=solve_cases.FIXED_DT, max_sweeps=solve_cases.SWEEPS)
    state, control, t0, toff, other = (a[:8] for a in lc.constraint_inputs(pkg, skidpad))

    def answers(m, knots):
        m.reset()
        m.step_(state, control, t0, other_car_state=other, time_offset=toff)
        out = b"".join(a.tobytes() for a in m.hji_constraint())
        if knots is None:
            with pytest.raises(pkg.PigeonError, match="no HJI grid installed"):
                m.hji_lookup(lc.lookup_queries(live[0])[0])
            return out
        V, g = m.hji_lookup(lc.lookup_queries(knots)[0])
        assert np.isfinite(V).sum() >= 50
        return out + V.tobytes() + g.tobytes()

    installs = [(live[0], lambda m: m.set_hji_cache(*live)), (knots_a, lambda m: m.solve_hji_cache(knots_a, l0, 1e9, **solve)), (None, lambda m: m.clear_hji_cache()),
                (live[0], lambda m: m.set_hji_cache(*live))]
    one = pkg.BatchedTrajectoryTrackingMPC(skidpad, 8, hji_eps=10.0, options={"hji_cell_dims": cell_dims})
    got, want = [], []
    for knots, install in installs:
        install(one)
        got.append(answers(one, knots))
        fresh = pkg.BatchedTrajectoryTrackingMPC(skidpad, 8, hji_eps=10.0, options={"hji_cell_dims": cell_dims})
        if knots is not None:
            install(fresh)
        want.append(answers(fresh, knots))
        fresh.close()
    one.close()
    assert got == want, [a == b for a, b in zip(got, want)]
    assert got[0] == got[3] and len({got[0], got[1], got[2]}) == 3          # (the three tables answer differently: none of the comparisons is of a handle with itself)


def test_long_tube_unstaged_nodes_kernel(pkg, oracle_mod, library):
    """A tube with more than 2048 nodes takes the global-memory search path of k_nodes; results must not depend on it."""
    tubes = library[0]
    t = tubes[0]
    # densify: insert two interior nodes per segment by the tube's own constant-acceleration law so the refined tube describes the same motion
    s = t.s; fine_s = np.unique(np.concatenate([s, s[:-1] + np.diff(s) / 3, s[:-1] + 2 * np.diff(s) / 3]))
    def lerp(ch): return np.interp(fine_s, s, ch)
    dense = pkg.TrajectoryTube(lerp(t.t), fine_s, lerp(t.V), lerp(t.A), lerp(t.E), lerp(t.N), lerp(t.psi), lerp(t.kappa))
    assert len(dense) > 2048
    n = 64
    state, control, t0, toff = pkg.synthetic.config2_inputs(dense, n, seed=5)
    mpc = pkg.BatchedTrajectoryTrackingMPC(dense, n)
    u, status, _ = mpc.step_(state, control, t0, time_offset=toff)
    assert np.all(status == pkg.SOLVED)
    qs, us, ps = mpc.nodes()
    orc = make_oracle(oracle_mod, dense)
    for b in range(n):
        ts, dt = orc.time_steps(t0[b])
        oq, ou, op = orc.nodes(state[b], control[b], ts, dt, time_offset=toff[b])
        assert rel_inf(qs[b], oq) < 1e-9 and rel_inf(us[b], ou) < 1e-9 and rel_inf(ps[b], op) < 1e-9, b
    mpc.close()
