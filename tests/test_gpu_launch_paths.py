"""Every launch arrangement of the step (launch_nodes / launch_solve / update_and_solve in csrc/pg_api.hip) at the smallest shapes that still select it: the thresholds are
lowered through the existing options, not by large batches.  Each case checks that the arrangement it names was the one that ran (the read-only "stat_*" options), that
every instance ends solved, and that its answer is the plain sequence's: the same bits for the coupled formulation (the arrangements run the same per-instance arithmetic),
the same point for the lateral one (its arrangements end at different verified KKT points of the same QP: tests/test_gpu_decoupled.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUPLED_STATS = ("stat_split_solve_launches", "stat_single_solve_launches")
LATERAL_STATS = ("stat_lat_one_per_wavefront_solves", "stat_lat_handover_solves", "stat_lat_two_launch_solves")
PLAIN_LATERAL = {"lateral_solver": 1, "lat_handover": 0, "lat_single_max": 0, "lat_split": 0}


def coupled_case(pkg, traj, B, N_long, options=None, fusion=0, pipeline=1, seed=12345):
    """One cold step of a coupled handle; returns (u, status, iters) and the growth of every launch counter."""
    names = COUPLED_STATS + ("stat_pipelined_launches",)
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=seed)
    mpc = pkg.BatchedTrajectoryTrackingMPC(traj, B, N_short=10, N_long=N_long, options=options, phase_timing=False)
    mpc.set_fusion(fusion); mpc.set_pipeline(pipeline)
    before = {n: mpc.get_option(n) for n in names}
    out = mpc.step_(state, control, t0, time_offset=toff)
    grew = {n: mpc.get_option(n) - before[n] for n in names}
    mpc.close()
    return out, grew


def lateral_case(pkg, traj, B, options, steps=1, seed=12345):
    """`steps` steps of a lateral handle on the same inputs (the first cold, the others warm); returns the last step's (u, status, iters) and what it added to the counters."""
    state, control, t0, toff = pkg.synthetic.config2_inputs(traj, B, seed=seed)
    mpc = pkg.DecoupledTrajectoryTrackingMPC(pkg.X1(), traj, B, N_short=10, N_long=10, options=options, phase_timing=False)
    assert mpc.get_option("lateral_solver_in_use") == 1.0
    for k in range(steps):
        before = {n: mpc.get_option(n) for n in LATERAL_STATS}
        out = mpc.step_(state, control, t0, time_offset=toff)
    grew = {n: mpc.get_option(n) - before[n] for n in LATERAL_STATS}
    mpc.close()
    return out, grew


def only(grew, family, name):
    """The counter `name` of `family` increased and no other one of the family did (name None: none did)."""
    return all((grew[n] > 0) == (n == name) for n in family)


def same_bits(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def same_point(pkg, a, b):
    """The bound of test_decoupled_matches_oracle on the applied control: steering within 1e-6, the rest to 1e-9 relative."""
    (u, st, _), (v, sv, _) = a, b
    return pkg.is_solved(st).all() and pkg.is_solved(sv).all() and np.max(np.abs(u[:, 0] - v[:, 0])) <= 1e-6 and \
        np.max(np.abs(u[:, 1:] - v[:, 1:])) <= 1e-9 * max(1.0, np.max(np.abs(v)))


# ---- coupled formulation, N = 30: pipelined nodes + update, split / single solve, fused ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain30(pkg, skidpad):
    """The plain sequence: one launch per phase, one solve kernel."""
    out, grew = coupled_case(pkg, skidpad, 128, 20, {"solve_split": 0}, fusion=0, pipeline=0)
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, "stat_single_solve_launches"), grew
    assert pkg.is_solved(out[1]).all(), out[1]
    return out


def test_pipelined_nodes_and_split_solve(pkg, skidpad, plain30):
    out, grew = coupled_case(pkg, skidpad, 128, 20, {"pipe_min": 64})
    assert grew["stat_pipelined_launches"] > 0 and only(grew, COUPLED_STATS, "stat_split_solve_launches"), grew
    assert pkg.is_solved(out[1]).all(), out[1]
    assert same_bits(out, plain30)


def test_pipelined_nodes_and_single_solve(pkg, skidpad, plain30):
    out, grew = coupled_case(pkg, skidpad, 128, 20, {"pipe_min": 64, "solve_split": 0})
    assert grew["stat_pipelined_launches"] > 0 and only(grew, COUPLED_STATS, "stat_single_solve_launches"), grew
    assert pkg.is_solved(out[1]).all(), out[1]
    assert same_bits(out, plain30)


def test_fused_update_and_solve(pkg, skidpad, plain30):
    out, grew = coupled_case(pkg, skidpad, 128, 20, {"pipe_min": 64}, fusion=1)
    assert grew["stat_pipelined_launches"] == 0 and only(grew, COUPLED_STATS, None), grew      # (the fused kernel is neither of the counted solve launches)
    assert pkg.is_solved(out[1]).all(), out[1]
    assert same_bits(out, plain30)


def test_ring_solve(pkg, skidpad):
    """N = 40: the dynamics blocks stream through the four-slot ring (no counter of its own)."""
    out, _ = coupled_case(pkg, skidpad, 64, 30)
    plain, _ = coupled_case(pkg, skidpad, 64, 30, {"solve_split": 0}, fusion=0, pipeline=0)
    assert pkg.is_solved(out[1]).all(), out[1]
    assert same_bits(out, plain)


# ---- lateral formulation, N = 20 through k_solve_lat: the four arrangements of its launches ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_lateral(pkg, skidpad):
    """The plain arrangement (four instances per wavefront, one launch): the cold step and the warm one behind it."""
    res = {}
    for B, steps in ((96, 1), (96, 2)):
        out, grew = lateral_case(pkg, skidpad, B, PLAIN_LATERAL, steps=steps)
        assert only(grew, LATERAL_STATS, None), grew
        assert pkg.is_solved(out[1]).all(), out[1]
        res[steps] = out
    return res


def test_lateral_plain_counts_nothing(pkg, skidpad, plain_lateral):
    out, grew = lateral_case(pkg, skidpad, 96, {"lateral_solver": 1, "lat_handover": 0, "lat_single_max": 0})
    assert grew["stat_lat_one_per_wavefront_solves"] == 0 and grew["stat_lat_handover_solves"] == 0, grew
    assert same_bits(out, plain_lateral[1])      # (a cold step: "lat_split" plays no part)


def test_lateral_one_per_wavefront(pkg, skidpad, plain_lateral):
    out, grew = lateral_case(pkg, skidpad, 96, {"lateral_solver": 1})
    assert only(grew, LATERAL_STATS, "stat_lat_one_per_wavefront_solves"), grew
    assert same_point(pkg, out, plain_lateral[1])


def test_lateral_handover(pkg, skidpad, plain_lateral):
    out, grew = lateral_case(pkg, skidpad, 96, {"lateral_solver": 1, "lat_single_max": 0, "lat_hand_batch": 64})
    assert only(grew, LATERAL_STATS, "stat_lat_handover_solves"), grew
    assert same_point(pkg, out, plain_lateral[1])


def test_lateral_two_launch_warm(pkg, skidpad, plain_lateral):
    out, grew = lateral_case(pkg, skidpad, 96, {"lateral_solver": 1}, steps=2)
    assert only(grew, LATERAL_STATS, "stat_lat_two_launch_solves"), grew
    assert same_point(pkg, out, plain_lateral[2])
