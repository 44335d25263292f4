"""CPU tests of the yardstick of pg_hji_solve: the numpy twin (tests/hji_solve_numpy.py) against the C++ oracle where the oracle has the piece, the properties the scheme
holds exactly, the threshold condition of the shared test grids, and the host-side pieces of the feature (hji_io.collision_target, the ctypes mirror)."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_oracle
import hji_solve_cases as cases
import hji_solve_numpy as hs
import safety_numpy as sn

N_STATES = 200


@pytest.fixture(scope="module", params=["analytic", "live"])
def pinned(request, pkg, oracle_mod, skidpad):
    """200 random relative states inside synthetic.hji_grid's box, as the oracle sees them, with the gradient its lookup gives there (the grid's analytic gradV,
    interpolated).  With the ego at the origin heading North (psi = 0) the relative state is (N, -E, psi, ...) of the other car (HJI_computation.jl:20-24).
    "analytic" is the grid as it stands: its gradient has no Uy and no r component, so optimal_control always answers (+delta_max, Fx_max).  "live" is a second
    case on top of it: the same V with a seeded perturbation on all seven gradient components (the lookup interpolates whatever gradV it is handed), so that the
    steer sign, the line search and every branch of optimal_disturbance are exercised."""
    knots, V, g = pkg.synthetic.hji_grid(dims=(7, 6, 5, 4, 4, 5, 4), seed=11)
    if request.param == "live":
        g = (g + np.random.default_rng(8).normal(0.0, [0.2, 0.2, 0.3, 0.1, 0.3, 0.05, 0.5], g.shape)).astype(np.float32)
    orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(knots, V, g); orc.set_hji_eps(1e9)         # every safety row active
    x = pkg.synthetic.hji_queries(knots, N_STATES, seed=21)
    x[:, 2] *= 0.999                                                                                    # (adiff maps +pi itself to -pi... keep the angle inside)
    state = np.stack([0 * x[:, 0], 0 * x[:, 0], 0 * x[:, 0], x[:, 3], x[:, 4], x[:, 6]], axis=1)
    other = np.stack([-x[:, 1], x[:, 0], x[:, 2], x[:, 5]], axis=1)
    x7 = np.stack([orc.hji_relative_state(state[i], other[i]) for i in range(N_STATES)])
    assert np.max(np.abs(x7 - x)) < 1e-12
    look = [orc.hji_lookup(x7[i]) for i in range(N_STATES)]
    assert all(l[2] for l in look)
    return orc, state, other, x7, np.stack([l[1] for l in look]), request.param


def test_twin_optimal_control_is_the_oracles(pinned):
    orc, state, other, x7, g, kind = pinned
    X = orc.vehicle()
    d, Fx = hs.optimal_control(X, x7, g)
    ref = np.stack([orc.hji_optimal_control(state[i], other[i])[1] for i in range(N_STATES)])
    assert np.array_equal(d, ref[:, 0])                                                                 # the steer sign: exact
    assert np.max(np.abs(Fx - ref[:, 1]) / np.maximum(1.0, np.abs(ref[:, 1]))) <= 1e-9
    if kind == "live":
        assert len(set(np.round(Fx, 3))) >= 3 and len(set(d)) == 2                                      # the line search and the sign both take several values


def test_twin_hamiltonian_is_the_oracles_constraint(pinned):
    """p . relative_dynamics(x, uR, uH*) = b + M . uR of compute_reachability_constraint (:160-170), at the twin's own optimal control"""
    orc, state, other, x7, g, kind = pinned
    X = orc.vehicle()
    H, f, uR, uH = hs.hamiltonian_terms(X, x7, g)
    worst = 0.0
    for i in range(N_STATES):
        Fx = uR[i, 1]
        c3 = [uR[i, 0], Fx * (X["fwd_frac"] if Fx > 0 else X["fwb_frac"]), Fx * (X["rwd_frac"] if Fx > 0 else X["rwb_frac"])]
        M, b, V = orc.hji_constraint(state[i], other[i], c3)
        ref = b + M[0] * c3[0] + M[1] * (c3[1] + c3[2])
        worst = max(worst, abs(H[i] - ref) / max(1.0, abs(ref)))
    assert worst <= 1e-9, worst
    assert np.any(uH[:, 1] != 0) and (kind != "live" or np.any(uH[:, 0] != 0))


def test_gradient_of_an_analytic_grid(pkg):
    """pbar of synthetic.hji_grid's V against its closed-form gradient: central differences of a smooth function on a 13 x 13 x 9^5-like spacing are second order
    in the interior; here only the linear dimensions are exact (Ux, V: 0.05, -0.02), and they are"""
    knots, V, g = pkg.synthetic.hji_grid(dims=(5, 4, 4, 3, 2, 3, 2), seed=2)
    p = hs.gradient(V, knots)
    assert np.max(np.abs(p[:, 3] - 0.05)) < 1e-5 and np.max(np.abs(p[:, 5] + 0.02)) < 1e-5           # float32 V over spacings >= 4: rounding / spacing
    assert np.all(p[:, 4] == 0) and np.all(p[:, 6] == 0)


@pytest.mark.parametrize("name,periodic", cases.CASES)
def test_properties_of_the_twin(name, periodic):
    knots, l0 = cases.grid(name, periodic)
    V6, g6, st6 = cases.twin(name, periodic)
    V5, _, st5 = cases.twin(name, periodic, sweeps=cases.SWEEPS - 1)
    assert st6["sweeps"] == cases.SWEEPS and st6["reached_horizon"] == 0
    assert np.all(np.isfinite(V6)) and np.all(V6 <= l0) and np.any(V6 < l0)
    assert np.all(V6 <= V5)                                                                             # non-increasing in the sweep count
    V0, g0, st0 = hs.solve(cases.vehicle("nominal"), knots, l0, 0.0, periodic_psi=periodic)
    assert st0["sweeps"] == 0 and st0["reached_horizon"] == 1 and np.array_equal(V0, l0)
    assert np.array_equal(g0, hs.gradient(l0, knots, periodic).astype(np.float32))
    # the speed dimension holds the knot V = 0, where the human's control is (0, 0)
    x = hs.node_states(knots, periodic)
    assert np.any(x[:, 5] == 0.0)
    uH = sn.optimal_disturbance(cases.vehicle("nominal"), x[x[:, 5] == 0.0][:8], np.ones((8, 7)))
    assert np.all(uH == 0.0)


@pytest.mark.parametrize("name,periodic", cases.CASES)
def test_no_node_sits_on_the_disturbance_threshold(name, periodic):
    """optimal_disturbance switches at lam_norm < 1e-3: over all sweeps of the shared runs no node lies within 1e-6 (relative) of it (target coefficients: collision
    rectangle 2.5 m x 1.0 m, + 0.05 Ux - 0.02 V), for either vehicle of the GPU tests"""
    assert cases.twin(name, periodic)[2]["near_threshold"] == 0
    if name == "A":
        assert cases.twin(name, periodic, veh="mu06")[2]["near_threshold"] == 0


def test_periodic_wrap_keeps_both_end_nodes_equal():
    """a target that depends on dpsi only through its cosine: the two copies of the same angle stay bit-identical, each computed on its own"""
    knots, _ = cases.grid("B", True)
    l0 = cases.target(knots, cos_psi=0.3)
    dims = [len(k) for k in knots]
    assert np.array_equal(l0.reshape(dims, order="F")[:, :, 0], l0.reshape(dims, order="F")[:, :, -1])
    V, g, st = hs.solve(cases.vehicle("nominal"), knots, l0, 1e9, fixed_dt=cases.FIXED_DT, max_sweeps=4, periodic_psi=True)
    Vn = V.reshape(dims, order="F")
    assert np.array_equal(Vn[:, :, 0], Vn[:, :, -1]) and np.any(V < l0)
    gn = g.reshape(dims + [7], order="F")
    assert np.array_equal(gn[:, :, 0], gn[:, :, -1])
    # and the wrap is what does it: without the flag the ends drift apart
    Vo = hs.solve(cases.vehicle("nominal"), knots, l0, 1e9, fixed_dt=cases.FIXED_DT, max_sweeps=4, periodic_psi=False)[0].reshape(dims, order="F")
    assert not np.array_equal(Vo[:, :, 0], Vo[:, :, -1])


def test_cfl_mode_of_the_twin_reaches_the_horizon():
    knots, l0 = cases.grid("A", False)
    V, g, st = hs.solve(cases.vehicle("nominal"), knots, l0, 0.1)
    assert st["reached_horizon"] == 1 and st["tau"] == 0.1 and 2 <= st["sweeps"] <= 20
    minsp = np.array([np.min(np.diff(k.astype(np.float64))) for k in knots])
    assert st["last_dt"] <= 0.8 / np.sum(st["alpha"] / minsp) * (1 + 1e-12)


def test_collision_target(pkg):
    knots, _ = cases.grid("A", False)
    l0 = pkg.hji_io.collision_target(knots, 2.5, 1.0)
    dims = [len(k) for k in knots]
    assert l0.dtype == np.float32 and l0.shape == (int(np.prod(dims)),)
    L = l0.reshape(dims, order="F")
    assert np.array_equal(L, np.broadcast_to(L[:, :, :1, :1, :1, :1, :1], dims))                        # the same for every value of the other five dimensions
    k1 = pkg.hji_io.collision_target([np.array([-4.0, 0.0, 2.5, 5.5], np.float32), np.array([-3.0, 0.5, 1.0, 5.0], np.float32)] + [np.zeros(2, np.float32)] * 5, 2.5, 1.0)
    S = k1.reshape(4, 4, 2, 2, 2, 2, 2, order="F")[:, :, 0, 0, 0, 0, 0]
    assert S[1, 1] == -0.5 and S[2, 2] == 0.0 and S[2, 1] == 0.0                                        # inside: minus the distance to the nearest side; on the edge: 0
    assert S[3, 1] == 3.0 and S[1, 3] == 4.0 and S[3, 3] == 5.0 and abs(S[0, 0] - np.hypot(1.5, 2.0)) < 1e-6   # outside: to the side, to the corner (3-4-5)
    with pytest.raises(ValueError):
        pkg.hji_io.collision_target(knots[:6], 2.5, 1.0)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ctypes_mirror_of_the_solver(pkg, precision):
    """the defaults and the struct sizes the header states; a null handle is refused before any device is touched"""
    from pigeon_jl_amd import _lib
    lib = pkg.load_library(precision)
    o = lib.pg_default_hji_solve_opts()
    assert (o.horizon, o.cfl, o.fixed_dt, o.max_sweeps, o.flags) == (3.0, 0.8, 0.0, 100000, 0)
    assert C.sizeof(_lib.pg_hji_solve_opts) == 32 and C.sizeof(_lib.pg_hji_solve_stats) == 104
    assert lib.pg_hji_solve(None, None, None, None, None, None, 0, None, None, None) == -2
