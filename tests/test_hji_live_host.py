"""Host half of tests/test_gpu_hji_live.py (no GPU): the live-gradient grid of tests/hji_live_cases.py is what it says it is, and -- with the oracle alone -- the cases the
device tests run on it make their assertions bite: every channel live, optimal_control with both steer signs and winners inside the Fx range, a tie set within its cap,
safety rows whose steering coefficient comes mostly from dV/dUy and dV/dr."""
import math

import numpy as np
import pytest

from conftest import make_oracle
import hji_live_cases as lc


@pytest.fixture(scope="module")
def live_oracle(oracle_mod, skidpad):
    orc = make_oracle(oracle_mod, skidpad)
    orc.set_hji_grid(*lc.live_grid())
    return orc


def test_grid_shape_box_and_liveness(pkg):
    knots, V, g = lc.live_grid()
    dims = tuple(len(k) for k in knots)
    assert dims == (7, 6, 5, 4, 3, 5, 2) and V.shape == (25200,) and g.shape == (25200, 7)
    assert V.dtype == np.float32 and g.dtype == np.float32 and all(k.dtype == np.float32 for k in knots)
    assert len({dims[3], dims[4], dims[6]}) == 3 and dims[6] == 2
    ref = pkg.synthetic.hji_grid(dims=dims, seed=lc.SEED)[0]                 # the same box and jitter: synthetic.hji_queries / other_cars land inside
    assert all(np.array_equal(a, b) for a, b in zip(knots, ref))
    assert np.mean(g[:, 4] != 0) > 0.5 and np.mean(g[:, 6] != 0) > 0.5
    ch = [V] + [g[:, k] for k in range(7)]
    assert not any(np.array_equal(ch[i], ch[j]) for i in range(8) for j in range(i))
    assert lc.channel_dependence().all()                                    # every channel varies along every dimension
    assert all((c > 0).any() and (c < 0).any() for c in ch[:4] + ch[5:])    # every channel takes both signs on the grid, dV/dUx (0.0225 .. 0.0775) apart
    assert np.all(np.isfinite(V)) and np.all(np.isfinite(g))


def test_gradient_is_the_gradient_of_v():
    """central differences of the analytic V (float64) at random points of the box: gradV is its gradient, channel by channel"""
    lo, hi = lc.bounds(lc.live_grid()[0])
    x = lo + (hi - lo) * np.random.default_rng(5).uniform(0, 1, (64, 7))
    _, _, g = lc.value_and_gradient(list(x.T))
    h = 1e-5
    for d in range(7):
        e = np.zeros(7); e[d] = h
        fd = (lc.value_and_gradient(list((x + e).T))[1] - lc.value_and_gradient(list((x - e).T))[1]) / (2 * h)
        assert np.max(np.abs(fd - g[:, d])) < 1e-8, d                       # truncation h^2 V'''/6 ~ 1e-11, rounding eps |V| / h ~ 1e-10


def test_lookup_queries_bite(live_oracle):
    knots, V, g = lc.live_grid()
    dims = [len(k) for k in knots]
    x, fam, idx = lc.lookup_queries(knots)
    res = [live_oracle.hji_lookup(p) for p in x]
    inb = np.array([r[2] for r in res])
    assert 50 <= inb[fam["random"]].sum() < 300 and inb[0] and inb[1]       # in- and out-of-bounds points, both corners inside
    assert inb[fam["nodes"]].all() and inb[fam["along4"]].all() and inb[fam["along6"]].all()
    assert np.any(idx[:, 4] == dims[4] - 1) and np.any(idx[:, 6] == dims[6] - 1)          # the high faces of dimensions 4 and 6
    stride = np.cumprod([1] + dims[:-1])
    for i, r in zip(idx, res[fam["nodes"]]):                                # at a node the lookup IS the node record (weights exactly 0 or 1)
        n = int(np.dot(i, stride))
        assert r[0] == float(V[n]) and np.array_equal(r[1], g[n].astype(np.float64))
    for name, d in (("along4", 4), ("along6", 6)):
        pts = x[fam[name]]
        assert np.all(np.delete(pts, d, axis=1) == np.delete(pts[0], d)) and len(np.unique(pts[:, d])) == 16
        G = np.stack([r[1] for r in res[fam[name]]])
        assert len(np.unique(G[:, 4])) == 16 and len(np.unique(G[:, 6])) == 16            # channels 5 and 7 move along the family
    cells4 = {int(np.searchsorted(knots[4], v, side="right")) for v in x[fam["along4"]][:, 4]}
    assert len(cells4) == dims[4] - 1                                       # every cell of dimension 4


def test_policy_cases_bite(pkg, live_oracle, skidpad):
    """What test_fallback_policy_on_the_live_grid asserts of the oracle's answers, without a GPU (on synthetic.hji_grid: 96 / 0 / 0 / 1)."""
    state, control, t0, toff, other = lc.policy_inputs(pkg, skidpad)
    R = lc.policy_reference(live_oracle, state, other)
    inb = R["inb"]
    assert inb.sum() == 96
    assert np.sum(R["u2"][inb, 0] > 0) >= 8 and np.sum(R["u2"][inb, 0] < 0) >= 8                # measured 86 / 10
    assert np.array_equal(R["u2"][inb, 0] > 0, R["Bc"][inb] >= 0)
    win = R["win"][inb]
    assert np.sum((win > 0) & (win < 49)) >= 24 and len(set(win.tolist())) >= 8                 # measured 44 interior, 16 distinct
    assert R["tie"].sum() <= lc.TIE_CAP                                                         # measured 0
    assert np.all(np.isfinite(R["scores"][inb]))
    unsafe = inb & (R["V"] <= 0.5) & ~np.isnan(toff)                                            # eps of the policy test: the instances the policy drives
    assert np.sum(R["u2"][unsafe, 1] > 0) >= 3 and np.sum(R["u2"][unsafe, 1] < 0) >= 3          # measured 9 / 5
    for i in np.nonzero(inb)[0]:                                                                # the accessor agrees with the call the tests had
        Vo, u2o = live_oracle.hji_optimal_control(state[i], other[i])
        assert Vo == R["V"][i] and np.array_equal(u2o, R["u2"][i])


def test_safety_row_cases_bite(pkg, oracle_mod, skidpad):
    """What test_constraint_rows_and_solve_on_the_live_grid asserts of the oracle's rows: at least 24 of the 48 active, and in at least half of those the steering
    coefficient comes more from g[4] d(dUy)/d(delta) + g[6] d(dr)/d(delta) than from g[3] d(dUx)/d(delta) (on synthetic.hji_grid the former is exactly 0)."""
    orc = make_oracle(oracle_mod, skidpad); orc.set_hji_grid(*lc.live_grid()); orc.set_hji_eps(10.0)
    state, control, t0, toff, other = lc.constraint_inputs(pkg, skidpad)
    nact = ndom = 0
    for i in range(48):
        M, b, V = orc.hji_constraint(state[i], other[i], control[i])
        if math.isinf(V) or V > 10.0:
            continue
        nact += 1
        assert np.all(np.isfinite(M)) and math.isfinite(b)
        x7 = orc.hji_relative_state(state[i], other[i])
        through_ux, through_uy_r = lc.steer_terms(orc, x7, orc.hji_lookup(x7)[1], control[i])
        assert abs(through_ux + through_uy_r - M[0]) <= 1e-6 * max(1.0, abs(M[0])), i           # the two parts are M0 (central differences, h = 1e-6)
        ndom += abs(through_uy_r) > abs(through_ux)
    assert nact >= 24 and 2 * ndom >= nact, (nact, ndom)                                        # measured 48 / 48
