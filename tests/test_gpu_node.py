"""GPU tests of the node callback (pg_node_step_dev / pg_simulate_node_dev / pg_get_node_state): the per-message decision of from_autobox_callback
(ros_integration.jl:48-151) -- pre_flag, the trajectory-time window, the low-speed pause, the NaN fallback -- for every instance of a batch, one-shot and in closed loop."""
import ctypes

import numpy as np
import pytest

from conftest import make_oracle
import node_numpy as nn

pytestmark = pytest.mark.gpu

DT = 0.01
NAN = float("nan")


@pytest.fixture(scope="module")
def grid(pkg):
    return pkg.synthetic.hji_grid(dims=(7, 6, 5, 4, 4, 5, 4), seed=11)


def _getters(m):
    ts = m.time_steps(); x = m.solution(); si = m.solve_info()
    return list(ts) + list(x) + list(si) + [m.polish_info(), m.multipliers()]


def _rows_equal(a, b, rows):
    for p, q in zip(a, b):
        assert np.array_equal(np.asarray(p)[rows], np.asarray(q)[rows], equal_nan=True)


# ---- 1. reduction -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,with_grid", [(4096, False), (256, True)])
def test_coupled_reduces_to_the_safety_rollout_bit_for_bit(pkg, skidpad, grid, B, with_grid):
    """Every gate open and no NaN: the node loop is pg_simulate_safety_dev -- states, controls, other car, V and summary, bit for bit, and the same pipelined launches."""
    steps = 6
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=2024)
    state[:, 3] = np.maximum(state[:, 3], 1.5)
    other = pkg.synthetic.other_cars(state, seed=5)
    runs = []
    for node in (False, True):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=0.5, phase_timing=False)
        if with_grid:
            m.set_hji_cache(*grid)
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        if node:
            s, c, t, o, a, H = m.simulate_node_(steps, use_HJI_policy=with_grid, human="worst", record=True)
            ctrl = H["applied"]
            assert np.all(np.isin(H["event"], [0, 1, 2]))
            assert np.array_equal(a, c)                                         # applied = message once every step published
            _, hb, cn = m.node_summary()
            assert np.all(hb == steps) and np.all(cn == 0)
            src = H["event"]
        else:
            s, c, t, o, H = m.simulate_safety_(steps, use_HJI_policy=with_grid, human="worst", record=True)
            ctrl = H["control"]; src = H["source"]
        runs.append(dict(s=s, c=c, t=t, o=o, state=H["state"], ctrl=ctrl, V=H["V"], src=src, summary=m.safety_summary(), pipe=m.get_option("stat_pipelined_launches")))
        m.close()
    a, b = runs
    for k in ("s", "c", "t", "o", "state", "ctrl", "V", "src"):
        assert np.array_equal(a[k], b[k]), k
    for p, q in zip(a["summary"], b["summary"]):
        assert np.array_equal(p, q)
    assert a["pipe"] == b["pipe"]
    if B >= 4096:
        assert a["pipe"] >= 1
    if with_grid:
        assert np.any(a["src"] == 1)


def test_decoupled_reduces_to_simulate_bit_for_bit(pkg, skidpad):
    """Lateral formulation with the wall rows, N = 50: the node loop (no safety row: V = +Inf) is pg_simulate_dev, fp64."""
    B, steps = 48, 8
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=77)
    state[:, 3] = np.maximum(state[:, 3], 1.5)
    res = []
    for node in (False, True):
        m = pkg.DecoupledTrajectoryTrackingMPC(pkg.X1(), skidpad, B, N_short=10, N_long=40, walls=True, wall_weight=1000.0)
        m.set_inputs(state, control, t0, time_offset=toff)
        if node:
            s, c, t, o, a, H = m.simulate_node_(steps, record=True)
            assert np.all(H["V"] == np.inf) and np.all(H["event"] == 0)
            res.append((s, c, t, H["state"], H["applied"]))
        else:
            s, c, t, qh, uh = m.simulate_(steps, record=True)
            res.append((s, c, t, qh, uh))
        m.close()
    for p, q in zip(*res):
        assert np.array_equal(p, q)


def test_f32_reduction(pkg, skidpad, grid):
    """fp32 library: one node step publishes what one safety step applies (same source, same bits of the control), and the plant lands where the safety step's does."""
    B = 96
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=33)
    state[:, 3] = np.maximum(state[:, 3], 1.5)
    other = pkg.synthetic.other_cars(state, seed=9)
    out = []
    for node in (False, True):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=0.5, precision="f32")
        m.set_hji_cache(*grid)
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        if node:
            s, c, t, o, a, H = m.simulate_node_(1, use_HJI_policy=True, human="worst", record=True)
            out.append((s, c, t, o, H["event"][0]))
        else:
            s, c, t, o, H = m.simulate_safety_(1, use_HJI_policy=True, human="worst", record=True)
            out.append((s, c, t, o, H["source"][0]))
        m.close()
    (s0, c0, t0_, o0, e0), (s1, c1, t1, o1, e1) = out
    assert np.array_equal(e0, e1) and np.array_equal(c0, c1) and np.array_equal(t0_, t1)
    assert np.max(np.abs(s0 - s1) / np.maximum(1.0, np.abs(s0))) < 1e-5 and np.max(np.abs(o0 - o1) / np.maximum(1.0, np.abs(o0))) < 1e-5


# ---- 2. warm state kept -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("formulation", ["coupled", "decoupled"])
def test_gated_out_instances_keep_their_warm_state(pkg, skidpad, formulation):
    """One node step for everyone, then one with pre_flag = 0 on a subset: the subset's time steps, solution, solve info, polish and multipliers are bit-identical to before,
    its neighbours to an ungated second step.  A third step with every gate open then gives the subset what a handle that never made the gated call gives (coupled: bit for
    bit, per-instance independence; lateral: within the lateral tests' KKT tolerance)."""
    B = 256
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=91)
    state[:, 3] = np.maximum(state[:, 3], 1.5)
    sub = np.zeros(B, bool); sub[::7] = True; sub[100:110] = True
    pf = np.where(sub, 0, 1).astype(np.uint8)
    make = (lambda: pkg.BatchedTrajectoryTrackingMPC(skidpad, B)) if formulation == "coupled" else \
           (lambda: pkg.DecoupledTrajectoryTrackingMPC(pkg.X1(), skidpad, B, N_short=10, N_long=40))
    A, Bh, Ch = make(), make(), make()
    for m in (A, Bh, Ch):
        m.set_inputs(state, control, t0, time_offset=toff)
        m.node_step_()
    before = _getters(A)
    cmdA, seA, evA, msgA = A.node_step_(pre_flag=pf)
    cmdB, seB, evB, msgB = Bh.node_step_()
    after = _getters(A)
    _rows_equal(before, after, sub)
    assert np.all(evA[sub] == nn.PRE_FLAG_OFF) and np.all(np.isnan(cmdA[sub]))
    _rows_equal(_getters(Bh), after, ~sub)
    assert np.array_equal(cmdA[~sub], cmdB[~sub]) and np.array_equal(evA[~sub], evB[~sub]) and np.array_equal(msgA[~sub], msgB[~sub])
    assert np.array_equal(seA, seB)
    cA, _, eA, mA = A.node_step_()
    cC, _, eC, mC = Ch.node_step_()
    assert np.array_equal(eA[sub], eC[sub])
    if formulation == "coupled":
        assert np.array_equal(cA[sub], cC[sub]) and np.array_equal(mA[sub], mC[sub])
        _rows_equal(_getters(A), _getters(Ch), sub)
    else:
        assert np.max(np.abs(cA[sub] - cC[sub])) < 1e-6
        st = A.solve_info()[0]
        assert np.all(pkg.is_solved(st[sub]))
    _, hb, cn = A.node_summary()
    assert np.all(hb[sub] == 2) and np.all(hb[~sub] == 3) and np.all(cn[sub, 0] == 1) and np.all(cn[~sub] == 0)
    for m in (A, Bh, Ch):
        m.close()


# ---- 3. each gate, one-shot ---------------------------------------------------------------------------------------------------------------------------------------
def test_each_gate_one_shot(pkg, skidpad):
    B = 64
    t_end = float(skidpad.t[-1])
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=13)
    state[:, 3] = np.maximum(state[:, 3], 1.5)
    rng = np.random.default_rng(4)
    pf = np.ones(B, np.uint8); pf[0:8] = 0
    state[8:16, 3] = rng.uniform(0.5, 1.0, 8)
    t0[16:20] = -rng.uniform(0.01, 1.0, 4)
    t0[20:24] = t_end + rng.uniform(0.01, 1.0, 4)
    t0[24:28] = -rng.uniform(0.01, 1.0, 4); toff[24:28] = NAN                # path mode: the window does not apply
    t0[28:32] = t_end + rng.uniform(0.01, 1.0, 4); toff[28:32] = NAN
    t0[32] = 0.0; t0[33] = t_end                                             # both ends inside
    state[34, 3] = 1.0                                                       # not paused
    expect = np.array([nn.gate(pf[b], toff[b], t0[b], t_end, state[b, 3]) for b in range(B)])
    assert np.all(expect[0:8] == 4) and np.all(expect[8:16] == 6) and np.all(expect[16:24] == 5) and np.all(expect[24:] == 0)
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    m.set_inputs(state, control, t0, time_offset=toff)
    cmd, se, ev, msg = m.node_step_(pre_flag=pf)
    gated = expect != 0
    assert np.array_equal(np.where(gated, ev, 0), expect)
    assert np.all(np.isin(ev[~gated], [0, 3]))
    assert np.all(np.isnan(cmd[gated])) and np.array_equal(msg[gated], control[gated])
    ok = ~gated & (ev == 0)
    assert ok.sum() >= 30 and np.array_equal(cmd[ok], msg[ok]) and np.all(np.isfinite(cmd[ok]))
    sep = m.path_coordinates()
    assert np.array_equal(se, sep[:, :2])
    a, hb, cn = m.node_summary()
    assert np.array_equal(hb, (~gated).astype(np.int32))
    for k, code in enumerate((4, 5, 6)):
        assert np.array_equal(cn[:, k], (expect == code).astype(np.int32))
    assert np.array_equal(cn[:, 3], (ev == 3).astype(np.int32))
    m.close()


# ---- 4. NaN fallback, one-shot ------------------------------------------------------------------------------------------------------------------------------------
def test_nan_fallback_one_shot(pkg, skidpad):
    B = 64
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=21)
    state[:, 3] = np.maximum(state[:, 3], 1.5)
    hit = np.zeros(B, bool); hit[[5, 17, 40, 63]] = True
    bad = state.copy(); bad[5, 0] = NAN; bad[17, 1] = np.inf; bad[40, 2] = NAN; bad[63, 0] = -np.inf
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    ref = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    m.set_inputs(bad, control, t0, time_offset=toff)
    cmd, se, ev, msg = m.node_step_()
    ref.set_inputs(state, control, t0, time_offset=toff)
    cr, _, er, mr = ref.node_step_()
    assert np.all(ev[hit] == nn.NAN_FALLBACK) and np.array_equal(cmd[hit], control[hit]) and np.all(msg[hit] == 0.0)
    assert np.all(ev[~hit] == 0) and np.array_equal(cmd[~hit], cr[~hit]) and np.array_equal(msg[~hit], mr[~hit])
    # a second NaN in a row publishes 0
    cmd2, _, ev2, msg2 = m.node_step_()
    assert np.all(ev2[hit] == nn.NAN_FALLBACK) and np.all(cmd2[hit] == 0.0) and np.all(msg2[hit] == 0.0)
    assert np.array_equal(m.node_summary()[2][:, 3], np.where(hit, 2, 0))
    # a clean pose: the fallback instances start cold -- bit-identical to a fresh handle's cold step with control 0
    m.set_inputs(state, msg2, t0, time_offset=toff)
    cmd3, _, ev3, msg3 = m.node_step_()
    fresh = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    fresh.set_inputs(state, msg2, t0, time_offset=toff)
    cf, _, ef, mf = fresh.node_step_()
    assert np.all(ev3[hit] == 0) and np.array_equal(cmd3[hit], cf[hit]) and np.array_equal(msg3[hit], mf[hit])
    xa, sa = m.solution(); xf, sf = fresh.solution()
    assert np.array_equal(xa[hit], xf[hit]) and np.array_equal(m.solve_info()[0][hit], fresh.solve_info()[0][hit])
    _, hb, cn = m.node_summary()
    assert np.all(hb == 3) and np.all(cn == 0)                                 # (set_inputs restarted the counts before the third step; the heartbeat goes on)
    for h in (m, ref, fresh):
        h.close()


# ---- 5. the H4 hazard in the rollout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_policy", [False, True])
def test_h4_hazard_in_the_rollout(pkg, skidpad, grid, use_policy):
    """An other car at speed 0, held, next to half of the ego cars, inside the grid with V <= eps: k_hji_constraint keeps the reference's NaN (H4).  Policy off: the node
    falls back exactly on the steps whose MPC command is NaN -- the steps with V <= eps, where the status is PG_NUMERICAL -- and the applied command follows node_numpy
    (the message first, then 0).  Policy on: those steps publish the policy (optimal_control does not use the other car's speed) and nothing falls back."""
    B, steps, eps = 32, 12, 2.0
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=5)
    state[:, 3] = np.maximum(state[:, 3], 3.0)
    other = np.zeros((B, 4))
    near = np.arange(B) % 2 == 0
    other[:, 0] = state[:, 0] + np.where(near, 1.0, 500.0); other[:, 1] = state[:, 1] + np.where(near, 1.5, 500.0); other[:, 2] = state[:, 2]
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=eps)
    m.set_hji_cache(*grid)
    m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
    H, st = [], []
    for k in range(steps):
        H.append(m.simulate_node_(1, use_HJI_policy=use_policy, human="hold", record=True)[5])
        st.append(m.solve_info()[0])
    ev = np.concatenate([h["event"] for h in H]); V = np.concatenate([h["V"] for h in H]); ap = np.concatenate([h["applied"] for h in H])
    st = np.array(st)
    unsafe = V <= eps
    assert unsafe[:, near].any() and not unsafe[:, ~near].any()
    assert np.array_equal(st == pkg.NUMERICAL, unsafe)
    if use_policy:
        assert np.array_equal(ev == nn.HJI_POLICY, unsafe) and not np.any(ev == nn.NAN_FALLBACK)
        assert np.all(np.isfinite(ap))
        return
    assert np.array_equal(ev == nn.NAN_FALLBACK, unsafe) and np.all(ev[~unsafe] == 0)
    a_end = m.node_summary()[0]
    for b in range(B):
        sel = [np.full(3, NAN) if ev[k, b] == nn.NAN_FALLBACK else (ap[k + 1, b] if k + 1 < steps else a_end[b]) for k in range(steps)]
        e, apx, _, _ = nn.run(np.zeros(steps, int), ev[:, b] * (ev[:, b] != nn.NAN_FALLBACK), sel, control[b], control[b])
        assert np.array_equal(e, ev[:, b]) and np.array_equal(apx, ap[:, b]), b
    b0 = np.nonzero(near)[0][0]
    k0 = np.nonzero(ev[:, b0] == nn.NAN_FALLBACK)[0]
    assert len(k0) >= 2 and np.array_equal(ap[k0[0] + 1, b0], control[b0]) and np.all(ap[k0[1] + 1, b0] == 0.0)
    m.close()


# ---- 6. pause, resume and window against an oracle loop -----------------------------------------------------------------------------------------------------------
def test_pause_resume_and_window_against_an_oracle_loop(pkg, oracle_mod, skidpad):
    """B = 32, 40 steps, no grid.  Some instances start below 1 m/s with a held drive command and resume; one instance's clock crosses its trajectory's end.  The host loop
    keeps one oracle per instance and steps it only when that instance's gate is open.  Instances that come within 1e-3 of the 1 m/s threshold are left out."""
    B, steps, margin = 32, 40, 1e-3
    t_end = float(skidpad.t[-1])
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=41)
    state[:, 3] = np.maximum(state[:, 3], 2.0)
    slow = np.arange(4, 10)
    state[slow, 3] = np.linspace(0.6, 0.95, len(slow)); state[slow, 4] = 0.0; state[slow, 5] = 0.0
    control[slow] = [0.0, 1500.0, 1500.0]
    t0[20] = t_end - 0.155                                                   # crosses t_end after ~16 steps
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    m.set_inputs(state, control, t0, time_offset=toff)
    s, c, t, o, a, H = m.simulate_node_(steps, record=True)
    clock = m.simulate_clock(steps + 1, t0, dt=DT)
    X = pkg.X1()
    un = np.array([X["delta_max"], max(-X["Fx_min"], X["Fx_max"]), max(-X["Fx_min"], X["Fx_max"])])
    keep = np.ones(B, bool); dev = np.zeros(B)
    ev_o = np.full((steps, B), -1, np.int32)
    upto = np.full(B, steps)                                                 # steps compared: the oracle's solver fails numerically just above 1 m/s (status -10) -- the
    rel = lambda p, q: np.max(np.abs(p - q) / np.maximum(1.0, np.abs(q)))   # comparison of that instance ends at the first such step (its event: gated in, both sides)
    for b in range(B):
        if b == 20:                                                          # (the oracle does not step a horizon that runs past the trajectory's end)
            keep[b] = False
            continue
        orc = make_oracle(oracle_mod, skidpad)
        q, msg, app = state[b].copy(), control[b].copy(), control[b].copy()
        for k in range(steps):
            tk = clock[k, b]
            dev[b] = max(dev[b], rel(H["state"][k, b], q), np.max(np.abs(H["applied"][k, b] - app) / un))
            if abs(q[3] - 1.0) < margin:
                keep[b] = False
            code = nn.gate(1, toff[b], tk, t_end, q[3])
            sel = np.full(3, NAN)
            if code == 0:
                u, _, _, stb, _ = orc.step_batch(q[None], msg[None], np.array([tk]), time_offsets=toff[b:b + 1], solver=0)
                sel = u[0]
                if stb[0] != pkg.SOLVED:
                    upto[b] = k; ev_o[k, b] = nn.MPC
                    break
            e, pub, msg = nn.decide(code, 0, sel, msg)
            ev_o[k, b] = e
            qn = orc.plant_step(q, app, DT)
            app = nn.applied_after(app, pub)
            q = qn
        if upto[b] == steps:
            dev[b] = max(dev[b], rel(s[b], q), np.max(np.abs(a[b] - app) / un), np.max(np.abs(c[b] - msg) / un))
    assert keep.sum() >= B * 3 // 4, keep.sum()
    for b in np.nonzero(keep)[0]:
        k = upto[b]
        assert np.array_equal(H["event"][:k, b], ev_o[:k, b]), b
        if k < steps:
            assert H["event"][k, b] not in nn.GATED, b
    assert np.sum(keep & (upto == steps)) >= B // 2
    assert np.array_equal(t, clock[steps])
    off = np.nonzero(keep & (dev >= 1e-5))[0]
    assert len(off) <= 1, (off, dev[off])
    assert np.any(H["event"][:, slow] == nn.LOW_SPEED) and np.any(H["event"][-1, slow] == 0)          # paused, then resumed
    out = clock[:steps, 20] > t_end                                          # the window instance: gated out exactly once its clock has passed t_end
    assert out.any() and not out[0]
    assert np.array_equal(H["event"][:, 20] == nn.OUTSIDE_TRAJECTORY, out) and np.all(np.isin(H["event"][~out, 20], [0, nn.NAN_FALLBACK]))
    resumed = [b for b in slow if keep[b] and np.any(ev_o[:upto[b], b] == nn.LOW_SPEED) and (upto[b] < steps or np.any(ev_o[:, b] == 0))]
    assert len(resumed) >= 3, (keep[slow], upto[slow])


# ---- 7. reproducible ----------------------------------------------------------------------------------------------------------------------------------------------
def test_node_rollout_is_reproducible_bit_for_bit(pkg, skidpad, grid):
    B, steps = 4096, 12
    t_end = float(skidpad.t[-1])
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=12345)
    rng = np.random.default_rng(8)
    state[rng.random(B) < 0.1, 3] = 0.8
    t0[rng.random(B) < 0.05] = t_end + 0.5
    state[rng.random(B) < 0.02, 0] = NAN
    pf = (rng.random((steps, B)) > 0.05).astype(np.uint8)
    other = pkg.synthetic.other_cars(state, seed=777)
    runs = []
    for rep in range(2):
        m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, hji_eps=0.5, phase_timing=False)
        m.set_hji_cache(*grid)
        m.set_inputs(state, control, t0, other_car_state=other, time_offset=toff)
        s, c, t, o, a, H = m.simulate_node_(steps, use_HJI_policy=True, human="worst", pre_flag=pf, record=True)
        runs.append([s, c, t, o, a] + [H[k] for k in sorted(H)] + list(m.node_summary()) + list(m.safety_summary()) + list(m.solve_info()[:3]))
        m.close()
    for p, q in zip(*runs):
        assert np.array_equal(np.asarray(p), np.asarray(q), equal_nan=True)
    ev = runs[0][5 + sorted(H).index("event")]
    for code in (0, 3, 4, 5, 6):
        assert np.any(ev == code), code


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, skidpad):
    B = 8
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=1)
    m = pkg.BatchedTrajectoryTrackingMPC(skidpad, B)
    m.set_inputs(state, control, t0, time_offset=toff)
    f = lambda steps, dt, mode, hu=None: m.lib.pg_simulate_node_dev(m.h, steps, ctypes.c_double(dt), 0, mode, hu, None, None, None, None, None)
    assert f(1, DT, 3) == -2 and f(1, DT, -1) == -2 and f(1, DT, 2) == -2
    assert f(0, DT, 0) == -2 and f(1, 0.0, 0) == -2 and f(1, -DT, 0) == -2
    with pytest.raises(ValueError):
        m.simulate_node_(1, human="script")
    s = m.simulate_node_(1)[0]
    assert np.all(np.isfinite(s))
    m.close()
    d = pkg.DecoupledTrajectoryTrackingMPC(pkg.X1(), skidpad, B)
    d.set_inputs(state, control, t0, time_offset=toff)
    assert d.lib.pg_simulate_node_dev(d.h, 1, ctypes.c_double(DT), 1, 0, None, None, None, None, None, None) == -4      # PG_ERR_STATE
    assert d.lib.pg_node_step_dev(d.h, 1, None, None, None, None) == -4
    d.node_step_()                                                           # policy off: fine
    d.close()
