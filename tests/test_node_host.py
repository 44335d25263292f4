"""CPU tests of the node callback (pg_node_step_dev / pg_simulate_node_dev / pg_get_node_state): the header, both release libraries and both bindings carry it, and the host
restatement tests/node_numpy.py decides as from_autobox_callback (ros_integration.jl:48-151) does on hand-built cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import node_numpy as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("pg_node_step_dev", "pg_simulate_node_dev", "pg_get_node_state")
NAN = float("nan")


def _header():
    return open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()


def test_header_declares_the_entry_points_and_the_events():
    h = _header()
    for name in ENTRY:
        assert re.search(r"\bint %s\(pg_handle\* h," % name, h), name
    want = ["PG_NODE_MPC = 0", "PG_NODE_HJI_POLICY = 1", "PG_NODE_FEATHER = 2", "PG_NODE_NAN_FALLBACK = 3", "PG_NODE_PRE_FLAG_OFF = 4", "PG_NODE_OUTSIDE_TRAJECTORY = 5",
            "PG_NODE_LOW_SPEED = 6"]
    body = h[h.index("enum pg_node_event"):]
    body = body[:body.index("};")]
    for w in want:
        assert w in body, w
    assert [nn.MPC, nn.HJI_POLICY, nn.FEATHER, nn.NAN_FALLBACK, nn.PRE_FLAG_OFF, nn.OUTSIDE_TRAJECTORY, nn.LOW_SPEED] == list(range(7))


@pytest.mark.parametrize("lib", ["libpigeon_hip.so", "libpigeon_hip_f32.so"])
def test_release_libraries_export_the_entry_points(lib):
    path = os.path.join(ROOT, "pigeon.jl_amd", "csrc", lib)
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path), lib])
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in ENTRY:
        assert re.search(r"\bT %s$" % name, out, re.M), (lib, name)


def test_bindings_carry_them(pkg):
    from pigeon_jl_amd import _lib
    for name in ENTRY:
        assert name in _lib.SYMBOLS
    for m in ("node_step_", "simulate_node_", "node_summary"):
        assert callable(getattr(pkg.BatchedTrajectoryTrackingMPC, m, None)), m
    assert pkg.BatchedTrajectoryTrackingMPC.NODE_EVENTS == {"mpc": 0, "hji_policy": 1, "feather": 2, "nan_fallback": 3, "pre_flag_off": 4, "outside_trajectory": 5,
                                                            "low_speed": 6}
    jl = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    for name in ENTRY:
        assert ":" + name in jl, name
    for f in ("from_autobox_step!", "simulate_node!"):
        assert "function " + f in jl, f


def test_gate_order():
    # pre_flag first: it wins over a time outside the window and a low speed
    assert nn.gate(0, 1.0, -5.0, 10.0, 0.2) == nn.PRE_FLAG_OFF
    # then the window, before the speed
    assert nn.gate(1, 1.0, -5.0, 10.0, 0.2) == nn.OUTSIDE_TRAJECTORY
    assert nn.gate(1, 1.0, 10.5, 10.0, 0.2) == nn.OUTSIDE_TRAJECTORY
    assert nn.gate(1, 1.0, 5.0, 10.0, 0.2) == nn.LOW_SPEED
    assert nn.gate(1, 1.0, 5.0, 10.0, 8.0) == 0


def test_window_applies_in_trajectory_mode_only():
    assert nn.gate(1, NAN, -5.0, 10.0, 8.0) == 0
    assert nn.gate(1, NAN, 50.0, 10.0, 8.0) == 0
    assert nn.gate(1, NAN, 50.0, 10.0, 0.5) == nn.LOW_SPEED
    assert nn.gate(1, 0.0, 50.0, 10.0, 8.0) == nn.OUTSIDE_TRAJECTORY


def test_window_ends_are_inside():
    assert nn.gate(1, 0.0, 0.0, 10.0, 8.0) == 0
    assert nn.gate(1, 0.0, 10.0, 10.0, 8.0) == 0
    assert nn.gate(1, 0.0, np.nextafter(10.0, 11.0), 10.0, 8.0) == nn.OUTSIDE_TRAJECTORY
    assert nn.gate(1, 0.0, -np.nextafter(0.0, 1.0), 10.0, 8.0) == nn.OUTSIDE_TRAJECTORY


def test_speed_one_is_not_paused():
    assert nn.gate(1, NAN, 0.0, 10.0, 1.0) == 0
    assert nn.gate(1, NAN, 0.0, 10.0, np.nextafter(1.0, 0.0)) == nn.LOW_SPEED


@pytest.mark.parametrize("k", [0, 1, 2])
def test_a_nan_in_any_component_falls_back_and_an_inf_does_not(k):
    msg = np.array([0.01, 200.0, 100.0])
    sel = np.array([0.02, 300.0, 150.0])
    bad = sel.copy(); bad[k] = NAN
    ev, pub, new = nn.decide(0, 0, bad, msg)
    assert ev == nn.NAN_FALLBACK and np.array_equal(pub, msg) and np.array_equal(new, np.zeros(3))
    inf = sel.copy(); inf[k] = np.inf
    ev, pub, new = nn.decide(0, 0, inf, msg)
    assert ev == nn.MPC and np.array_equal(pub, inf) and np.array_equal(new, inf)
    ev, pub, new = nn.decide(0, 1, sel, msg)
    assert ev == nn.HJI_POLICY and np.array_equal(pub, sel) and np.array_equal(new, sel)


def test_two_nans_in_a_row_publish_zero():
    msg = np.array([0.01, 200.0, 100.0]); nanc = np.full(3, NAN)
    ev, ap, m, a = nn.run([0, 0], [0, 0], [nanc, nanc], msg, msg)
    assert list(ev) == [nn.NAN_FALLBACK, nn.NAN_FALLBACK]
    assert np.array_equal(ap[0], msg) and np.array_equal(ap[1], msg)          # the first fallback publishes the message: the vehicle keeps it
    assert np.array_equal(a, np.zeros(3)) and np.array_equal(m, np.zeros(3))  # the second publishes 0


@pytest.mark.parametrize("code", nn.GATED)
def test_a_gated_out_instance_changes_neither_message_nor_applied(code):
    msg = np.array([0.01, 200.0, 100.0]); app = np.array([0.03, -50.0, -40.0]); sel = np.array([0.5, 1.0, 2.0])
    ev, pub, new = nn.decide(code, 0, sel, msg)
    assert ev == code and pub is None and np.array_equal(new, msg)
    assert np.array_equal(nn.applied_after(app, pub), app)
    ev, ap, m, a = nn.run([code, 0], [0, 0], [sel, sel], msg, app)
    assert list(ev) == [code, nn.MPC] and np.array_equal(ap[1], app) and np.array_equal(a, sel) and np.array_equal(m, sel)
