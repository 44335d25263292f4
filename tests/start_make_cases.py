"""The one case the start-maker tests share (tests/test_gpu_start_make.py, tests/test_start_make_host.py) and the twin's result over it, computed once.

Library of three tubes:
  0  straight_trajectory(50 m, 8 m/s): 2 knots, the smallest L -- both searches clamp on both sides
  1  the skidpadoval fixture: 1000 knots 0.236 m apart, constant speed (A = 0: the branch |A_i| < 1e-3), E and N 100 to 200 m from the origin
  2  the variable_speed fixture: 28 knots about 2 m apart, A != 0 on 25 of its 27 intervals (the square-root branch), two intervals with |A_i| < 1e-3
B = 64, instance b runs under set b % 8 on tube (b // 8) % 3 with a stream id whose high word is not zero for two thirds of the batch.  Eight sets:
  0  the default: the first knot of each tube (count_less and count_leq both clamp from below)
  1  s_mode 1 with s = 1: the last knot of each tube (count_leq clamps from above); e and dpsi random
  2  e_mode 1, f in [-1, 1], s in [3, 30] m
  3  steady 1 with every offset random
  4  other_mode 1, the ranges of synthetic.other_cars
  5  time_mode 1, s = knot 13 of variable_speed exactly: on tube 2 count_less and count_leq pick different intervals (instances 21 and 45)
  6  every range random, s_mode 0, other_mode 1
  7  every range random, s_mode 1 with s in [0.6, 1.6] (beyond the end: clamped), e_mode 1, time_mode 1, other_mode 1"""
import functools
import sys

import numpy as np

import start_make_numpy as twin

B, N_SETS, SEED = 64, 8, 0x123456789ABCDEF0
KNOT = 13
STEADY_SET = 3                                                    # the one set with steady = 1
INDEX = np.arange(B, dtype=np.int32) % N_SETS
TUBE_INDEX = (np.arange(B, dtype=np.int32) // 8) % 3
STREAMS = (np.arange(B, dtype=np.uint64) % np.uint64(3)) * np.uint64(1 << 32) + np.uint64(1000) + np.uint64(7) * np.arange(B, dtype=np.uint64)
SINCOS = (0, 1)                                                   # E and N of the ego and of the other car carry sincos; both headings are sums of exact terms


def pkg():
    if "pigeon_jl_amd" not in sys.modules:                            # (a test that takes no `pkg` fixture ran first)
        import conftest
        conftest.load_pkg()
    return sys.modules["pigeon_jl_amd"]


@functools.lru_cache(maxsize=None)
def tubes():
    p = pkg()
    return (p.straight_trajectory(50.0, 8.0), p.load_path_fixture("skidpadoval"), p.load_path_fixture("variable_speed"))


@functools.lru_cache(maxsize=None)
def _sets():
    s13 = float(tubes()[2].s[KNOT])
    rnd = dict(e=(-0.6, 0.4), dpsi=(-0.1, 0.15), v=(0.8, 1.2), uy=(-0.2, 0.3), dr=(-0.05, 0.04), delta=(-0.05, 0.03), fx=(-900.0, 700.0), dt0=(-0.3, 0.2),
               other_dx=(-15.0, 15.0), other_dy=(-4.0, 4.0), other_dpsi=(-0.3, 0.3), other_v=(2.0, 10.0))
    return (twin.start(),
            twin.start(s=1.0, s_mode=1, e=(-0.5, 0.5), dpsi=(-0.1, 0.1)),
            twin.start(s=(3.0, 30.0), e=(-1.0, 1.0), e_mode=1),
            twin.start(s=(3.0, 30.0), v=(0.9, 1.1), uy=(-0.1, 0.1), dr=(-0.02, 0.02), delta=(-0.01, 0.01), fx=(-200.0, 200.0), steady=1),
            twin.start(s=(3.0, 30.0), e=(-0.5, 0.5), other_dx=(-15.0, 15.0), other_dy=(-4.0, 4.0), other_dpsi=(-0.3, 0.3), other_v=(2.0, 10.0), other_mode=1),
            twin.start(s=s13, e=(-0.5, 0.5), v=(0.9, 1.1), time_mode=1),
            twin.start(s=(0.0, 45.0), other_mode=1, **rnd),
            twin.start(s=(0.6, 1.6), s_mode=1, e_mode=1, time_mode=1, other_mode=1, **dict(rnd, e=(-0.9, 0.9))))


def sets():
    """the eight sets as dicts of the structure's fields (what pack_starts takes)"""
    return [dict(s) for s in _sets()]


@functools.lru_cache(maxsize=None)
def _reference(single):
    ref = twin.make(tubes(), TUBE_INDEX, _sets(), INDEX, SEED, STREAMS, pkg().X1(), single=single)
    if single is np.float64:
        # the case holds what its description says: the pins, both branches, a clamped draw
        look, s = ref["look"], ref["placed"][:, 0]
        for b in (21, 45):
            assert TUBE_INDEX[b] == 2 and INDEX[b] == 5 and s[b] == tubes()[2].s[KNOT] and look[b]["i"] == KNOT - 1 and look[b]["j"] == KNOT
        for b in range(B):
            if INDEX[b] == 0:
                assert s[b] == tubes()[TUBE_INDEX[b]].s[0] and look[b]["i"] == 0 and look[b]["j"] == 0
            if INDEX[b] == 1:
                t = tubes()[TUBE_INDEX[b]]
                assert s[b] == t.s[-1] and look[b]["i"] == len(t) - 2 and look[b]["j"] == len(t) - 2
        v = twin.draws(_sets(), INDEX, SEED, STREAMS)[:, 0]
        assert any(INDEX[b] == 7 and v[b] > 1.0 and s[b] == tubes()[TUBE_INDEX[b]].s[-1] for b in range(B))
        on2 = [look[b]["branch"] for b in range(B) if TUBE_INDEX[b] == 2]
        assert "sqrt" in on2 and all(look[b]["branch"] == "linear" for b in range(B) if TUBE_INDEX[b] != 2)
        assert any(look[b]["branch"] == "linear" and abs(look[b]["A"]) < 1e-3 for b in range(B))
    return ref


def reference(single=np.float64):
    """the twin's result over the case for a library whose element type is `single`; computed once, shared, never modified"""
    return _reference(single)


def sincos_bars(ref, single=np.float64):
    """What E, N of the ego and of the other car may differ by from the twin, [B] each: (bar_ego, bar_other).  The device's sincos is within 2 ulp of the true value (the
    OpenCL bound its math library states), libm's within 1, so the two disagree by at most 3 * 2^-52 in sin or cos (|sin|, |cos| <= 1).  E = E_p - e cos psi: the product
    carries that error times |e| and moves the rounding of the product and of the sum by an ulp each: 3 * 2^-52 |e| + 2^-52 |e| + 2^-52 |E| -- bounded by
    4 * 2^-52 (|e| + max(|E|, |N|)).  The other car adds two more products on top of the ego's sum: 4 * 2^-52 (|dx| + |dy| + max(|E_o|, |N_o|)) + the ego's bar.
    A library that stores float rounds the sums once more: one ulp of the stored value may flip, 2^-23 of it."""
    u = 2.0 ** -52
    e = np.abs(ref["placed"][:, 1])
    big = np.maximum(np.abs(ref["state"][:, 0]), np.abs(ref["state"][:, 1]))
    ego = 4.0 * u * (e + big)
    o = ref["other"]
    reach = np.hypot(o[:, 0] - ref["state"][:, 0], o[:, 1] - ref["state"][:, 1])      # sqrt(dx^2 + dy^2) <= |dx| + |dy|
    other = np.where(o[:, 3] != 0.0, ego + 4.0 * u * (2.0 * reach + np.maximum(np.abs(o[:, 0]), np.abs(o[:, 1]))), 0.0)
    if single is np.float32:
        ego = ego + 2.0 ** -23 * big
        other = np.where(o[:, 3] != 0.0, other + 2.0 ** -23 * np.maximum(np.abs(o[:, 0]), np.abs(o[:, 1])), 0.0)
    return ego, other
