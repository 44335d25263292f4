"""The decoder of tests/rollout_libs.py without a GPU: rollout() and join() driven by a stub handle whose simulate_, simulate_safety_ and simulate_node_ build their return
tuples as pigeon.jl_amd/mpc.py does -- the state after the call, the records (positional for simulate_, a dictionary for the other two), then the measured and the estimated
history, then, for simulate_ under an actuator or a disturbance library, a dictionary of that library's records.  Every array is filled with a constant of its own, so a
slot that lands under another name shows."""
import itertools

import numpy as np
import pytest

import rollout_libs as rl

B, STEPS, DT = 3, 5, 0.01
WIDTH = {"state": 6, "control": 3, "other": 4, "human": 2, "V": 0, "source": 0, "event": 0, "command": 3, "applied": 3, "disturbance": 4, "human_u": 2, "measured": 6,
         "estimated": 6, "final_state": 6, "final_control": 3, "final_t": 0, "final_other": 4, "final_applied": 3, "V_min": 0, "first_breach": 0, "policy_steps": 0}
CODE = {k: float(i + 1) for i, k in enumerate(WIDTH)}             # the constant each slot is filled with
ON_OFF = [False, True]


class Stub:
    """what the three rollout methods return, from step `clock` on: a record's row k holds CODE + (clock + k) / 100, a final value CODE + clock / 100 after the call"""

    def __init__(self, extras=()):
        self.extras = extras                                      # the records the installed libraries add
        self.clock = 0
        self.summaries = 0

    def rec(self, name, steps):
        rows = CODE[name] + (self.clock + np.arange(steps)) / 100.0
        return np.broadcast_to(rows.reshape((steps, 1) + (1,) * bool(WIDTH[name])), (steps, B) + (WIDTH[name],) * bool(WIDTH[name])).copy()

    def fin(self, name):
        return np.full((B,) + (WIDTH[name],) * bool(WIDTH[name]), CODE[name] + self.clock / 100.0)

    def tail(self, steps, measured, estimated):
        return tuple(self.rec(k, steps) for k, on in (("measured", measured), ("estimated", estimated)) if on)

    def simulate_(self, steps, dt=0.01, record=False, measured=False, estimated=False):
        assert record
        hist = (self.rec("state", steps), self.rec("control", steps))
        tail = self.tail(steps, measured, estimated)
        act = {k: self.rec(k, steps) for k in ("command", "applied", "disturbance") if k in self.extras}
        self.clock += steps
        return (self.fin("final_state"), self.fin("final_control"), self.fin("final_t")) + hist + tail + ((act,) if act else ())

    def simulate_safety_(self, steps, dt=0.01, use_HJI_policy=True, human="hold", human_u=None, record=False, measured=False, estimated=False):
        assert record
        out = {k: self.rec(k, steps) for k in ("state", "control", "other", "human", "V", "source") + tuple(self.extras)}
        tail = self.tail(steps, measured, estimated)
        self.clock += steps
        return tuple(self.fin(k) for k in rl.FINALS[:4]) + (out,) + tail

    def simulate_node_(self, steps, dt=0.01, use_HJI_policy=False, human="hold", human_u=None, pre_flag=None, record=False, measured=False, estimated=False):
        assert record
        out = {k: self.rec(k, steps) for k in ("state", "applied", "V", "event") + tuple(k for k in self.extras if k != "applied")}
        tail = self.tail(steps, measured, estimated)
        self.clock += steps
        return tuple(self.fin(k) for k in rl.FINALS) + (out,) + tail

    def safety_summary(self):
        self.summaries += 1
        return tuple(self.fin(k) for k in rl.SUMMARY)


# kind -> the records the rollout always makes; the finals it returns; the library records it can carry
ALWAYS = {"simulate": ("state", "control"), "safety": ("state", "control", "other", "human", "V", "source"), "node": ("state", "control", "applied", "V", "event")}
FINALS = {"simulate": rl.FINALS[:3], "safety": rl.FINALS[:4], "node": rl.FINALS}
EXTRAS = {"simulate": [(), ("command", "applied"), ("disturbance",), ("command", "applied", "disturbance")],
          "safety": [(), ("human_u",), ("command", "applied"), ("disturbance",), ("human_u", "command", "applied", "disturbance")],
          "node": [(), ("human_u",), ("command", "applied"), ("disturbance",), ("human_u", "command", "applied", "disturbance")]}
CASES = [(kind, extras, measured, estimated) for kind in ALWAYS for extras in EXTRAS[kind] for measured, estimated in itertools.product(ON_OFF, ON_OFF)]


def expected(kind, extras, measured, estimated, summary, step0, steps):
    """the dictionary rollout() must give: the name -> CODE of that name (the node rollout's "control" is its "applied" record), None for everything not produced"""
    made = set(ALWAYS[kind]) | set(extras) | {k for k, on in (("measured", measured), ("estimated", estimated)) if on}
    want = dict.fromkeys(rl.KEYS)
    for k in made:
        source = "applied" if kind == "node" and k == "control" else k
        want[k] = CODE[source] + (step0 + np.arange(steps)) / 100.0
    for k in FINALS[kind] + (rl.SUMMARY if summary else ()):
        want[k] = CODE[k] + (step0 + steps) / 100.0
    return want


def check(r, want, steps):
    assert tuple(r) == rl.KEYS                                    # the fixed key set, in its fixed order
    for k in rl.KEYS:
        if want[k] is None:
            assert r[k] is None, k
            continue
        assert r[k] is not None, k
        shape = ((steps, B) if k in rl.RECORDS else (B,)) + (WIDTH[k],) * bool(WIDTH[k])
        assert r[k].shape == shape, (k, r[k].shape)
        rows = np.asarray(want[k]).reshape((-1,) + (1,) * (len(shape) - 1)) if k in rl.RECORDS else want[k]
        assert np.array_equal(r[k], np.broadcast_to(rows, shape)), (k, r[k].ravel()[0])


def test_the_codes_are_distinct_and_cover_the_keys():
    assert set(WIDTH) == set(rl.KEYS) and len(set(CODE.values())) == len(rl.KEYS)
    assert rl.KEYS == rl.RECORDS + rl.FINALS + rl.SUMMARY and len(set(rl.KEYS)) == len(rl.KEYS)


@pytest.mark.parametrize("kind,extras,measured,estimated", CASES, ids=lambda v: "+".join(v) or "plain" if isinstance(v, tuple) else str(v))
def test_every_slot_lands_under_its_name(kind, extras, measured, estimated):
    for summary in ON_OFF:
        m = Stub(extras)
        r = rl.rollout(m, kind, STEPS, DT, measured=measured, estimated=estimated, summary=summary)
        check(r, expected(kind, extras, measured, estimated, summary, 0, STEPS), STEPS)
        assert m.summaries == int(summary)                        # the synchronising call: only when asked for


@pytest.mark.parametrize("kind,extras,measured,estimated", CASES, ids=lambda v: "+".join(v) or "plain" if isinstance(v, tuple) else str(v))
def test_join_of_two_calls_is_the_one_call(kind, extras, measured, estimated):
    opts = dict(measured=measured, estimated=estimated, summary=True)
    whole = rl.rollout(Stub(extras), kind, STEPS, DT, **opts)
    m = Stub(extras)
    parts = [rl.rollout(m, kind, 2, DT, **opts), rl.rollout(m, kind, 3, DT, **opts)]
    check(parts[1], expected(kind, extras, measured, estimated, True, 2, 3), 3)
    split = rl.join(parts)
    assert tuple(split) == rl.KEYS
    for k in rl.KEYS:
        assert rl.same(whole[k], split[k]), k
    check(split, expected(kind, extras, measured, estimated, True, 0, STEPS), STEPS)


def test_the_options_reach_the_method():
    seen = {}

    class Spy(Stub):
        def simulate_safety_(self, steps, dt=0.01, **kw):
            seen["safety"] = (steps, dt, kw)
            return super().simulate_safety_(steps, dt, **kw)

        def simulate_node_(self, steps, dt=0.01, **kw):
            seen["node"] = (steps, dt, kw)
            return super().simulate_node_(steps, dt, **kw)
    script = np.zeros((STEPS, B, 2)); pre = np.ones((STEPS, B), dtype=np.uint8)
    rl.rollout(Spy(), "safety", STEPS, 0.02, use_HJI_policy=True, human="script", human_u=script, measured=True)
    assert seen["safety"] == (STEPS, 0.02, dict(use_HJI_policy=True, human="script", human_u=script, record=True, measured=True, estimated=False))
    rl.rollout(Spy(), "node", STEPS, DT, pre_flag=pre, estimated=True)
    assert seen["node"] == (STEPS, DT, dict(use_HJI_policy=False, human="hold", human_u=None, pre_flag=pre, record=True, measured=False, estimated=True))


def test_an_unknown_record_or_a_leftover_output_is_refused():
    class Grown(Stub):
        def simulate_safety_(self, steps, dt=0.01, **kw):
            out = super().simulate_safety_(steps, dt, **kw)
            return out[:4] + (dict(out[4], jerk=np.zeros((steps, B))),) + out[5:]

        def simulate_(self, steps, dt=0.01, **kw):
            return super().simulate_(steps, dt, **kw) + (np.zeros((steps, B, 6)),)
    with pytest.raises(AssertionError):
        rl.rollout(Grown(), "safety", STEPS, DT)
    with pytest.raises(AssertionError):
        rl.rollout(Grown(), "simulate", STEPS, DT)
    with pytest.raises(AssertionError):
        rl.rollout(Stub(), "rollout", STEPS, DT)


def test_the_measures():
    assert rl.same(None, None) and not rl.same(None, np.zeros(2)) and not rl.same(np.zeros(2), None)
    assert rl.same(np.array([np.nan, 1.0]), np.array([np.nan, 1.0])) and not rl.same(np.array([0.0]), np.array([-0.0]))
    assert rl.same(np.array([1, 2], dtype=np.int32), np.array([1, 2])) and not rl.same(np.zeros(2), np.zeros(3))
    assert rl.same(np.float32(0.1) * np.ones(2, dtype=np.float32), np.full(2, float(np.float32(0.1))))          # an fp32 result against its fp64 record
    assert np.array_equal(rl.rel([2.0, 0.5], [4.0, 0.25]), [0.5, 0.25])
    ids = rl.stream_ids(70)
    assert ids.dtype == np.uint64 and ids[0] == 7 and np.all(ids[1:] > 1 << 32)
    assert len(set(ids & np.uint64(0xFFFFFFFF))) == 70 and len(set(ids >> np.uint64(32))) == 70
