"""numpy twin of the route library (pg_set_route_sets; include/pigeon_mpc.h): which event of a set fires at which clock step, where it sends the instance (absolute and
relative targets, the relative ones modulo the library with negative wrap), the four anchors of the new time offset, and the schedule a rollout records (the trajectory
each step's controller ran on).  The projection of the PROJECT anchor is oracle/spec_numpy.py's path_coordinates (trajectories.jl:71-94): nothing of it is restated here."""
import numpy as np

from oracle import spec_numpy

EVENTS = 4
ABSOLUTE, RELATIVE = 0, 1
KEEP, PATH, STAMP, PROJECT = 0, 1, 2, 3
FIELDS = ("step", "target", "target_mode", "anchor", "cold", "reserved", "t_join")


def event(step, target, anchor=STAMP, relative=False, cold=True, t_join=0.0):
    return dict(step=int(step), target=int(target), target_mode=RELATIVE if relative else ABSOLUTE, anchor=int(anchor), cold=int(bool(cold)), reserved=0, t_join=float(t_join))


def route(*events):
    """a set: the events, then unused slots (step -1) up to EVENTS; route() is the identity"""
    assert len(events) <= EVENTS
    return [dict(e) for e in events] + [event(-1, 0) for _ in range(EVENTS - len(events))]


def fires(rset, step):
    """the event of the set that fires at clock step `step`, or None (the steps of a set's used slots are strictly increasing: at most one)"""
    hit = [e for e in rset if e["step"] >= 0 and e["step"] == step]
    assert len(hit) <= 1
    return hit[0] if hit else None


def target_of(e, current, n_traj):
    """Python's % already wraps a negative sum into [0, n_traj)"""
    return (current + e["target"]) % n_traj if e["target_mode"] == RELATIVE else e["target"]


def offset_of(e, t0, toff, t_proj=None):
    """(the new time offset, t_at) of an event at clock time t0 for an instance whose offset is toff; t_proj: the third path coordinate on the target (PROJECT only)"""
    a = e["anchor"]
    if a == KEEP:
        return toff, t0 - toff
    if a == PATH:
        return np.nan, np.nan
    if a == STAMP:
        return t0 - e["t_join"], e["t_join"]
    assert a == PROJECT and t_proj is not None
    return t0 - (t_proj + e["t_join"]), t_proj


def project(traj_data, E, N):
    """(s, e, t) of a position on a trajectory given as its 12 channels"""
    return spec_numpy.Trajectory(traj_data).path_coordinates(E, N)


def schedule(sets, index, home, n_traj, step0, steps):
    """(ran [steps][B]: the trajectory the controller of clock step step0 + k ran on, fired [B], last_step [B]) from the home index, for a clock that started at step 0"""
    home = np.asarray(home, dtype=np.int32)
    B = len(home)
    cur = home.copy(); fired = np.zeros(B, dtype=np.int32); last = np.full(B, -1, dtype=np.int32)
    ran = np.zeros((steps, B), dtype=np.int32)
    for k in range(step0 + steps):
        for b in range(B):
            e = fires(sets[0 if index is None else index[b]], k)
            if e is not None:
                cur[b] = target_of(e, cur[b], n_traj); fired[b] += 1; last[b] = k
        if k >= step0:
            ran[k - step0] = cur
    return ran, fired, last


# why pg_set_route_sets refuses a set, in the order route_set_problem (csrc/pg_api.hip) tests: its texts, word for word
BAD_TARGET_MODE = "target_mode must be 0 (absolute) or 1 (relative)"
BAD_ANCHOR = "anchor must be 0 (keep), 1 (path), 2 (stamp) or 3 (project)"
BAD_COLD = "cold must be 0 or 1"
BAD_RESERVED = "reserved must be 0"
BAD_T_JOIN = "t_join must be finite"
T_JOIN_UNUSED = "t_join must be 0 under the anchors keep and path"
USED_BEHIND_UNUSED = "a used slot (step >= 0) stands behind an unused one"
NOT_INCREASING = "the steps of the used slots must be strictly increasing"
NEGATIVE_TARGET = "an absolute target must be >= 0"
PROBLEMS = (BAD_TARGET_MODE, BAD_ANCHOR, BAD_COLD, BAD_RESERVED, BAD_T_JOIN, T_JOIN_UNUSED, USED_BEHIND_UNUSED, NOT_INCREASING, NEGATIVE_TARGET)


def problem(rset):
    """why a set is refused, or None"""
    unused_seen, last = False, -1
    for e in rset:
        if e["target_mode"] not in (ABSOLUTE, RELATIVE):
            return BAD_TARGET_MODE
        if not KEEP <= e["anchor"] <= PROJECT:
            return BAD_ANCHOR
        if e["cold"] not in (0, 1):
            return BAD_COLD
        if e["reserved"] != 0:
            return BAD_RESERVED
        if not np.isfinite(e["t_join"]):
            return BAD_T_JOIN
        if e["anchor"] in (KEEP, PATH) and e["t_join"] != 0.0:
            return T_JOIN_UNUSED
        if e["step"] < 0:
            unused_seen = True
            continue
        if unused_seen:
            return USED_BEHIND_UNUSED
        if e["step"] <= last:
            return NOT_INCREASING
        last = e["step"]
        if e["target_mode"] == ABSOLUTE and e["target"] < 0:
            return NEGATIVE_TARGET
    return None
