"""Host restatement of the node callback (from_autobox_callback, ros_integration.jl:48-151) for one instance and one message, as pg_node_step_dev /
pg_simulate_node_dev reproduce it per instance (include/pigeon_mpc.h): the gates in the reference's order, the NaN fallback, and the update of the to_autobox message
and of the command the vehicle applies.  Written from the reference, independent of the device code; the GPU tests take their expected events from it."""
import math

import numpy as np

MPC, HJI_POLICY, FEATHER, NAN_FALLBACK, PRE_FLAG_OFF, OUTSIDE_TRAJECTORY, LOW_SPEED = range(7)
GATED = (PRE_FLAG_OFF, OUTSIDE_TRAJECTORY, LOW_SPEED)


def gate(pre_flag, time_offset, t, t_end, Ux):
    """0 when the callback goes on to the compute calls, else the event of its early return: pre_flag == 0 (:70-73), then -- trajectory mode only (time_offset not NaN)
    -- t outside [0, t_end] (:79-82, both ends inside), then Ux < 1 (:84-87, the literal 1 m/s)."""
    if pre_flag == 0:
        return PRE_FLAG_OFF
    if not math.isnan(time_offset) and (t < 0 or t > t_end):
        return OUTSIDE_TRAJECTORY
    if Ux < 1:
        return LOW_SPEED
    return 0


def decide(code, source, selected, message):
    """One callback after the gates: code from gate(), source of the selection (0 MPC, 1 HJI policy, 2 V <= eps with the policy off: :114-124), selected control [3],
    message = the to_autobox command last published (current_control, :52).  Returns (event, published or None, the message after the callback)."""
    message = np.asarray(message, dtype=np.float64)
    if code:
        return code, None, message.copy()                                        # an early return publishes nothing
    selected = np.asarray(selected, dtype=np.float64)
    if np.any(np.isnan(selected)):                                               # :134-147 (isnan: an Inf is published)
        return NAN_FALLBACK, message.copy(), np.zeros(3)
    return source, selected.copy(), selected.copy()


def applied_after(applied, published):
    """The command the vehicle executes from the next step on: the published one, or the last one when nothing was published (the autobox keeps it)."""
    return np.asarray(applied if published is None else published, dtype=np.float64).copy()


def run(codes, sources, selected, message, applied):
    """A sequence of callbacks for one instance: codes / sources [steps], selected [steps][3].  Returns the events [steps], the applied command at the start of every
    step [steps][3] (what the plant integrates over that step) and the final (message, applied)."""
    ev, ap = [], []
    msg = np.asarray(message, dtype=np.float64).copy(); app = np.asarray(applied, dtype=np.float64).copy()
    for k, code in enumerate(codes):
        ap.append(app.copy())
        e, pub, msg = decide(code, sources[k], selected[k], msg)
        app = applied_after(app, pub)
        ev.append(e)
    return np.array(ev, dtype=np.int32), np.array(ap), msg, app
