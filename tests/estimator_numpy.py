"""The yardstick of the estimator-set tests: the fixed-gain observer of the rollouts (pg_set_estimator_sets) in numpy, per instance.  Written from the law in
include/pigeon_mpc.h, not from the device code:

  p_k     = plant_step(vehicle, xh_{k-1}, u_{k-1}, dt)   predict == 1 (the CONTROLLER's vehicle; plant_numpy.plant_step_vec, RK4 with nsub sub-steps)
          = xh_{k-1}                                    predict == 0
  xh_k[c] = p_k[c] + gain[c] (y_k[c] - p_k[c])          gain 1 copies y_k[c], gain 0 copies p_k[c]; every product and sum rounded once, in `dtype`
  xh_k    = y_k                                         at the first step, for a set whose six gains are all 1, and where p_k has a non-finite component

The prior is computed in fp64 and rounded to `dtype`; the correction runs in `dtype`, so given the prior it agrees with the device to the last bit."""
import numpy as np

import plant_numpy

FIELDS = ("predict", "reserved", "gain")
CHANNELS = ("E", "N", "psi", "Ux", "Uy", "r")


def identity(**overrides):
    e = dict(predict=1, reserved=0, gain=[1.0] * 6)
    for k, v in overrides.items():
        if k not in e:
            raise KeyError(k)
        e[k] = v
    g = e["gain"]
    e["gain"] = [float(g)] * 6 if isinstance(g, (int, float)) else [float(x) for x in g]
    assert len(e["gain"]) == 6
    return e


def four_estimators():
    """The sets of the GPU tests: the identity; gain 0.2 with the model as the prior; gain 0.5 as a plain low-pass; a mix with two copied channels (E, N) and a
    dead-reckoned one (Uy)."""
    return [identity(), identity(gain=0.2, predict=1), identity(gain=0.5, predict=0), identity(gain=[1.0, 1.0, 0.2, 0.2, 0.0, 0.2], predict=1)]


def gains(sets, idx, B):
    """(gain [B][6], predict [B]) of the instances"""
    idx = np.zeros(B, dtype=np.int64) if idx is None else np.asarray(idx)
    return np.array([sets[i]["gain"] for i in idx], dtype=np.float64), np.array([int(sets[i]["predict"]) for i in idx])


def prior(sets, idx, xh_prev, u_prev, dt, vehicle, nsub=10, dtype=np.float64):
    """p_k [B][6] in `dtype` from the estimates xh_{k-1} [B][6] and the controls u_{k-1} [B][3]"""
    xh_prev = np.asarray(xh_prev, dtype=np.float64); B = xh_prev.shape[0]
    _, pred = gains(sets, idx, B)
    p = xh_prev.copy()
    if pred.any():
        with np.errstate(all="ignore"):
            stepped = plant_numpy.plant_step_vec(vehicle, xh_prev, u_prev, dt, nsub)
        p[pred == 1] = stepped[pred == 1]
    return p.astype(dtype)


def correct(sets, idx, p, y, dtype=np.float64):
    """xh_k [B][6] from the prior p and the measurement y, both already in `dtype`; the copies by selection, not by arithmetic"""
    p = np.asarray(p, dtype=dtype); y = np.asarray(y, dtype=dtype); B = y.shape[0]
    g, _ = gains(sets, idx, B)
    gd = g.astype(dtype)
    with np.errstate(all="ignore"):
        blend = p + gd * (y - p)
    xh = np.where(g == 1.0, y, np.where(g == 0.0, p, blend))
    restart = (g == 1.0).all(axis=1) | ~np.isfinite(p).all(axis=1)
    xh[restart] = y[restart]
    return xh.astype(dtype)


def step(sets, idx, xh_prev, y, u_prev, dt, vehicle, nsub=10, dtype=np.float64):
    """one step of the law: xh_k [B][6] (fp64 values of `dtype` numbers)"""
    p = prior(sets, idx, xh_prev, u_prev, dt, vehicle, nsub, dtype)
    return correct(sets, idx, p, np.asarray(y, dtype=np.float64).astype(dtype), dtype).astype(np.float64)


def response(sets, idx, y, u, dt, vehicle, nsub=10, dtype=np.float64):
    """y [steps][B][6], u [steps][B][3] (u[k]: the control the controller is handed at step k) -> xh [steps][B][6] from a fresh state: xh[0] = y[0]"""
    y = np.asarray(y, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    out = np.empty_like(y)
    out[0] = y[0].astype(dtype).astype(np.float64)
    for k in range(1, y.shape[0]):
        out[k] = step(sets, idx, out[k - 1], y[k], u[k - 1], dt, vehicle, nsub, dtype)
    return out
