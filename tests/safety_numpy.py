"""numpy restatement of the other car of the safety rollout (pg_simulate_safety_dev, include/pigeon_mpc.h) for the tests: the human's worst case
optimal_disturbance (dMode :min, HJI_computation.jl:90-131), the other car's RK4 with the clamp V >= 0 after each sub-step (build-defined), and the relative state
HJIRelativeState (HJI_computation.jl:20-24).  Vectorised over instances; written from the reference's equations, independent of the device code."""
import numpy as np


def optimal_disturbance(X, x7, gradV):
    """(omega, a) [B, 2] at relative states x7 [B, 7] = (dE, dN, dpsi, Ux, Uy, V, r) and gradients gradV [B, 7]; the rows with V <= 0 get (0, 0) (build-defined:
    the reference divides by V there)."""
    x7 = np.atleast_2d(np.asarray(x7, dtype=np.float64)); g = np.atleast_2d(np.asarray(gradV, dtype=np.float64))
    out = np.zeros((x7.shape[0], 2))
    Ax_max = X["Fx_max"] / X["m"]; Pmx_max = X["Px_max"] / X["m"]; maxA = 0.9 * X["mu"] * X["G"]
    for i in range(x7.shape[0]):
        V = x7[i, 5]
        if not V > 0.0:
            continue
        lam_Ax = g[i, 5]; lam_Ay = g[i, 2] / V
        lam_norm = np.hypot(lam_Ax, lam_Ay)
        if lam_norm < 1e-3:                                                     # :106-107
            continue
        desAx = -lam_Ax * maxA / lam_norm; desAy = -lam_Ay * maxA / lam_norm
        maxAx = min(Ax_max, Pmx_max / V); maxAy = X["kappa_max"] * V * V
        if desAx > maxAx:                                                       # :113-117
            if abs(desAy) < maxAy:
                maxAy = min(maxAy, np.sqrt(maxA * maxA - maxAx * maxAx))
            out[i] = (np.copysign(maxAy, desAy) / V, maxAx)
        elif abs(desAy) > maxAy:                                                # :119-125
            if desAx > 0:
                maxAx = min(np.sqrt(maxA * maxA - maxAy * maxAy), maxAx)
                out[i] = (np.copysign(maxAy, desAy) / V, maxAx)
            else:
                out[i] = (np.copysign(maxAy, desAy) / V, -np.sqrt(maxA * maxA - maxAy * maxAy))
        else:                                                                   # :127
            out[i] = (desAy / V, maxAx)
    return out


def unicycle_rhs(y, w, a):
    """(-V sin psi, V cos psi, omega, a): SimpleCarState with psi measured from North (vehicle_dynamics.jl:127-129)."""
    return np.stack([-y[:, 3] * np.sin(y[:, 2]), y[:, 3] * np.cos(y[:, 2]), w, a], axis=1)


def other_car_step(other, human_u, dt, nsub=10):
    """other [B, 4] = (E, N, psi, V) after one step of nsub RK4 sub-steps with human_u [B, 2] = (omega, a) held; V <- max(V, 0) after every sub-step."""
    x = np.array(other, dtype=np.float64).reshape(-1, 4)
    u = np.asarray(human_u, dtype=np.float64).reshape(-1, 2)
    w, a = u[:, 0], u[:, 1]
    h = dt / nsub
    for _ in range(nsub):
        k1 = unicycle_rhs(x, w, a)
        k2 = unicycle_rhs(x + k1 * (h * 0.5), w, a)
        k3 = unicycle_rhs(x + k2 * (h * 0.5), w, a)
        k4 = unicycle_rhs(x + k3 * h, w, a)
        x = x + (k1 + 2.0 * k2 + 2.0 * k3 + k4) * (h / 6.0)
        x[:, 3] = np.where(x[:, 3] < 0.0, 0.0, x[:, 3])
    return x


def relative_state(state, other):
    """HJIRelativeState(us, them) [B, 7] (HJI_computation.jl:20-24; cpsi = sin(-psi), spsi = cos(-psi) as the reference names them)."""
    us = np.atleast_2d(np.asarray(state, dtype=np.float64)); th = np.atleast_2d(np.asarray(other, dtype=np.float64))
    cpsi = np.sin(-us[:, 2]); spsi = np.cos(-us[:, 2])
    dE = th[:, 0] - us[:, 0]; dN = th[:, 1] - us[:, 1]
    d = np.mod(th[:, 2] - us[:, 2], 2 * np.pi)
    d = np.where(d <= np.pi, d, d - 2 * np.pi)                                  # adiff (PigeonViz.jl:24-28)
    return np.stack([cpsi * dE + spsi * dN, -spsi * dE + cpsi * dN, d, us[:, 3], us[:, 4], th[:, 3], us[:, 5]], axis=1)
