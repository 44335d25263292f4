"""Float64 twin of pg_tune_smoothing, written from the scheme stated in include/pigeon_mpc.h (not from the kernel): one (path, set) pair at a time.  F and the final solve
are wp_smooth_numpy.smooth, the twin of pg_smooth_waypoints; the ladder is one rounded product and one rounded square root per midpoint; the comparisons are exact.  The
scheme has only + - * / sqrt, so the library's output is this one's bit for bit."""
import math

import wp_smooth_numpy as smoother

CAND = 17
TUNE_STATS = ("lam", "lo", "hi", "rms_lo", "rms_hi", "verdict", "rounds_done", "monotone", "reserved")
SET_DEFAULTS = dict(target=1e-3, lambda_lo=1e-6, lambda_hi=1e3, rounds=3)


def tune_set(target=1e-3, lambda_lo=1e-6, lambda_hi=1e3, rounds=3, **smooth_kw):
    if "lam" in smooth_kw:
        raise KeyError("lam")
    return dict(base=smoother.smooth_set(**smooth_kw), target=float(target), lambda_lo=float(lambda_lo), lambda_hi=float(lambda_hi), rounds=int(rounds))


def ladder(lo, hi):
    """Ladder: c_0 = lo, c_16 = hi, then four levels of midpoints, each sqrt((left right)) of its two neighbours on the level above"""
    c = [0.0] * CAND
    c[0] = float(lo); c[16] = float(hi)
    half = 8
    while half >= 1:
        for j in range(half, 16, 2 * half):
            c[j] = math.sqrt(c[j - half] * c[j + half])
        half //= 2
    return c


def tune(waypoints, closed=False, t=None, cache=None):
    """t: tune_set(...) -> dict(stats: the fields of pg_tune_stats; solve: wp_smooth_numpy.smooth under base with the chosen weight; rounds: per evaluated round the
    candidates and F at them).  cache: a dict the caller may share between calls on the SAME waypoints (F by (base, lambda): evaluation is deterministic)."""
    t = tune_set() if t is None else t
    base = t["base"]
    if float(base["lam"]) != 0.0:
        raise ValueError("base.lam must be 0")
    cache = {} if cache is None else cache
    key = (bool(closed), bool(base["pin_ends"]), bool(base["keep_walls"]), tuple(tuple(w) for w in base["windows"]))

    def F(lam):
        if (key, lam) not in cache:
            r = smoother.smooth(waypoints, closed, dict(base, lam=lam))
            if not all(p > 0.0 for p in r["pivots"]) or not math.isfinite(r["stats"]["dev_rms"]):
                raise ArithmeticError("a pivot that is not > 0 or an F that is not finite at a candidate")
            cache[(key, lam)] = r["stats"]["dev_rms"]
        return cache[(key, lam)]
    target = t["target"]
    lo, hi = t["lambda_lo"], t["lambda_hi"]
    verdict = 0.0; rounds_done = 0.0; monotone = 1.0; rms_lo = rms_hi = 0.0
    rounds = []
    for rnd in range(t["rounds"]):
        c = ladder(lo, hi)
        if rnd >= 1 and any(c[j] == c[j + 1] for j in range(16)):
            break                                                   # Stop: the round evaluates nothing
        f = [F(x) for x in c]
        rounds.append((c, f))
        rounds_done += 1.0
        if not all(f[j] <= f[j + 1] for j in range(16)):
            monotone = 0.0
        if rnd == 0 and f[0] > target:
            verdict = -1.0; hi = lo; rms_lo = rms_hi = f[0]
            break
        if rnd == 0 and f[16] <= target:
            verdict = 1.0; lo = hi; rms_lo = rms_hi = f[16]
            break
        j = min(k for k in range(1, CAND) if f[k] > target)         # Narrowing: the smallest j in 1 .. 16 with F(c_j) > target
        lo, hi, rms_lo, rms_hi = c[j - 1], c[j], f[j - 1], f[j]
    stats = dict(lam=lo, lo=lo, hi=hi, rms_lo=rms_lo, rms_hi=rms_hi, verdict=verdict, rounds_done=rounds_done, monotone=monotone, reserved=0.0)
    return dict(stats=stats, solve=smoother.smooth(waypoints, closed, dict(base, lam=lo)), rounds=rounds)


def bisect(waypoints, closed, t, steps=64):
    """A plain bisection on dev_rms between lambda_lo and lambda_hi with math.sqrt midpoints: the largest weight found whose dev_rms <= target (the caller has seen
    F(lambda_lo) <= target < F(lambda_hi))"""
    lo, hi = t["lambda_lo"], t["lambda_hi"]
    for _ in range(steps):
        mid = math.sqrt(lo * hi)
        if mid == lo or mid == hi:
            break
        if smoother.smooth(waypoints, closed, dict(t["base"], lam=mid))["stats"]["dev_rms"] <= t["target"]:
            lo = mid
        else:
            hi = mid
    return lo, hi
