"""The shared case of the pg_tune_smoothing tests (host twin and device): PATHS x SETS, the smallest shapes at which each code path can go wrong.

Paths, taken from or built as tests/wp_smooth_cases.py builds its own:
  open2 (no row: F = 0 everywhere, verdict +1 in round 0), open3 (one row), closed5 (the smallest border);
  open256 and closed257: the block width of Sum changes from 1 to 2 between them, and both have more rows than the 64 the search keeps in LDS;
  open1100 and closed1030: more rows than the 1024 the final solve keeps in LDS (the three short paths are below both limits);
  skidpadoval (999, closed): the real survey.
Sets (every bracket is [1e-4, 1e2] unless said; targets in metres):
  0  3 rounds, target 2e-3;
  1  rounds = 1, target 2e-3;
  2  rounds = 8 on a bracket 2^-24 wide in ratio, whose lower end is the weight set 0 ends on for closed5 and whose target is that weight's dev_rms: on closed5 the
     ladder runs out of doubles and the search stops after 7 rounds on equal neighbours; every other path ends round 0 with a verdict;
  3  a window of factor 0 and pin_ends, rounds 2, target 1e-3;
  4  keep_walls, rounds 2, target 5e-4;
  5  target 1e-9, below F(lambda_lo) on every path of three waypoints or more: verdict -1;
  6  target 10, above F(lambda_hi) everywhere: verdict +1;
  7  the library's default, pg_default_tune_set: target 1e-3 between 1e-6 and 1e3 in 3 rounds.
The twin's results are computed once (reference()) and shared."""
import functools

import wp_smooth_cases as smooth_cases
import wp_tune_numpy as twin

LO, HI = 1e-4, 1e2
SETS = [twin.tune_set(target=2e-3, lambda_lo=LO, lambda_hi=HI, rounds=3),
        twin.tune_set(target=2e-3, lambda_lo=LO, lambda_hi=HI, rounds=1),
        twin.tune_set(target=0.0019948854444653617, lambda_lo=0.021845172011711232, lambda_hi=0.021845172011711232 * (1.0 + 2.0 ** -24), rounds=8),
        twin.tune_set(target=1e-3, lambda_lo=LO, lambda_hi=HI, rounds=2, pin_ends=True, windows=[(2.0, 6.0, 0.0)]),
        twin.tune_set(target=5e-4, lambda_lo=LO, lambda_hi=HI, rounds=2, keep_walls=True),
        twin.tune_set(target=1e-9, lambda_lo=LO, lambda_hi=HI, rounds=3),
        twin.tune_set(target=10.0, lambda_lo=LO, lambda_hi=HI, rounds=3),
        twin.tune_set()]
WINDOWED = (3,)                                                 # the sets on which monotone may be 0
OVAL = twin.tune_set(target=1.6e-5, lambda_lo=1e-4, lambda_hi=1e2, rounds=2)      # the oval's own case: EXPERIMENTS 41 has rms 1.6e-5 m at lambda = 0.1


@functools.lru_cache(maxsize=None)
def paths():
    by_name = {name: (name, closed, w) for name, closed, w in smooth_cases.paths()}
    out = [by_name["open2"], by_name["open3"], by_name["closed5"]]
    out += [("open256", False, smooth_cases.arc(256, False, 7)), ("closed257", True, smooth_cases.arc(257, True, 3))]
    out += [by_name["open1100"], by_name["closed1030"], by_name["skidpadoval"]]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference():
    """ref[path][set]: the twin's result of every pair; F is shared between the sets of a path"""
    out = []
    for _, closed, w in paths():
        cache = {}
        out.append(tuple(twin.tune(w, closed, t, cache) for t in SETS))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oval_reference():
    name, closed, w = paths()[-1]
    return twin.tune(w, closed, OVAL)


def fit_paths_list():
    """the paths as mpc.tune_smoothing takes them"""
    return [dict(waypoints=w, closed=closed) for _, closed, w in paths()]


def as_vehicle_set(t):
    """a twin set as the dict vehicles.tune(...) makes"""
    return dict(base=dict(t["base"], windows=list(t["base"]["windows"])), target=t["target"], lambda_lo=t["lambda_lo"], lambda_hi=t["lambda_hi"], rounds=t["rounds"])
