"""The shared case of the pg_optimize_line tests (host twin and device): PATHS x SETS, the smallest shapes at which each code path can go wrong.

Paths (name, closed, waypoints), the shapes of tests/wp_smooth_cases.py:
  open5 (the shortest open path the list holds), open64 (a 240 degree arc of R = 30 m, unequal chords about 2 m, varying edges);
  closed5 (the smallest closed path: band and border adjacent), closed63 (skidpadoval taken every 16th point, mean chord 3.74 m: the converging case of EXPERIMENTS 43);
  open1100 and closed1030: more rows than the 1024 the kernel keeps in LDS, so the recurrence's state is in the call's scratch; `iters` = 8 there.
Sets (mu and rho are 1e-6 and 0.1 over 3.74^3, the oval's scale): the plain set; a window with its own margin and a later, overlapping one that pins, with keep_walls;
tol = 1e-3, which stops early; pin_ends with keep_walls, a wider margin and a small alpha_max.  The twin's results are computed once (reference()) and shared."""
import functools

import line_opt_numpy as twin
import wp_smooth_cases as shapes

SCALE = 1.0 / 3.74 ** 3
BASE = dict(mu=1e-6 * SCALE, rho=0.1 * SCALE, margin=0.5, alpha_max=2.0)
SET_NAMES = ("plain", "windows", "tol", "ends")
BIG = ("open1100", "closed1030")


def sets_for(name):
    iters = 8 if name in BIG else 1000 if name == "closed63" else 300
    return [twin.line_set(iters=iters, **BASE),
            twin.line_set(iters=iters, keep_walls=True, windows=[(5.0, 12.0, 0.25, False), (10.0, 20.0, 0.0, True)], **BASE),
            twin.line_set(iters=iters, tol=1e-3, **BASE),
            twin.line_set(iters=iters, pin_ends=True, keep_walls=True, **dict(BASE, margin=1.0, alpha_max=0.75))]


@functools.lru_cache(maxsize=None)
def paths():
    by_name = {name: (closed, w) for name, closed, w in shapes.paths()}
    oval = shapes.golden("skidpadoval", True)[::16]
    return (("open5", False, by_name["open5"][1]), ("open64", False, shapes.arc(64, False, 7)), ("closed5", True, by_name["closed5"][1]), ("closed63", True, oval),
            ("open1100", False, by_name["open1100"][1]), ("closed1030", True, by_name["closed1030"][1]))


def path(name):
    return next((closed, w) for n, closed, w in paths() if n == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the twin's result of the path under each of its four sets"""
    closed, w = path(name)
    return tuple(twin.optimize(w, closed, s) for s in sets_for(name))


BATCH_PATHS = ("open5", "closed5", "open64")      # one call of 3 paths x 4 sets (the sets of the small paths are the same four)


def fit_paths_list(names):
    """the paths as mpc.optimize_line takes them"""
    return [dict(waypoints=path(n)[1], closed=path(n)[0]) for n in names]


as_bits = shapes.as_bits
