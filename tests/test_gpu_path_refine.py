"""pg_refine_paths on the device against its float64 numpy twin (tests/path_refine_numpy.py) over the shared case of tests/path_refine_cases.py: three sources x five
refine sets in one call, Lmax = 258, Lmax_out = 900.  Then the fp32 library (the fp64 library's output rounded to float), independence of the batch and of both
capacities, the exact fit into Lmax_out, the install path against pg_set_trajectories, the chains refine -> offset -> install and refine -> clip on the two failures the
knot-wise makers document, and every refusal with its whole text.

fp64 library: every operation of the scheme is rounded once in both places, so L_out, t, s, V, A, psi, kappa and both edges are the twin's bit for bit (they carry no libm
call but sqrt), and so is every stat but closure_pos_max.  E, N and closure_pos_max carry sin and cos of the 4-point rule: within 8 * 2^-52 * (|E or N| + ds_max of the
source), the form of the bar pg_offset_paths states for its sin / cos channels (there |d| is the length the sincos multiplies, here it is the interval)."""
import math

import numpy as np
import pytest

import path_refine_cases as cases
import tube_clip_cases
from path_libs import INVALID, OK, c_dp, c_i32p, handle, install_equals_set_trajectories, lib, step_bits

pytestmark = pytest.mark.gpu

NP, NS = cases.N_PATH, cases.N_SETS
EXACT = ((0, "t"), (1, "s"), (2, "V"), (3, "A"), (6, "psi"), (7, "kappa"), (8, "edge_L"), (9, "edge_R"))
EXACT_STATS = ("length", "ds_min", "ds_max", "closure_psi_max", "kappa_abs_max", "n_added", "m_max", "reserved")
WHO = "pg_refine_paths: "


def raw_refine(m, L, cl, ch, sets, Lmax_out=cases.LMAX_OUT, install=False, want=OK):
    n = len(L) * len(sets)
    out = np.full((n, 10, Lmax_out), np.nan)
    Lo = np.full(n, -1, dtype=np.int32); co = np.full(n, -1, dtype=np.int32)
    st = (lib().pg_refine_stats * n)()
    rc = m.lib.pg_refine_paths(m.h, len(L), ch.shape[2], L.ctypes.data_as(c_i32p), cl.ctypes.data_as(c_i32p), ch.ctypes.data_as(c_dp), len(sets), sets, Lmax_out, int(install),
                               Lo.ctypes.data_as(c_i32p), co.ctypes.data_as(c_i32p), out.ctypes.data_as(c_dp), st)
    assert rc == want, m.lib.pg_last_error(m.h)
    return out, st, Lo, co


@pytest.fixture(scope="module")
def made(pkg):
    """the shared case through the fp64 library, once: (channels_out [15][10][900], stats, L_out, closed_out)"""
    m = handle(pkg)
    out = raw_refine(m, *cases.packed())
    m.close()
    return out


def test_fp64_library_against_the_twin(made):
    out, st, Lo, co = made
    ref = cases.reference()
    exp = cases.expected_channels()
    src = cases.sources()
    assert list(Lo) == [len(r["s"]) for row in ref for r in row] and list(co) == [cases.CLOSED[k // NS] for k in range(NP * NS)]
    assert 257 in Lo and max(Lo) > 3 * 256                          # one knot past the workgroup's threads; a fourth knot for some threads
    worst = dict(E=0.0, N=0.0); differ = dict(E=0, N=0)
    for k in range(NP * NS):
        p, q = divmod(k, NS)
        r = ref[p][q]
        n = len(r["s"])
        assert np.all(out[k][:, n:] == 0.0), k
        for c, name in EXACT:
            assert out[k, c, :n].tobytes() == exp[k, c, :n].tobytes(), (p, q, name)
        ds_src = float(np.max(np.diff(src[p, 1, :cases.N_KNOTS[p]])))
        for c, name in ((4, "E"), (5, "N")):
            d = np.abs(out[k, c, :n] - exp[k, c, :n])
            worst[name] = max(worst[name], float(d.max())); differ[name] += int(np.count_nonzero(d))
            assert np.all(d <= 8.0 * 2.0 ** -52 * (np.abs(exp[k, c, :n]) + ds_src)), (p, q, name, float(d.max()))
            at = np.array(r["o"])                                   # the source knots are copies
            assert out[k, c, at].tobytes() == np.ascontiguousarray(src[p, c, :cases.N_KNOTS[p]]).tobytes(), (p, q, name)
        for f in EXACT_STATS:
            assert getattr(st[k], f) == r["stats"][f], (p, q, f)
        assert abs(st[k].closure_pos_max - r["stats"]["closure_pos_max"]) <= 8.0 * 2.0 ** -52 * (float(np.max(np.abs(exp[k, 4:6, :n]))) + ds_src), (p, q)
    total = int(sum(Lo))
    print(f"worst |E - twin| {worst['E']:.3e} m ({differ['E']} of {total} knots differ), |N - twin| {worst['N']:.3e} m ({differ['N']})")


def test_fp32_library_is_the_fp64_output_rounded(pkg, made):
    out, st, Lo, co = made
    m = handle(pkg, "f32")
    o32, s32, L32, c32 = raw_refine(m, *cases.packed())
    m.close()
    assert o32.tobytes() == out.astype(np.float32).astype(np.float64).tobytes()
    assert bytes(s32) == bytes(st) and L32.tobytes() == Lo.tobytes() and c32.tobytes() == co.tobytes()


def test_independence_of_the_batch_and_of_both_capacities(pkg, made):
    out, st, Lo, co = made
    m = handle(pkg)
    for p in range(NP):                                             # each pair alone, Lmax = the path's own knot count, Lmax_out = the pair's own: it fits exactly
        for q in range(NS):
            k = p * NS + q
            n = int(Lo[k])
            one, s1, L1, c1 = raw_refine(m, *cases.packed([p], [q], Lmax=cases.N_KNOTS[p]), Lmax_out=n)
            assert one[0].tobytes() == np.ascontiguousarray(out[k][:, :n]).tobytes(), (p, q)
            assert bytes(s1[0]) == bytes(st[k]) and L1[0] == n and c1[0] == cases.CLOSED[p], (p, q)
    # ... and one knot less is refused, naming the pair, its count and the capacity
    raw_refine(m, *cases.packed([2], [0, 1]), Lmax_out=256, want=INVALID)
    assert m.lib.pg_last_error(m.h).decode() == WHO + "path 0, set 1 has 257 knots, more than Lmax_out = 256"
    rev, srev, Lrev, _ = raw_refine(m, *cases.packed(reversed(range(NP)), reversed(range(NS))))
    for p in range(NP):
        for q in range(NS):
            a, b = (NP - 1 - p) * NS + (NS - 1 - q), p * NS + q
            assert rev[a].tobytes() == out[b].tobytes() and bytes(srev[a]) == bytes(st[b]) and Lrev[a] == Lo[b], (p, q)
    big, sbig, Lbig, _ = raw_refine(m, *cases.packed([1, 0, 1], Lmax=777), Lmax_out=1301)      # a larger Lmax and Lmax_out, one source given twice
    for q in range(NS):
        for a, b in ((q, NS + q), (NS + q, q), (2 * NS + q, NS + q)):
            assert np.ascontiguousarray(big[a][:, :cases.LMAX_OUT]).tobytes() == out[b].tobytes() and np.all(big[a][:, cases.LMAX_OUT:] == 0.0), (a, b)
            assert bytes(sbig[a]) == bytes(st[b]) and Lbig[a] == Lo[b], (a, b)
    # the Python method returns the same tubes and stats, and sizes the output itself
    V = pkg.vehicles
    sets = [V.refine(ds=S["ds"], windows=[w for w in S["windows"] if w[0] < math.inf]) for S in cases.sets()]
    src = [m.tubes_from_channels(np.array(cases.sources()[p:p + 1]), [cases.N_KNOTS[p]])[0] for p in range(NP)]
    tubes, stats = m.refine_paths(src, sets, closed=cases.CLOSED)
    assert [len(t) for t in tubes] == list(Lo)
    for k, t in enumerate(tubes):
        n = int(Lo[k])
        assert t.E.tobytes() == out[k, 4, :n].tobytes() and t.s.tobytes() == out[k, 1, :n].tobytes() and t.t.tobytes() == out[k, 0, :n].tobytes(), k
    assert stats.tobytes() == bytes(st)
    m.close()


def test_install_equals_set_trajectories_with_the_returned_channels(pkg, made):
    out, st, Lo, co = made
    a, b = handle(pkg), handle(pkg)
    raw_refine(a, *cases.packed(), install=True)
    k = 1 * NS + 1                                                  # the starts lie on the oval cut by ds = 0.25 m (2 .. 20 m)
    tube = a.tubes_from_channels(out[k:k + 1], [Lo[k]])[0]
    install_equals_set_trajectories(pkg, a, b, out, Lo, cases.LMAX_OUT, np.full(5, k, dtype=np.int32), tube)
    a.close(); b.close()


def test_the_chain_refine_offset_install_on_the_short_lane_change(pkg):
    """The host test's outcome on the device: the 1.5 m change over 5 m is 0.127 m short on the line's own knots and 8.3e-11 m after refine_for(set, knots=10)
    (tests/test_path_refine_host.py); the offset of the refined path is installed from the device buffer and drives one step."""
    m = handle(pkg)
    V = pkg.vehicles
    line = m.tubes_from_channels(cases.documented_line()[None], [40])
    lane = V.lane_change(0.0, 1.5, 212.0, 217.0)
    exact = cases.trapezoid_length(1.5, 212.0, 217.0, 390.0)
    _, coarse = m.offset_paths(line, [lane])
    fine, rst = m.refine_paths(line, V.refine_for(lane, knots=10))
    assert len(fine[0]) == 59 and rst["m_max"][0] == 20 and rst["n_added"][0] == 19 and rst["length"][0] == 390.0
    lanes, ost = m.offset_paths(fine, [lane], install=True)
    err = abs(coarse["length"][0] - exact), abs(ost["length"][0] - exact)
    print(f"length error: {err[0]:.3e} m on the source, {err[1]:.3e} m refined")
    assert abs(err[0] - 0.127) < 1e-3 and err[1] <= 2 * 8.254e-11
    assert m.trajectories[0] is lanes[0] and len(lanes[0]) == 59
    t = lanes[0]
    at = np.array([5, 20])                                          # 50 m and 200 m: before the window
    state = np.stack([t.E[at], t.N[at], t.psi[at], t.V[at], np.zeros(2), t.V[at] * t.kappa[at]], axis=1)
    m.set_inputs(state, np.zeros((2, 3)), t.t[at], time_offset=np.zeros(2))
    m.simulate_(1, dt=0.01)
    assert np.all(pkg.is_solved(m.solve_info()[0]))
    m.close()


def test_the_chain_refine_clip_on_the_disc_between_two_knots(pkg):
    """The host test's outcome on the device: the disc of tests/tube_clip_cases.py between the line's knots at 210 and 220 m comes back side = 0; on the path refined by
    refine_around it is seen, a side is decided, and the pass-by proposed from the report clears it."""
    m = handle(pkg)
    V = pkg.vehicles
    line = m.tubes_from_channels(cases.documented_line()[None], [40])
    disc = V.obstacle(*tube_clip_cases.obstacles()[8])
    oset = V.obstacle_set([disc])
    _, st0, rep0 = m.clip_tubes(line, [oset])
    assert rep0[0, 0]["side"] == 0 and st0["n_ignored"][0] == 1
    fine, rst = m.refine_paths(line, V.refine_around(rep0[0, 0], line[0], 0.5, 2.0, radius=1.5))
    assert rst["m_max"][0] == 20 and rst["ds_min"][0] == 0.5
    clipped, st1, rep1 = m.clip_tubes(fine, [oset])
    r = rep1[0, 0]
    assert r["side"] != 0 and st1["n_seen"][0] == 1 and r["k_last"] - r["k_first"] >= 4 and st1["n_clip_L"][0] + st1["n_clip_R"][0] >= 5
    by = V.pass_by_around(r, fine[0], 10.0)
    assert abs(by["d1"] - r["a_at"]) > 1.5 and -4.0 < by["d1"] < 4.0
    lanes, ost = m.offset_paths(clipped, [by])
    assert ost["n_outside"][0] == 0                                 # the pass-by stays inside the clipped tube
    m.close()


def test_every_refusal_has_its_whole_text_and_leaves_the_installed_library_alone(pkg):
    m = handle(pkg)
    before = step_bits(m, pkg)
    nan, inf = math.nan, math.inf

    def call(n_path=None, n_sets=NS, Lmax=cases.LMAX, Lmax_out=cases.LMAX_OUT, L=None, closed=None, knot=None, sset=None, null=None, paths=range(NP)):
        """the shared case with one edit: L = (path, value), closed = (path, value), knot = (path, channel, knot, value), sset = (set, field, slot or None, value)"""
        Lk, cl, ch, sets = cases.packed(paths)
        n_path = len(Lk) if n_path is None else n_path
        if L:
            Lk[L[0]] = L[1]
        if closed:
            cl[closed[0]] = closed[1]
        if knot:
            ch[knot[0], knot[1], knot[2]] = knot[3]
        for e in ([sset] if isinstance(sset, tuple) else sset or []):
            if e[2] is None:
                setattr(sets[e[0]], e[1], e[3])
            else:
                getattr(sets[e[0]], e[1])[e[2]] = e[3]
        arg = dict(L=Lk.ctypes.data_as(c_i32p), ch=ch.ctypes.data_as(c_dp), sets=sets)
        if null:
            arg[null] = None
        return m.lib.pg_refine_paths(m.h, n_path, Lmax, arg["L"], cl.ctypes.data_as(c_i32p), arg["ch"], n_sets, arg["sets"], Lmax_out, 1, None, None, None, None)

    big = 2**31 - 1
    NULL, NEED = "null argument", "need n_path >= 1, n_sets >= 1 and Lmax >= 2"
    LENGTH, FINITE, RISING = "every path needs 2 <= L[k] <= Lmax", "a geometry value of a valid knot is not finite", "s must increase strictly over the valid knots"
    WINDOW, SPACING = "a window of a set needs a finite s_hi > s_lo", "a window of a set needs a finite ds_w > 0"
    DS, S_LO, UNUSED = "ds of a set is +Inf or finite and > 0", "s_lo of a window is finite or +Inf", "s_hi or ds_w of an unused window is NaN"
    refused = {
        "null L": (dict(null="L"), NULL), "null channels": (dict(null="ch"), NULL), "null sets": (dict(null="sets"), NULL),
        "n_path 0": (dict(n_path=0), NEED), "n_sets 0": (dict(n_sets=0), NEED), "Lmax 1": (dict(Lmax=1), NEED), "Lmax_out 1": (dict(Lmax_out=1), "need Lmax_out >= 2"),
        "L 1": (dict(L=(2, 1)), LENGTH), "L above Lmax": (dict(L=(0, 259)), LENGTH), "closed with 2 knots": (dict(closed=(2, 1)), "a closed path needs >= 3 knots"),
        "s equal": (dict(knot=(0, 1, 7, 3.0)), RISING), "s decreasing": (dict(knot=(1, 1, 3, 0.5)), RISING), "s nan": (dict(knot=(0, 1, 3, nan)), FINITE),
        "E inf": (dict(knot=(1, 4, 0, inf)), FINITE), "N nan": (dict(knot=(2, 5, 1, nan)), FINITE), "psi nan": (dict(knot=(0, 6, 100, nan)), FINITE),
        "kappa inf": (dict(knot=(0, 7, 257, -inf)), FINITE), "edge_L nan": (dict(knot=(1, 8, 27, nan)), FINITE), "edge_R inf": (dict(knot=(2, 9, 1, inf)), FINITE),
        "V zero": (dict(knot=(0, 2, 39, 0.0)), "V of a valid knot is not finite and > 0"), "V nan": (dict(knot=(1, 2, 0, nan)), "V of a valid knot is not finite and > 0"),
        "t_0 inf": (dict(knot=(1, 0, 0, inf)), "t of a valid knot is not finite"), "t nan inside": (dict(knot=(0, 0, 200, nan)), "t of a valid knot is not finite"),
        "ds 0": (dict(sset=(1, "ds", None, 0.0)), DS), "ds -1": (dict(sset=(0, "ds", None, -1.0)), DS), "ds nan": (dict(sset=(4, "ds", None, nan)), DS),
        "ds -inf": (dict(sset=(4, "ds", None, -inf)), DS),
        "s_lo nan": (dict(sset=(2, "s_lo", 0, nan)), S_LO), "s_lo -inf": (dict(sset=(2, "s_lo", 0, -inf)), S_LO),
        "s_hi = s_lo": (dict(sset=(2, "s_hi", 0, 10.1)), WINDOW), "s_hi < s_lo": (dict(sset=(3, "s_hi", 1, 24.0)), WINDOW), "s_hi inf": (dict(sset=(3, "s_hi", 0, inf)), WINDOW),
        "s_hi nan": (dict(sset=(3, "s_hi", 0, nan)), WINDOW),
        "ds_w 0": (dict(sset=(2, "ds_w", 0, 0.0)), SPACING), "ds_w -1": (dict(sset=(3, "ds_w", 1, -1.0)), SPACING), "ds_w inf": (dict(sset=(3, "ds_w", 0, inf)), SPACING),
        "ds_w nan": (dict(sset=(4, "ds_w", 0, nan)), SPACING),
        "s_hi nan in an unused slot": (dict(sset=(0, "s_hi", 3, nan)), UNUSED), "ds_w nan in an unused slot": (dict(sset=(2, "ds_w", 2, nan)), UNUSED),
        "reserved": (dict(sset=(3, "reserved", 1, 1.0)), "reserved of a set must be 0"),
        # the pairs: 4097 parts (the line of 64 m alone under 64 / 4097 m), and one knot too many for Lmax_out
        "an interval of 4097 parts": (dict(paths=[2], sset=(1, "ds", None, 64.0 / 4097.0)), "path 0, set 1, interval 0 would be cut into more than 4096 parts"),
        "more knots than Lmax_out": (dict(Lmax_out=832), "path 1, set 1 has 833 knots, more than Lmax_out = 832"),
        "too many elements": (dict(n_path=big, n_sets=1, Lmax=big), "n_path * n_sets * 10 * Lmax elements are more than the allocation arithmetic holds"),
        "too many output elements": (dict(n_path=big, n_sets=1, Lmax_out=big), "n_path * n_sets * 10 * Lmax elements are more than the allocation arithmetic holds"),
        "n_path * n_sets past 31 bits": (dict(n_path=big, n_sets=big), "n_path * n_sets must fit 31 bits"),
    }
    assert call() == OK                                             # the unedited call is accepted (and installs: put the first library back)
    m.set_trajectory(pkg.load_path_fixture("skidpadoval"))
    assert step_bits(m, pkg) == before
    for name, (kw, text) in refused.items():
        assert call(**kw) == INVALID, name
        assert m.lib.pg_last_error(m.h).decode() == WHO + text, name
        assert step_bits(m, pkg) == before, name
    # 4096 parts are accepted: the line alone under 64 / 4096 m
    Lk, cl, ch, sets = cases.packed([2], [1])
    sets[0].ds = 64.0 / 4096.0
    _, st, Lo, _ = raw_refine(m, Lk, cl, ch, sets, Lmax_out=4097)
    assert Lo[0] == 4097 and st[0].m_max == 4096 and st[0].ds_min == st[0].ds_max == 64.0 / 4096.0
    assert step_bits(m, pkg) == before
    m.close()
    # after the launch: knots so close that s does not increase as a float holds it.  The line with its s counted from 2^20 m (a float carries 0.125 m there; the source's
    # own 64 m survive) cut into 2048 parts of 0.03125 m; the fp64 library accepts the same call
    f = handle(pkg, "f32")
    before32 = step_bits(f, pkg)
    for h, want in ((f, INVALID), (handle(pkg), OK)):
        Lk, cl, ch, sets = cases.packed([2], [1])
        ch[0, 1, :2] += 2.0 ** 20
        sets[0].ds = 0.03125
        raw_refine(h, Lk, cl, ch, sets, Lmax_out=2049, install=True, want=want)
        if h is not f:
            h.close()
    assert f.lib.pg_last_error(f.h).decode() == WHO + "path 0, set 0: the refined knots are so dense that s does not increase strictly in the library's element type (ds_min 0.031250)"
    assert step_bits(f, pkg) == before32
    f.close()
