"""Build check of the fp32 instantiation (libpigeon_hip_f32.so): no fp64 ARITHMETIC in the device code outside the kernels that own absolute time.

  python tools/check_f32_purity.py [pigeon.jl_amd/csrc/pg_api_f32.s]      (the .s comes from `make -C pigeon.jl_amd/csrc pg_api_f32.s`)

The kernels are written against the scalar type `real`; a stray `double` (or an unwrapped floating literal) would silently promote part of an
expression to fp64 in the fp32 build.  This reads the gfx950 assembly of that build and fails when a kernel issues an fp64 arithmetic
instruction it is not entitled to:
  * every kernel may convert / compare / frexp fp64 values (v_cvt_*, v_cmp_*, v_frexp_*: reading the double time grid, libm's sincosf reduction);
  * the kernels that compute with ABSOLUTE TIME (tdouble: k_time_steps and the k_project<true> instantiation that carries the time grid in the fused launch, the
    warm-branch interpolation weights of k_nodes / k_nodes_warm / k_nodes_recheck, the clock of k_advance, k_advance_safety and k_node_finish and of their library forms, the templates k_advance_lib, k_advance_safety_lib and
    k_node_finish_lib -- each with and without a disturbance; k_speed_plan, which accumulates the time channel of a planned profile in double; k_path_make, which makes a path library in double in
    both builds and rounds on store -- E and N of the recorded tracks sit 300 m from the origin, where a float carries 3e-5 m, psi accumulates over laps, and a library is
    made once per sweep: the fp32 library's paths are exactly the fp64 library's rounded to float; k_path_fit, which fits a path library to waypoints under the same rule
    and for the same reasons; k_path_offset, which offsets a path library into lanes, lane changes and pass-bys under the same rule -- the source is read as the doubles
    given --; k_tube_clip, which narrows the tubes of a path library around obstacle sets under the same rule (the stats and reports are the same doubles in both
    libraries); k_path_refine, which inserts knots into a path library under the same rule; k_wp_smooth, which smooths waypoints, doubles in both libraries: both return the same bits; k_wp_tune, which searches the smoothing weight and smooths under it by the same text; k_line_opt, which moves waypoints along their normals to the least bending energy, doubles in both libraries; k_make_starts, which places a batch on the installed library in double -- draws, the controller's lookup restated in double on the channels as
    held, placement -- and rounds on store; k_route, whose time offset of a switched instance is t0 - (t_proj + t_join) in double -- its
    projection is in the library's element type) may use fp64 arithmetic;
  * everything else (k_solve, k_linearize, k_limits, k_qp_dec, k_project, k_hji_*) must be pure fp32.
Exit status 0 = clean; 1 = violations (listed)."""
import collections
import os
import re
import sys

TIME_KERNELS = ("k_time_steps", "k_nodes", "k_nodes_linearize", "k_nodes_warm", "k_nodes_dec", "k_advance", "k_advance_safety", "k_node_finish", "k_nodes_recheck",
                "k_advance_lib", "k_advance_safety_lib", "k_node_finish_lib", "k_speed_plan", "k_path_make", "k_path_fit", "k_path_offset", "k_tube_clip", "k_path_refine", "k_wp_smooth", "k_wp_tune", "k_line_opt", "k_make_starts", "k_route")
HARMLESS = re.compile(r"^v_(cvt_|cmp_|cmpx_|frexp_)")


def scan(path):
    per = collections.defaultdict(collections.Counter)
    cur = None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        if cur and line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur:
            t = line.split()
            if t and re.match(r"^v_\w*f64", t[0]):
                per[cur][t[0]] += 1
    return per


def kernel_name(mangled):
    m = re.match(r"^_ZN2pg(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1)); s = mangled[len(m.group(0)):]
    return s[:n]


def violations(path):
    bad = {}
    for k, cnt in scan(path).items():
        name = kernel_name(k)
        if name in TIME_KERNELS or "k_projectILb1E" in k:          # k_project<true> hosts the time grid of the fused launch
            continue
        arith = {op: n for op, n in cnt.items() if not HARMLESS.match(op)}
        if arith:
            bad[name] = arith
    return bad


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    p = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "pigeon.jl_amd", "csrc", "pg_api_f32.s")
    bad = violations(p)
    for k, v in bad.items():
        print(f"fp64 arithmetic in the fp32 build of {k}: {v}")
    print("fp32 purity:", "FAILED" if bad else "ok")
    sys.exit(1 if bad else 0)
