"""CPU tests of the control-parameter library (pg_set_control_param_sets and its companions, include/pigeon_mpc.h): header, export map, ctypes prototypes, the packing of
dicts and structures in the Python mirror, the Julia binding, and the no-library state pg_create leaves in DevCfg."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ("pg_set_control_param_sets", "pg_set_control_param_index", "pg_clear_control_param_sets", "pg_get_control_param_sets")
CSRC = os.path.join(ROOT, "pigeon.jl_amd", "csrc")


def test_header_declares_and_export_map_lists_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "pigeon_mpc.h")).read()
    for name in NEW:
        assert f"int {name}(pg_handle* h" in txt, name
    assert "one\n * set of control parameters, one reference trajectory" not in txt          # the opening paragraph no longer promises ONE set per batch
    ver = open(os.path.join(CSRC, "pg_exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", ver)
    assert pats and all(any(re.fullmatch(p.strip().replace("*", ".*"), name) for p in pats) for name in NEW)
    api = open(os.path.join(CSRC, "pg_api.hip")).read()
    for name in NEW:
        assert re.search(rf"^int {name}\(pg_handle\* h", api, re.M), name


def test_ctypes_prototypes(pkg):
    from pigeon_jl_amd import _lib
    assert set(_lib.CONTROL_PARAM_SET_PROTOTYPES) == set(NEW)
    for name in NEW:
        assert name in pkg.SYMBOLS
    assert _lib.CONTROL_PARAM_SET_PROTOTYPES["pg_set_control_param_sets"][2] == C.POINTER(_lib.pg_control_params)
    lib = pkg.load_library("f64")
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.CONTROL_PARAM_SET_PROTOTYPES[name], name


def test_dicts_and_structures_pack_into_the_same_bytes(pkg):
    from pigeon_jl_amd import _lib
    lib = pkg.load_library("f64")
    cfg = _lib.pg_config(); lib.pg_default_config(C.byref(cfg))
    fake = pkg.BatchedTrajectoryTrackingMPC.__new__(pkg.BatchedTrajectoryTrackingMPC)      # no handle, no GPU: only the packing is exercised
    fake.cfg = cfg; fake.h = None
    d = dict(pkg.CoupledControlParams()); d["Q_e"] = 4.0; d["deltadot_max"] = 0.2
    st = _lib.pg_control_params()
    for name, _ in _lib.pg_control_params._fields_:
        if name != "_pad":
            setattr(st, name, int(d[name]) if name == "N_HJI" else float(d[name]))
    a = fake.pack_control_params([d, st, {"Q_e": 4.0, "deltadot_max": 0.2}])               # full dict, structure, partial dict over the handle's own set
    raw = [bytes(C.string_at(C.byref(a[k]), C.sizeof(_lib.pg_control_params))) for k in range(3)]
    assert raw[0] == raw[1] == raw[2]
    assert a[0].Q_e == 4.0 and a[0].N_HJI == cfg.control.N_HJI and a[0].V_max == cfg.control.V_max


def test_julia_binding_names_the_entry_points():
    txt = open(os.path.join(ROOT, "julia", "PigeonMI355X.jl")).read()
    for name in NEW:
        assert f":{name}" in txt, name


def test_pg_create_leaves_the_no_library_state():
    api = open(os.path.join(CSRC, "pg_api.hip")).read()
    create = api[api.index("int pg_create(const pg_config* cfg"):api.index("int pg_destroy(")]
    assert "C.cp_sets = nullptr; C.cp_idx = nullptr; C.n_cp = 0; C.cp_epoch = 0;" in create
    ker = open(os.path.join(CSRC, "pg_kernels.hip")).read()
    cfg = ker[ker.index("struct DevCfg {"):ker.index("PG_DEV TrajView traj_of")]
    for field in ("const DevControlRec* cp_sets;", "const int* cp_idx;", "int n_cp;", "DevControl cp;"):
        assert field in cfg, field
    # every kernel read goes through the view: behind the accessor block (ControlView, the seeding gains, PG_CP -- the macro closes it) no direct read of the uniform set
    # is left (N_HJI is structure)
    body = ker[ker.index("#define PG_CP("):]
    lat = open(os.path.join(CSRC, "pg_solve_lat.hip")).read()
    for src in (body.split("\n", 1)[1], lat):
        for m in re.finditer(r"C\.cp\.(\w+)|C\.ux_dummy", src):
            assert m.group(1) in ("N_HJI", "deltadot_max"), m.group(0)          # deltadot_max: the uniform value k_nodes_linearize writes, rewritten by k_rate_limits
