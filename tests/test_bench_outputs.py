"""bench.py's plain run and `--dump-outputs DIR`: what the last timed step computed, written as .npy files (float32 / float64, at most 64 MB in all)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_dump_outputs_types_and_size_cap(tmp_path):
    import bench
    rng = np.random.default_rng(0)
    arrays = {"controls": rng.random((4096, 3)).astype(np.float32), "status": np.arange(4096, dtype=np.int32), "solution_x": rng.random((4096, 31, 8))}
    bench.dump_outputs(str(tmp_path / "small"), arrays)
    assert sorted(os.listdir(tmp_path / "small")) == ["controls.npy", "solution_x.npy", "status.npy"]
    assert np.load(tmp_path / "small" / "controls.npy").dtype == np.float32 and np.array_equal(np.load(tmp_path / "small" / "controls.npy"), arrays["controls"])
    st = np.load(tmp_path / "small" / "status.npy")
    assert st.dtype == np.float64 and np.array_equal(st, np.arange(4096))
    # above the cap: every array keeps the same seeded sample of its rows, and the row indices go beside it; two runs write the same files
    big = dict(arrays, solution_x=rng.random((4096, 31, 80)))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, limit=20 << 20)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "solution_x_rows.npy" in files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 20 << 20
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    rows = np.load(tmp_path / "a" / "solution_x_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "solution_x.npy"), big["solution_x"][rows])
    assert np.array_equal(np.load(tmp_path / "a" / "controls.npy"), big["controls"][np.load(tmp_path / "a" / "controls_rows.npy").astype(np.int64)])


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_its_last_step_computed(pkg, skidpad, tmp_path):
    """A plain run times exactly --steps steps and builds nothing else; the dumped controls and status are those of the same seeded batch stepped directly."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "512", "--dump-outputs", str(out),
                        "--full-record", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["timing"]["repeats"] == 1 and d["ms_per_step"] > 0 and d["solved"] == "512/512"
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 512) < 1e-3 * 512
    for k in ("cpu_baseline", "phase_ms_short", "secondary"):
        assert not d.get(k), k
    assert sorted(os.listdir(out)) == ["controls.npy", "ipm_iters.npy", "solution_x.npy", "status.npy"]
    u = np.load(out / "controls.npy"); st = np.load(out / "status.npy"); x = np.load(out / "solution_x.npy")
    assert u.dtype == np.float64 and u.shape == (512, 3) and st.shape == (512,) and x.shape[0] == 512
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, 512, seed=12345, traj_mode=True)
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, 512, phase_timing=False)
    u_ref, st_ref, _ = mpc.step_(state, control, t0, time_offset=toff)
    mpc.close()
    assert np.array_equal(st, st_ref.astype(np.float64))
    np.testing.assert_allclose(u, u_ref, rtol=1e-9, atol=1e-9 * max(1.0, float(np.max(np.abs(u_ref)))))
