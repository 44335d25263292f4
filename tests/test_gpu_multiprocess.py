"""Multi-process GPU tests (BASELINE configs[3]): launch -> shard -> REAL step on the GPU -> gather, end to end.

An 8-GPU node is not available to the test tier, so the ranks share the GPU(s) present and the gather runs over gloo (RCCL refuses two ranks on one
device); everything else is the product path: one process per rank, `shard_range` partition, pg_step_dev on device-resident inputs, gather of the controls."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(nproc, script_args, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + script_args
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("B,precision", [(1024, "f64"), (1001, "f64"), (400, "f64"), (2048, "f64"), (1024, "f32")])      # (400 = 2 x 200, 1024 = 2 x 512, 2048 = 2 x 1024: shards and whole batch use different lane splits of k_linearize -- 8, 4, 2 lanes per interval, and 1 for the whole 2048)
def test_two_ranks_step_their_shards_and_gather(pkg, skidpad, tmp_path, B, precision):
    """Both ranks run the real pg_step_dev on their shard; the gathered controls are BIT-identical to one process stepping the whole batch
    (instances are independent: nothing in the path depends on the batch an instance sits in)."""
    out = str(tmp_path / "gathered.npz")
    r = _launch(2, [os.path.join(ROOT, "tests", "_mp_gpu_worker.py"), out, str(B), precision])
    assert r.returncode == 0, r.stderr[-2000:]
    G = np.load(out)
    assert int(G["all_solved"]) == 1
    state, control, t0, toff = pkg.synthetic.config2_inputs(skidpad, B, seed=2024)
    real = np.float64 if precision == "f64" else np.float32
    mpc = pkg.BatchedTrajectoryTrackingMPC(skidpad, B, precision=precision)
    u, st, _ = mpc.step_(state.astype(real), control.astype(real), t0, time_offset=toff)
    assert np.all(st == pkg.SOLVED)
    assert G["u"].shape == (B, 3)
    assert np.array_equal(G["u"].astype(np.float64), u), float(np.max(np.abs(G["u"] - u)))
    mpc.close()


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` started as a plain process spawns its two ranks itself (before touching the GPU) and rank 0 prints ONE JSON line with
    n_gpus = 2 and the whole-job rate (here in the gloo test mode, ranks sharing the GPU)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--batch", "512",
                        "--no-cpu-baseline", "--no-hji", "--no-decoupled", "--no-f32", "--full-record", os.devnull], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["solved"] == "512/512"
    assert d["gather_ok"] is True
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * 512) < 1e-3 * 2 * 512          # value = all ranks' solves / max-over-ranks time


def test_config4_workload_line_over_two_ranks():
    """BASELINE configs[3] through the bench's own launcher in its test mode: fp32, 8192 instances per rank, two ranks (gloo: both on the GPU present).  The line names
    that configuration, carries the whole-job rate over the max-over-ranks time and the per-rank times, and -- a scaling run being the timed loop, the gather check and
    one JSON line -- none of the secondary objects rank 0 would otherwise build while the other ranks wait."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--batch", "8192",
                        "--precision", "f32", "--full", "--full-record", os.devnull], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dtype"] == "f32" and d["ranks"] == 2 and d["collective"] == "gloo" and d["gather_ok"] is True
    assert d["config"]["workload"].startswith("configs[3]: Batch=16384 coupled MPC, N=30, fp32, sharded 8192/GPU x2")
    assert d["solved"] == "8192/8192"
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * 8192) < 1e-3 * 2 * 8192
    assert d["per_rank_ms_per_step"]["min"] <= d["per_rank_ms_per_step"]["max"] == pytest.approx(d["ms_per_step"], rel=1e-4)
    for k in ("closed_loop_rollout", "hji_lookup", "decoupled_n50", "fp32", "cpu_baseline", "interior_point_only", "two_half_batches_on_two_streams"):
        assert k not in d, k


def test_rccl_gather_when_two_gpus_are_present():
    """The product's collective: RCCL all_gather of the controls (backend nccl), one rank per GPU.  Runs wherever at least two GPUs are visible (the 1-GPU test box skips)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "nccl", "--steps", "3", "--warmup", "1", "--batch", "1024"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["collective"] == "rccl" and d["ranks"] == 2 and d["gather_ok"] is True and d["solved"] == "1024/1024"


def test_bench_scaling_line_over_four_ranks_is_compact():
    """The scaling run the driver does at round end (`bench.py --gpus N`), rehearsed through the bench's own launcher with as many ranks as the GPU box lets one card
    carry (its process guard allows 6 GPU processes: this test process + 4 ranks; the 8-rank shard / gather logic runs in tests/test_distributed_gloo.py on the CPU).
    The LAST stdout line is the compact record: strict JSON within 4 KB with the contract keys, `ranks`, `collective` and `per_rank_ms_per_step`."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--batch", "512",
                        "--precision", "f32", "--full", "--full-record", os.devnull], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) <= 4096

    def bad(c):
        raise ValueError(c)
    d = json.loads(last, parse_constant=bad)
    assert d["n_gpus"] == 4 and d["ranks"] == 4 and d["collective"] == "gloo" and d["gather_ok"] is True and d["solved"] == "512/512" and d["dtype"] == "f32"
    assert d["per_rank_ms_per_step"]["min"] <= d["per_rank_ms_per_step"]["max"] == pytest.approx(d["ms_per_step"], rel=1e-4)
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 4 * 512) < 1e-3 * 4 * 512
    for k in ("metric", "unit", "config", "roofline", "scaling", "vs_baseline", "data", "higher_is_better"):
        assert k in d, k
    assert "cpu_baseline" not in d
