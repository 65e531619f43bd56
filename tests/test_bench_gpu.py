"""bench.py's contract at N > 1 without a launcher.

The driver runs `python3 bench.py --gpus N`: bench.py must form the N ranks
itself (one process per GPU; here two processes share the box's one GPU),
run the 256 MiB fp32 SUM allreduce of the metric
(coll_base_allreduce.c:618-856 under coll/tuned's fixed decision) and print
one JSON line from rank 0 with n_gpus = the ranks formed and parity checked
bit-exact against the oracle (bench.py allreduce_parity).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_gpus_2_without_launcher_runs_the_allreduce():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                           "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup",
                        "1", "--full", "--no-sweep", "--no-cpu-baseline"], capture_output=True, text=True, env=env,
                       timeout=280, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert "MPI_Allreduce fp32 SUM 256 MiB" in d["config"]["workload"], d.get("allreduce_error")
    assert d["parity"] == "ok", d.get("parity")
    assert d["value"] > 0 and d["unit"] == "GB/s"
    for name in ("staged_push", "staged_pull", "zero_copy_gather", "zero_copy"):
        ab = d["config"]["data_path_ab"][name]
        assert ab.get("parity") == "ok", (name, ab)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_its_output(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` times K steps and prints the
    headline fields; the legs beside it (parity, CPU baselines, size-1
    allreduce, pack / unpack, op call cost) need --full.  --dump-outputs
    writes the inout buffer of the last timed step as a float32 sample of at
    most 64 MB."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                           "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup",
                        "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env,
                       timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value is the 3 x 1 GiB of one step over ms_per_step
    assert d["value"] == pytest.approx(3 * (1 << 30) / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    for k in ("parity", "cpu_baseline", "cpu_baseline_allreduce", "allreduce_n1", "pack_unpack",
              "op_reduce_call_us"):
        assert k not in d, k
    files = sorted(os.listdir(tmp_path))
    assert files == ["reduce_local_inout.npy"]
    out = np.load(tmp_path / files[0])
    assert out.dtype == np.float32 and 0 < out.nbytes <= 64 << 20
    # inout = b0 + (W + K) a with a, b0 uniform in (-1, 1): finite, within +-4, not constant
    assert np.isfinite(out).all() and np.abs(out).max() <= 4.0 and out.std() > 0.5


def test_bench_rejects_a_launcher_that_formed_other_ranks():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True,
                       text=True, env=env, timeout=60, cwd=ROOT)
    assert p.returncode == 2
    assert "WORLD_SIZE=2" in p.stdout
