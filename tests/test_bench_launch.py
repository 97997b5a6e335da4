"""CPU: bench.py's multi-GPU launcher. `--gpus N` without torch.distributed.run
spawns N ranks itself (no GPU is touched in --dry-run) and reports n_gpus: N;
a rank count that disagrees with --gpus fails loudly. And the plain run:
what it prints and what --dump-outputs writes (the one GPU test here)."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e,
                          capture_output=True, text=True, timeout=300)


def test_gpus2_spawns_two_ranks():
    r = _run(["--gpus", "2", "--dry-run"])
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    assert lines[0]["n_gpus"] == 2 and lines[0]["dry_run"] and lines[0]["parity"]
    assert lines[0]["records_total"] == 2 * (1 << 20)
    assert lines[0]["torch_free_ranks"]  # no rank process imported torch


def test_torch_distributed_run_launcher():
    """The driver's N>1 launch: python -m torch.distributed.run ... bench.py
    --gpus 2 (the ranks come from the environment; the control channel keys its
    rendezvous on the agent's pid and MASTER_PORT)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BDLS_CTRL_DIR"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                        str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run",
                        "--config", "5"], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 2 and out["records_total"] == 1 << 26 and out["torch_free_ranks"]


def test_config5_is_one_batch_split_over_ranks():
    r = _run(["--gpus", "2", "--dry-run", "--config", "5"])
    assert r.returncode == 0, r.stderr
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["records_total"] == 1 << 26


def test_dump_outputs_files(tmp_path):
    """--dump-outputs writes float32 valid / reason arrays; outputs past 64 MB
    are cut to the same seeded sample of records on every call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    reason = (np.arange(1000) % 7 == 0).astype(np.uint8) * 3
    bench.dump_outputs(str(tmp_path / "small"), 0, reason == 0, reason)
    v, r = (np.load(tmp_path / "small" / f) for f in ("valid.npy", "reason.npy"))
    assert v.dtype == r.dtype == np.float32
    assert (r == reason).all() and (v == (reason == 0)).all()
    bench.dump_outputs(str(tmp_path / "small"), 2, reason == 0, reason)
    assert (np.load(tmp_path / "small" / "reason.rank2.npy") == reason).all()
    n = bench.DUMP_MAX_BYTES // 8 + 1  # one record too many for both arrays whole
    reason = (np.arange(n) % 251).astype(np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, reason == 0, reason)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["reason.npy", "sample_index.npy", "valid.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_MAX_BYTES
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and (np.diff(idx) > 0).all() and idx[-1] < n
    assert (np.load(tmp_path / "a" / "reason.npy") == reason[idx.astype(np.int64)]).all()
    for f in files:
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone(tmp_path):
    """A run without --full: --steps timed resident passes, the headline
    fields and nothing of --full's on the line, and --dump-outputs holding the
    last step's verdicts -- those of the seeded batch, the same on every run."""
    import numpy as np
    from bdls_amd import workload
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "40000", "--nkeys", "2000"]
    outs = []
    for d in ("a", "b"):
        r = _run(args + ["--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0]))
    out = outs[0]
    assert out["steps"] == 2 and out["warmup"] == 1 and out["parity"] is True
    assert out["unit"] == "verifies/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert out["ms_per_step"] > 0
    # value = records / the time of one step (ms_per_step is rounded to 1 us)
    assert abs(out["value"] * out["ms_per_step"] / 1e3 / 40000 - 1) <= 0.0006 / out["ms_per_step"]
    assert "2 timed passes" in r.stderr
    for k in ("host_path", "host_path_e2e", "roofline", "cpu_baseline", "side_configs",
              "kernel_ms_per_step"):
        assert k not in out
    want = workload.generate(40000, 2000, 256, 16, seed=2).reason
    for d in ("a", "b"):
        reason = np.load(tmp_path / d / "reason.npy")
        valid = np.load(tmp_path / d / "valid.npy")
        assert reason.dtype == valid.dtype == np.float32
        assert (reason == want).all() and (valid == (want == 0)).all()


def test_world_mismatch_fails():
    r = _run(["--gpus", "2", "--dry-run"], env={"WORLD_SIZE": "1", "RANK": "0",
                                                "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr
