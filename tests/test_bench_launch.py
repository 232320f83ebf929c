"""bench.py's launcher (CPU, no GPU work): `--gpus N` starts N rank processes itself when no launcher
did (torchrun's per-rank environment, rendezvous on 127.0.0.1), and refuses a rank count it cannot
honour rather than printing a line whose n_gpus misstates the run. One GPU test: the plain run's line
and `--dump-outputs`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True,
                          text=True, timeout=240)


def test_gpus_2_starts_two_ranks():
    r = _bench(["--gpus", "2", "--check-launch"], LK_BENCH_BACKEND="gloo")
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["spawned"] is True
    assert line["master"].startswith("127.0.0.1:")


def test_gpus_disagreeing_with_world_size_is_refused():
    r = _bench(["--gpus", "2", "--check-launch"], WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2
    assert "WORLD_SIZE" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_outputs(gpu, tmp_path):
    """A plain run is the timed steps alone (every other section is behind --full), and --dump-outputs
    writes each matrix's dst vectors of the last step as float32 [layers, M]."""
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--layers", "2", "--dump-outputs", str(tmp_path / "d")])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(line["config"]["bytes_per_token"] / line["ms_per_step"] / 1e6, rel=1e-2)
    full_only = {"roofline", "decode_chain", "persistent_chain", "multi_gpu_throughput", "headline_q4_0_4096x4096_n1",
                 "n1_configs", "batched", "next_rows", "multi_gpu_world1", "host_path_pcie", "cpu_baseline"}
    assert not full_only & set(line), sorted(full_only & set(line))
    shapes = {"q": 4096, "k": 4096, "v": 4096, "o": 4096, "gate": 11008, "up": 11008, "down": 4096}
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in shapes)
    for name, M in shapes.items():
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == (2, M), (name, a.dtype, a.shape)
        assert np.isfinite(a).all() and (np.abs(a).max(axis=1) > 0).all(), name  # every layer was written


def test_more_gpus_than_visible_is_refused():
    # this container has no GPU: an RCCL run of 2 ranks cannot be honoured, and nothing is spawned
    r = _bench(["--gpus", "2"])
    assert r.returncode == 2
    assert "visible" in r.stderr
