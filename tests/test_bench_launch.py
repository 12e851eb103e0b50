"""bench.py --gpus N (BASELINE.json metric "1/2/4/8 MI355X"): without
WORLD_SIZE the bench starts N ranks itself (torch.distributed.run on
127.0.0.1) before touching the GPU; with WORLD_SIZE set it must equal N.
CPU only: the launched ranks stop before any GPU work (--ranks-check)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_launch_plan():
    assert bench.launch_plan(1, {}) == "inproc"
    assert bench.launch_plan(2, {}) == "spawn"
    assert bench.launch_plan(8, {}) == "spawn"
    assert bench.launch_plan(2, {"WORLD_SIZE": "2"}) == "inproc"
    assert bench.launch_plan(1, {"WORLD_SIZE": "1"}) == "inproc"
    assert bench.launch_plan(8, {"WORLD_SIZE": "1"}).startswith("error")
    assert bench.launch_plan(1, {"WORLD_SIZE": "4"}).startswith("error")


def test_rank_command():
    cmd = bench.rank_command(4, ["--gpus", "4", "--steps", "3"], 29500)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-port=29500" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True,
                          timeout=240, env=env, cwd=str(ROOT))


def test_gpus_2_starts_two_ranks():
    r = _run(["--gpus", "2", "--ranks-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert sorted(l["rank"] for l in lines) == [0, 1]
    assert all(l["world"] == 2 and l["gpus"] == 2 for l in lines)


def test_world_mismatch_exits_nonzero():
    r = _run(["--gpus", "8", "--ranks-check"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr


@pytest.mark.parametrize("gpus", [1])
def test_single_gpu_runs_in_process(gpus):
    r = _run(["--gpus", str(gpus), "--ranks-check"])
    assert r.returncode == 0
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"rank": 0, "world": 1, "gpus": 1}


def test_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: D as float32, I as float64 (ids exact below 2^53)."""
    import numpy as np
    D = np.arange(12, dtype=np.float32).reshape(3, 4) / 64
    I = np.array([[0, 1, 2**31 + 5, -1]] * 3, dtype=np.int64)
    out = tmp_path / "sub" / "dump"
    bench.dump_outputs(out, D, I)
    assert sorted(p.name for p in out.iterdir()) == ["D.npy", "I.npy"]
    Dd, Id = np.load(out / "D.npy"), np.load(out / "I.npy")
    assert Dd.dtype == np.float32 and (Dd == D).all()
    assert Id.dtype == np.float64 and (Id.astype(np.int64) == I).all()


def test_steps_must_be_positive():
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


SIDE_LEGS = ("pcie_inclusive", "latency_nq1", "latency_nq1_f32", "cpu_baseline", "recall_at_10")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """A plain run on a small fp32 index: the line carries the headline fields,
    --steps is the number of timed steps, none of the --full legs ran, and
    the dumped D / I are the exact top-k of the same synthetic workload."""
    import numpy as np
    from oracle import cpu as C
    rows, d, nq, k = 20_000, 384, 64, 10
    r = _run(["--gpus", "1", "--config", "b", "--rows", str(rows), "--nq", str(nq), "--steps", "3", "--warmup", "1",
              "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["roofline"]["launches"] == 3
    assert line["metric"] == bench.METRIC and line["unit"] == "queries/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert abs(line["value"] - nq / (line["ms_per_step"] / 1e3)) <= 0.01 * line["value"]
    assert not [leg for leg in SIDE_LEGS if leg in line]
    D, I = np.load(tmp_path / "D.npy"), np.load(tmp_path / "I.npy")
    assert D.dtype == np.float32 and I.dtype == np.float64 and D.shape == I.shape == (nq, k)
    Dr, Ir = C.knn_exact_synth(bench.CORPUS_SEED, rows, d, C.synth(bench.QUERY_SEED, 0, nq, d), k)
    assert (I.astype(np.int64) == Ir).all()
    assert (np.abs(D - Dr) <= 1e-5 * np.maximum(1.0, np.abs(Dr))).all()
