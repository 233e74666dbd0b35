"""The driver contract: bench.py emits one valid JSON line, and the
torchrun multi-rank path (the exact launch the driver uses for SCALE_rNN,
gloo here instead of RCCL) works end-to-end."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
TINY = ["--steps", "2", "--warmup", "1", "--rollout-length", "8",
        "--batch-size", "8", "--envs-per-actor", "4", "--num-actors", "2",
        "--device", "cpu", "--dtype", "fp32"]


def _parse_last_json(stdout: str) -> dict:
    for line in reversed(stdout.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{stdout}")


def test_bench_single_rank_json_contract():
    r = subprocess.run([sys.executable, BENCH] + TINY, capture_output=True,
                       text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _parse_last_json(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in j, key
    assert j["value"] > 0
    assert j["scaling"] == "weak"
    assert j["config"]["parallelism"] == "dp1"


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float32 .npy
    (at most 64 MB in all), identically from run to run; the diagnostics
    report appears only with --full."""
    import numpy as np

    def run(out_dir, *extra):
        r = subprocess.run(
            [sys.executable, BENCH] + TINY + ["--dump-outputs", str(out_dir)]
            + list(extra), capture_output=True, text=True, timeout=600,
            cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        j = _parse_last_json(r.stdout)
        assert j["steps"] == 2 and j["ms_per_step"] > 0
        return r, {f: np.load(os.path.join(out_dir, f))
                   for f in sorted(os.listdir(out_dir))}

    r1, a = run(tmp_path / "a")
    r2, b = run(tmp_path / "b", "--full")
    assert "[bench] learner timings" not in r1.stderr
    assert "[bench] learner timings" in r2.stderr
    assert set(a) == {"total_loss.npy", "pg_loss.npy", "baseline_loss.npy",
                      "entropy_loss.npy", "flat_grad.npy", "flat_params.npy"}
    assert set(a) == set(b)
    assert sum(x.nbytes for x in a.values()) <= 64 * 1024 * 1024
    for name, x in a.items():
        assert x.dtype == np.float32 and x.size > 0, name
        assert np.isfinite(x).all(), name
        # same seeded inputs, same fp32 CPU math; the tolerance only allows
        # for a different summation order in threaded reductions
        np.testing.assert_allclose(x, b[name], rtol=1e-4, atol=1e-6,
                                   err_msg=name)
    assert np.abs(a["flat_grad.npy"]).max() > 0


def test_tuned_perf_db_is_merged_not_overwritten(tmp_path):
    """The shipped MIOpen perf-db records are added to the user db; a
    record the user db already holds for the same key is kept."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    shipped = sorted(f for f in os.listdir(bench._TUNED_DB_DIR)
                     if f.endswith(".udb.txt"))
    assert shipped
    with open(os.path.join(bench._TUNED_DB_DIR, shipped[0])) as f:
        ours = [ln for ln in f.read().splitlines() if ln]
    assert len(ours) >= 8 and all("=" in ln for ln in ours)

    bench._install_tuned_perf_db(str(tmp_path))
    with open(tmp_path / shipped[0]) as f:
        assert f.read().splitlines() == ours

    key = ours[0].split("=", 1)[0]
    (tmp_path / shipped[0]).write_text(f"{key}=Mine:1\nother=Solver:2\n")
    bench._install_tuned_perf_db(str(tmp_path))
    got = (tmp_path / shipped[0]).read_text().splitlines()
    assert got[:2] == [f"{key}=Mine:1", "other=Solver:2"]
    assert sorted(got[2:]) == sorted(ours[1:])
    bench._install_tuned_perf_db(str(tmp_path))  # idempotent
    assert (tmp_path / shipped[0]).read_text().splitlines() == got


@pytest.mark.timeout(900)
def test_bench_torchrun_two_ranks_cpu():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29617", BENCH] + TINY
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=800,
                       cwd=REPO, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    j = _parse_last_json(r.stdout)
    assert j["config"]["parallelism"] == "dp2"
    # whole-job value: 2 ranks × 2 steps × 8×8 env steps / elapsed
    assert j["value"] > 0


@pytest.mark.timeout(1200)
def test_bench_torchrun_eight_ranks_cpu_dryrun():
    """8-rank process topology dry-run on CPU (tiny shapes): proves the
    torchrun launch, per-rank actor farms, gloo all-reduce and the timed
    loop all come up at the driver's SCALE rank count."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", "29629", BENCH, "--steps", "2", "--warmup", "1",
           "--rollout-length", "8", "--batch-size", "8", "--envs-per-actor",
           "4", "--num-actors", "2", "--device", "cpu", "--dtype", "fp32"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100,
                       cwd=REPO, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    j = _parse_last_json(r.stdout)
    assert j["config"]["parallelism"] == "dp8"
    assert j["n_gpus"] == 0  # CPU dry-run
    assert j["value"] > 0
