"""Driver-contract tests for bench.py: single-rank CPU fallback JSON and a
torchrun-style world-2 gloo run (the exact invocation shape the round-end
scaling harness uses)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse_last_json(out: str) -> dict:
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, out
    return json.loads(lines[-1])


def _cpu_env() -> dict:
    """Environment for the CPU (gloo) runs: no torchrun variables, and no
    visible GPU, so that they take the CPU path on every machine instead
    of stacking several ranks on one device."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    return env


def test_bench_single_rank_contract():
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _parse_last_json(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["data"] == "synthetic"
    assert j["scaling"] == "weak" and j["higher_is_better"] is True
    assert j["value"] > 0


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's flow as float32 .npy;
    weights and inputs are seeded, so two runs with the same arguments
    (one of them with --full) dump identical arrays on the CPU path.
    --steps sets the number of timed steps and ms_per_step is the time
    of one."""
    import numpy as np
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "0", "--dump-outputs", str(d)] + extra,
            cwd=REPO, capture_output=True, text=True, timeout=600,
            env=_cpu_env())
        assert r.returncode == 0, r.stderr[-2000:]
        j = _parse_last_json(r.stdout)
        assert j["steps"] == 2
        # one frame pair per step: fps * (ms per step) == 1000
        assert abs(j["ms_per_step"] * j["value"] - 1e3) < 1e-3
        assert sorted(p.name for p in d.iterdir()) == ["flow.npy"]
        dumps.append(np.load(d / "flow.npy"))
    a, b = dumps
    assert a.dtype == np.float32 and a.shape == (1, 2, 128, 256)
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a, b)


def test_bench_dump_budget_sampling(tmp_path):
    """An output over its share of the 64 MB budget is stored as a fixed
    seeded sample; small outputs and scalars are stored whole."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
    big = torch.arange(20_000_000, dtype=torch.float32).reshape(4, -1)
    out = {"big": big, "small": torch.ones(3, dtype=torch.bfloat16),
           "loss": 0.5, "dbl": torch.zeros(2, dtype=torch.float64)}
    for name in ("x", "y"):
        bench.dump_outputs(out, str(tmp_path / name))
    x = {p.stem: np.load(p) for p in (tmp_path / "x").iterdir()}
    y = {p.stem: np.load(p) for p in (tmp_path / "y").iterdir()}
    assert sorted(x) == ["big", "dbl", "loss", "small"]
    assert sum(a.nbytes for a in x.values()) <= 64 * 1000 * 1000
    assert x["big"].dtype == np.float32 and x["big"].ndim == 1
    assert x["big"].size == 16_000_000 // 4
    # arange input: each stored value is its own flat index (to float32
    # rounding above 2**24), so the sample is in ascending order
    assert np.all(np.diff(x["big"]) >= 0) and x["big"].max() <= 20_000_000
    assert np.array_equal(x["big"], y["big"])
    assert x["small"].dtype == np.float32 and x["small"].shape == (3,)
    # a Python float is a double and stays one
    assert x["loss"].dtype == np.float64 and float(x["loss"]) == 0.5
    assert x["dbl"].dtype == np.float64


def test_bench_torchrun_world2_gloo():
    """The driver launches N>1 via torch.distributed.run; verify the
    distributed path end to end on CPU (gloo): exactly one JSON line, from
    rank 0, with n_gpus == world size."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29731", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1"],
        cwd=REPO, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    jsons = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(jsons) == 1, jsons
    j = json.loads(jsons[0])
    assert j["n_gpus"] == 2
    assert j["config"]["parallelism"] == "dp2"


def test_bench_torchrun_world4_gloo():
    """The driver's scaling run goes up to 8 ranks; verify nothing in the
    path assumes world <= 2 (4 CPU ranks, short step)."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", "29735", "bench.py", "--gpus", "4",
         "--steps", "1", "--warmup", "0"],
        cwd=REPO, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    jsons = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(jsons) == 1, jsons
    j = json.loads(jsons[0])
    assert j["n_gpus"] == 4
    assert j["config"]["parallelism"] == "dp4"


def test_bench_gpus_flag_self_spawns():
    """`python bench.py --gpus 2` WITHOUT torchrun must spawn the ranks
    itself (r1 verdict: the flag was silently ignored and benched 1 GPU)."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "2",
         "--steps", "1", "--warmup", "0"],
        cwd=REPO, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    jsons = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(jsons) == 1, jsons
    j = json.loads(jsons[0])
    assert j["n_gpus"] == 2
    assert j["config"]["parallelism"] == "dp2"


def test_val_mode_torchrun_world2_gloo():
    """DP-sharded eval: two gloo ranks split the seeds
    and all-reduce the mean EPE; rank 0 prints one JSON result whose mean
    aggregates BOTH ranks' shards (4 local batches each of 8 seeds)."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29741", "infer_raft.py", "-m", "val",
         "--small", "--iters", "1", "--no-graph"],
        cwd=REPO, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    jsons = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(jsons) == 1, jsons
    j = json.loads(jsons[0])
    assert j["world"] == 2
    assert len(j["epe_per_batch"]) == 4      # rank 0's shard of 8 seeds
    assert 0 < j["epe_mean"] < 50


def test_bench_trace_table():
    """--trace-table prints a torch-profiler op table (tracing story,
    SURVEY §5.1) without disturbing the JSON contract line."""
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "1", "--warmup", "0",
         "--trace-table"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    j = _parse_last_json(r.stdout)
    assert j["steps"] == 1
    assert "Self CPU" in r.stderr     # profiler table went to stderr
