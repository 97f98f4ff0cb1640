"""bench.py's multi-rank contract on the CPU (gloo, tiny models): launched the way the driver launches N > 1
(``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N``),
every rank runs its own engine and index shard, queries search every shard, and rank 0 prints ONE JSON line
with the whole-job value, n_gpus = N, dp parallelism and the global batch (max step time over ranks)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(600)
def test_bench_torchrun_two_ranks_tiny():
    n, batch, steps = 2, 3, 1
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", str(n), "--steps", str(steps), "--warmup", "0", "--model", "tiny", "--embedder", "tiny",
           "--index-size", "1500", "--batch", str(batch), "--max-tokens", "6", "--chunk-tokens", "48",
           "--no-probes", "--no-graphs", "--full", "--served-steps", "1"]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == steps and out["warmup"] == 0
    assert out["config"]["parallelism"] == f"dp{n}" and out["config"]["global_batch"] == n * batch
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["scaling"] == "weak" and out["tokens_per_query"] == 6
    # value is the whole-job rate: n * batch * steps queries over the slowest rank's timed seconds
    assert abs(out["value"] - n * batch * steps / (out["ms_per_step"] * steps / 1000)) < 1e-3 * out["value"] + 1e-3
    # --full: the served pass (POST /generate SSE through each rank's chain server) rides along, outside the timed steps
    sv = out["served"]
    assert sv["value"] > 0 and sv["steps"] == 1 and sv["p50_ttft_s"] > 0 and "vs_in_process" in sv


TINY = ["--model", "tiny", "--embedder", "tiny", "--index-size", "1500", "--batch", "3", "--max-tokens", "6",
        "--chunk-tokens", "48", "--no-graphs"]


def _plain_run(out_dir, steps):
    import numpy as np

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           *TINY, "--dump-outputs", str(out_dir)]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


@pytest.mark.timeout(300)
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step and nothing that needs a run of its own (probes,
    served pass: --full); --dump-outputs writes the last timed step's results as float .npy files, and the same
    arguments give the same inputs: the retrieval outputs of two runs are equal."""
    import numpy as np

    out, err, a = _plain_run(tmp_path / "a", steps=2)
    assert out["steps"] == 2 and err.count("[bench] step ") == 2 and err.count("[bench] warmup ") == 1
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert abs(out["value"] - 3 * 2 / (out["ms_per_step"] * 2 / 1000)) < 1e-3 * out["value"] + 1e-3
    for k in ("served", "poisson", "p50_ttft_c1_s", "vs_baseline_single_stream"):
        assert k not in out
    assert set(a) == {"output_ids", "retrieved_rows", "retrieval_relevance", "query_embeddings"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["output_ids"].shape == (3, 6) and a["retrieved_rows"].shape == (3, 4)
    assert a["retrieval_relevance"].shape == (3, 4) and a["query_embeddings"].shape[0] == 3
    # every query retrieved its own planted rows of the last timed step (step 1: query ids 3..5)
    want = [sorted((q * 2654435761 + j * 40503 + 12345) % 1500 for j in range(4)) for q in range(3, 6)]
    assert [sorted(r) for r in a["retrieved_rows"].astype(int).tolist()] == want
    _, _, b = _plain_run(tmp_path / "b", steps=2)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_dump_outputs_samples_beyond_the_limit(tmp_path, monkeypatch):
    """Beyond the byte limit every array keeps the same seeded sample of its rows on every call."""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = {"x": np.arange(4000, dtype=np.float64).reshape(1000, 4), "y": np.arange(1000, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), big)
    bench.dump_outputs(str(tmp_path / "b"), big)
    xa, ya = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert xa.nbytes + ya.nbytes <= 4096 and xa.shape[0] == ya.shape[0] > 0
    assert (xa[:, 0] == 4 * ya).all()  # the same rows of both, in order
    np.testing.assert_array_equal(xa, np.load(tmp_path / "b" / "x.npy"))
