"""bench.py contract: one JSON line from rank 0 with the driver's keys, value =
whole-job req/s aggregated over ranks (weak scaling), on 1 and 2 ranks
(torch.distributed.run, gloo; the tunnel workload itself is host-side)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _run(argv, timeout=300):
    out = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                         env={**os.environ, "MASTER_ADDR": "127.0.0.1"})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _check(d, n, steps, warmup):
    assert KEYS <= set(d)
    assert d["n_gpus"] == n and d["steps"] == steps and d["warmup"] == warmup
    assert d["scaling"] == "weak" and d["higher_is_better"] is True and d["errors"] == 0
    assert d["config"]["global_batch"] == 8 * n
    # 8 streams per rank, one 5-token completion (~0.5 s) per step: ~16 req/s per rank
    assert 12 * n < d["value"] < 17 * n
    assert abs(d["value"] - 8 * n * steps / (d["ms_per_step"] * steps / 1e3)) < 1e-6 * d["value"]


def test_bench_single_rank():
    d = _run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--curve", "1",
              "--curve-steps", "1"])
    _check(d, 1, 2, 1)
    assert "1" in d["curve_rank0"] and "8" in d["curve_rank0"]
    assert d["curve_steps"] == 1
    # The host the numbers came from (rows move 20-40 % between boxes).
    assert {"cpu_model", "host_hash", "governor", "deepest_idle", "cpus_allowed", "cgroup_cpus", "io_uring"} <= set(d["box"])
    assert d["config"]["assoc"] == int(os.environ.get("TUNNEL_ASSOC", "3"))


def test_bench_curve_points_default_to_the_headline_steps():
    d = _run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--curve", "2",
              "--no-jumbo-extra"])
    _check(d, 1, 2, 1)
    assert d["curve_steps"] == 2


def test_bench_two_ranks_torchrun():
    from p2p_llm_tunnel_amd.utils.procs import free_port
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
              "127.0.0.1", "--master-port", str(free_port()), "bench.py", "--gpus", "2", "--full", "--steps", "2",
              "--warmup", "1", "--curve", "", "--curve-steps", "1"])
    _check(d, 2, 2, 1)


def test_bench_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """Without --full: no curve, direct or jumbo legs (their fields null / empty);
    --dump-outputs writes the last timed step's response bodies, the same bytes
    every run: 5 token events, the stop event and [DONE] on each of 8 streams."""
    import numpy as np
    runs = []
    for name in ("a", "b"):
        d = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs",
                  str(tmp_path / name)])
        _check(d, 1, 2, 1)
        assert d["full"] is False and d["curve_rank0"] == {} and d["jumbo_rank0"] is None
        # the benchmark process runs on the compiled core it reports
        assert d["native_core"]["module"].startswith("_native") and d["native_core"]["protocol"]
        assert d["added_p50_ttft_ms"] is None and d["added_p99_ttft_ms"] is None
        assert sorted(os.listdir(tmp_path / name)) == ["response_bytes.npy", "response_len.npy"]
        runs.append((np.load(tmp_path / name / "response_bytes.npy"), np.load(tmp_path / name / "response_len.npy")))
    (b0, l0), (b1, l1) = runs
    assert b0.dtype == np.float32 and l0.dtype == np.float32
    assert b0.shape == (8, int(l0.max())) and l0.min() == l0.max() > 0
    assert np.array_equal(b0, b1) and np.array_equal(l0, l1)
    body = bytes(b0[0].astype(np.uint8))
    events = body.split(b"\n\n")
    assert len(events) == 8 and events[-1] == b"" and events[-2] == b"data: [DONE]"
    text = "".join(json.loads(e[6:])["choices"][0]["delta"].get("content", "") for e in events[:6])
    assert text == "Hello from the tunnel!"
