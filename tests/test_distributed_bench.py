"""Multi-process bench-path test: world_size=2 over gloo on CPU (the same
aggregation code the driver exercises at N=1..8 over RCCL on the GPU node).
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TestBenchSingleProcess:
    def test_bench_contract_json(self):
        out = subprocess.run(
            [sys.executable, "bench.py", "--clusters", "20", "--steps", "1",
             "--warmup", "0", "--workers-per-cluster", "1"],
            capture_output=True, text=True, cwd=REPO, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = out.stdout.strip().splitlines()[-1]
        d = json.loads(line)
        assert d["metric"] == "rayclusters_to_ready_per_sec"
        assert d["value"] > 0
        assert d["higher_is_better"] is True
        assert d["scaling"] == "weak"
        assert d["n_gpus"] == 1
        assert d["config"]["p50_cr_to_ready_s"] > 0
        assert d["vs_baseline"] > 0

    def test_dump_outputs_and_full(self, tmp_path):
        """--dump-outputs writes the last timed step's per-cluster status as
        float64 .npy arrays: one file per output column, every value as the
        arguments imply, and identical from one run to the next; --full is
        accepted and keeps the result line intact."""
        import numpy as np
        sys.path.insert(0, REPO)
        try:
            from bench import OUTPUT_COLUMNS
        finally:
            sys.path.remove(REPO)
        n, wpc, gpw = 7, 2, 1

        def run(out_dir):
            out = subprocess.run(
                [sys.executable, "bench.py", "--gpus", "1", "--clusters",
                 str(n), "--steps", "2", "--warmup", "0",
                 "--workers-per-cluster", str(wpc), "--gpus-per-worker",
                 str(gpw), "--full", "--dump-outputs", str(out_dir)],
                capture_output=True, text=True, cwd=REPO, timeout=300)
            assert out.returncode == 0, out.stderr[-2000:]
            d = json.loads(out.stdout.strip().splitlines()[-1])
            return d, {p.stem: np.load(p) for p in out_dir.glob("*.npy")}

        d, arrays = run(tmp_path / "first")
        assert d["metric"] == "rayclusters_to_ready_per_sec"
        assert d["unit"] == "clusters/s"
        assert d["dtype"] == "bf16"
        assert d["steps"] == 2
        assert d["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region
        assert d["value"] == pytest.approx(
            n / (d["ms_per_step"] / 1000.0), rel=1e-2)

        assert set(arrays) == set(OUTPUT_COLUMNS) | {"pods_at_scale"}
        total = 0
        for name, a in arrays.items():
            assert a.dtype in (np.float32, np.float64), (name, a.dtype)
            total += a.nbytes
        assert total <= 64 * 1024 * 1024
        # simple_raycluster: head 1 cpu / 2Gi, each worker 1 cpu / 1Gi /
        # gpw GPUs, min 0, max max(workers, 8); a Ready cluster has the
        # HeadPodReady and RayClusterProvisioned conditions true and the
        # five default head-service endpoints
        per_cluster = {
            "state_is_ready": 1,
            "desired_cpu": 1 + wpc,
            "desired_memory_bytes": (2 + wpc) * 2**30,
            "desired_gpu": wpc * gpw,
            "ready_worker_replicas": wpc,
            "available_worker_replicas": wpc,
            "desired_worker_replicas": wpc,
            "min_worker_replicas": 0,
            "max_worker_replicas": max(wpc, 8),
            "observed_generation": 1,
            "conditions_true": 2,
            "n_endpoints": 5,
        }
        assert set(per_cluster) == set(OUTPUT_COLUMNS)
        for key, want in per_cluster.items():
            np.testing.assert_array_equal(arrays[key], np.full(n, float(want)),
                                          err_msg=key)
        np.testing.assert_array_equal(arrays["pods_at_scale"],
                                      [n * (wpc + 1)])

        _, again = run(tmp_path / "second")
        assert set(again) == set(arrays)
        for key, a in arrays.items():
            np.testing.assert_array_equal(again[key], a, err_msg=key)


@pytest.mark.timeout(600)
class TestBenchDistributed:
    def test_world2_gloo(self):
        """Two ranks, gloo backend, 127.0.0.1 rendezvous — mirrors the
        driver's torch.distributed.run launch."""
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
             "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
             "--master-port", "29517", "bench.py", "--clusters", "15",
             "--steps", "1", "--warmup", "0", "--workers-per-cluster", "1"],
            capture_output=True, text=True, cwd=REPO, timeout=540,
            env={**os.environ, "MASTER_ADDR": "127.0.0.1"})
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, "exactly one JSON line from rank 0"
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2
        # whole-job aggregate: 2 ranks x 15 clusters
        assert d["config"]["global_batch"] == 30
        assert d["config"]["parallelism"] == "dp2"

    def test_world8_gloo(self):
        """Eight ranks with tiny per-rank work — pre-proves rendezvous and
        MAX/SUM aggregation at the driver's full N=8 scaling point so
        `bench.py --gpus 8` just works when the driver gets an 8-GPU node."""
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
             "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
             "--master-port", "29521", "bench.py", "--clusters", "4",
             "--steps", "1", "--warmup", "0", "--workers-per-cluster", "1",
             "--controller-workers", "2"],
            capture_output=True, text=True, cwd=REPO, timeout=540,
            env={**os.environ, "MASTER_ADDR": "127.0.0.1"})
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["n_gpus"] == 8
        assert d["config"]["global_batch"] == 32  # 8 ranks x 4 clusters
        assert d["config"]["parallelism"] == "dp8"

    def test_world4_gloo(self):
        """Four ranks — same shape the driver uses for the N=4 scaling
        point; validates rendezvous + MAX/SUM aggregation at higher fan-out."""
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
             "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
             "--master-port", "29519", "bench.py", "--clusters", "8",
             "--steps", "1", "--warmup", "0", "--workers-per-cluster", "1"],
            capture_output=True, text=True, cwd=REPO, timeout=540,
            env={**os.environ, "MASTER_ADDR": "127.0.0.1"})
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["n_gpus"] == 4
        assert d["config"]["global_batch"] == 32  # 4 ranks x 8 clusters
        assert d["config"]["parallelism"] == "dp4"
