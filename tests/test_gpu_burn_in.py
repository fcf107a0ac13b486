"""GPU burn-in level of the health gate: data-verifying HBM pattern sweep and
exact MFMA checks (kuberay_amd/_native/gpuhealth.hip over gpuhealth_ref.hpp),
through the Python gate, the probe CLI, the pod builder's opt-in startup probe
and the metrics.

The CPU part needs no GPU: the host-only bindings, the pod builder, the sample
and the metrics. The GPU part (``@pytest.mark.gpu``) proves the operand lane
maps with exact asymmetric data, and the sweep with host-seeded mismatches; a
seeded mismatch only makes a comparison fail, it provokes no fault.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from kuberay_amd.common import pod as podlib
from kuberay_amd.models import RayCluster, RayNodeType
from kuberay_amd.testing import simple_raycluster
from kuberay_amd.utils import constants as C

ROOT = os.path.join(os.path.dirname(__file__), "..")
DTYPES = ("bf16", "f16", "fp8", "mxfp4")
MIB = 1 << 20


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


# ---------------------------------------------------------------------------
# Python transcription of gpuhealth_ref.hpp (pattern + generators): shared with
# tests/test_gpu_probe_kernels.py, in tests/gpuhealth_model.py
# ---------------------------------------------------------------------------
from gpuhealth_model import operands as _operands          # noqa: E402
from gpuhealth_model import pattern_word as _pattern_word  # noqa: E402


# ---------------------------------------------------------------------------
# CPU: host-only bindings
# ---------------------------------------------------------------------------
def test_pattern_word_matches_python(native):
    seed = native.DEFAULT_SEED
    indices = list(range(400)) + [(1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    indices += [(7 << 32) + 13 * i for i in range(300)]
    indices += [(1 << 40) * i + 977 * i for i in range(1, 298)]
    assert len(indices) == 1000
    for idx in indices:
        assert native.pattern_word(seed, idx) == _pattern_word(seed, idx), idx
    assert native.pattern_word(3, 5) == _pattern_word(3, 5)
    assert native.pattern_word(seed, 5) != native.pattern_word(seed, 5 + (1 << 32))


@pytest.mark.parametrize("dtype", ["mxfp4", "fp8"])
@pytest.mark.parametrize("wg", [0, 1])
def test_reference_tile_matches_numpy(native, dtype, wg):
    seed = native.DEFAULT_SEED
    A, B, C_ = _operands(dtype, seed, wg)
    expected = A @ B + C_
    got = np.array(native.reference_tile(dtype, seed, wg), dtype=np.float64)
    assert got.shape == (16, 16)
    assert np.array_equal(got, expected)
    assert not np.array_equal(got, got.T)


def test_reference_tile_rejects_unknown_dtype(native):
    with pytest.raises(ValueError):
        native.reference_tile("int8", 1, 0)


def test_header_is_a_rebuild_dependency(tmp_path, monkeypatch):
    """Editing gpuhealth_ref.hpp must rebuild the extension."""
    from kuberay_amd._native import build
    seen = {}

    def fake_needs_rebuild(src, out, *deps):
        seen["deps"] = deps
        return False
    monkeypatch.setattr(build, "_needs_rebuild", fake_needs_rebuild)
    build.build_gpuhealth()
    assert build.HERE / "gpuhealth_ref.hpp" in seen["deps"]


def test_check_gpu_burn_in_raises_off_gpu(monkeypatch):
    from kuberay_amd.gpu import health
    monkeypatch.setattr(health, "gpu_node", lambda: False)
    with pytest.raises(health.GpuHealthError):
        health.check_gpu_burn_in()


def test_health_report_new_fields_default_to_none():
    from kuberay_amd.gpu.health import HealthReport
    r = HealthReport(healthy=True)
    assert r.mfma_exact is None and r.hbm_pattern_ok is None
    assert r.hbm_bytes_checked is None and r.hbm_flipped_bits is None


def test_probe_deep_fails_loudly_off_gpu():
    if os.path.exists("/dev/kfd"):
        pytest.skip("running on a GPU node")
    out = subprocess.run(
        [sys.executable, "-m", "kuberay_amd.gpu.probe", "--deep", "--json"],
        capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert out.returncode == 2
    assert "not a GPU node" in out.stdout + out.stderr


# ---------------------------------------------------------------------------
# CPU: pod builder
# ---------------------------------------------------------------------------
FQDN = "demo-head-svc.default.svc.cluster.local"


def _cluster(gpus=1, annotation="true", head_annotation=None, startup_probe=None):
    d = simple_raycluster("demo", gpus_per_worker=gpus).to_dict()
    tmpl = d["spec"]["workerGroupSpecs"][0]["template"]
    if annotation is not None:
        tmpl.setdefault("metadata", {})["annotations"] = {
            C.GPU_BURN_IN_ANNOTATION_KEY: annotation}
    if startup_probe is not None:
        tmpl["spec"]["containers"][0]["startupProbe"] = startup_probe
    if head_annotation is not None:
        head = d["spec"]["headGroupSpec"]["template"]
        head.setdefault("metadata", {})["annotations"] = {
            C.GPU_BURN_IN_ANNOTATION_KEY: head_annotation}
        head["spec"]["containers"][0]["resources"]["limits"][C.AMD_GPU_RESOURCE_NAME] = "1"
    return RayCluster.from_dict(d)


def _worker_pod(cluster):
    group = cluster.spec.worker_group_specs[0]
    template = podlib.default_worker_pod_template(cluster, group, "demo-worker-", FQDN, "6379")
    return podlib.build_pod(template, RayNodeType.WORKER, group.ray_start_params,
                            "6379", False, None, FQDN,
                            ray_version=cluster.spec.ray_version)


def _head_pod(cluster):
    head = cluster.spec.head_group_spec
    template = podlib.default_head_pod_template(cluster, head, "demo-head-", "6379")
    return podlib.build_pod(template, RayNodeType.HEAD, head.ray_start_params, "6379",
                            False, None, "", ray_version=cluster.spec.ray_version)


def test_annotation_value():
    assert C.GPU_BURN_IN_ANNOTATION_KEY == "amd.com/gpu-burn-in"


def test_annotated_gpu_worker_gets_startup_probe():
    ray = _worker_pod(_cluster()).to_dict()["spec"]["containers"][0]
    probe = ray["startupProbe"]
    assert probe["exec"]["command"][-1] == "python -m kuberay_amd.gpu.probe --deep"
    assert probe["timeoutSeconds"] == C.GPU_BURN_IN_PROBE_TIMEOUT_SECONDS
    assert probe["failureThreshold"] == C.GPU_BURN_IN_PROBE_FAILURE_THRESHOLD
    # the kubelet must not cut a burn-in off before it can finish
    assert C.GPU_BURN_IN_PROBE_TIMEOUT_SECONDS >= 10
    assert C.GPU_BURN_IN_PROBE_FAILURE_THRESHOLD >= 1


def test_annotation_adds_nothing_but_the_startup_probe():
    plain = _worker_pod(_cluster(annotation=None)).to_dict()
    assert "startupProbe" not in plain["spec"]["containers"][0]
    annotated = _worker_pod(_cluster()).to_dict()
    # liveness and readiness are exactly as built without the annotation
    for key in ("livenessProbe", "readinessProbe"):
        assert annotated["spec"]["containers"][0][key] == plain["spec"]["containers"][0][key]
    del annotated["spec"]["containers"][0]["startupProbe"]
    del annotated["metadata"]["annotations"][C.GPU_BURN_IN_ANNOTATION_KEY]
    for d in (annotated, plain):
        if not d["metadata"].get("annotations"):
            d["metadata"].pop("annotations", None)
    assert annotated == plain


def test_annotation_false_is_off():
    ray = _worker_pod(_cluster(annotation="false")).to_dict()["spec"]["containers"][0]
    assert "startupProbe" not in ray


def test_head_never_gets_startup_probe():
    ray = _head_pod(_cluster(head_annotation="true")).to_dict()["spec"]["containers"][0]
    assert "startupProbe" not in ray


def test_cpu_worker_never_gets_startup_probe():
    ray = _worker_pod(_cluster(gpus=0)).to_dict()["spec"]["containers"][0]
    assert "startupProbe" not in ray


def test_user_startup_probe_is_preserved():
    user = {"exec": {"command": ["true"]}, "timeoutSeconds": 3, "failureThreshold": 7}
    ray = _worker_pod(_cluster(startup_probe=user)).to_dict()["spec"]["containers"][0]
    assert ray["startupProbe"] == user


def test_probe_injection_off_suppresses_startup_probe(monkeypatch):
    monkeypatch.setenv(C.ENABLE_PROBES_INJECTION, "false")
    ray = _worker_pod(_cluster()).to_dict()["spec"]["containers"][0]
    assert "startupProbe" not in ray


def test_sample_validates_and_builds_startup_probe():
    from kuberay_amd.utils import validation
    path = os.path.join(ROOT, "deploy", "samples", "ray-cluster.burn-in-mi355x.yaml")
    with open(path) as f:
        cluster = RayCluster.from_dict(yaml.safe_load(f))
    assert validation.validate_raycluster_metadata(cluster.metadata) == []
    assert validation.validate_raycluster_spec(cluster) == []
    ray = _worker_pod(cluster).to_dict()["spec"]["containers"][0]
    assert ray["startupProbe"]["exec"]["command"][-1].endswith("gpu.probe --deep")
    assert "--quick" in ray["readinessProbe"]["exec"]["command"][-1]
    assert "startupProbe" not in _head_pod(cluster).to_dict()["spec"]["containers"][0]


# ---------------------------------------------------------------------------
# CPU: metrics
# ---------------------------------------------------------------------------
def test_burn_in_metrics():
    from kuberay_amd.gpu.health import HealthReport
    from kuberay_amd.metrics import OperatorMetrics
    m = OperatorMetrics()
    before = m.exposition().decode()
    good = HealthReport(healthy=True, mfma_ok=True, hbm_gb_s=4000.0,
                        mfma_exact={d: True for d in DTYPES}, hbm_pattern_ok=True,
                        hbm_bytes_checked=1 << 30, hbm_flipped_bits=0)
    bad = HealthReport(healthy=False, mfma_ok=True, hbm_gb_s=4000.0,
                       mfma_exact={"bf16": True, "f16": True, "fp8": False, "mxfp4": True},
                       hbm_pattern_ok=False, hbm_bytes_checked=1 << 30,
                       hbm_flipped_bits=3)
    m.observe_gpu_burn_in("node-a", good)
    m.observe_gpu_burn_in("node-b", bad)
    text = m.exposition().decode()
    assert 'kuberay_mi355x_gpu_burn_in_flipped_bits{node="node-a"} 0.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_flipped_bits{node="node-b"} 3.0' in text
    for check in ("hbm_pattern", "mfma_bf16", "mfma_f16", "mfma_fp8", "mfma_mxfp4"):
        assert f'kuberay_mi355x_gpu_burn_in_ok{{check="{check}",node="node-a"}} 1.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="hbm_pattern",node="node-b"} 0.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="mfma_fp8",node="node-b"} 0.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="mfma_bf16",node="node-b"} 1.0' in text
    # every series of today is still declared, name and help unchanged
    for line in before.splitlines():
        if line.startswith("# ") and "kuberay_mi355x_" in line:
            assert line in text, line
    for name in ("kuberay_mi355x_gpu_utilization_pct", "kuberay_mi355x_hbm_used_fraction",
                 "kuberay_mi355x_autoscaler_decisions_total", "kuberay_mi355x_gpu_health"):
        assert f"# TYPE {name} " in text


# ---------------------------------------------------------------------------
# GPU: exact MFMA verification
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wg", [0, 1023])
def test_mfma_tile_is_exact(native, dtype, wg):
    """Fails if an operand lane map, the scale-byte selection or the FP4
    nibble order is wrong: the data is asymmetric, the comparison exact."""
    A, B, C_, D = (np.array(x, dtype=np.float64)
                   for x in native.mfma_verify_tile(0, dtype, native.DEFAULT_SEED, wg))
    K = 128 if dtype == "mxfp4" else 32
    assert A.shape == (16, K) and B.shape == (K, 16)
    assert C_.shape == (16, 16) and D.shape == (16, 16)
    expected = A @ B + C_
    print(f"{dtype} wg {wg}: {int((D != expected).sum())} of 256 elements differ")
    assert np.array_equal(D, expected)
    assert not np.array_equal(D, D.T)
    assert np.array_equal(
        D, np.array(native.reference_tile(dtype, native.DEFAULT_SEED, wg), dtype=np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mfma_verify_clean(native, dtype):
    r = native.mfma_verify(0, dtype, workgroups=1024)
    assert r["tiles"] == 1024 and r["mismatches"] == 0 and r["first_bad"] is None
    r = native.mfma_verify(0, dtype, workgroups=1)
    assert r["tiles"] == 1 and r["mismatches"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mfma_verify_seeded_mismatch(native, dtype):
    element = (517 * 16 + 9) * 16 + 3
    r = native.mfma_verify(0, dtype, workgroups=1024, corrupt_element=element)
    assert r["mismatches"] == 1
    assert tuple(r["first_bad"][:3]) == (517, 9, 3)
    got, expected = r["first_bad"][3:]
    assert got != expected


@pytest.mark.gpu
def test_mfma_verify_rejects_out_of_range(native):
    with pytest.raises(ValueError):
        native.mfma_verify(0, "bf16", workgroups=4, corrupt_element=4 * 256)
    with pytest.raises(ValueError):
        native.mfma_verify(0, "bf16", workgroups=4, corrupt_element=-2)
    with pytest.raises(ValueError):
        native.mfma_verify(0, "e5m2", workgroups=4)


# ---------------------------------------------------------------------------
# GPU: HBM pattern sweep
# ---------------------------------------------------------------------------
def _assert_clean(r, nbytes):
    assert r["mismatched_words"] == 0 and r["flipped_bits"] == 0
    assert r["bad_bit_mask"] == 0 and r["first_bad_offset"] == -1
    assert r["bytes_checked"] == nbytes


def _assert_one_flip(r, word, bit):
    assert r["mismatched_words"] == 1 and r["flipped_bits"] == 1
    assert r["bad_bit_mask"] == 1 << bit
    assert r["first_bad_offset"] == 4 * word


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", [16, 4096 + 16, MIB + 16, 64 * MIB])
def test_hbm_pattern_clean(native, nbytes):
    r = native.hbm_pattern_check(0, bytes=nbytes)
    _assert_clean(r, nbytes)
    assert r["chunks"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("word,bit", [(64 * MIB // 4 - 1, 7), (0, 0)])
def test_hbm_pattern_seeded_mismatch(native, word, bit):
    r = native.hbm_pattern_check(0, bytes=64 * MIB, corrupt_word=word, corrupt_bit=bit)
    _assert_one_flip(r, word, bit)
    assert r["bytes_checked"] == 64 * MIB


@pytest.mark.gpu
def test_hbm_pattern_default_is_256_mib(native):
    _assert_clean(native.hbm_pattern_check(0), 256 * MIB)


@pytest.mark.gpu
def test_hbm_pattern_64_bit_addressing(native):
    nbytes = (4 << 30) + 16 * MIB
    word = ((4 << 30) + 5 * MIB + 64) // 4   # byte offset >= 2^32
    r = native.hbm_pattern_check(0, bytes=nbytes, corrupt_word=word, corrupt_bit=31)
    assert r["bytes_checked"] == nbytes
    _assert_one_flip(r, word, 31)
    assert r["first_bad_offset"] >= 1 << 32


@pytest.mark.gpu
def test_hbm_pattern_chunking(native):
    nbytes = 96 * MIB + 16
    r = native.hbm_pattern_check(0, bytes=nbytes, max_chunk_mib=32)
    _assert_clean(r, nbytes)
    assert r["chunks"] == 4
    word = (64 * MIB + 4096) // 4            # inside the third chunk
    r = native.hbm_pattern_check(0, bytes=nbytes, max_chunk_mib=32,
                                 corrupt_word=word, corrupt_bit=12)
    assert r["chunks"] == 4
    _assert_one_flip(r, word, 12)
    last = nbytes // 4 - 1                   # the 16-byte fourth chunk
    r = native.hbm_pattern_check(0, bytes=nbytes, max_chunk_mib=32,
                                 corrupt_word=last, corrupt_bit=3)
    _assert_one_flip(r, last, 3)


@pytest.mark.gpu
def test_hbm_pattern_rejects_out_of_range(native):
    with pytest.raises(ValueError):
        native.hbm_pattern_check(0, bytes=4096, corrupt_word=1024)
    with pytest.raises(ValueError):
        native.hbm_pattern_check(0, bytes=4096, corrupt_word=0, corrupt_bit=32)
    with pytest.raises(ValueError):
        native.hbm_pattern_check(0, bytes=4096 + 4)


# ---------------------------------------------------------------------------
# GPU: Python gate and probe CLI
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_check_gpu_burn_in_healthy(native):
    from kuberay_amd.gpu.health import check_gpu_burn_in
    report = check_gpu_burn_in(hbm_fraction=0.01)
    assert report.healthy, report
    assert report.mfma_exact == {d: True for d in DTYPES}
    assert report.hbm_pattern_ok is True
    assert report.hbm_bytes_checked > 0
    assert report.hbm_flipped_bits == 0
    assert report.detail == ""


@pytest.mark.gpu
def test_probe_cli_deep(native, capsys):
    from kuberay_amd.gpu.probe import main
    assert main(["--deep", "--hbm-fraction", "0.01", "--json"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["healthy"] is True
    assert out["mfma_exact"] == {d: True for d in DTYPES}
    assert out["hbm_pattern_ok"] is True
    assert out["hbm_bytes_checked"] > 0 and out["hbm_flipped_bits"] == 0


@pytest.mark.gpu
def test_probe_cli_quick_keys_unchanged(native, capsys):
    from kuberay_amd.gpu.probe import main
    assert main(["--quick", "--json"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(out) == {"healthy", "mfma_ok", "hbm_gb_s", "rocm_smi_ok", "detail"}
