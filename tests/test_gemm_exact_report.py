"""The Python side of the burn-in's GEMM check, against fake native modules, and
the pod annotation that asks for it."""
import json
import types

import pytest

from test_mfma_load_report import _burn_in_result, _probe
from test_pod_burn_in_load import BURN_IN, _startup

TILE = {"xcc": 3, "se": 1, "sh": 0, "cu": 7, "tile": (2, 5), "mismatches": 9,
        "first_bad": (130, 321)}


def _gemm_result(dtype, faulty=()):
    bad = sum(f["mismatches"] for f in faulty)
    return {"dtype": dtype, "m": 1472, "n": 1472, "k": 1024, "ok": not faulty,
            "mismatches": bad, "first_bad": (130, 321, -40.0, 24.0) if faulty else None,
            "faulty": list(faulty), "workgroups": 529, "cu_total": 256, "cu_seen": 256,
            "elapsed_ms": 0.1, "tflops": 40.0}


def _fake_gate(monkeypatch, faulty=None, with_gemm=True):
    from kuberay_amd.gpu import health, rocm_smi
    calls = []
    fake = types.SimpleNamespace(device_count=lambda: 1,
                                 burn_in=lambda *a: calls.append("burn_in") or _burn_in_result())
    if with_gemm:
        fake.gemm_exact = lambda device, dtype: calls.append(dtype) or _gemm_result(
            dtype, (faulty or {}).get(dtype, ()))
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    return calls


def test_clean_gemm_fills_the_fields(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(gemm=True)
    assert report.healthy is True and report.detail == ""
    assert report.gemm_exact == {"bf16": True, "f16": True} and report.gemm_faulty == []
    assert calls == ["burn_in", "bf16", "f16"]
    code, out, _ = _probe(capsys, ["--deep", "--gemm", "--json"])
    parsed = json.loads(out)
    assert code == 0 and list(parsed.items())[-2:] == [
        ("gemm_exact", {"bf16": True, "f16": True}), ("gemm_faulty", [])]
    code, out, _ = _probe(capsys, ["--deep", "--gemm"])
    assert code == 0 and out.endswith("gemm_exact={'bf16': True, 'f16': True} gemm_faulty=[]")


def test_faulty_tile_is_unhealthy_and_named(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    from kuberay_amd.metrics import OperatorMetrics
    _fake_gate(monkeypatch, {"f16": [TILE]})
    report = health.check_gpu_burn_in(gemm=True)
    assert report.healthy is False and report.gemm_exact == {"bf16": True, "f16": False}
    assert report.gemm_faulty == ["f16 xcc3/se1/cu7"]
    assert report.detail == ("gemm f16 1472x1472x1024: 9 bad elements, first [130][321] "
                             "got -40.0 expected 24.0 on cu xcc3/se1/sh0/cu7")
    code, out, err = _probe(capsys, ["--deep", "--gemm", "--json"])
    assert code == 1 and json.loads(out)["detail"] == report.detail
    m = OperatorMetrics()
    m.observe_gpu_burn_in("node-a", report)
    text = m.exposition().decode()
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="gemm_f16",node="node-a"} 0.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="gemm_bf16",node="node-a"} 1.0' in text


def test_native_module_without_the_gemm_is_unhealthy_when_asked(monkeypatch):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, with_gemm=False)
    report = health.check_gpu_burn_in(gemm=True)
    assert report.healthy is False and report.detail == (
        "gemm: asked for, but this native module has no gemm_exact")


def test_without_gemm_the_report_is_the_one_of_before(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    from kuberay_amd.metrics import OperatorMetrics
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in()
    assert report == health.check_gpu_burn_in(gemm=False)
    assert (report.gemm_exact, report.gemm_faulty, calls) == (None, None, ["burn_in"] * 2)
    for argv in (["--deep", "--json"], ["--deep"]):
        code, out, _ = _probe(capsys, argv)
        assert code == 0 and "gemm" not in out
    m = OperatorMetrics()
    m.observe_gpu_burn_in("node-a", report)
    assert "gemm_" not in m.exposition().decode()


@pytest.mark.parametrize("argv", [["--gemm"], ["--quick", "--gemm"]])
def test_probe_gemm_needs_deep(monkeypatch, capsys, argv):
    from kuberay_amd.gpu import probe
    calls = _fake_gate(monkeypatch)
    with pytest.raises(SystemExit) as e:
        probe.main(argv)
    assert e.value.code == 2 and calls == []
    assert "--gemm needs --deep" in capsys.readouterr().err


def test_pod_gets_the_flag_only_with_the_annotation():
    from kuberay_amd.utils import constants as C
    key = C.GPU_BURN_IN_GEMM_ANNOTATION_KEY
    assert key == "amd.com/gpu-burn-in-gemm"
    plain, with_gemm = _startup(BURN_IN), _startup(dict(BURN_IN, **{key: "true"}))
    assert plain["exec"]["command"] == ["bash", "-c", C.GPU_BURN_IN_PROBE_COMMAND]
    assert with_gemm["exec"]["command"] == ["bash", "-c", C.GPU_BURN_IN_PROBE_COMMAND + " --gemm"]
    assert dict(with_gemm, exec=None) == dict(plain, exec=None)  # the timeout stays
    assert _startup(dict(BURN_IN, **{key: "false"})) == plain
    assert _startup({key: "true"}) is None  # nothing without the burn-in annotation
    both = _startup(dict(BURN_IN, **{key: "true", "amd.com/gpu-burn-in-load-seconds": "8"}))
    assert both["exec"]["command"][2].endswith("--deep --load-seconds 8 --gemm")
