"""The Python side of the burn-in's narrow GEMM check (fp8, mxfp4), against fake
native modules, and the pod annotation that asks for it."""
import json
import types

import pytest

from test_gemm_exact_report import TILE, _gemm_result
from test_mfma_load_report import _burn_in_result, _probe
from test_pod_burn_in_load import BURN_IN, _startup

CLEAN = {"fp8": True, "mxfp4": True}


def _fake_gate(monkeypatch, faulty=None, with_narrow=True):
    from kuberay_amd.gpu import health, rocm_smi
    calls = []
    fake = types.SimpleNamespace(
        device_count=lambda: 1,
        burn_in=lambda *a: calls.append("burn_in") or _burn_in_result(),
        gemm_exact=lambda device, dtype: calls.append(dtype) or _gemm_result(dtype))
    if with_narrow:
        fake.gemm_narrow_exact = lambda device, dtype: calls.append(dtype) or _gemm_result(
            dtype, (faulty or {}).get(dtype, ()))
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    return calls


def test_clean_check_fills_its_fields_after_the_gemm_ones(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(gemm=True, gemm_narrow=True)
    assert report.healthy is True and report.detail == ""
    assert report.gemm_narrow_exact == CLEAN and report.gemm_narrow_faulty == []
    assert calls == ["burn_in", "bf16", "f16", "fp8", "mxfp4"]
    alone = health.check_gpu_burn_in(gemm_narrow=True)
    assert (alone.gemm_exact, alone.gemm_faulty, alone.gemm_narrow_exact) == (None, None, CLEAN)
    code, out, _ = _probe(capsys, ["--deep", "--gemm-narrow", "--gemm", "--json"])
    assert code == 0 and list(json.loads(out).items())[-4:] == [
        ("gemm_exact", {"bf16": True, "f16": True}), ("gemm_faulty", []),
        ("gemm_narrow_exact", CLEAN), ("gemm_narrow_faulty", [])]
    code, out, _ = _probe(capsys, ["--deep", "--gemm-narrow", "--gemm"])
    assert code == 0 and out.endswith(f"gemm_exact={{'bf16': True, 'f16': True}} gemm_faulty=[] "
                                      f"gemm_narrow_exact={CLEAN} gemm_narrow_faulty=[]")


def test_faulty_tile_is_unhealthy_and_named(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    from kuberay_amd.metrics import OperatorMetrics
    _fake_gate(monkeypatch, {"mxfp4": [TILE]})
    report = health.check_gpu_burn_in(gemm_narrow=True)
    assert report.healthy is False and report.gemm_narrow_exact == {"fp8": True, "mxfp4": False}
    assert report.gemm_narrow_faulty == ["mxfp4 xcc3/se1/cu7"]
    assert report.detail == ("gemm mxfp4 1472x1472x1024: 9 bad elements, first [130][321] "
                             "got -40.0 expected 24.0 on cu xcc3/se1/sh0/cu7")
    code, out, _ = _probe(capsys, ["--deep", "--gemm-narrow", "--json"])
    assert code == 1 and json.loads(out)["detail"] == report.detail
    m = OperatorMetrics()
    m.observe_gpu_burn_in("node-a", report)
    text = m.exposition().decode()
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="gemm_mxfp4",node="node-a"} 0.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="gemm_fp8",node="node-a"} 1.0' in text
    assert "gemm_bf16" not in text


def test_native_module_without_it_is_unhealthy_when_asked(monkeypatch):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, with_narrow=False)
    assert health.check_gpu_burn_in(gemm_narrow=True).detail == (
        "gemm narrow: asked for, but this native module has no gemm_narrow_exact")


def test_without_the_option_report_and_probe_are_those_of_before(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(gemm=True)
    assert report == health.check_gpu_burn_in(gemm=True, gemm_narrow=False)
    assert (report.gemm_narrow_exact, report.gemm_narrow_faulty) == (None, None)
    assert calls == ["burn_in", "bf16", "f16"] * 2
    for argv in (["--deep", "--gemm", "--json"], ["--deep", "--gemm"], ["--deep"]):
        code, out, _ = _probe(capsys, argv)
        assert code == 0 and "narrow" not in out


@pytest.mark.parametrize("argv", [["--gemm-narrow"], ["--quick", "--gemm-narrow"]])
def test_probe_gemm_narrow_needs_deep(monkeypatch, capsys, argv):
    from kuberay_amd.gpu import probe
    calls = _fake_gate(monkeypatch)
    with pytest.raises(SystemExit) as e:
        probe.main(argv)
    assert e.value.code == 2 and calls == []
    assert "--gemm-narrow needs --deep" in capsys.readouterr().err


def test_pod_gets_the_flag_only_with_the_annotation():
    from kuberay_amd.utils import constants as C
    key = C.GPU_BURN_IN_GEMM_NARROW_ANNOTATION_KEY
    assert key == "amd.com/gpu-burn-in-gemm-narrow"
    plain, narrow = _startup(BURN_IN), _startup(dict(BURN_IN, **{key: "true"}))
    assert narrow["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND + " --gemm-narrow"
    assert dict(narrow, exec=None) == dict(plain, exec=None)  # the timeout stays
    assert _startup(dict(BURN_IN, **{key: "false"})) == plain
    assert _startup({key: "true"}) is None  # nothing without the burn-in annotation
    both = _startup(dict(BURN_IN, **{key: "true", C.GPU_BURN_IN_GEMM_ANNOTATION_KEY: "true"}))
    assert both["exec"]["command"][2].endswith("--deep --gemm --gemm-narrow")
