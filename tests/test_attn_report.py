"""The Python side of the burn-in's attention check, against fake native modules,
and the pod annotation that asks for it."""
import json
import types

import pytest

from test_gemm_exact_report import TILE, _gemm_result
from test_mfma_load_report import _burn_in_result, _probe
from test_pod_burn_in_load import BURN_IN, _startup

CLEAN = {"bf16": True, "f16": True}


def _attn_result(dtype, faulty=()):
    r = dict(_gemm_result(dtype, faulty), m=32768, n=1024, head_dim=64)
    del r["k"]
    return r


def _fake_gate(monkeypatch, faulty=None, with_attn=True):
    from kuberay_amd.gpu import health, rocm_smi
    calls = []
    fake = types.SimpleNamespace(
        device_count=lambda: 1,
        burn_in=lambda *a: calls.append("burn_in") or _burn_in_result(),
        gemm_narrow_exact=lambda device, dtype: calls.append(dtype) or _gemm_result(dtype))
    if with_attn:
        fake.attn_exact = lambda device, dtype: calls.append("attn " + dtype) or _attn_result(
            dtype, (faulty or {}).get(dtype, ()))
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    return calls


def test_clean_check_fills_its_fields_after_the_gemm_ones(monkeypatch, capsys):
    from kuberay_amd.gpu import health, probe
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(gemm_narrow=True, attention=True)
    assert (report.healthy, report.detail, report.attn_exact, report.attn_faulty) == (True, "", CLEAN, [])
    assert calls == ["burn_in", "fp8", "mxfp4", "attn bf16", "attn f16"]
    plain = health.check_gpu_burn_in()
    assert (plain.attn_exact, plain.attn_faulty) == (None, None)
    code, out, _ = _probe(capsys, ["--deep", "--attention", "--gemm-narrow", "--json"])
    assert code == 0 and list(json.loads(out).items())[-3:] == [
        ("gemm_narrow_faulty", []), ("attn_exact", CLEAN), ("attn_faulty", [])]
    code, out, _ = _probe(capsys, ["--deep", "--attention"])
    assert code == 0 and out.endswith(f" attn_exact={CLEAN} attn_faulty=[]")
    code, out, _ = _probe(capsys, ["--deep"])
    assert code == 0 and "attn" not in out
    del calls[:]
    for argv in (["--attention"], ["--quick", "--attention"]):
        with pytest.raises(SystemExit) as e:
            probe.main(argv)
        assert e.value.code == 2 and calls == []
        assert "--attention needs --deep" in capsys.readouterr().err


def test_faulty_tile_and_missing_entry_are_unhealthy_and_named(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, {"f16": [TILE]})
    report = health.check_gpu_burn_in(attention=True)
    assert (report.healthy, report.attn_exact) == (False, {"bf16": True, "f16": False})
    assert report.detail == ("attention f16 32768x1024x64: 9 bad elements, first [130][321] "
                             "got -40.0 expected 24.0 on cu xcc3/se1/sh0/cu7")
    code, out, _ = _probe(capsys, ["--deep", "--attention", "--json"])
    assert code == 1 and json.loads(out)["detail"] == report.detail
    _fake_gate(monkeypatch, with_attn=False)
    report = health.check_gpu_burn_in(attention=True)
    assert report.healthy is False
    assert report.detail == "attention: asked for, but this native module has no attn_exact"


def test_pod_gets_the_flag_only_with_the_annotation():
    from kuberay_amd.utils import constants as C
    key = C.GPU_BURN_IN_ATTENTION_ANNOTATION_KEY
    assert key == "amd.com/gpu-burn-in-attention"
    plain, attn = _startup(BURN_IN), _startup(dict(BURN_IN, **{key: "true"}))
    assert attn["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND + " --attention"
    assert dict(attn, exec=None) == dict(plain, exec=None)  # the timeout stays
    assert _startup(dict(BURN_IN, **{key: "false"})) == plain and _startup({key: "true"}) is None
    both = _startup(dict(BURN_IN, **{key: "true", C.GPU_BURN_IN_GEMM_NARROW_ANNOTATION_KEY: "true"}))
    assert both["exec"]["command"][2].endswith("--deep --gemm-narrow --attention")
