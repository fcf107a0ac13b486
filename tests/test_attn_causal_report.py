"""The Python side of the burn-in's causal attention check, against fake native
modules, and the pod annotation that asks for it."""
import json

import pytest

from test_attn_report import CLEAN, _fake_gate as _attention_gate
from test_gemm_exact_report import TILE, _gemm_result
from test_mfma_load_report import _probe
from test_pod_burn_in_load import BURN_IN, _startup


def _fake_gate(monkeypatch, faulty=None, with_causal=True):
    """The attention check's fake native module, with the causal entry added; its
    result has heads and seq where the GEMM's has m, n and k."""
    from kuberay_amd.gpu import health
    calls = _attention_gate(monkeypatch)

    def attn_causal_exact(device, dtype):
        calls.append("causal " + dtype)
        r = _gemm_result(dtype, (faulty or {}).get(dtype, ()))
        return {x: r[x] for x in r if x not in "mnk"} | {"heads": 64, "seq": 1024, "head_dim": 128}
    if with_causal:
        health._load_native().attn_causal_exact = attn_causal_exact
    return calls


def test_clean_check_fills_its_fields_after_the_attention_ones(monkeypatch, capsys):
    from kuberay_amd.gpu import health, probe
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(attention=True, attention_causal=True)
    assert (report.healthy, report.detail, report.attn_causal_exact,
            report.attn_causal_faulty) == (True, "", CLEAN, [])
    assert calls == ["burn_in", "attn bf16", "attn f16", "causal bf16", "causal f16"]
    assert health.check_gpu_burn_in(attention=True).attn_causal_exact is None
    code, out, _ = _probe(capsys, ["--deep", "--attention", "--attention-causal", "--json"])
    assert code == 0 and list(json.loads(out).items())[-3:] == [
        ("attn_faulty", []), ("attn_causal_exact", CLEAN), ("attn_causal_faulty", [])]
    code, out, _ = _probe(capsys, ["--deep", "--attention-causal"])
    assert code == 0 and out.endswith(f" attn_causal_exact={CLEAN} attn_causal_faulty=[]")
    code, out, _ = _probe(capsys, ["--deep", "--attention"])
    assert code == 0 and "attn_causal" not in out
    del calls[:]
    with pytest.raises(SystemExit) as e:
        probe.main(["--quick", "--attention-causal"])
    assert e.value.code == 2 and calls == []
    assert "--attention-causal needs --deep" in capsys.readouterr().err


def test_faulty_tile_and_missing_entry_are_unhealthy_and_named(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    from kuberay_amd.metrics import OperatorMetrics
    _fake_gate(monkeypatch, {"f16": [TILE]})
    report = health.check_gpu_burn_in(attention_causal=True)
    assert (report.healthy, report.attn_causal_exact, report.attn_causal_faulty) == (
        False, {"bf16": True, "f16": False}, ["f16 xcc3/se1/cu7"])
    assert report.detail == ("attention causal f16 64x1024x128: 9 bad elements, first [130][321] "
                             "got -40.0 expected 24.0 on cu xcc3/se1/sh0/cu7")
    code, out, _ = _probe(capsys, ["--deep", "--attention-causal", "--json"])
    assert code == 1 and json.loads(out)["detail"] == report.detail
    metrics = OperatorMetrics()
    metrics.observe_gpu_burn_in("n", report)
    text = metrics.exposition().decode()
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="attn_causal_bf16",node="n"} 1.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="attn_causal_f16",node="n"} 0.0' in text
    _fake_gate(monkeypatch, with_causal=False)
    report = health.check_gpu_burn_in(attention_causal=True)
    assert (report.healthy, report.detail) == (
        False, "attention causal: asked for, but this native module has no attn_causal_exact")


def test_pod_gets_the_flag_only_with_the_annotation():
    from kuberay_amd.utils import constants as C
    key = C.GPU_BURN_IN_ATTENTION_CAUSAL_ANNOTATION_KEY
    assert key == "amd.com/gpu-burn-in-attention-causal"
    plain, causal = _startup(BURN_IN), _startup(dict(BURN_IN, **{key: "true"}))
    assert plain["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND  # byte for byte what it was
    assert causal["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND + " --attention-causal"
    assert dict(causal, exec=None) == dict(plain, exec=None)  # the timeout stays
    assert _startup(dict(BURN_IN, **{key: "false"})) == plain and _startup({key: "true"}) is None
    both = _startup(dict(BURN_IN, **{key: "true", C.GPU_BURN_IN_ATTENTION_ANNOTATION_KEY: "true"}))
    assert both["exec"]["command"][2].endswith("--deep --attention --attention-causal")
