"""The Python side of the burn-in's decode attention check, against fake native
modules, and the pod annotation that asks for it."""
import json

import pytest

from test_attn_causal_report import _fake_gate as _causal_gate
from test_attn_report import CLEAN
from test_gemm_exact_report import TILE, _gemm_result
from test_mfma_load_report import _probe
from test_pod_burn_in_load import BURN_IN, _startup

SHAPE = {"batch": 16, "kv_heads": 8, "group": 8, "splits": 4, "max_ctx": 2048, "head_dim": 128}


def _fake_gate(monkeypatch, faulty=None, with_decode=True, merge=False):
    """The causal check's fake native module, with the decode entry added; with
    ``merge`` its faulty tiles carry no CU, as a bad merge over splits does."""
    from kuberay_amd.gpu import health
    calls = _causal_gate(monkeypatch)

    def attn_decode_exact(device, dtype):
        calls.append("decode " + dtype)
        r = _gemm_result(dtype, (faulty or {}).get(dtype, ()))
        if merge:
            r["faulty"] = [{"tile": (3, 4), "mismatches": 9, "first_bad": (130, 321)}]
        return {x: r[x] for x in r if x not in "mnk"} | SHAPE
    if with_decode:
        health._load_native().attn_decode_exact = attn_decode_exact
    return calls


def test_clean_check_fills_its_fields_after_the_causal_ones(monkeypatch, capsys):
    from kuberay_amd.gpu import health, probe
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(attention_causal=True, attention_decode=True)
    assert (report.healthy, report.detail, report.attn_decode_exact,
            report.attn_decode_faulty) == (True, "", CLEAN, [])
    assert calls == ["burn_in", "causal bf16", "causal f16", "decode bf16", "decode f16"]
    assert health.check_gpu_burn_in(attention_causal=True).attn_decode_exact is None
    code, out, _ = _probe(capsys, ["--deep", "--attention-causal", "--attention-decode", "--json"])
    assert code == 0 and list(json.loads(out).items())[-3:] == [
        ("attn_causal_faulty", []), ("attn_decode_exact", CLEAN), ("attn_decode_faulty", [])]
    code, out, _ = _probe(capsys, ["--deep", "--attention-decode"])
    assert code == 0 and out.endswith(f" attn_decode_exact={CLEAN} attn_decode_faulty=[]")
    del calls[:]
    with pytest.raises(SystemExit) as e:
        probe.main(["--quick", "--attention-decode"])
    assert e.value.code == 2 and calls == []
    assert "--attention-decode needs --deep" in capsys.readouterr().err


@pytest.mark.parametrize("merge,short,place", [(False, "xcc3/se1/cu7", "xcc3/se1/sh0/cu7"),
                                               (True, "merge", "merge")])
def test_faulty_tile_and_missing_entry_are_unhealthy_and_named(monkeypatch, capsys, merge, short,
                                                               place):
    from kuberay_amd.gpu import health
    from kuberay_amd.metrics import OperatorMetrics
    _fake_gate(monkeypatch, {"f16": [TILE]}, merge=merge)
    report = health.check_gpu_burn_in(attention_decode=True)
    assert (report.healthy, report.attn_decode_exact, report.attn_decode_faulty) == (
        False, {"bf16": True, "f16": False}, [f"f16 {short}"])
    assert report.detail == ("attention decode f16 16x8x8 ctx 2048: 9 bad elements, first "
                             f"[130][321] got -40.0 expected 24.0 on cu {place}")
    code, out, _ = _probe(capsys, ["--deep", "--attention-decode", "--json"])
    assert code == 1 and json.loads(out)["detail"] == report.detail
    (metrics := OperatorMetrics()).observe_gpu_burn_in("n", report)
    text = metrics.exposition().decode()
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="attn_decode_bf16",node="n"} 1.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="attn_decode_f16",node="n"} 0.0' in text
    _fake_gate(monkeypatch, with_decode=False)
    report = health.check_gpu_burn_in(attention_decode=True)
    assert (report.healthy, report.detail) == (
        False, "attention decode: asked for, but this native module has no attn_decode_exact")


def test_pod_gets_the_flag_only_with_the_annotation():
    from kuberay_amd.utils import constants as C
    key = C.GPU_BURN_IN_ATTENTION_DECODE_ANNOTATION_KEY
    assert key == "amd.com/gpu-burn-in-attention-decode"
    plain, decode = _startup(BURN_IN), _startup(dict(BURN_IN, **{key: "true"}))
    assert plain["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND  # byte for byte what it was
    assert decode["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND + " --attention-decode"
    assert dict(decode, exec=None) == dict(plain, exec=None)  # the timeout stays
    assert _startup(dict(BURN_IN, **{key: "false"})) == plain and _startup({key: "true"}) is None
    both = _startup(dict(BURN_IN, **{key: "true",
                                     C.GPU_BURN_IN_ATTENTION_CAUSAL_ANNOTATION_KEY: "true"}))
    assert both["exec"]["command"][2].endswith("--deep --attention-causal --attention-decode")
