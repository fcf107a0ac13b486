"""The Python side of the burn-in's MoE check, against fake native modules, and
the pod annotation that asks for it."""
import json

import pytest

from test_attn_decode_report import _fake_gate as _decode_gate
from test_attn_report import CLEAN
from test_gemm_exact_report import TILE, _gemm_result
from test_mfma_load_report import _probe
from test_pod_burn_in_load import BURN_IN, _startup

SHAPE = {"tokens": 832, "experts": 16, "top_k": 2, "k": 1024, "n": 1024, "entries": 1664, "tiles": 33}


def _fake_gate(monkeypatch, faulty=None, with_moe=True, scatter=False):
    """The decode check's fake module plus the MoE entry; ``scatter``: a faulty tile without a CU."""
    from kuberay_amd.gpu import health
    calls = _decode_gate(monkeypatch)

    def moe_exact(device, dtype):
        calls.append("moe " + dtype)
        r = _gemm_result(dtype, (faulty or {}).get(dtype, ()))
        if scatter:
            r["faulty"] = [{"place": "scatter", "tile": (0, 0), "mismatches": 9, "first_bad": (130, 321)}]
        return {x: r[x] for x in r if x not in "mnk"} | SHAPE
    if with_moe:
        health._load_native().moe_exact = moe_exact
    return calls


def test_clean_check_fills_its_fields_after_the_decode_ones(monkeypatch, capsys):
    from kuberay_amd.gpu import health, probe
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(attention_decode=True, moe=True)
    assert (report.healthy, report.detail, report.moe_exact, report.moe_faulty) == (
        True, "", CLEAN, [])
    assert calls == ["burn_in", "decode bf16", "decode f16", "moe bf16", "moe f16"]
    assert health.check_gpu_burn_in(attention_decode=True).moe_exact is None
    code, out, _ = _probe(capsys, ["--deep", "--attention-decode", "--moe", "--json"])
    assert code == 0 and list(json.loads(out).items())[-3:] == [
        ("attn_decode_faulty", []), ("moe_exact", CLEAN), ("moe_faulty", [])]
    code, out, _ = _probe(capsys, ["--deep", "--moe"])
    assert code == 0 and out.endswith(f" moe_exact={CLEAN} moe_faulty=[]")
    del calls[:]
    with pytest.raises(SystemExit) as e:
        probe.main(["--quick", "--moe"])
    assert e.value.code == 2 and calls == []
    assert "--moe needs --deep" in capsys.readouterr().err


@pytest.mark.parametrize("scatter,short,place", [(False, "xcc3/se1/cu7", "xcc3/se1/sh0/cu7"),
                                                 (True, "scatter", "scatter")])
def test_faulty_tile_and_missing_entry_are_unhealthy_and_named(monkeypatch, capsys, scatter,
                                                               short, place):
    from kuberay_amd.gpu import health
    from kuberay_amd.metrics import OperatorMetrics
    _fake_gate(monkeypatch, {"f16": [TILE]}, scatter=scatter)
    report = health.check_gpu_burn_in(moe=True)
    assert (report.healthy, report.moe_exact, report.moe_faulty) == (
        False, {"bf16": True, "f16": False}, [f"f16 {short}"])
    assert report.detail == ("moe f16 832x16 top2 1024x1024: 9 bad elements, first "
                             f"[130][321] got -40.0 expected 24.0 on cu {place}")
    code, out, _ = _probe(capsys, ["--deep", "--moe", "--json"])
    assert code == 1 and json.loads(out)["detail"] == report.detail
    (metrics := OperatorMetrics()).observe_gpu_burn_in("n", report)
    text = metrics.exposition().decode()
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="moe_bf16",node="n"} 1.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="moe_f16",node="n"} 0.0' in text
    _fake_gate(monkeypatch, with_moe=False)
    report = health.check_gpu_burn_in(moe=True)
    assert (report.healthy, report.detail) == (
        False, "moe: asked for, but this native module has no moe_exact")


def test_pod_gets_the_flag_only_with_the_annotation():
    from kuberay_amd.utils import constants as C
    key = C.GPU_BURN_IN_MOE_ANNOTATION_KEY
    assert key == "amd.com/gpu-burn-in-moe"
    plain, moe = _startup(BURN_IN), _startup(dict(BURN_IN, **{key: "true"}))
    assert plain["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND  # byte for byte what it was
    assert moe["exec"]["command"][2] == C.GPU_BURN_IN_PROBE_COMMAND + " --moe"
    assert dict(moe, exec=None) == dict(plain, exec=None)  # the timeout stays
    assert _startup(dict(BURN_IN, **{key: "false"})) == plain and _startup({key: "true"}) is None
    both = _startup(dict(BURN_IN, **{key: "true",
                                     C.GPU_BURN_IN_ATTENTION_DECODE_ANNOTATION_KEY: "true"}))
    assert both["exec"]["command"][2].endswith("--deep --attention-decode --moe")
