"""The Python side of the burn-in's CU sweep, against fake native modules: how
``check_gpu_burn_in`` and ``probe --deep`` turn the ``cu_sweep`` / ``cu_ok`` /
``cu_coverage_complete`` keys of ``burn_in()`` into a report, and that a native
module without those keys gives the report and the JSON it gave before."""
import json
import types

import pytest

DTYPES = ("bf16", "f16", "fp8", "mxfp4")
CLEAN_PATTERN = {"bytes_checked": 1 << 30, "chunks": 1, "mismatched_words": 0,
                 "flipped_bits": 0, "bad_bit_mask": 0, "first_bad_offset": -1, "gb_s": 3000.0}
FAULTY_CU = {"xcc": 3, "se": 1, "sh": 0, "cu": 7,
             "lds": {"bad_words": 2, "flipped_bits": 2, "bad_bit_mask": 0x100,
                     "first_bad_word": 1234},
             "mfma": [(2, "fp8")]}
MFMA_ONLY_CU = {"xcc": 0, "se": 2, "sh": 0, "cu": 11,
                "lds": {"bad_words": 0, "flipped_bits": 0, "bad_bit_mask": 0,
                        "first_bad_word": -1},
                "mfma": [(0, "bf16"), (3, "mxfp4")]}


def _old_result():
    """What burn_in() returned before the CU sweep existed."""
    return {"mfma_ok": True, "hbm_gb_s": 4000.0, "hbm_ok": True,
            "mfma_exact": {d: True for d in DTYPES},
            "mfma_first_bad": {d: None for d in DTYPES},
            "hbm_pattern_ok": True, "hbm_pattern": dict(CLEAN_PATTERN),
            "healthy": True}


def _result(faulty=(), covered=256, total=256, rounds=1):
    faulty = list(faulty)
    sweep = {"cu_total": total, "cu_covered": covered, "rounds": rounds,
             "lds_bytes": 160 << 10, "xcc_covered": {x: covered // 8 for x in range(8)},
             "simd_complete": True, "faulty": faulty,
             "locations": [{"xcc": 0, "se": 0, "sh": 0, "cu": 0, "visits": 4,
                            "simd_seen": 15}]}
    out = _old_result()
    out.update(cu_sweep=sweep, cu_ok=not faulty, cu_coverage_complete=covered >= total,
               healthy=not faulty)
    return out


def _fake_gate(monkeypatch, result):
    from kuberay_amd.gpu import health, rocm_smi
    calls = []

    def burn_in(device, hbm_fraction, hbm_floor_gb_s):
        calls.append((device, hbm_fraction, hbm_floor_gb_s))
        return result

    fake = types.SimpleNamespace(device_count=lambda: 1, burn_in=burn_in)
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    return calls


def _probe_json(capsys, argv):
    from kuberay_amd.gpu import probe
    capsys.readouterr()
    code = probe.main(argv)
    return code, json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_clean_sweep_is_healthy_and_fills_the_fields(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch, _result())
    report = health.check_gpu_burn_in()
    assert report.healthy is True and report.detail == ""
    assert (report.cu_total, report.cu_covered, report.cu_faulty) == (256, 256, [])
    assert calls == [(0, health.DEFAULT_BURN_IN_HBM_FRACTION, health.DEFAULT_HBM_FLOOR_GB_S)]
    code, out = _probe_json(capsys, ["--deep", "--json"])
    assert code == 0 and out["healthy"] is True
    assert (out["cu_total"], out["cu_covered"], out["cu_faulty"]) == (256, 256, [])


def test_faulty_cu_is_unhealthy_and_named(monkeypatch, capsys):
    from kuberay_amd.gpu import health, probe
    _fake_gate(monkeypatch, _result(faulty=[FAULTY_CU, MFMA_ONLY_CU]))
    report = health.check_gpu_burn_in()
    assert report.healthy is False
    assert report.cu_faulty == ["xcc3/se1/cu7", "xcc0/se2/cu11"]
    entries = report.detail.split("; cu ")
    assert ("cu xcc3/se1/sh0/cu7: lds 2 bad words mask 0x00000100 first word 1234; "
            "mfma fp8 on simd 2") in report.detail
    assert "cu xcc0/se2/sh0/cu11: mfma bf16 on simd 0; mfma mxfp4 on simd 3" in report.detail
    assert len(entries) == 2 and "lds" not in entries[1]
    assert "coverage" not in report.detail
    code, out = _probe_json(capsys, ["--deep", "--json"])
    assert code == 1 and out["healthy"] is False
    assert out["cu_faulty"] == report.cu_faulty and out["detail"] == report.detail
    # without --json the fields are printed and the detail goes to stderr
    assert probe.main(["--deep"]) == 1
    text = capsys.readouterr()
    assert "cu_total=256 cu_covered=256 cu_faulty=['xcc3/se1/cu7', 'xcc0/se2/cu11']" in text.out
    assert report.detail in text.err


def test_cu_ok_false_alone_is_unhealthy(monkeypatch):
    """``healthy`` of the fake says True: the report still follows ``cu_ok``."""
    from kuberay_amd.gpu import health
    result = _result(faulty=[FAULTY_CU])
    result["healthy"] = True
    _fake_gate(monkeypatch, result)
    assert health.check_gpu_burn_in().healthy is False


def test_incomplete_coverage_is_reported_and_fatal_only_on_request(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, _result(covered=251, rounds=8))
    report = health.check_gpu_burn_in()
    assert report.healthy is True
    assert report.detail == "cu coverage 251/256 after 8 rounds"
    assert (report.cu_total, report.cu_covered, report.cu_faulty) == (256, 251, [])
    strict = health.check_gpu_burn_in(require_cu_coverage=True)
    assert strict.healthy is False and strict.detail == report.detail

    code, out = _probe_json(capsys, ["--deep", "--json"])
    assert code == 0 and out["healthy"] is True and out["cu_covered"] == 251
    assert out["detail"] == report.detail
    code, out = _probe_json(capsys, ["--deep", "--json", "--require-cu-coverage"])
    assert code == 1 and out["healthy"] is False and out["cu_covered"] == 251


def test_complete_coverage_passes_the_strict_gate(monkeypatch, capsys):
    _fake_gate(monkeypatch, _result())
    code, out = _probe_json(capsys, ["--deep", "--json", "--require-cu-coverage"])
    assert code == 0 and out["healthy"] is True


OLD_JSON_KEYS = ["healthy", "mfma_ok", "hbm_gb_s", "rocm_smi_ok", "detail", "mfma_exact",
                 "hbm_pattern_ok", "hbm_bytes_checked", "hbm_flipped_bits"]


@pytest.mark.parametrize("strict", [False, True])
def test_native_module_without_the_sweep_reports_as_before(monkeypatch, capsys, strict):
    from kuberay_amd.gpu import health, probe
    _fake_gate(monkeypatch, _old_result())
    report = health.check_gpu_burn_in(require_cu_coverage=strict)
    assert report == health.HealthReport(
        healthy=True, mfma_ok=True, hbm_gb_s=4000.0, rocm_smi_ok=True, detail="",
        mfma_exact={d: True for d in DTYPES}, hbm_pattern_ok=True,
        hbm_bytes_checked=1 << 30, hbm_flipped_bits=0)
    assert report.cu_total is None and report.cu_covered is None and report.cu_faulty is None

    argv = ["--deep"] + (["--require-cu-coverage"] if strict else [])
    capsys.readouterr()
    assert probe.main(argv + ["--json"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps({
        "healthy": True, "mfma_ok": True, "hbm_gb_s": 4000.0, "rocm_smi_ok": True,
        "detail": "", "mfma_exact": {d: True for d in DTYPES}, "hbm_pattern_ok": True,
        "hbm_bytes_checked": 1 << 30, "hbm_flipped_bits": 0})
    assert list(json.loads(line)) == OLD_JSON_KEYS
    assert probe.main(argv) == 0
    assert capsys.readouterr().out.strip() == (
        "healthy=True mfma_ok=True hbm_gb_s=4000.0 rocm_smi_ok=True "
        f"mfma_exact={ {d: True for d in DTYPES} } hbm_pattern_ok=True "
        f"hbm_bytes_checked={1 << 30} hbm_flipped_bits=0")


def test_quick_and_full_outputs_have_no_cu_fields(monkeypatch, capsys):
    from kuberay_amd.gpu import health, probe, rocm_smi
    fake = types.SimpleNamespace(
        device_count=lambda: 1,
        health_check=lambda d, floor, quick: {"mfma_ok": True, "hbm_gb_s": 4000.0,
                                              "hbm_ok": True, "healthy": True})
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    for argv in (["--quick"], []):
        code, out = _probe_json(capsys, argv + ["--json"])
        assert code == 0
        assert list(out) == ["healthy", "mfma_ok", "hbm_gb_s", "rocm_smi_ok", "detail"]
        assert probe.main(argv) == 0
        assert "cu_" not in capsys.readouterr().out
