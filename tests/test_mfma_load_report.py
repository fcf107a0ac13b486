"""The Python side of the burn-in's MFMA load, against fake native modules: how
``check_gpu_burn_in(load_seconds=...)`` and ``probe --deep --load-seconds``
turn the results of ``mfma_load`` into a report, a detail and metrics; that
``load_seconds=0`` makes the native calls and gives the outputs of before; and
that a native module without ``mfma_load`` that is asked for a load is
unhealthy and says so."""
import json
import types

import pytest

DTYPES = ("bf16", "f16", "fp8", "mxfp4")
CLEAN_PATTERN = {"bytes_checked": 1 << 30, "chunks": 1, "mismatched_words": 0,
                 "flipped_bits": 0, "bad_bit_mask": 0, "first_bad_offset": -1, "gb_s": 3000.0}
RATES = {"bf16": 2300.0, "f16": 2310.0, "fp8": 2350.0, "mxfp4": 6800.0}
CLOCKS = {"bf16": 2340.0, "f16": 2350.0, "fp8": 2380.0, "mxfp4": 1800.0}
FAULTY = {"xcc": 3, "se": 1, "sh": 0, "cu": 7, "simd": 2, "dtype": "bf16", "bad_elements": 5}
OLD_JSON_KEYS = ["healthy", "mfma_ok", "hbm_gb_s", "rocm_smi_ok", "detail", "mfma_exact",
                 "hbm_pattern_ok", "hbm_bytes_checked", "hbm_flipped_bits"]
SWEEP_KEYS = ["cu_total", "cu_covered", "cu_faulty"]
LOAD_KEYS = ["mfma_load_ok", "mfma_load_tflops", "mfma_load_clock_mhz", "mfma_load_faulty"]


def _burn_in_result():
    sweep = {"cu_total": 256, "cu_covered": 256, "rounds": 1, "lds_bytes": 160 << 10,
             "xcc_covered": {x: 32 for x in range(8)}, "simd_complete": True, "faulty": [],
             "locations": []}
    return {"mfma_ok": True, "hbm_gb_s": 4000.0, "hbm_ok": True,
            "mfma_exact": {d: True for d in DTYPES},
            "mfma_first_bad": {d: None for d in DTYPES},
            "hbm_pattern_ok": True, "hbm_pattern": dict(CLEAN_PATTERN),
            "cu_sweep": sweep, "cu_ok": True, "cu_coverage_complete": True, "healthy": True}


def _load_result(dtype, floor, tflops=None, faulty=(), clock=None, cycles=16.7):
    tflops = RATES[dtype] if tflops is None else tflops
    return {"dtype": dtype, "mfmas": 10 ** 9, "flop": 10 ** 13, "elapsed_ms": 500.0,
            "tflops": tflops, "clock_mhz": CLOCKS[dtype] if clock is None else clock,
            "cycles_per_mfma": cycles, "launches": 10, "cu_total": 256, "cu_covered": 256,
            "faulty": list(faulty), "locations": [], "slowest_cu": None,
            "floor_tflops": floor, "ok": not faulty and tflops >= floor}


def _fake_gate(monkeypatch, overrides=None, with_load=True):
    """overrides: dtype -> keyword arguments of _load_result."""
    from kuberay_amd.gpu import health, rocm_smi
    calls = []

    def burn_in(device, hbm_fraction, hbm_floor_gb_s):
        calls.append(("burn_in", device, hbm_fraction, hbm_floor_gb_s))
        return _burn_in_result()

    def mfma_load(device, dtype, seconds, floor_tflops):
        calls.append(("mfma_load", device, dtype, seconds, floor_tflops))
        return _load_result(dtype, floor_tflops, **(overrides or {}).get(dtype, {}))

    fake = types.SimpleNamespace(device_count=lambda: 1, burn_in=burn_in)
    if with_load:
        fake.mfma_load = mfma_load
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    return calls


def _probe(capsys, argv):
    from kuberay_amd.gpu import probe
    capsys.readouterr()
    code = probe.main(argv)
    text = capsys.readouterr()
    return code, text.out.strip(), text.err


def test_clean_load_fills_the_fields(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in(load_seconds=8.0)
    assert report.healthy is True and report.detail == ""
    assert report.mfma_load_ok is True and report.mfma_load_faulty == []
    assert report.mfma_load_tflops == RATES and report.mfma_load_clock_mhz == CLOCKS
    assert report.mfma_load_ok_by_dtype == {d: True for d in DTYPES}
    floors = health.DEFAULT_MFMA_FLOOR_TFLOPS
    assert calls == [("burn_in", 0, health.DEFAULT_BURN_IN_HBM_FRACTION,
                      health.DEFAULT_HBM_FLOOR_GB_S)] + [
        ("mfma_load", 0, d, 2.0, floors[d]) for d in DTYPES]

    code, out, _ = _probe(capsys, ["--deep", "--json", "--load-seconds", "8"])
    parsed = json.loads(out)
    assert code == 0 and list(parsed) == OLD_JSON_KEYS + SWEEP_KEYS + LOAD_KEYS
    assert parsed["mfma_load_ok"] is True and parsed["mfma_load_tflops"] == RATES
    assert parsed["mfma_load_clock_mhz"] == CLOCKS and parsed["mfma_load_faulty"] == []
    code, out, _ = _probe(capsys, ["--deep", "--load-seconds", "8"])
    assert code == 0
    assert out.endswith(f"cu_faulty=[] mfma_load_ok=True mfma_load_tflops={RATES} "
                        f"mfma_load_clock_mhz={CLOCKS} mfma_load_faulty=[]")


def test_default_floors_are_half_of_what_was_measured():
    """docs/benchmarks.md, "MFMA load": the lowest 2 s run per data type of
    both sessions, halved, rounded down to two digits."""
    from kuberay_amd.gpu import health
    lowest = {"bf16": 2312.8, "f16": 2330.4, "fp8": 2361.0, "mxfp4": 6782.7}
    for dtype, rate in lowest.items():
        half = rate / 2
        digits = 10 ** (len(str(int(half))) - 2)
        assert health.DEFAULT_MFMA_FLOOR_TFLOPS[dtype] == int(half) // digits * digits
    assert tuple(health.DEFAULT_MFMA_FLOOR_TFLOPS) == DTYPES == health.MFMA_LOAD_DTYPES


def test_faulty_cu_is_unhealthy_and_named(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, {"bf16": {"faulty": [FAULTY]}})
    report = health.check_gpu_burn_in(load_seconds=4.0)
    assert report.healthy is False and report.mfma_load_ok is False
    assert report.detail == "mfma load bf16: cu xcc3/se1/sh0/cu7 simd 2: 5 bad elements"
    assert report.mfma_load_faulty == ["bf16 xcc3/se1/cu7 simd 2"]
    assert report.mfma_load_ok_by_dtype == {"bf16": False, "f16": True, "fp8": True,
                                            "mxfp4": True}
    code, out, err = _probe(capsys, ["--deep", "--load-seconds", "4"])
    assert code == 1 and "mfma_load_ok=False" in out and report.detail in err
    code, out, _ = _probe(capsys, ["--deep", "--json", "--load-seconds", "4"])
    assert code == 1 and json.loads(out)["detail"] == report.detail


def test_rate_under_the_floor_is_unhealthy_with_the_clock(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, {"bf16": {"tflops": 212.4, "clock": 810.2, "cycles": 16.12}})
    report = health.check_gpu_burn_in(load_seconds=4.0, mfma_floor_tflops={"bf16": 600})
    assert report.healthy is False and report.mfma_load_ok is False
    assert report.mfma_load_faulty == []
    assert report.detail == ("mfma load bf16: 212 TFLOP/s below the floor of 600 "
                             "(clock 810 MHz, 16.1 cycles/MFMA)")
    assert report.mfma_load_tflops["bf16"] == 212.4
    # the same run passes a floor it reaches; the other floors stay the defaults
    calls = _fake_gate(monkeypatch, {"bf16": {"tflops": 212.4}})
    assert health.check_gpu_burn_in(load_seconds=4.0,
                                    mfma_floor_tflops={"bf16": 200.0}).healthy is True
    assert [c[4] for c in calls[1:]] == [200.0] + [
        health.DEFAULT_MFMA_FLOOR_TFLOPS[d] for d in DTYPES[1:]]
    code, out, _ = _probe(capsys, ["--deep", "--json", "--load-seconds", "4",
                                   "--mfma-floor-tflops", "bf16=600",
                                   "--mfma-floor-tflops", "fp8=100"])
    assert code == 1 and "below the floor of 600" in json.loads(out)["detail"]


def test_ok_false_of_the_native_module_alone_is_unhealthy(monkeypatch):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    fake = health._load_native()
    inner = fake.mfma_load
    fake.mfma_load = lambda *a, **k: dict(inner(*a, **k), ok=False)
    report = health.check_gpu_burn_in(load_seconds=1.0)
    assert report.healthy is False and "mfma load bf16: not ok" in report.detail
    assert len(calls) == 5


def test_no_load_makes_the_calls_and_the_outputs_of_before(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    report = health.check_gpu_burn_in()
    assert report == health.HealthReport(
        healthy=True, mfma_ok=True, hbm_gb_s=4000.0, rocm_smi_ok=True, detail="",
        mfma_exact={d: True for d in DTYPES}, hbm_pattern_ok=True,
        hbm_bytes_checked=1 << 30, hbm_flipped_bits=0, cu_total=256, cu_covered=256,
        cu_faulty=[])
    assert health.check_gpu_burn_in(load_seconds=0.0) == report
    assert calls == [("burn_in", 0, health.DEFAULT_BURN_IN_HBM_FRACTION,
                      health.DEFAULT_HBM_FLOOR_GB_S)] * 2
    for field in LOAD_KEYS + ["mfma_load_ok_by_dtype"]:
        assert getattr(report, field) is None

    code, out, _ = _probe(capsys, ["--deep", "--json"])
    assert code == 0 and out == json.dumps({
        "healthy": True, "mfma_ok": True, "hbm_gb_s": 4000.0, "rocm_smi_ok": True,
        "detail": "", "mfma_exact": {d: True for d in DTYPES}, "hbm_pattern_ok": True,
        "hbm_bytes_checked": 1 << 30, "hbm_flipped_bits": 0, "cu_total": 256,
        "cu_covered": 256, "cu_faulty": []})
    code, out, _ = _probe(capsys, ["--deep"])
    assert code == 0 and out == (
        "healthy=True mfma_ok=True hbm_gb_s=4000.0 rocm_smi_ok=True "
        f"mfma_exact={ {d: True for d in DTYPES} } hbm_pattern_ok=True "
        f"hbm_bytes_checked={1 << 30} hbm_flipped_bits=0 cu_total=256 cu_covered=256 "
        "cu_faulty=[]")
    assert all(c[0] == "burn_in" for c in calls)


def test_native_module_without_the_load_is_unhealthy_when_asked(monkeypatch, capsys):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch, with_load=False)
    assert health.check_gpu_burn_in().healthy is True
    report = health.check_gpu_burn_in(load_seconds=4.0)
    assert report.healthy is False and report.mfma_load_ok is False
    assert report.detail == "mfma load: asked for, but this native module has no mfma_load"
    code, out, err = _probe(capsys, ["--deep", "--json", "--load-seconds", "4"])
    assert code == 1 and json.loads(out)["mfma_load_ok"] is False


def test_hip_error_in_the_load_is_the_verdict(monkeypatch):
    from kuberay_amd.gpu import health
    _fake_gate(monkeypatch)
    fake = health._load_native()

    def broken(*a, **k):
        raise RuntimeError("HIP error: unspecified launch failure")
    fake.mfma_load = broken
    report = health.check_gpu_burn_in(load_seconds=1.0)
    assert report.healthy is False and "unspecified launch failure" in report.detail


@pytest.mark.parametrize("kwargs", [dict(load_seconds=-1.0), dict(load_seconds=60.5),
                                    dict(load_seconds=float("nan")),
                                    dict(load_seconds=1.0, mfma_floor_tflops={"int8": 1.0}),
                                    dict(load_seconds=1.0, mfma_floor_tflops={"bf16": -1.0})])
def test_bad_load_arguments_raise(monkeypatch, kwargs):
    from kuberay_amd.gpu import health
    calls = _fake_gate(monkeypatch)
    with pytest.raises(ValueError):
        health.check_gpu_burn_in(**kwargs)
    assert calls == []


@pytest.mark.parametrize("argv", [["--load-seconds", "1"], ["--quick", "--load-seconds", "1"],
                                  ["--deep", "--mfma-floor-tflops", "bf16=5"],
                                  ["--deep", "--load-seconds", "1", "--mfma-floor-tflops", "bf16"],
                                  ["--deep", "--load-seconds", "1", "--mfma-floor-tflops", "x=1"],
                                  ["--deep", "--load-seconds", "61"]])
def test_probe_rejects_bad_load_options(monkeypatch, capsys, argv):
    from kuberay_amd.gpu import probe
    calls = _fake_gate(monkeypatch)
    with pytest.raises(SystemExit) as e:
        probe.main(argv)
    assert e.value.code == 2 and calls == []
    capsys.readouterr()


def test_plain_deep_still_raises_on_a_bad_hbm_fraction(monkeypatch):
    """The path without a load is as it was: no usage error in place of the
    ValueError of check_gpu_burn_in."""
    from kuberay_amd.gpu import probe
    _fake_gate(monkeypatch)
    with pytest.raises(ValueError):
        probe.main(["--deep", "--hbm-fraction", "2"])


def test_quick_and_full_json_key_sets_are_unchanged(monkeypatch, capsys):
    from kuberay_amd.gpu import health, rocm_smi
    fake = types.SimpleNamespace(
        device_count=lambda: 1,
        health_check=lambda d, floor, quick: {"mfma_ok": True, "hbm_gb_s": 4000.0,
                                              "hbm_ok": True, "healthy": True})
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", lambda: [{"gpu": 0}])
    for argv in (["--quick"], []):
        code, out, _ = _probe(capsys, argv + ["--json"])
        assert code == 0
        assert list(json.loads(out)) == ["healthy", "mfma_ok", "hbm_gb_s", "rocm_smi_ok",
                                         "detail"]
        code, out, _ = _probe(capsys, argv)
        assert code == 0 and "mfma_load" not in out and "cu_" not in out


def test_metrics_of_the_load_only_when_the_report_has_them():
    from kuberay_amd.gpu.health import HealthReport
    from kuberay_amd.metrics import OperatorMetrics
    m = OperatorMetrics()
    base = dict(mfma_ok=True, hbm_gb_s=4000.0, mfma_exact={d: True for d in DTYPES},
                hbm_pattern_ok=True, hbm_bytes_checked=1 << 30, hbm_flipped_bits=0)
    m.observe_gpu_burn_in("node-a", HealthReport(healthy=True, **base))
    text = m.exposition().decode()
    assert 'node="node-a"' in text
    assert "mfma_load_bf16" not in text
    assert "kuberay_mi355x_gpu_mfma_load_tflops{" not in text
    assert "kuberay_mi355x_gpu_mfma_load_clock_mhz{" not in text

    by_dtype = {"bf16": False, "f16": True, "fp8": True, "mxfp4": True}
    m.observe_gpu_burn_in("node-b", HealthReport(
        healthy=False, mfma_load_ok=False, mfma_load_tflops=dict(RATES, bf16=212.0),
        mfma_load_clock_mhz=dict(CLOCKS, bf16=810.0), mfma_load_faulty=[],
        mfma_load_ok_by_dtype=by_dtype, **base))
    text = m.exposition().decode()
    assert 'kuberay_mi355x_gpu_mfma_load_tflops{dtype="bf16",node="node-b"} 212.0' in text
    assert 'kuberay_mi355x_gpu_mfma_load_tflops{dtype="mxfp4",node="node-b"} 6800.0' in text
    assert 'kuberay_mi355x_gpu_mfma_load_clock_mhz{dtype="bf16",node="node-b"} 810.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="mfma_load_bf16",node="node-b"} 0.0' in text
    assert 'kuberay_mi355x_gpu_burn_in_ok{check="mfma_load_fp8",node="node-b"} 1.0' in text
    assert 'check="mfma_load_bf16",node="node-a"' not in text
