"""The burn-in's CU sweep on the device: the LDS march's fill word for word
against tests/gpuhealth_model.py, a clean sweep's coverage map (the count of
distinct locations is the check of the register decode), the smallest shapes,
seeded LDS and MFMA faults found at the place the faulted workgroup recorded,
bad arguments, and ``burn_in()`` with the sweep in it.

A seeded fault is an xor the kernel applies to its own LDS or to its own D
register before its own compare: it makes a comparison fail and provokes no
device fault. Every comparison is exact.
"""
import numpy as np
import pytest

from gpuhealth_model import DTYPES, pattern_words

pytestmark = pytest.mark.gpu

SEED2 = 0x0BADC0DE
CLEAN_LDS = {"bad_words": 0, "flipped_bits": 0, "bad_bit_mask": 0, "first_bad_word": -1}


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


@pytest.fixture(scope="module")
def clean(native):
    """One sweep at the defaults, shared and left unchanged; run once more with
    32 rounds when 8 did not reach every CU."""
    result = native.cu_sweep()
    if result["cu_covered"] < result["cu_total"]:
        print(f"8 rounds covered {result['cu_covered']}/{result['cu_total']}; 32 rounds next")
        result = native.cu_sweep(max_rounds=32)
    return result


@pytest.fixture(scope="module")
def lds_max(clean):
    return clean["lds_bytes"]


def _where(d):
    return (d["xcc"], d["se"], d["sh"], d["cu"])


# ---------------------------------------------------------------------------
# 1. what the fill leaves in the LDS
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("visit", [0, 0xC0000005])
@pytest.mark.parametrize("size", ["one_vector", "stride_plus_one", "device_max"])
def test_lds_dump_matches_model(native, lds_max, size, visit):
    """Would fail on a wrong .x/.y/.z/.w order, a visit that is not the high
    half of the index, an ignored invert, a skipped stride step or a short
    tail (a skipped word reads back as 0x5A bytes)."""
    nbytes = {"one_vector": 16, "stride_plus_one": 4096 + 16, "device_max": lds_max}[size]
    for seed in (native.DEFAULT_SEED, SEED2):
        expected = pattern_words(seed, visit << 32, nbytes // 4)
        for invert in (False, True):
            raw = native.debug_cu_lds_dump(0, nbytes, seed, invert, visit)
            assert len(raw) == nbytes
            got = np.frombuffer(raw, dtype="<u4")
            want = expected ^ np.uint32(0xFFFFFFFF) if invert else expected
            bad = np.flatnonzero(got != want)
            print(f"seed {seed:#x} invert {invert}: {bad.size} of {want.size} words differ, "
                  f"first {bad[:4]}")
            assert np.array_equal(got, want)


def test_lds_dump_default_is_device_max(native, lds_max):
    assert len(native.debug_cu_lds_dump()) == lds_max
    assert lds_max % 16 == 0 and lds_max >= 64 << 10


# ---------------------------------------------------------------------------
# 2. clean sweep at the defaults
# ---------------------------------------------------------------------------
def test_clean_sweep_covers_every_cu(native, clean):
    """The decode is right exactly when the distinct locations a saturating
    sweep sees are as many as the device has CUs: too few means merged CUs (a
    field too narrow) or CUs never reached, too many means a mask that takes
    in bits that are no part of the place."""
    info = native.device_info(0)
    print(f"cu_total {clean['cu_total']} cu_covered {clean['cu_covered']} rounds "
          f"{clean['rounds']} blocks_per_round {clean['blocks_per_round']} lds_bytes "
          f"{clean['lds_bytes']} elapsed_ms {clean['elapsed_ms']:.2f} xcc_covered "
          f"{clean['xcc_covered']}")
    assert clean["faulty"] == []
    assert clean["simd_complete"] is True
    assert clean["cu_total"] == info["multi_processor_count"]
    assert clean["cu_covered"] <= clean["cu_total"]
    assert clean["blocks_per_round"] == 4 * clean["cu_total"]
    assert all(0 <= xcc < 8 for xcc in clean["xcc_covered"])
    assert len(set(clean["xcc_covered"].values())) == 1, clean["xcc_covered"]
    assert sum(clean["xcc_covered"].values()) == clean["cu_covered"]
    locations = clean["locations"]
    assert len(locations) == clean["cu_covered"]
    assert len({_where(l) for l in locations}) == len(locations)
    assert all(l["simd_seen"] == 0b1111 and l["visits"] >= 1 for l in locations)
    assert sum(l["visits"] for l in locations) == clean["rounds"] * clean["blocks_per_round"]
    assert "record" not in clean
    assert clean["cu_covered"] == clean["cu_total"]


def test_decode_location_binding_matches_the_sweep(native, clean):
    """The binding decodes a register pair to a place the sweep reported."""
    r = native.cu_sweep(blocks_per_round=1, max_rounds=1,
                        inject_mfma=(0, 0, "bf16", 0, 1 << 20))
    rec = r["record"]
    d = native.decode_location(rec["xcc_id_reg"], rec["hw_id_reg"])
    assert _where(d) == _where(rec) and d["simd"] == rec["simd"][0]
    assert _where(d) in {_where(l) for l in clean["locations"]}


# ---------------------------------------------------------------------------
# 3. minimal shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lds_bytes", [0, 16, 4096 + 16])
def test_one_block(native, lds_max, lds_bytes):
    r = native.cu_sweep(lds_bytes=lds_bytes, blocks_per_round=1, max_rounds=1)
    assert r["lds_bytes"] == (lds_bytes or lds_max)
    assert r["rounds"] == 1 and r["cu_covered"] == 1 and r["faulty"] == []
    assert len(r["locations"]) == 1
    assert r["locations"][0]["visits"] == 1 and r["locations"][0]["simd_seen"] == 0b1111
    assert r["simd_complete"] is True
    assert list(r["xcc_covered"].values()) == [1]


def test_rounds_stop_at_max_rounds(native):
    r = native.cu_sweep(blocks_per_round=2, max_rounds=3, passes=2)
    assert r["rounds"] == 3 and r["faulty"] == []
    assert sum(l["visits"] for l in r["locations"]) == 6
    assert 1 <= r["cu_covered"] <= 6


# ---------------------------------------------------------------------------
# 4. seeded LDS faults
# ---------------------------------------------------------------------------
def _expect_one_lds_fault(r, word, mask):
    rec = r["record"]
    assert rec is not None
    assert len(r["faulty"]) == 1, r["faulty"]
    f = r["faulty"][0]
    want = {"bad_words": 2, "flipped_bits": 2 * bin(mask).count("1"),
            "bad_bit_mask": mask, "first_bad_word": word}
    assert _where(f) == _where(rec)
    assert f["lds"] == want and f["mfma"] == []
    assert rec["lds"] == want


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("full_round", [False, True])
def test_seeded_lds_fault(native, clean, lds_max, full_round, phase):
    """Each of the two verifies (16-byte reads, rotated dword reads) counts the
    word once, in the phase that was named; every other slot stays clean."""
    blocks = clean["blocks_per_round"] if full_round else 1
    visit = blocks - 1
    n_words = lds_max // 4
    for word in (0, n_words - 1, 4096 // 4 + 1):
        for mask in (1, 1 << 31, 0xFFFFFFFF):
            r = native.cu_sweep(blocks_per_round=blocks, max_rounds=1,
                                inject_lds=(visit, word, mask, phase))
            _expect_one_lds_fault(r, word, mask)
            assert sum(l["visits"] for l in r["locations"]) == blocks


def test_seeded_lds_fault_small_lds_and_passes(native):
    """The rotation wraps inside a 16-byte LDS; with two passes the fault is
    seeded in the first pass only."""
    r = native.cu_sweep(lds_bytes=16, passes=2, blocks_per_round=3, max_rounds=2,
                        inject_lds=(4, 3, 0x00010000, 1))
    assert r["rounds"] == 2
    _expect_one_lds_fault(r, 3, 0x00010000)


# ---------------------------------------------------------------------------
# 5. seeded MFMA faults
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_mfma_fault(native, dtype):
    """Reported on the SIMD the wave itself recorded, for that data type only,
    at that workgroup's place only."""
    for wave in range(4):
        for element in (0, 255):
            r = native.cu_sweep(blocks_per_round=8, max_rounds=1,
                                inject_mfma=(5, wave, dtype, element, 1 << 20))
            rec = r["record"]
            assert sorted(rec["simd"]) == [0, 1, 2, 3]
            assert len(r["faulty"]) == 1, r["faulty"]
            f = r["faulty"][0]
            assert _where(f) == _where(rec)
            assert f["mfma"] == [(rec["simd"][wave], dtype)]
            assert f["lds"] == CLEAN_LDS and rec["lds"] == CLEAN_LDS


def test_seeded_lds_and_mfma_fault_together(native):
    r = native.cu_sweep(blocks_per_round=4, max_rounds=1, inject_lds=(2, 77, 4, 0),
                        inject_mfma=(2, 3, "mxfp4", 128, 1 << 20))
    rec = r["record"]
    assert len(r["faulty"]) == 1
    f = r["faulty"][0]
    assert _where(f) == _where(rec)
    assert f["mfma"] == [(rec["simd"][3], "mxfp4")]
    assert f["lds"] == {"bad_words": 2, "flipped_bits": 2, "bad_bit_mask": 4,
                        "first_bad_word": 77}


# ---------------------------------------------------------------------------
# 6. bad arguments
# ---------------------------------------------------------------------------
def test_bad_arguments_raise_and_leave_the_device_usable(native, lds_max):
    n_words = lds_max // 4
    small = dict(blocks_per_round=2, max_rounds=1)
    bad = [
        dict(lds_bytes=24), dict(lds_bytes=8), dict(lds_bytes=lds_max + 16),
        dict(passes=0), dict(passes=65), dict(max_rounds=0), dict(max_rounds=65),
        dict(blocks_per_round=-1), dict(blocks_per_round=(1 << 14) + 1),
        dict(blocks_per_round=1 << 14, max_rounds=64),
        dict(device=-1), dict(device=native.device_count()),
        dict(small, inject_lds=(-1, 0, 1, 0)), dict(small, inject_lds=(2, 0, 1, 0)),
        dict(small, inject_lds=(0, n_words, 1, 0)), dict(small, inject_lds=(0, -1, 1, 0)),
        dict(small, lds_bytes=16, inject_lds=(0, 4, 1, 0)),
        dict(small, inject_lds=(0, 0, 0, 0)), dict(small, inject_lds=(0, 0, 1 << 32, 0)),
        dict(small, inject_lds=(0, 0, -1, 0)), dict(small, inject_lds=(0, 0, 1, 2)),
        dict(small, inject_mfma=(-1, 0, "bf16", 0, 1)),
        dict(small, inject_mfma=(2, 0, "bf16", 0, 1)),
        dict(small, inject_mfma=(0, 4, "bf16", 0, 1)),
        dict(small, inject_mfma=(0, 0, "fp64", 0, 1)),
        dict(small, inject_mfma=(0, 0, "bf16", 256, 1)),
        dict(small, inject_mfma=(0, 0, "bf16", -1, 1)),
        dict(small, inject_mfma=(0, 0, "bf16", 0, 0)),
        dict(small, inject_lds=(0, 0, 1, 0), inject_mfma=(1, 0, "bf16", 0, 1)),
        dict(small, inject_lds_stuck=(-1, 0, 1, 0)), dict(small, inject_lds_stuck=(2, 0, 1, 0)),
        dict(small, inject_lds_stuck=(0, n_words, 1, 0)),
        dict(small, inject_lds_stuck=(0, -1, 1, 0)),
        dict(small, lds_bytes=16, inject_lds_stuck=(0, 4, 1, 0)),
        dict(small, inject_lds_stuck=(0, 0, 0, 0)),
        dict(small, inject_lds_stuck=(0, 0, 1 << 32, 0)),
        dict(small, inject_lds_stuck=(0, 0, -1, 0)), dict(small, inject_lds_stuck=(0, 0, 1, 2)),
        dict(small, inject_lds_stuck=(0, 0, 1, -1)),
        dict(small, inject_lds=(0, 0, 1, 0), inject_lds_stuck=(0, 0, 1, 0)),
        dict(small, inject_lds=(0, 0, 1, 0), inject_lds_stuck=(0, 1, 1, 0)),
        dict(small, inject_lds_stuck=(0, 0, 1, 0), inject_mfma=(1, 0, "bf16", 0, 1)),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError):
            native.cu_sweep(**kwargs)
            pytest.fail(f"accepted {kwargs}")
    for args in [(0, 24), (0, lds_max + 16), (0, 16, 0, False, -1), (0, 16, 0, False, 1 << 32),
                 (native.device_count(), 16)]:
        with pytest.raises(ValueError):
            native.debug_cu_lds_dump(*args)
            pytest.fail(f"accepted {args}")
    r = native.cu_sweep(blocks_per_round=16, max_rounds=1)
    assert r["faulty"] == [] and r["simd_complete"] and 1 <= r["cu_covered"] <= 16


# ---------------------------------------------------------------------------
# 7. burn_in() with the sweep in it
# ---------------------------------------------------------------------------
def test_burn_in_runs_the_sweep(native, clean):
    result = native.burn_in(0, 0.001, 0.0)
    sweep = result["cu_sweep"]
    print(f"burn_in cu_sweep: covered {sweep['cu_covered']}/{sweep['cu_total']} rounds "
          f"{sweep['rounds']} elapsed_ms {sweep['elapsed_ms']:.2f}")
    assert result["cu_ok"] is True and sweep["faulty"] == []
    assert result["cu_coverage_complete"] is (sweep["cu_covered"] == sweep["cu_total"])
    assert sweep["cu_total"] == clean["cu_total"] and sweep["lds_bytes"] == clean["lds_bytes"]
    assert result["healthy"] is True
    for key in ("mfma_ok", "hbm_gb_s", "hbm_ok", "mfma_exact", "mfma_first_bad",
                "hbm_pattern_ok", "hbm_pattern"):
        assert key in result


def test_check_gpu_burn_in_fills_the_cu_fields(native, clean):
    from kuberay_amd.gpu.health import check_gpu_burn_in
    report = check_gpu_burn_in(hbm_fraction=0.001)
    assert report.cu_total == clean["cu_total"]
    assert 1 <= report.cu_covered <= report.cu_total
    assert report.cu_faulty == []
    assert "cu xcc" not in report.detail
