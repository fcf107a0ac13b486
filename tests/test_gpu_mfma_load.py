"""The burn-in's MFMA load on the device: the accumulators the production loop
leaves after 1, 2, 3 and 33 MFMAs against tests/mfma_load_model.py bit for bit,
a clean run's counts, coverage and time stamps, a seeded accumulator fault
found once and at the place the faulted workgroup recorded, the TFLOP/s floor,
the timed mode, and bad arguments.

A seeded fault is an xor the kernel applies to one of its own accumulator
registers before its own compare: it makes a comparison fail and provokes no
device fault. Every data comparison is exact. Every run here is one short
launch (``seconds=0`` with explicit counts) but the duration test's 0.2 s.
"""
import numpy as np
import pytest

from gpuhealth_model import DTYPES
from mfma_load_model import (TILES, WAVES, accumulator_after_mfma, expected_dump,
                             flop_per_mfma, nonzero_target, tile_index)

pytestmark = pytest.mark.gpu

SEED2 = 0x0BADC0DE
CHECK_EVERY = 33
CHUNKS = 4
# Measured on two MI355X (docs/benchmarks.md, "MFMA load"): elapsed_ms - 200 of
# three runs each of the duration test's call was 17.5, 17.2, 14.0 and 12.8,
# 13.1, 14.9 ms (the launch in flight when the time is reached runs to its
# end); the bound is three times the largest, rounded up.
DURATION_MARGIN_MS = 53.0
# clock_mhz is a ratio of two counter differences over some 8.4k cycles
# (4 chunks x 33 x 4 MFMAs of about 16 cycles), that is about 350 ticks of the
# 100 MHz counter: one tick at either end is 0.6 %, and the two counters are
# read one after the other, some tens of cycles apart, under 1 %. Measured at
# this shape on two MI355X whose device_info clock_mhz is 2400, seven runs per
# data type: bf16 2011 to 2164 MHz, f16 2023 to 2173, fp8 2111 to 2236, mxfp4
# 1879 to 2040 (a 0.2 s run held 2313 to 2347), so the bound of 2400 x 1.03
# was 10 % away.
CLOCK_MARGIN = 1.03


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


def _small(native, dtype, **kw):
    return native.mfma_load(0, dtype, seconds=0.0, check_every=CHECK_EVERY, chunks=CHUNKS,
                            blocks=0, **kw)


@pytest.fixture(scope="module")
def clean(native):
    """One small run per data type, shared and left unchanged."""
    return {dtype: _small(native, dtype) for dtype in DTYPES}


def _where(d):
    return (d["xcc"], d["se"], d["sh"], d["cu"])


# ---------------------------------------------------------------------------
# 1. what the loop leaves in the accumulators
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mfmas", [1, 2, 3, 33])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dump_matches_model(native, dtype, mfmas):
    """Would fail on an A that is never negated (an even count would not come
    back to C), a negation that misses elements or touches a scale, a chain
    that starts from something other than C, a count off by one, and a tile
    index other than (visit, wave, tile) (an unwritten element reads as NaN)."""
    for seed, visit in ((native.DEFAULT_SEED, 0), (SEED2, 7)):
        raw = native.debug_mfma_load_dump(0, dtype, mfmas, seed, visit)
        got = np.frombuffer(raw, dtype="<f4").reshape(WAVES, TILES, 16, 16)
        want = expected_dump(dtype, seed, visit, mfmas)
        assert not np.any(np.frombuffer(raw, dtype="<u4") == 0xFFFFFFFF)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        print(f"{dtype} mfmas {mfmas} seed {seed:#x} visit {visit}: {len(bad)} of "
              f"{want.size} elements differ, first {bad[:3].tolist()}")
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        # the data is no trivial fixed point: odd and even counts differ
        assert not np.array_equal(want, expected_dump(dtype, seed, visit, mfmas + 1))


# ---------------------------------------------------------------------------
# 2. a clean run
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_run(native, clean, dtype):
    r = clean[dtype]
    info = native.device_info(0)
    blocks = 4 * r["cu_total"]
    print(f"{dtype}: mfmas {r['mfmas']} elapsed_ms {r['elapsed_ms']:.3f} tflops "
          f"{r['tflops']:.1f} clock_mhz {r['clock_mhz']:.0f} (device max "
          f"{info['clock_mhz']}) cycles_per_mfma {r['cycles_per_mfma']:.2f} covered "
          f"{r['cu_covered']}/{r['cu_total']} slowest {r['slowest_cu']}")
    assert r["faulty"] == [] and r["ok"] is True and "record" not in r
    assert r["cu_total"] == info["multi_processor_count"]
    assert (r["blocks"], r["launches"], r["chunks"]) == (blocks, 1, CHUNKS)
    assert r["tiles_per_wave"] == TILES == native.MFMA_LOAD_TILES
    assert r["mfmas"] == blocks * WAVES * TILES * CHECK_EVERY * CHUNKS
    assert r["flop"] == r["mfmas"] * flop_per_mfma(dtype)
    assert native.flop_per_mfma(dtype) == flop_per_mfma(dtype)
    assert 1 <= r["cu_covered"] <= r["cu_total"]
    locations = r["locations"]
    assert len(locations) == r["cu_covered"]
    assert len({_where(l) for l in locations}) == len(locations)
    assert all(l["simd_seen"] == 0b1111 and l["visits"] >= 1 for l in locations)
    assert sum(l["visits"] for l in locations) == blocks
    assert 0 < r["clock_mhz"] <= info["clock_mhz"] * CLOCK_MARGIN
    assert r["cycles_per_mfma"] > 0
    assert r["slowest_cu"]["cycles_per_mfma"] >= r["cycles_per_mfma"]
    assert r["elapsed_ms"] > 0
    assert r["tflops"] == pytest.approx(r["flop"] / (r["elapsed_ms"] * 1e-3) / 1e12, rel=1e-12)


# ---------------------------------------------------------------------------
# 3. a seeded accumulator fault
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_fault_is_found_once_and_where_it_ran(native, clean, dtype):
    """The sign bit of a non-zero accumulator in the middle of chunk 1 of 4:
    the error is a whole number of units, so it stays until the check at the
    end of that chunk. One bad element and no more: the reset to C at the chunk
    boundary keeps chunks 2 and 3 clean."""
    visit, chunk, after = 5, 1, CHECK_EVERY // 2
    wave, tile, reg = nonzero_target(dtype, native.DEFAULT_SEED, visit, after)
    r = _small(native, dtype, inject_acc=(visit, wave, tile, chunk, after, reg, 0x80000000))
    rec = r["record"]
    print(f"{dtype}: inject wave {wave} tile {tile} reg {reg}; record {rec}; faulty {r['faulty']}")
    assert rec is not None and len(set(rec["simd"])) == WAVES
    assert r["faulty"] == [{"xcc": rec["xcc"], "se": rec["se"], "sh": rec["sh"],
                            "cu": rec["cu"], "simd": rec["simd"][wave], "dtype": dtype,
                            "bad_elements": 1}]
    assert r["ok"] is False
    assert r["mfmas"] == clean[dtype]["mfmas"]
    assert clean[dtype]["faulty"] == [] and clean[dtype]["ok"] is True


def test_seeded_fault_in_the_last_mfma_and_chunk(native):
    """The hook's corner: the last MFMA of the last chunk, the last wave and
    tile, found by the check that follows it."""
    visit, chunk, after = 0, CHUNKS - 1, CHECK_EVERY - 1
    acc = accumulator_after_mfma("bf16", SEED2, tile_index(visit, WAVES - 1, TILES - 1), after)
    reg = int(np.flatnonzero(acc[:4, 0])[0])
    r = native.mfma_load(0, "bf16", seconds=0.0, check_every=CHECK_EVERY, chunks=CHUNKS,
                         blocks=2, seed=SEED2,
                         inject_acc=(visit, WAVES - 1, TILES - 1, chunk, after, reg, 0x80000000))
    assert [(f["simd"], f["bad_elements"]) for f in r["faulty"]] == [
        (r["record"]["simd"][WAVES - 1], 1)]


# ---------------------------------------------------------------------------
# 4. the floor, the timed mode, bad arguments
# ---------------------------------------------------------------------------
def test_floor_gates_ok_alone(native):
    low = _small(native, "bf16", floor_tflops=1e9)
    assert low["ok"] is False and low["faulty"] == [] and low["floor_tflops"] == 1e9
    assert _small(native, "bf16", floor_tflops=0.0)["ok"] is True


def test_timed_run_lasts_as_long_as_asked(native):
    r = native.mfma_load(0, "bf16", seconds=0.2, launch_ms=20.0)
    print(f"elapsed_ms {r['elapsed_ms']:.2f} launches {r['launches']} chunks {r['chunks']} "
          f"tflops {r['tflops']:.1f} clock_mhz {r['clock_mhz']:.0f} cycles_per_mfma "
          f"{r['cycles_per_mfma']:.2f}")
    assert r["faulty"] == [] and r["launches"] >= 1
    assert 200.0 <= r["elapsed_ms"] <= 200.0 + DURATION_MARGIN_MS


@pytest.mark.parametrize("kwargs", [
    dict(check_every=32), dict(check_every=0), dict(check_every=4097),
    dict(seconds=60.5), dict(seconds=-1.0), dict(device=64), dict(device=-1),
    dict(dtype="fp4"), dict(blocks=(1 << 14) + 1), dict(blocks=-1), dict(chunks=0),
    dict(chunks=1 << 24), dict(launch_ms=0.0), dict(floor_tflops=-1.0),
    dict(inject_acc=(0, WAVES, 0, 0, 0, 0, 1)), dict(inject_acc=(0, 0, TILES, 0, 0, 0, 1)),
    dict(inject_acc=(0, 0, 0, CHUNKS, 0, 0, 1)), dict(inject_acc=(0, 0, 0, 0, CHECK_EVERY, 0, 1)),
    dict(inject_acc=(0, 0, 0, 0, 0, 4, 1)), dict(inject_acc=(0, 0, 0, 0, 0, 0, 0)),
    dict(inject_acc=(0, 0, 0, 0, 0, 0, 1 << 32)), dict(inject_acc=(-1, 0, 0, 0, 0, 0, 1)),
    dict(inject_acc=(8, 0, 0, 0, 0, 0, 1), blocks=8),
    dict(inject_acc=(0, 0, 0, 0, 0, 0, 1), seconds=0.1),
])
def test_bad_arguments_raise_value_error(native, kwargs):
    args = dict(device=0, dtype="bf16", seconds=0.0, check_every=CHECK_EVERY, chunks=CHUNKS,
                blocks=4)
    args.update(kwargs)
    with pytest.raises(ValueError):
        native.mfma_load(**args)


def test_bad_dump_arguments_raise_value_error(native):
    for kwargs in (dict(mfmas=0), dict(mfmas=4096), dict(visit=-1), dict(visit=1 << 32),
                   dict(dtype="int8"), dict(device=64)):
        with pytest.raises(ValueError):
            native.debug_mfma_load_dump(**kwargs)
