"""The MFMA load's loop on the device: how many MFMAs it issues, where its
test hook sits, and what the timed mode counts.

``tflops``, the TFLOP/s floor and ``ok`` all rest on the count the kernel
asserts about itself (tiles x check_every x chunks per wave). The alternating
chain pins only the parity of what the loop really issued, so:

a. ``debug_mfma_load_dump(alternate=False)`` runs the same loop with +A in
   both operand sets and leaves C + n·A·B, compared bit for bit with
   ``expected_sum_after`` at counts on every side of the unrolled trip, the
   remainder loop and the tail;
b. the alternating dump at the same boundaries, and at visits whose tile
   index wraps in 32 bits;
c. a sign flip seeded after every single MFMA position of a chunk is found
   once each (a position that does not exist finds nothing, one that exists
   twice flips back);
d. every single-bit flip right before the check is found: the compare is
   exact;
e. the timed mode's ``mfmas``, ``visits`` and ``launches`` agree, with and
   without the calibration launch;
f. the claimed count against the waves' own cycle stamps: a loop that issues
   fewer MFMAs than it counts reads below the 16 cycles an MFMA takes;
g. ``health._mfma_load`` on the device against the shipped floors.

A seeded fault is an xor the kernel applies to one of its own accumulator
registers before its own compare: it makes a comparison fail and provokes no
device fault. Every data comparison is exact. Every launch is under a
millisecond but those of the timed tests (e: 50 and 20 ms, g: 1 s in all).
"""
import numpy as np
import pytest

from gpuhealth_model import DTYPES
from mfma_load_model import (TILES, WAVES, bit_flip_target, expected_dump, expected_sum_dump,
                             flop_per_mfma, nonzero_target, tile_index)

pytestmark = pytest.mark.gpu

SEED2 = 0x0BADC0DE
# pairs = (n - 1) // 2 go through trips of 8 and a remainder loop, an even n
# adds a tail MFMA: no pair (1), tail only (2), remainder only (3, 15),
# remainder and tail (16), exactly one trip (17), trip and tail (18), trip and
# remainder (19, 33: two trips), two trips and a remainder (35), production's
# 14 trips and 7 remainder pairs (239), the longest chunk (4095, and 4094 with
# a tail)
COUNTS = (1, 2, 3, 15, 16, 17, 18, 19, 33, 35, 239)
LONG_COUNTS = (4094, 4095)  # MXFP4's same-sign sums are not exact there (the model asserts)
INTEGER_DTYPES = ("bf16", "f16", "fp8")
SIGN = 0x80000000

# test_cycles_per_mfma: cycles_per_mfma of mfma_load(seconds=0,
# check_every=4095, chunks=4, blocks=0), one launch of some 0.5 ms.
# The lower bound is the issue cost of a back-to-back 16x16 MFMA from one wave
# of a SIMD, 16 cycles; docs/benchmarks.md ("MFMA load") has 16.28 at this
# check_every for bf16, f16 and fp8 and 16.41 for MXFP4 from runs of 0.4 s.
# A loop of seven pairs a trip that counts eight would read 14.2.
CYCLES_PER_MFMA_MIN = 16.0
# The upper bound: the largest measured value plus three times the spread
# seen. Measured at this shape on an MI355X (docs/benchmarks.md, "MFMA load",
# cycles per MFMA at the test's shape): two rounds of seven runs per data type
# in one process after a 0.2 s warm-up, at clocks from 1896 to 2420 MHz, and
# this test's own cold run in another process.
#   bf16   16.2832, then 13 times 16.2829        (cold 16.283)
#   f16    14 times 16.2813                      (cold 16.281)
#   fp8    16.2800 to 16.2822                    (cold 16.282)
#   mxfp4  14 times 16.4165                      (cold 16.416)
# Within f16 and within MXFP4 the runs do not differ in the fourth decimal, so
# a spread per data type would leave no room at all. The spread taken is that
# of the three types that run the same loop around a 16x16x32 MFMA, taken
# together: 16.2832 - 16.2800 = 0.0032. The bounds are the largest value of
# that group, and MXFP4's, plus 3 x 0.0032: 16.2928 and 16.4261, that is 0.013
# and 0.016 above the 16.28 and 16.41 of docs/benchmarks.md (runs of 0.4 s on
# other nodes). The slowest single CU of any run read 16.2904 (MXFP4 16.4189).
CYCLES_PER_MFMA_MAX = {"bf16": 16.2928, "f16": 16.2928, "fp8": 16.2928, "mxfp4": 16.4261}


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


def _seeds_and_visits(native):
    return ((native.DEFAULT_SEED, 0), (SEED2, 7))


def _dump(native, dtype, mfmas, seed, visit, alternate):
    raw = native.debug_mfma_load_dump(0, dtype, mfmas, seed, visit, alternate=alternate)
    assert not np.any(np.frombuffer(raw, dtype="<u4") == 0xFFFFFFFF)  # every element written
    return np.frombuffer(raw, dtype="<f4").reshape(WAVES, TILES, 16, 16)


def _assert_same_bits(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    print(f"{what}: {len(bad)} of {want.size} elements differ, first {bad[:3].tolist()}")
    if len(bad):
        w, t, r, c = bad[0]
        print(f"  got {got[w, t, r, c]!r} want {want[w, t, r, c]!r}")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


# ---------------------------------------------------------------------------
# a. the count of MFMAs the loop issues
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mfmas", [(d, n) for d in DTYPES for n in COUNTS]
                         + [(d, n) for d in INTEGER_DTYPES for n in LONG_COUNTS])
def test_issued_count_bit_for_bit(native, dtype, mfmas):
    """C + n·A·B names n: would fail on an unrolled trip of seven pairs, a
    remainder loop or a tail that is missing or runs twice, and a skipped
    trip, none of which the alternating chain can see at an unchanged parity."""
    for seed, visit in _seeds_and_visits(native):
        want = expected_sum_dump(dtype, seed, visit, mfmas)
        # the model tells n from n - 1 and n + 1 (and so from n - 2), in every tile
        for other in (mfmas - 1, mfmas + 1):
            if other >= 1:
                near = expected_sum_dump(dtype, seed, visit, other)
                assert all(not np.array_equal(want[w, t], near[w, t])
                           for w in range(WAVES) for t in range(TILES))
        got = _dump(native, dtype, mfmas, seed, visit, alternate=False)
        _assert_same_bits(got, want, f"{dtype} +A only, mfmas {mfmas} seed {seed:#x} "
                                     f"visit {visit}")


# ---------------------------------------------------------------------------
# b. the alternating chain at the loop's boundaries, and wrapping tile indices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mfmas", [15, 16, 17, 18, 19, 35, 239, 4094, 4095])
@pytest.mark.parametrize("dtype", DTYPES)
def test_alternating_dump_at_the_loop_boundaries(native, dtype, mfmas):
    for seed, visit in _seeds_and_visits(native):
        got = _dump(native, dtype, mfmas, seed, visit, alternate=True)
        _assert_same_bits(got, expected_dump(dtype, seed, visit, mfmas),
                          f"{dtype} alternating, mfmas {mfmas} seed {seed:#x} visit {visit}")
        # alternate=True is the default
        raw = native.debug_mfma_load_dump(0, dtype, mfmas, seed, visit)
        assert np.array_equal(np.frombuffer(raw, dtype="<f4"), got.ravel())


@pytest.mark.parametrize("visit,same_tiles_as", [((1 << 32) - 1, None), ((1 << 28) + 3, 3)])
def test_tile_index_wraps_in_32_bits(native, visit, same_tiles_as):
    """(visit x 4 + wave) x 4 + tile passes 2^32 at these visits: the device's
    uint32 arithmetic and the model's mask have to agree. 2^28 + 3 lands on
    the tiles of visit 3; 2^32 - 1 ends on tile index 2^32 - 1, whose hash
    input (index + 1) wraps as well."""
    assert all(tile_index(visit, w, t) < 1 << 32 for w in range(WAVES) for t in range(TILES))
    assert visit * WAVES * TILES >= 1 << 32
    assert tile_index((1 << 32) - 1, WAVES - 1, TILES - 1) == (1 << 32) - 1
    for mfmas in (17, 18, 239):
        for alternate, model in ((True, expected_dump), (False, expected_sum_dump)):
            got = _dump(native, "bf16", mfmas, SEED2, visit, alternate=alternate)
            _assert_same_bits(got, model("bf16", SEED2, visit, mfmas),
                              f"bf16 visit {visit:#x} mfmas {mfmas} alternate {alternate}")
            if same_tiles_as is not None:
                other = _dump(native, "bf16", mfmas, SEED2, same_tiles_as, alternate=alternate)
                assert np.array_equal(got.view(np.uint32), other.view(np.uint32))


# ---------------------------------------------------------------------------
# c. every hook point exists once
# ---------------------------------------------------------------------------
def _flip_is_found_once(native, dtype, check_every, chunks, visit, chunk, after):
    """A sign flip of a non-zero accumulator is a whole number of units: it
    stays until the check at the end of its chunk. Found once, one element,
    on the SIMD the faulted workgroup recorded for that wave. A hook that is
    missing finds nothing; one that sits at two places flips back."""
    seed = SEED2
    wave, tile, reg = nonzero_target(dtype, seed, visit, after, first=after)
    r = native.mfma_load(0, dtype, seconds=0.0, check_every=check_every, chunks=chunks,
                         blocks=2, seed=seed,
                         inject_acc=(visit, wave, tile, chunk, after, reg, SIGN))
    rec = r["record"]
    print(f"{dtype} check_every {check_every} chunk {chunk} after {after}: wave {wave} tile "
          f"{tile} reg {reg}; record {rec}; faulty {r['faulty']}")
    assert rec is not None and len(set(rec["simd"])) == WAVES
    assert r["faulty"] == [{"xcc": rec["xcc"], "se": rec["se"], "sh": rec["sh"],
                            "cu": rec["cu"], "simd": rec["simd"][wave], "dtype": dtype,
                            "bad_elements": 1}]
    assert r["ok"] is False
    assert r["mfmas"] == 2 * WAVES * TILES * check_every * chunks


@pytest.mark.parametrize("after", range(35))
def test_every_hook_point_exists_once_bf16(native, after):
    """check_every 35: the first MFMA, two unrolled trips (positions 1 to 32)
    and one remainder pair (33 and 34)."""
    _flip_is_found_once(native, "bf16", 35, 3, visit=after % 2, chunk=after % 3, after=after)


@pytest.mark.parametrize("after", [0, 1, 2, 31, 32, 33, 34])
@pytest.mark.parametrize("dtype", ["f16", "fp8", "mxfp4"])
def test_hook_points_at_the_ends_of_the_unrolled_part(native, dtype, after):
    _flip_is_found_once(native, dtype, 35, 3, visit=after % 2, chunk=after % 3, after=after)


@pytest.mark.parametrize("after", [0, 223, 224, 225, 237, 238])
def test_hook_points_of_the_production_chunk(native, after):
    """check_every 239: 119 pairs, 14 unrolled trips (positions 1 to 224) and
    7 remainder pairs (225 to 238); in chunk 1 of 2."""
    _flip_is_found_once(native, "fp8", 239, 2, visit=1, chunk=1, after=after)


# ---------------------------------------------------------------------------
# d. the compare at the check point is exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "mxfp4"])
def test_every_single_bit_flip_before_the_check_is_found(native, dtype):
    """An error below one unit can be rounded away by the MFMAs that follow it
    inside a chunk; at the check itself nothing follows, and any bit counts."""
    check_every, chunks, visit = 33, 2, 1
    after = check_every - 1
    wave, tile, reg = bit_flip_target(dtype, SEED2, visit, after, first=5)
    found = {}
    for bit in range(32):
        r = native.mfma_load(0, dtype, seconds=0.0, check_every=check_every, chunks=chunks,
                             blocks=2, seed=SEED2,
                             inject_acc=(visit, wave, tile, chunks - 1, after, reg, 1 << bit))
        found[bit] = [(f["simd"], f["bad_elements"]) for f in r["faulty"]]
        assert r["record"] is not None
        assert found[bit] == [(r["record"]["simd"][wave], 1)], (bit, found[bit])
    print(f"{dtype}: wave {wave} tile {tile} reg {reg}: {found}")


# ---------------------------------------------------------------------------
# e. what the timed mode counts
# ---------------------------------------------------------------------------
def _assert_covered_and_clean(r):
    assert r["faulty"] == []
    assert len(r["locations"]) == r["cu_covered"] >= 1
    assert all(l["simd_seen"] == 0b1111 for l in r["locations"])
    assert sum(l["visits"] for l in r["locations"]) == r["launches"] * r["blocks"]
    assert r["flop"] == r["mfmas"] * flop_per_mfma(r["dtype"])


def test_timed_run_counts_the_calibration_launch_as_it_ran(native):
    """chunks left at 0: a first launch of CALIBRATION // check_every chunks
    sizes the others. Every launch counts with the chunks it ran with."""
    check_every = 33
    r = native.mfma_load(0, "bf16", seconds=0.05, launch_ms=5.0, check_every=check_every)
    cal = max(1, native.MFMA_LOAD_CALIBRATION_MFMAS // check_every)
    per_chunk = r["blocks"] * WAVES * TILES * check_every
    print(f"launches {r['launches']} blocks {r['blocks']} chunks {r['chunks']} calibration "
          f"chunks {cal} mfmas {r['mfmas']} = {per_chunk} x {r['mfmas'] / per_chunk} "
          f"elapsed_ms {r['elapsed_ms']:.2f}")
    assert r["launches"] >= 2 and r["chunks"] >= 1 and r["blocks"] == 4 * r["cu_total"]
    assert r["mfmas"] == per_chunk * (cal + (r["launches"] - 1) * r["chunks"])
    _assert_covered_and_clean(r)
    assert r["elapsed_ms"] >= 50.0


def test_timed_run_with_given_chunks_has_no_calibration_launch(native):
    check_every, chunks, blocks = 33, 64, 8
    r = native.mfma_load(0, "bf16", seconds=0.02, check_every=check_every, chunks=chunks,
                         blocks=blocks)
    print(f"launches {r['launches']} mfmas {r['mfmas']} elapsed_ms {r['elapsed_ms']:.2f}")
    assert r["launches"] >= 1 and (r["chunks"], r["blocks"]) == (chunks, blocks)
    assert r["mfmas"] == r["launches"] * blocks * WAVES * TILES * check_every * chunks
    _assert_covered_and_clean(r)
    assert r["elapsed_ms"] >= 20.0


# ---------------------------------------------------------------------------
# f. the claimed count against the cycle stamps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_cycles_per_mfma(native, dtype):
    """The production kernel at its longest chunk. The bounds are constants
    (above), not figures of this run."""
    r = native.mfma_load(0, dtype, seconds=0.0, check_every=4095, chunks=4, blocks=0)
    print(f"{dtype}: cycles_per_mfma {r['cycles_per_mfma']:.3f} (bounds {CYCLES_PER_MFMA_MIN} "
          f"to {CYCLES_PER_MFMA_MAX[dtype]}) clock_mhz {r['clock_mhz']:.0f} slowest "
          f"{r['slowest_cu']} elapsed_ms {r['elapsed_ms']:.3f}")
    assert r["faulty"] == [] and r["launches"] == 1
    assert r["mfmas"] == r["blocks"] * WAVES * TILES * 4095 * 4
    assert r["cycles_per_mfma"] >= CYCLES_PER_MFMA_MIN
    assert r["cycles_per_mfma"] <= CYCLES_PER_MFMA_MAX[dtype]


# ---------------------------------------------------------------------------
# g. the probe's own call, against the shipped floors
# ---------------------------------------------------------------------------
def test_health_mfma_load_on_the_device(native):
    from kuberay_amd.gpu import health
    floors = dict(health.DEFAULT_MFMA_FLOOR_TFLOPS)
    health._mfma_load(native, 0, 0.2, floors)  # warm-up
    ok, tflops, clock, faulty, problems = health._mfma_load(native, 0, 0.8, floors)
    print(f"tflops {tflops} clock_mhz {clock} floors {floors} problems {problems}")
    assert tuple(ok) == tuple(tflops) == tuple(clock) == health.MFMA_LOAD_DTYPES == DTYPES
    assert problems == [] and faulty == []
    assert all(ok.values())
    for dtype in DTYPES:
        assert tflops[dtype] >= floors[dtype]
        assert clock[dtype] > 0
