"""The burn-in probe's kernels against references that share no code with them.

The sweep's fill and verify kernels both call the device build of
``gh::pattern_word`` and the MFMA check kernel calls the device build of
``reference_element``, so a mistake made on the device is made on both sides.
Here the other side is tests/gpuhealth_model.py (Python and numpy) and the host
build of the reference:

* GPU (``@pytest.mark.gpu``): what the fill leaves in memory, word for word,
  with pattern indices below, across and far above 2^32; the verify's counters
  for many mismatches per lane, wave, block, grid-stride step, chunk, phase and
  pass; the stream kernel's copy and its upper bound; 64 MFMA tiles per data
  type bit for bit; the MFMA check's counters.
* CPU: the numpy pattern against the scalar one and the host binding; the
  unhealthy path of the Python gate and of ``probe --deep``; which operand bits
  the generators toggle; whether the generated data exposes each routing fault
  the probe claims to catch.

Every comparison is exact. A seeded corruption is a host write inside a live
allocation: it makes a comparison fail and provokes no fault.
"""
import json
import math
import struct
import types

import numpy as np
import pytest

import gpuhealth_model as model
from gpuhealth_model import DTYPES, pattern_word, pattern_words

MIB = 1 << 20
SEED2 = 0x0BADC0DE
HIGH_BASES = [0, (1 << 32) - 8, (5 << 32) + 12345, (1 << 36) + 3]
GRID_THREADS = 4096 * 256          # the sweep's and the stream kernel's grid


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


# ---------------------------------------------------------------------------
# CPU: the model itself
# ---------------------------------------------------------------------------
def test_pattern_words_matches_scalar_and_native(native):
    for seed in (native.DEFAULT_SEED, SEED2, 0, 0xFFFFFFFF):
        for start in HIGH_BASES + [(1 << 64) - 300]:
            got = pattern_words(seed, start, 300)
            assert got.dtype == np.uint32 and got.shape == (300,)
            for j in (0, 1, 7, 8, 9, 150, 299):
                assert int(got[j]) == pattern_word(seed, start + j), (seed, start, j)
                assert int(got[j]) == native.pattern_word(seed, start + j), (seed, start, j)
    # the low half wraps inside this window and the high half must count
    w = pattern_words(native.DEFAULT_SEED, (1 << 32) - 8, 16)
    assert int(w[8]) == pattern_word(native.DEFAULT_SEED, 1 << 32)
    assert int(w[8]) != pattern_word(native.DEFAULT_SEED, 0)
    assert len(set(w.tolist())) == 16


def test_elem_hash_grid_matches_scalar():
    for dtype in DTYPES:
        for which in (model.GEN_A, model.GEN_SB):
            grid = model.elem_hash_grid(SEED2, 1023, dtype, which, 16, 128)
            for i, k in ((0, 0), (3, 17), (15, 127), (8, 32)):
                assert int(grid[i, k]) == model.elem_hash(SEED2, 1023, dtype, which, i, k)


def test_encoders_agree_with_independent_decoders():
    """Every integer the generators emit survives encode -> decode, with the
    decoders taken from numpy (f16), the bit layout (bf16) and the OCP
    definition (e4m3), not from the encoders."""
    for v in range(-8, 9):
        assert model.bf16_to_f32(model.f32_to_bf16(float(v))) == v
        assert model.f16_to_f32(model.f32_to_f16(float(v))) == v
        assert model.f32_to_f16(float(v)) == int(np.array([v], np.float16).view(np.uint16)[0])
        assert model.e4m3_to_f32(model.f32_to_e4m3(float(v))) == v
    assert model.f32_to_e4m3(448.0) == 0x7E and model.e4m3_to_f32(0x7E) == 448.0
    assert math.isnan(model.e4m3_to_f32(0x7F))


# ---------------------------------------------------------------------------
# CPU: what the operands exercise
# ---------------------------------------------------------------------------
def _toggled(codes, width):
    """Bit positions that take both values over the codes."""
    codes = np.asarray(codes, dtype=np.uint64).ravel()
    ones = int(np.bitwise_or.reduce(codes))
    zeros = int(np.bitwise_or.reduce(~codes & np.uint64((1 << width) - 1)))
    return ones & zeros


def _operand_codes(dtype, seed, tiles):
    """Every A and B operand code of the tiles, as the kernel encodes them."""
    table = {v: model.ENCODE[dtype](float(v)) for v in range(-8, 9)}
    out = []
    for wg in tiles:
        for which in (model.GEN_A, model.GEN_B):
            ints = ((model.elem_hash_grid(seed, wg, dtype, which, 16, 32) >> np.uint64(8))
                    % np.uint64(17)).astype(np.int64) - 8
            out.append(np.vectorize(table.__getitem__)(ints))
    return np.concatenate(out, axis=None)


@pytest.mark.parametrize("dtype,width,mask", [("bf16", 16, 0xFFE0), ("f16", 16, 0xFF00),
                                               ("fp8", 8, 0xFE)])
def test_operand_bits_toggled(native, dtype, width, mask):
    """Integers in [-8, 8] toggle the sign, every exponent bit and the top two
    mantissa bits. The low mantissa bits stay 0 in every operand, so a
    stuck-at-0 fault there is outside what the data can show."""
    codes = _operand_codes(dtype, native.DEFAULT_SEED, range(64))
    assert _toggled(codes, width) == mask
    assert int(np.bitwise_or.reduce(codes.astype(np.uint64))) & ~mask == 0
    # the vectorised generator is the scalar one
    assert int(codes[0]) == model.ENCODE[dtype](
        float(model.gen_int(native.DEFAULT_SEED, 0, dtype, model.GEN_A, 0, 0)))


def test_operand_bits_toggled_mxfp4(native):
    seed = native.DEFAULT_SEED
    fp4, scales = [], []
    for wg in range(64):
        for which in (model.GEN_A, model.GEN_B):
            fp4.append((model.elem_hash_grid(seed, wg, "mxfp4", which, 16, 128)
                        >> np.uint64(8)) & np.uint64(15))
        for which in (model.GEN_SA, model.GEN_SB):
            scales.append(np.uint64(126) + (model.elem_hash_grid(seed, wg, "mxfp4", which, 16, 4)
                                            >> np.uint64(8)) % np.uint64(3))
    assert _toggled(np.concatenate(fp4, axis=None), 4) == 0xF
    assert _toggled(np.concatenate(scales, axis=None), 8) == 0xFF
    assert int(fp4[0][2, 5]) == model.gen_fp4_code(seed, 0, model.GEN_A, 2, 5)
    assert int(scales[1][7, 3]) == model.gen_scale_code(seed, 0, model.GEN_SB, 7, 3)


# ---------------------------------------------------------------------------
# CPU: routing sensitivity of the data (tests the generators, not the device)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wg", [0, 1, 1023])
def test_data_exposes_routing_faults(native, dtype, wg):
    """Packs the operands into per-lane registers by the documented lane maps.
    The right unpacking gives the host reference; each single wrong one gives a
    different D, so the device's exact check would see that fault."""
    seed = native.DEFAULT_SEED
    regs = model.pack_registers(dtype, seed, wg)
    ref = np.array(native.reference_tile(dtype, seed, wg), dtype=np.float64)
    assert np.array_equal(model.tile_from_registers(dtype, regs), ref)
    faults = model.FAULTS_ALL + (model.FAULTS_MXFP4 if dtype == "mxfp4" else ())
    for fault in faults:
        wrong = model.tile_from_registers(dtype, regs, fault)
        assert not np.array_equal(wrong, ref), f"{dtype} tile {wg}: {fault} does not show"


def test_fp4_only_faults_do_nothing_elsewhere():
    """The three FP4 faults are wired to the FP4 path only: elsewhere they
    leave D alone, so the loop above does not pass by accident."""
    regs = model.pack_registers("bf16", 7, 0)
    right = model.tile_from_registers("bf16", regs)
    for fault in model.FAULTS_MXFP4:
        assert np.array_equal(model.tile_from_registers("bf16", regs, fault), right)


# ---------------------------------------------------------------------------
# CPU: the unhealthy path of the Python gate and of `probe --deep`
# ---------------------------------------------------------------------------
CLEAN_PATTERN = {"bytes_checked": 1 << 30, "chunks": 1, "mismatched_words": 0,
                 "flipped_bits": 0, "bad_bit_mask": 0, "first_bad_offset": -1, "gb_s": 3000.0}
BAD_PATTERN = dict(CLEAN_PATTERN, mismatched_words=3, flipped_bits=17,
                   bad_bit_mask=0x00010004, first_bad_offset=4096)
BAD_TILE = (517, 9, 3, 12.5, 13.0)


def _burn_in_result(bad_dtype=None, pattern=CLEAN_PATTERN):
    exact = {d: d != bad_dtype for d in DTYPES}
    pattern_ok = pattern["mismatched_words"] == 0
    return {"mfma_ok": True, "hbm_gb_s": 4000.0, "hbm_ok": True,
            "mfma_exact": exact,
            "mfma_first_bad": {d: (None if ok else BAD_TILE) for d, ok in exact.items()},
            "hbm_pattern_ok": pattern_ok, "hbm_pattern": dict(pattern),
            "healthy": all(exact.values()) and pattern_ok}


def _fake_gate(monkeypatch, result, devices=1, smi_raises=False):
    from kuberay_amd.gpu import health, rocm_smi
    calls = []

    def burn_in(device, hbm_fraction, hbm_floor_gb_s):
        calls.append((device, hbm_fraction, hbm_floor_gb_s))
        return result

    def get_gpu_stats():
        if smi_raises:
            raise RuntimeError("rocm-smi: no response")
        return [{"gpu": 0}]
    fake = types.SimpleNamespace(device_count=lambda: devices, burn_in=burn_in)
    monkeypatch.setattr(health, "gpu_node", lambda: True)
    monkeypatch.setattr(health, "_load_native", lambda: fake)
    monkeypatch.setattr(rocm_smi, "get_gpu_stats", get_gpu_stats)
    return calls


GATE_CASES = {
    # name: (bad dtype, pattern, devices, smi raises, what detail must name)
    "mfma": ("fp8", CLEAN_PATTERN, 1, False,
             ["mfma fp8", "tile 517", "[9][3]", "got 12.5", "expected 13.0"]),
    "pattern": (None, BAD_PATTERN, 1, False,
                ["3 bad words", "17 flipped bits", "0x00010004", "first bad offset 4096"]),
    "both": ("mxfp4", BAD_PATTERN, 1, False,
             ["mfma mxfp4", "tile 517", "[9][3]", "got 12.5", "expected 13.0",
              "3 bad words", "17 flipped bits", "0x00010004", "first bad offset 4096"]),
    "rocm_smi": (None, CLEAN_PATTERN, 1, True, ["rocm-smi did not respond"]),
    "no_device": (None, CLEAN_PATTERN, 0, False, ["device 0 not visible to HIP"]),
}


@pytest.mark.parametrize("case", sorted(GATE_CASES))
def test_burn_in_gate_unhealthy(monkeypatch, capsys, case):
    from kuberay_amd.gpu import health, probe
    bad_dtype, pattern, devices, smi_raises, named = GATE_CASES[case]
    calls = _fake_gate(monkeypatch, _burn_in_result(bad_dtype, pattern), devices, smi_raises)

    report = health.check_gpu_burn_in()
    assert report.healthy is False
    for text in named:
        assert text in report.detail, (text, report.detail)
    assert report.rocm_smi_ok is (not smi_raises)
    if devices:
        assert calls == [(0, health.DEFAULT_BURN_IN_HBM_FRACTION, health.DEFAULT_HBM_FLOOR_GB_S)]
        assert report.mfma_exact == {d: d != bad_dtype for d in DTYPES}
        assert report.hbm_pattern_ok is (pattern is CLEAN_PATTERN)
        assert report.hbm_flipped_bits == pattern["flipped_bits"]
        assert report.hbm_bytes_checked == 1 << 30
        # only what failed is named
        assert ("hbm pattern" in report.detail) == (pattern is BAD_PATTERN)
        assert ("mfma " in report.detail) == (bad_dtype is not None)
        assert ("rocm-smi" in report.detail) == smi_raises
    else:
        assert calls == [] and report.mfma_exact is None and report.hbm_pattern_ok is None

    capsys.readouterr()
    assert probe.main(["--deep", "--json"]) == 1
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["healthy"] is False
    assert out["detail"] == report.detail
    assert out["rocm_smi_ok"] is report.rocm_smi_ok
    assert out["mfma_exact"] == report.mfma_exact
    assert out["hbm_pattern_ok"] == report.hbm_pattern_ok
    assert out["hbm_bytes_checked"] == report.hbm_bytes_checked
    assert out["hbm_flipped_bits"] == report.hbm_flipped_bits
    assert out["mfma_ok"] == report.mfma_ok and out["hbm_gb_s"] == report.hbm_gb_s

    # without --json the detail goes to stderr and the exit code is the same
    assert probe.main(["--deep"]) == 1
    assert report.detail in capsys.readouterr().err


def test_burn_in_gate_fake_healthy(monkeypatch, capsys):
    """The same fake with nothing wrong is healthy: the cases above fail for
    the reason they name."""
    from kuberay_amd.gpu import health, probe
    _fake_gate(monkeypatch, _burn_in_result())
    report = health.check_gpu_burn_in()
    assert report.healthy is True and report.detail == ""
    assert probe.main(["--deep", "--json"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["healthy"] is True


# ---------------------------------------------------------------------------
# GPU: what the fill leaves in memory
# ---------------------------------------------------------------------------
FILL_SIZES = [16,                 # one vector
              4096 + 16,          # a partial second block
              16 * MIB + 16]      # n_vec = grid + 1: one thread takes a second step
FILL_CASES = [(n, b, None) for n in FILL_SIZES for b in HIGH_BASES]
FILL_CASES += [(4096 + 16, (1 << 32) - 8, SEED2), (16 * MIB + 16, (5 << 32) + 12345, SEED2)]


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes,base,seed", FILL_CASES)
def test_fill_matches_reference(native, nbytes, base, seed):
    """Would fail on a wrong .x/.y/.z/.w order, a truncated 64-bit index, an
    ignored invert_mask, a skipped or repeated grid-stride step."""
    seed = native.DEFAULT_SEED if seed is None else seed
    assert (nbytes // 16 > GRID_THREADS) == (nbytes == 16 * MIB + 16)
    expected = pattern_words(seed, base, nbytes // 4)
    plain = np.frombuffer(native.debug_pattern_fill(0, nbytes, seed, False, base), dtype="<u4")
    inverted = np.frombuffer(native.debug_pattern_fill(0, nbytes, seed, True, base), dtype="<u4")
    assert plain.shape == inverted.shape == expected.shape
    bad = np.flatnonzero(plain != expected)
    print(f"plain: {bad.size} of {expected.size} words differ, first {bad[:4]}")
    assert np.array_equal(plain, expected)
    bad = np.flatnonzero(inverted != (expected ^ np.uint32(0xFFFFFFFF)))
    print(f"inverted: {bad.size} of {expected.size} words differ, first {bad[:4]}")
    assert np.array_equal(inverted, expected ^ np.uint32(0xFFFFFFFF))
    # moving inversion: every bit of every word is driven to 0 and to 1
    assert np.array_equal(plain ^ inverted, np.full(expected.shape, 0xFFFFFFFF, np.uint32))


@pytest.mark.gpu
def test_fill_seed_and_base_matter(native):
    a = native.debug_pattern_fill(0, 4096, native.DEFAULT_SEED, False, 0)
    assert a != native.debug_pattern_fill(0, 4096, SEED2, False, 0)
    assert a != native.debug_pattern_fill(0, 4096, native.DEFAULT_SEED, False, 1 << 32)
    assert a == native.debug_pattern_fill(0, 4096)


@pytest.mark.gpu
def test_debug_hooks_reject_bad_arguments(native):
    for nbytes in (0, 8, 4096 + 4, 256 * MIB + 16):
        with pytest.raises(ValueError):
            native.debug_pattern_fill(0, nbytes)
    with pytest.raises(ValueError):
        native.debug_pattern_fill(0, 4096, base_word=(1 << 64) - 1)
    for nbytes in (0, 15, 256 * MIB + 16):
        with pytest.raises(ValueError):
            native.debug_stream_copy_check(0, nbytes)
    for wgs in (0, 4097):
        with pytest.raises(ValueError):
            native.debug_mfma_dump(0, "bf16", wgs)
    with pytest.raises(ValueError):
        native.debug_mfma_dump(0, "int8", 1)
    for bad in ((0, 64, "a", 0, 1), (0, -1, "b", 0, 1), (0, 0, "a", 4, 1), (0, 0, "c", 4, 1),
                (0, 0, "sb", 0, 1), (0, 0, "b", 0, 0), (0, 0, "b", 0, 1 << 32),
                (1, 0, "a", 0, 1), (-1, 0, "a", 0, 1), (0, 0, "d", 0, 1)):
        with pytest.raises(ValueError):
            native.debug_mfma_dump(0, "bf16", 1, inject_operand=bad)
    for dtype, bad in (("fp8", (0, 0, "a", 2, 1)), ("mxfp4", (0, 0, "a", 8, 1)),
                       ("mxfp4", (0, 0, "sa", 1, 1))):
        with pytest.raises(ValueError):
            native.debug_mfma_dump(0, dtype, 1, inject_operand=bad)


# ---------------------------------------------------------------------------
# GPU: the verify at pattern indices >= 2^32
# ---------------------------------------------------------------------------
def _assert_clean(r, nbytes):
    assert r["mismatched_words"] == 0 and r["flipped_bits"] == 0
    assert r["bad_bit_mask"] == 0 and r["first_bad_offset"] == -1
    assert r["bytes_checked"] == nbytes


def _assert_counts(r, corruptions):
    """The four counters, computed here from the corruption list."""
    print({k: r[k] for k in ("mismatched_words", "flipped_bits", "bad_bit_mask",
                             "first_bad_offset")})
    assert r["mismatched_words"] == len(corruptions)
    assert r["flipped_bits"] == sum(bin(m).count("1") for _, m in corruptions)
    mask = 0
    for _, m in corruptions:
        mask |= m
    assert r["bad_bit_mask"] == mask
    assert r["first_bad_offset"] == 4 * min(w for w, _ in corruptions)


@pytest.mark.gpu
@pytest.mark.parametrize("base", HIGH_BASES)
def test_verify_clean_at_high_indices(native, base):
    nbytes = 4096 + 16
    r = native.hbm_pattern_check(0, bytes=nbytes, base_word=base)
    _assert_clean(r, nbytes)
    # offsets stay relative to the sweep, whatever the base
    r = native.hbm_pattern_check(0, bytes=nbytes, base_word=base, corruptions=[(1027, 0x10)])
    _assert_counts(r, [(1027, 0x10)])


@pytest.mark.gpu
def test_verify_where_the_low_half_wraps(native):
    nbytes = 4096 + 16
    base = (1 << 32) - 8
    for word in (8, 7):            # pattern index 2^32 (lo == 0) and 2^32 - 1
        r = native.hbm_pattern_check(0, bytes=nbytes, base_word=base,
                                     corruptions=[(word, 1 << 31)])
        _assert_counts(r, [(word, 1 << 31)])
        assert r["first_bad_offset"] == 4 * word


# ---------------------------------------------------------------------------
# GPU: many mismatches through the reductions and the atomics
# ---------------------------------------------------------------------------
MULTI_BYTES = 32 * MIB + 16        # n_vec = 2 * grid + 1: up to three steps per thread
MULTI_WORDS = MULTI_BYTES // 4


def _w(vector, j=0):
    return 4 * vector + j


def _random_corruptions():
    rng = np.random.default_rng(20240607)
    words = rng.choice(MULTI_WORDS, size=200, replace=False)
    masks = rng.integers(1, 1 << 32, size=200, dtype=np.uint64)
    return [(int(w), int(m)) for w, m in zip(words, masks)]


MULTI_CASES = {
    "same_vector": [(_w(777, 0), 0x1), (_w(777, 3), 0x80000000)],
    "same_wave": [(_w(63, 2), 0x6), (_w(0, 1), 0x3000)],
    "same_block_other_wave": [(_w(64, 0), 0xF0), (_w(0, 3), 0x1)],
    "different_blocks": [(_w(256 * 4095 + 255, 1), 0x8), (_w(256 * 9 + 70, 2), 0x18),
                         (_w(5, 0), 0x10000)],
    # one thread meets all three on successive grid-stride steps; the last
    # vector is thread 0's third step
    "grid_stride_steps": [(_w(12345 + GRID_THREADS, 1), 0x4), (_w(12345, 2), 0x400),
                          (_w(2 * GRID_THREADS, 3), 0x40000)],
    "full_mask": [(_w(100000, 2), 0xFFFFFFFF), (_w(100001, 2), 0x1)],
    # the smallest word sits in lane 63 of block 300; the others in low lanes
    # of earlier blocks, one grid-stride step later
    "smallest_in_higher_lane_later_block": [
        (_w(GRID_THREADS + 256 * 5 + 1, 0), 0x2), (_w(256 * 300 + 63, 3), 0x20),
        (_w(GRID_THREADS + 256 * 10 + 2, 1), 0x200)],
    "random_200": _random_corruptions(),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(MULTI_CASES))
def test_verify_counts_many_mismatches(native, case):
    """Would fail on a sum that drops a lane, a min that keeps the wrong side,
    a wrong popcount, an atomic that overwrites instead of accumulating."""
    corruptions = MULTI_CASES[case]
    r = native.hbm_pattern_check(0, bytes=MULTI_BYTES, corruptions=corruptions)
    assert r["bytes_checked"] == MULTI_BYTES and r["chunks"] == 1
    _assert_counts(r, corruptions)


@pytest.mark.gpu
def test_verify_counts_across_chunks(native):
    corruptions = [(MULTI_WORDS - 1, 0x80), ((16 * MIB + 4096) // 4 + 1, 0x7), (5, 0x100)]
    r = native.hbm_pattern_check(0, bytes=MULTI_BYTES, max_chunk_mib=8, corruptions=corruptions)
    assert r["chunks"] == 5        # four of 8 MiB and the 16-byte tail
    _assert_counts(r, corruptions)
    # the smallest word is the one with the larger offset inside its chunk
    chunk_words = 8 * MIB // 4
    corruptions = [(3 * chunk_words + 10, 0x1), (chunk_words + 5000, 0x2)]
    r = native.hbm_pattern_check(0, bytes=MULTI_BYTES, max_chunk_mib=8, corruptions=corruptions)
    _assert_counts(r, corruptions)


@pytest.mark.gpu
def test_legacy_corrupt_word_is_one_corruption(native):
    a = native.hbm_pattern_check(0, bytes=4096, corrupt_word=9, corrupt_bit=5)
    b = native.hbm_pattern_check(0, bytes=4096, corruptions=[(9, 1 << 5)])
    _assert_counts(a, [(9, 1 << 5)])
    _assert_counts(b, [(9, 1 << 5)])
    c = native.hbm_pattern_check(0, bytes=4096, corrupt_word=9, corrupt_bit=5,
                                 corruptions=[(12, 0x3)])
    _assert_counts(c, [(9, 1 << 5), (12, 0x3)])


@pytest.mark.gpu
def test_corruption_arguments_are_checked(native):
    check = native.hbm_pattern_check
    for bad in ([(1024, 1)], [(-1, 1)], [(3, 0)], [(3, 1 << 32)], [(3, -1)],
                [(3, 1), (3, 2)]):
        with pytest.raises(ValueError):
            check(0, bytes=4096, corruptions=bad)
    with pytest.raises(ValueError):
        check(0, bytes=4096, corrupt_word=3, corruptions=[(3, 2)])
    for at in ((1, 0), (0, 2), (-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            check(0, bytes=4096, corruptions=[(3, 1)], corrupt_at=at)
    with pytest.raises(ValueError):
        check(0, bytes=4096, passes=2, corruptions=[(3, 1)], corrupt_at=(2, 0))
    with pytest.raises(ValueError):
        check(0, bytes=4096, base_word=(1 << 64) - 1024)
    for bad in ([(1024, 1, 0)], [(-1, 1, 0)], [(3, 0, 0)], [(3, 1 << 32, 1)], [(3, -1, 1)],
                [(3, 1, 2)], [(3, 1, -1)], [(3, 1, 0), (3, 2, 1)]):
        with pytest.raises(ValueError):
            check(0, bytes=4096, stuck=bad)
    with pytest.raises(ValueError):
        check(0, bytes=4096, corruptions=[(3, 1)], stuck=[(5, 1, 0), (1024, 1, 0)])
    for bad in ((0, 64, "a", 0, 1), (0, 0, "a", 4, 1), (0, 0, "sa", 0, 1), (0, 0, "a", 0, 0),
                (0, 0, "a", 0, 1 << 32), (4, 0, "a", 0, 1), (0, 0, "e", 0, 1)):
        with pytest.raises(ValueError):
            native.mfma_verify(0, "bf16", workgroups=4, inject_operand=bad)
    for bad in ([(4 * 256, 1)], [(-1, 1)], [(3, 0)], [(3, 1 << 32)], [(3, 1), (3, 2)]):
        with pytest.raises(ValueError):
            native.mfma_verify(0, "bf16", workgroups=4, corruptions=bad)
    with pytest.raises(ValueError):
        native.mfma_verify(0, "bf16", workgroups=4, corrupt_element=3, corruptions=[(3, 2)])


# ---------------------------------------------------------------------------
# GPU: the inverted phase and later passes detect too
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("passes,at", [(1, (0, 0)), (1, (0, 1)), (2, (1, 0)), (2, (1, 1)),
                                        (2, (0, 1))])
def test_every_phase_and_pass_detects(native, passes, at):
    """The same two words, whichever fill they follow, are reported alike and
    once: the later fills overwrite them and the counters only accumulate."""
    nbytes = MIB + 16
    corruptions = [(nbytes // 4 - 1, 0x00F00000), (4 * 64 + 2, 0x5)]
    r = native.hbm_pattern_check(0, bytes=nbytes, passes=passes, corruptions=corruptions,
                                 corrupt_at=at)
    assert r["bytes_checked"] == nbytes
    _assert_counts(r, corruptions)


# ---------------------------------------------------------------------------
# GPU: the stream kernel copies, and stops where it should
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", [16, 4096 + 16, 16 * MIB + 16, MIB + 20])
def test_stream_kernel_copies_exactly(native, nbytes):
    """The readiness gate's kernel with its production grid: the destination
    holds the source's pattern over exactly n_vec vectors (a size that is no
    multiple of 16 floors), and the vector after them is untouched."""
    n_vec = nbytes // 16
    for seed in (native.DEFAULT_SEED, SEED2):
        r = native.debug_stream_copy_check(0, nbytes, seed)
        print(r)
        assert r["mismatched_words"] == 0 and r["flipped_bits"] == 0
        assert r["bad_bit_mask"] == 0 and r["first_bad_offset"] == -1
        assert r["bytes_checked"] == 16 * n_vec
        assert r["guard_intact"] is True


# ---------------------------------------------------------------------------
# GPU: MFMA over many tiles, bit for bit
# ---------------------------------------------------------------------------
MFMA_TILES = 64


@pytest.fixture(scope="module")
def reference_tiles(native):
    """Host reference of tiles 0..63, float32 [64, 16, 16], computed once per
    (dtype, seed) and shared."""
    cache = {}

    def get(dtype, seed):
        if (dtype, seed) not in cache:
            ref = np.array([native.reference_tile(dtype, seed, wg) for wg in range(MFMA_TILES)],
                           dtype=np.float32)
            ref.setflags(write=False)
            cache[dtype, seed] = ref
        return cache[dtype, seed]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [None, SEED2])
def test_mfma_tiles_match_host_reference(native, reference_tiles, dtype, seed):
    seed = native.DEFAULT_SEED if seed is None else seed
    raw = native.debug_mfma_dump(0, dtype, MFMA_TILES, seed)
    D = np.frombuffer(raw, dtype="<f4").reshape(MFMA_TILES, 16, 16)
    ref = reference_tiles(dtype, seed)
    bad = np.argwhere(D.view(np.uint32) != ref.view(np.uint32))
    print(f"{dtype} seed {seed:#x}: {len(bad)} of {D.size} elements differ, first {bad[:4].tolist()}")
    assert np.array_equal(D.view(np.uint32), ref.view(np.uint32))
    for wg in (0, 1, 63):
        A, B, C_ = model.operands(dtype, seed, wg)
        assert np.array_equal(D[wg].astype(np.float64), A @ B + C_), wg
    # the tiles differ from each other and from their transposes
    assert not np.array_equal(D[0], D[1]) and not np.array_equal(D[0], D[0].T)


# ---------------------------------------------------------------------------
# GPU: the MFMA check's counters
# ---------------------------------------------------------------------------
def _el(wg, row, col):
    return (wg * 16 + row) * 16 + col


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


MFMA_CORRUPTIONS = {
    # lane 16 * 2 + 5 holds rows 8..11 of column 5
    "one_lane": [(_el(7, 11, 5), 1 << 3), (_el(7, 8, 5), 1 << 22)],
    "one_wave_other_lanes": [(_el(20, 13, 2), 1 << 20), (_el(20, 1, 15), 1 << 1),
                             (_el(20, 6, 0), 0x00700000)],
    "different_tiles": [(_el(63, 0, 0), 1 << 10), (_el(3, 15, 15), 1 << 12),
                        (_el(40, 7, 9), 1 << 31)],
    "first_and_last": [(_el(63, 15, 15), 1 << 20), (0, 1 << 20)],
}


def _assert_mfma_counts(r, corruptions, ref):
    print(r)
    assert r["tiles"] == MFMA_TILES
    assert r["mismatches"] == len(corruptions)
    first, mask = min(corruptions)
    wg, row, col, got, expected = r["first_bad"]
    assert (wg, row, col) == (first // 256, first // 16 % 16, first % 16)
    want = float(ref[wg, row, col])
    assert expected == want
    want_got = _f32_bits(want) ^ mask
    if (want_got & 0x7F800000) == 0x7F800000 and want_got & 0x007FFFFF:
        assert math.isnan(got)
    else:
        assert _f32_bits(got) == want_got


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(MFMA_CORRUPTIONS))
def test_mfma_check_counts_many_mismatches(native, reference_tiles, dtype, case):
    corruptions = MFMA_CORRUPTIONS[case]
    r = native.mfma_verify(0, dtype, workgroups=MFMA_TILES, corruptions=corruptions)
    _assert_mfma_counts(r, corruptions, reference_tiles(dtype, native.DEFAULT_SEED))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mfma_check_sees_a_nan(native, reference_tiles, dtype):
    """A NaN compares false with everything: the check must count it, not
    skip it. The mask is computed from the expected value."""
    ref = reference_tiles(dtype, native.DEFAULT_SEED)
    element = _el(31, 10, 6)
    mask = _f32_bits(float(ref[31, 10, 6])) ^ 0x7FC00000
    assert mask != 0
    corruptions = [(element, mask), (_el(50, 2, 2), 1 << 20)]
    r = native.mfma_verify(0, dtype, workgroups=MFMA_TILES, corruptions=corruptions)
    _assert_mfma_counts(r, corruptions, ref)
    assert math.isnan(r["first_bad"][3])


@pytest.mark.gpu
def test_legacy_corrupt_element_is_bit_20(native, reference_tiles):
    r = native.mfma_verify(0, "f16", workgroups=MFMA_TILES, corrupt_element=_el(9, 4, 4))
    _assert_mfma_counts(r, [(_el(9, 4, 4), 1 << 20)], reference_tiles("f16", native.DEFAULT_SEED))
