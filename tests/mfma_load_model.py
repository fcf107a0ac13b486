"""Python model of the MFMA load's alternating-sign chain (the section "MFMA
load" of kuberay_amd/_native/gpuhealth_ref.hpp), over the generators of
tests/gpuhealth_model.py. Nothing here imports the extension.

A wave of workgroup visit ``visit`` keeps ``TILES`` chains going; chain
``tile`` of wave ``wave`` works on the exact tile ``tile_index(visit, wave,
tile)``. From acc = C it issues +A·B, -A·B, +A·B, ...: after an odd number of
MFMAs acc is C + A·B, after an even number C. All values are exact in fp32
(integers below 2^13, or multiples of 1/16 below 2^16), so float64 numpy
arithmetic rounded to float32 is the exact expectation.

``debug_mfma_load_dump(alternate=False)`` runs the same loop with +A in both
operand sets: after n MFMAs acc is C + n·A·B (``expected_sum_after``), which
differs for every n. That chain is exact only while its partial sums stay
below 2^24 units, which the model asserts for every tile and n it is asked for.
"""
import functools

import numpy as np

from gpuhealth_model import f32_bits, k_of, operands

WAVES = 4
TILES = 4
NEGATE_MASK = {"bf16": 0x80008000, "f16": 0x80008000, "fp8": 0x80808080,
               "mxfp4": 0x88888888}


def flop_per_mfma(dtype):
    return 2 * 16 * 16 * k_of(dtype)


def tile_index(visit, wave, tile):
    return ((visit * WAVES + wave) * TILES + tile) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _operands(dtype, seed, wg):
    """operands() of one tile, generated once and left unchanged."""
    A, B, C_ = operands(dtype, seed, wg)
    for M in (A, B, C_):
        M.setflags(write=False)
    return A, B, C_


@functools.lru_cache(maxsize=None)
def _c_and_d(dtype, seed, wg):
    A, B, C_ = _operands(dtype, seed, wg)
    D = A @ B + C_
    # the premise: both are exact in fp32
    assert np.array_equal(D.astype(np.float32).astype(np.float64), D)
    c32, d32 = C_.astype(np.float32), D.astype(np.float32)
    c32.setflags(write=False)
    d32.setflags(write=False)
    return c32, d32


def expected_after(dtype, seed, wg, n_mfmas):
    """The 16 x 16 accumulator tile after n_mfmas MFMAs of the chain."""
    c32, d32 = _c_and_d(dtype, seed, wg)
    return d32 if n_mfmas % 2 else c32


def expected_dump(dtype, seed, visit, n_mfmas):
    """What debug_mfma_load_dump returns, as float32 [WAVES, TILES, 16, 16]."""
    return np.stack([np.stack([expected_after(dtype, seed, tile_index(visit, w, t), n_mfmas)
                               for t in range(TILES)]) for w in range(WAVES)])


def accumulator_after_mfma(dtype, seed, wg, mfma):
    """The tile right after MFMA number ``mfma`` (0-based) of a chunk."""
    return expected_after(dtype, seed, wg, mfma + 1)


def _chains_from(first):
    """Every (wave, tile), in order, beginning with chain number ``first``."""
    for n in range(WAVES * TILES):
        yield divmod((first + n) % (WAVES * TILES), TILES)


def nonzero_target(dtype, seed, visit, after, first=0):
    """(wave, tile, register) of lane 0 whose accumulator is not zero right
    after MFMA ``after``: lane 0 holds D[r][0] in register r. The search
    begins at chain ``first`` (wave first // TILES, tile first % TILES), so a
    caller can spread its targets over the waves and tiles."""
    for wave, tile in _chains_from(first):
        acc = accumulator_after_mfma(dtype, seed, tile_index(visit, wave, tile), after)
        for reg in range(4):
            if acc[reg, 0] != 0:
                return wave, tile, reg
    raise AssertionError("every candidate accumulator is zero")


def bit_flip_target(dtype, seed, visit, after, first=0):
    """(wave, tile, register) of lane 0 whose accumulator right after MFMA
    ``after`` stays a normal, finite, non-zero number under every single-bit
    flip: its exponent field has at least two bits clear (no flip makes it
    all ones, an infinity or a NaN) and at least two set (none makes it zero,
    a zero or a denormal). Every ``value ^ (1 << b)`` then differs from the
    value as a number, whatever the denormal mode of the compare."""
    for wave, tile in _chains_from(first):
        acc = accumulator_after_mfma(dtype, seed, tile_index(visit, wave, tile), after)
        for reg in range(4):
            ones = bin((f32_bits(float(acc[reg, 0])) >> 23) & 0xFF).count("1")
            if 2 <= ones <= 6:
                return wave, tile, reg
    raise AssertionError("no candidate accumulator keeps clear of the exponent's ends")


# ---------------------------------------------------------------------------
# the same-sign chain of debug_mfma_load_dump(alternate=False): +A·B every time
# ---------------------------------------------------------------------------
EXACT_UNITS = 1 << 24  # integers of fp32 below this are all representable


def unit_of(dtype):
    """What every operand product and every C is a whole multiple of."""
    return 1.0 / 16.0 if dtype == "mxfp4" else 1.0


@functools.lru_cache(maxsize=None)
def _product_terms(dtype, seed, wg):
    """C, A·B and sum over k of |a_k b_k| of one tile, float64 (all exact:
    whole multiples of the unit far below 2^53 units)."""
    A, B, C_ = _operands(dtype, seed, wg)
    unit = unit_of(dtype)
    for M in (A @ B, C_, np.abs(A) @ np.abs(B)):
        assert np.array_equal(np.round(M / unit) * unit, M)
    return C_, A @ B, np.abs(A) @ np.abs(B)


def sum_premise_units(dtype, seed, wg, n):
    """The largest, over the tile's elements, of |C| + (n - 1)·|A·B| + sum over
    k of |a_k b_k|, in units: a bound on every partial sum the n-th MFMA can
    form, in any order of k, on top of the accumulator the first n - 1 left."""
    C_, P, absP = _product_terms(dtype, seed, wg)
    return float((np.abs(C_) + (n - 1) * np.abs(P) + absP).max() / unit_of(dtype))


def expected_sum_after(dtype, seed, wg, n):
    """C + n·A·B, the 16 x 16 accumulator tile after n MFMAs that all add
    +A·B. Asserts its premise: every partial sum stays below 2^24 units, so
    each is exact in fp32 in whatever order the matrix pipe adds, and float64
    arithmetic rounded to float32 is the exact expectation."""
    assert n >= 1
    worst = sum_premise_units(dtype, seed, wg, n)
    assert worst < EXACT_UNITS, (
        f"{dtype} seed {seed:#x} tile {wg} n {n}: partial sums reach {worst:.0f} units, "
        f"not below 2^24")
    C_, P, _ = _product_terms(dtype, seed, wg)
    D = C_ + n * P
    d32 = D.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), D)
    return d32


def expected_sum_dump(dtype, seed, visit, n):
    """What debug_mfma_load_dump(alternate=False) returns, as float32
    [WAVES, TILES, 16, 16]."""
    return np.stack([np.stack([expected_sum_after(dtype, seed, tile_index(visit, w, t), n)
                               for t in range(TILES)]) for w in range(WAVES)])
