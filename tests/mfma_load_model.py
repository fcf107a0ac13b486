"""Python model of the MFMA load's alternating-sign chain (the section "MFMA
load" of kuberay_amd/_native/gpuhealth_ref.hpp), over the generators of
tests/gpuhealth_model.py. Nothing here imports the extension.

A wave of workgroup visit ``visit`` keeps ``TILES`` chains going; chain
``tile`` of wave ``wave`` works on the exact tile ``tile_index(visit, wave,
tile)``. From acc = C it issues +A·B, -A·B, +A·B, ...: after an odd number of
MFMAs acc is C + A·B, after an even number C. All values are exact in fp32
(integers below 2^13, or multiples of 1/16 below 2^16), so float64 numpy
arithmetic rounded to float32 is the exact expectation.
"""
import functools

import numpy as np

from gpuhealth_model import k_of, operands

WAVES = 4
TILES = 4
NEGATE_MASK = {"bf16": 0x80008000, "f16": 0x80008000, "fp8": 0x80808080,
               "mxfp4": 0x88888888}


def flop_per_mfma(dtype):
    return 2 * 16 * 16 * k_of(dtype)


def tile_index(visit, wave, tile):
    return ((visit * WAVES + wave) * TILES + tile) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _c_and_d(dtype, seed, wg):
    A, B, C_ = operands(dtype, seed, wg)
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
