"""The MFMA load's Python-free core (the "MFMA load" section of
kuberay_amd/_native/gpuhealth_ref.hpp) as a stand-alone program:
tests/native/mfma_load_ref_check.cpp checks that ``negate_mask`` negates every
element for every code (±0, the e2m1 half-steps and the e4m3 NaN codes
included), that the alternating-sign chain accumulated in fp32 equals
``expected_after`` bit for bit after 1, 2, 3, 31 and 32 MFMAs in forward,
reverse and shuffled k order, ``flop_per_mfma`` and the tile index. It is
built with g++ plain, at -O0, and with AddressSanitizer + UBSan linked into the
program itself, and run as its own process; nothing is loaded into Python under
a sanitizer. The Python model of the same chain (tests/mfma_load_model.py) is
checked against its own premise here too, without a device, and so is its
model of the same-sign chain (``expected_sum_after``, C + n·A·B): against
float32 additions in a scrambled order of k, that its premise fires where the
sums stop being exact (MXFP4 at 4095 MFMAs) and holds where the device tests
use it, and that it starts as the alternating chain does."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from gpuhealth_model import DTYPES, operands
from mfma_load_model import (EXACT_UNITS, NEGATE_MASK, TILES, WAVES, expected_after,
                             expected_dump, expected_sum_after, expected_sum_dump,
                             flop_per_mfma, sum_premise_units, tile_index, unit_of)

DEFAULT_SEED = 0x5EED1234  # gh::kDefaultSeed (gpuhealth_ref.hpp)

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "mfma_load_ref_check.cpp"
INCLUDE = ROOT / "kuberay_amd" / "_native"
CXX = os.environ.get("CXX", "g++")


def _build(tmp_path, name, flags):
    if shutil.which(CXX) is None:
        pytest.skip(f"{CXX} not available")
    exe = tmp_path / name
    cmd = [CXX, "-std=c++17", "-Wall", "-Wextra", *flags, f"-I{INCLUDE}",
           str(SRC), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        missing = ("cannot find -l", "libasan", "libubsan", "unrecognized",
                   "unsupported")
        if "-fsanitize" in " ".join(flags) and any(m in proc.stderr for m in missing):
            pytest.skip("toolchain lacks the sanitizer runtime: "
                        + proc.stderr.strip().splitlines()[-1])
        pytest.fail(proc.stderr)
    return exe


def _run(exe, env_extra):
    env = dict(os.environ, **env_extra)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, env=env,
                          timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "mfma_load_ref_check OK" in proc.stdout


def test_mfma_load_ref_plain(tmp_path):
    _run(_build(tmp_path, "load_plain", ["-O2"]), {})


def test_mfma_load_ref_O0(tmp_path):
    """Unoptimised: no result may depend on how the compiler folds or
    contracts the float arithmetic."""
    _run(_build(tmp_path, "load_O0", ["-O0"]), {})


def test_mfma_load_ref_address_and_undefined(tmp_path):
    exe = _build(tmp_path, "load_asan",
                 ["-O1", "-g1", "-fno-omit-frame-pointer",
                  "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                  "-static-libasan", "-static-libubsan"])
    _run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
               "UBSAN_OPTIONS": "print_stacktrace=1"})


def test_python_model_of_the_chain():
    assert [flop_per_mfma(d) for d in DTYPES] == [16384, 16384, 16384, 65536]
    assert NEGATE_MASK == {"bf16": 0x80008000, "f16": 0x80008000, "fp8": 0x80808080,
                           "mxfp4": 0x88888888}
    indices = {tile_index(v, w, t) for v in range(8) for w in range(WAVES) for t in range(TILES)}
    assert indices == set(range(8 * WAVES * TILES))
    for dtype in DTYPES:
        wg = tile_index(3, 2, 1)
        c, d = expected_after(dtype, 7, wg, 0), expected_after(dtype, 7, wg, 1)
        assert c.dtype == d.dtype == np.float32 and c.shape == d.shape == (16, 16)
        assert np.array_equal(expected_after(dtype, 7, wg, 2), c)
        assert np.array_equal(expected_after(dtype, 7, wg, 33), d)
        assert np.abs(c).max() <= 8 and not np.array_equal(c, d)
        dump = expected_dump(dtype, 7, 3, 1)
        assert dump.shape == (WAVES, TILES, 16, 16) and np.array_equal(dump[2, 1], d)


# ---------------------------------------------------------------------------
# the same-sign chain (debug_mfma_load_dump(alternate=False)): C + n·A·B
# ---------------------------------------------------------------------------
def _fp32_chain_scrambled(dtype, seed, wg, n, rng):
    """acc = C, then n times acc += a_k · b_k over a fresh random order of k,
    every product and every addition rounded to float32: what a matrix pipe
    that adds in some order of its own would leave."""
    A, B, C_ = operands(dtype, seed, wg)
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    assert np.array_equal(A32, A) and np.array_equal(B32, B)
    acc = C_.astype(np.float32)
    for _ in range(n):
        for k in rng.permutation(A.shape[1]):
            acc = (acc + A32[:, k, None] * B32[None, k, :]).astype(np.float32)
    return acc


@pytest.mark.parametrize("dtype,n", [("bf16", 4095), ("f16", 239), ("fp8", 18), ("mxfp4", 239),
                                     ("mxfp4", 3)])
def test_same_sign_chain_is_order_independent(dtype, n):
    """expected_sum_after against float32 additions in a scrambled order of k:
    under the premise the model asserts, the order cannot matter."""
    rng = np.random.default_rng(20 + n)
    wg = tile_index(7, 1, 2)
    want = expected_sum_after(dtype, 0x0BADC0DE, wg, n)
    got = _fp32_chain_scrambled(dtype, 0x0BADC0DE, wg, n, rng)
    assert want.dtype == got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the count shows: one MFMA more or fewer is another tile
    for other in (n - 1, n + 1):
        if other >= 1:
            assert not np.array_equal(want, expected_sum_after(dtype, 0x0BADC0DE, wg, other))


def test_same_sign_premise_fires_for_mxfp4_at_4095():
    """MXFP4 counts in 1/16: 2^24 units are 2^20, and 4094 x |A·B| passes that
    for every tile of the visits the device tests use. 239 holds."""
    for seed, visit in ((DEFAULT_SEED, 0), (0x0BADC0DE, 7)):
        for wave in range(WAVES):
            for tile in range(TILES):
                wg = tile_index(visit, wave, tile)
                assert sum_premise_units("mxfp4", seed, wg, 239) < EXACT_UNITS
                assert sum_premise_units("mxfp4", seed, wg, 4095) >= EXACT_UNITS
                with pytest.raises(AssertionError, match="not below 2\\^24"):
                    expected_sum_after("mxfp4", seed, wg, 4095)
    with pytest.raises(AssertionError):
        expected_sum_dump("mxfp4", DEFAULT_SEED, 0, 4095)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_sign_premise_holds_where_the_device_tests_use_it(dtype):
    """Counts up to 4095 for the integer-valued types and up to 239 for MXFP4,
    visits 0 and 7 under two seeds: the margin is printed."""
    n = 239 if dtype == "mxfp4" else 4095
    worst = max(sum_premise_units(dtype, seed, tile_index(visit, w, t), n)
                for seed, visit in ((DEFAULT_SEED, 0), (0x0BADC0DE, 7))
                for w in range(WAVES) for t in range(TILES))
    print(f"{dtype} n {n}: partial sums reach {worst:.0f} of {EXACT_UNITS} units")
    assert worst < EXACT_UNITS
    assert unit_of(dtype) == (1.0 / 16.0 if dtype == "mxfp4" else 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_sign_chain_starts_as_the_alternating_one(dtype):
    for seed, visit in ((DEFAULT_SEED, 0), (7, 3)):
        wg = tile_index(visit, 2, 1)
        assert np.array_equal(expected_sum_after(dtype, seed, wg, 1).view(np.uint32),
                              expected_after(dtype, seed, wg, 1).view(np.uint32))
        assert np.array_equal(expected_sum_dump(dtype, seed, visit, 1).view(np.uint32),
                              expected_dump(dtype, seed, visit, 1).view(np.uint32))
