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
checked against its own premise here too, without a device."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from gpuhealth_model import DTYPES
from mfma_load_model import (NEGATE_MASK, TILES, WAVES, expected_after, expected_dump,
                             flop_per_mfma, tile_index)

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
