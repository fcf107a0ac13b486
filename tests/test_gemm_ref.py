"""tests/native/gemm_ref_check.cpp, a stand-alone program over gpuhealth_ref.hpp:
built plain and with ASan + UBSan linked into the program itself, run as a process."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = os.environ.get("CXX", "g++")
SANITIZE = ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("flags", [["-O2"], SANITIZE], ids=["plain", "asan_ubsan"])
def test_gemm_ref_check(tmp_path, flags):
    if shutil.which(CXX) is None:
        pytest.skip(f"{CXX} not available")
    exe = tmp_path / "gemm_ref_check"
    cmd = [CXX, "-std=c++17", "-Wall", "-Wextra", *flags, f"-I{ROOT / 'kuberay_amd' / '_native'}",
           str(ROOT / "tests" / "native" / "gemm_ref_check.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and flags is SANITIZE and "asan" in build.stderr:
        pytest.skip("toolchain lacks the sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "gemm_ref_check OK" in run.stdout, run.stdout + run.stderr
