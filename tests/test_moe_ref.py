"""tests/native/moe_ref_check.cpp, a stand-alone g++ program over gpuhealth_ref.hpp."""
import shutil
import subprocess

import pytest

from test_attn_ref import CXX, ROOT


def test_moe_ref_check(tmp_path):
    if shutil.which(CXX) is None:
        pytest.skip(f"{CXX} not available")
    exe = tmp_path / "moe_ref_check"
    build = subprocess.run(
        [CXX, "-std=c++17", "-Wall", "-Wextra", "-O2", f"-I{ROOT / 'kuberay_amd' / '_native'}",
         str(ROOT / "tests" / "native" / "moe_ref_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "moe_ref_check OK" in run.stdout, run.stdout + run.stderr
