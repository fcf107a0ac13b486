"""The CU sweep's device-free core (decode_location, location_key,
lds_pattern_index in kuberay_amd/_native/gpuhealth_ref.hpp) as a stand-alone
program: tests/native/cu_location_check.cpp checks that each register field is
extracted alone and with every other bit set, that the location key is a
bijection onto [0, kCuSlots) which ignores the SIMD, and that the LDS march's
pattern index puts the visit in the high half so that two visits share no word
of 160 KiB. It is built with g++ plain, at -O0, and with AddressSanitizer +
UBSan linked into the program itself, and run as its own process; nothing is
loaded into Python under a sanitizer."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "cu_location_check.cpp"
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
                          timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "cu_location_check OK" in proc.stdout


def test_cu_location_plain(tmp_path):
    _run(_build(tmp_path, "cu_plain", ["-O2"]), {})


def test_cu_location_O0(tmp_path):
    _run(_build(tmp_path, "cu_O0", ["-O0"]), {})


def test_cu_location_address_and_undefined(tmp_path):
    exe = _build(tmp_path, "cu_asan",
                 ["-O1", "-g1", "-fno-omit-frame-pointer",
                  "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                  "-static-libasan", "-static-libubsan"])
    _run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
               "UBSAN_OPTIONS": "print_stacktrace=1"})
