"""The Service views of the Python-free store core
(kuberay_amd/_native/store_core.hpp) under sanitizers:
tests/native/service_view_check.cpp is a stand-alone program that drives
create, spec update, status write, a full write without a view, remove and
readers racing writers. It is built once with AddressSanitizer + UBSan and
once with ThreadSanitizer and run as a subprocess, with the sanitizer runtime
linked into the program itself; nothing is loaded into Python under a
sanitizer (the extraction from PyObject trees is covered by
test_service_view.py instead)."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "service_view_check.cpp"
INCLUDE = ROOT / "kuberay_amd" / "_native"
CXX = os.environ.get("CXX", "g++")


def _build(tmp_path, name, flags):
    if shutil.which(CXX) is None:
        pytest.skip(f"{CXX} not available")
    exe = tmp_path / name
    # -O0 -g1: the program runs for a fraction of a second either way, and
    # the build is what the test's time goes to
    cmd = [CXX, "-std=c++17", "-O0", "-g1", "-fno-omit-frame-pointer", *flags,
           f"-I{INCLUDE}", str(SRC), "-o", str(exe), "-pthread"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        missing = ("cannot find -l", "libasan", "libtsan", "libubsan",
                   "unrecognized", "unsupported")
        if any(m in proc.stderr for m in missing):
            pytest.skip("toolchain lacks the sanitizer runtime: "
                        + proc.stderr.strip().splitlines()[-1])
        pytest.fail(proc.stderr)
    return exe


def _run(exe, env_extra):
    env = dict(os.environ, **env_extra)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, env=env,
                          timeout=120)
    bad_mapping = "FATAL: ThreadSanitizer: unexpected memory mapping"
    if proc.returncode != 0 and bad_mapping in proc.stderr:
        # older TSan runtimes cannot place their shadow under a kernel's
        # high-entropy address randomization; run this one process without it
        setarch = shutil.which("setarch")
        if setarch:
            proc = subprocess.run([setarch, os.uname().machine, "-R", str(exe)],
                                  capture_output=True, text=True, env=env,
                                  timeout=120)
        if proc.returncode != 0 and (bad_mapping in proc.stderr
                                     or "setarch" in proc.stderr):
            pytest.skip("ThreadSanitizer runtime cannot map its shadow on this kernel")
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "service_view_check OK" in proc.stdout


def test_service_view_address_and_undefined(tmp_path):
    exe = _build(tmp_path, "check_asan",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                  "-static-libasan", "-static-libubsan"])
    _run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
               "UBSAN_OPTIONS": "print_stacktrace=1"})


def test_service_view_thread(tmp_path):
    exe = _build(tmp_path, "check_tsan", ["-fsanitize=thread", "-static-libtsan"])
    _run(exe, {"TSAN_OPTIONS": "halt_on_error=1"})


def test_service_view_plain(tmp_path):
    """Same program without instrumentation (runs even where the sanitizer
    runtimes are missing)."""
    exe = _build(tmp_path, "check_plain", [])
    _run(exe, {})
