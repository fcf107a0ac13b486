"""The Python-free tokenizer of kuberay_amd/_native/json_decode.hpp under
sanitizers: tests/native/json_decode_check.cpp is a stand-alone program that
feeds it values of every kind, every unsupported class (integers outside
int64, NaN / Infinity, lone surrogates, duplicate keys, nesting past the
limit, floats out of range), bad escapes, broken UTF-8, every proper prefix
of a small document, and a three-section entry whose event sequence must be
that of the assembled blob. It is built once with AddressSanitizer + UBSan and
run as a subprocess, with the sanitizer runtime linked into the program
itself; nothing is loaded into Python under a sanitizer (the tree builder is
covered by test_native_decoder.py instead)."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "json_decode_check.cpp"
INCLUDE = ROOT / "kuberay_amd" / "_native"
CXX = os.environ.get("CXX", "g++")


def _build(tmp_path, name, flags):
    if shutil.which(CXX) is None:
        pytest.skip(f"{CXX} not available")
    exe = tmp_path / name
    # -O0 -g1: the program runs for a fraction of a second either way, and
    # the build is what the test's time goes to
    cmd = [CXX, "-std=c++17", "-O0", "-g1", "-fno-omit-frame-pointer", *flags,
           f"-I{INCLUDE}", str(SRC), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        missing = ("cannot find -l", "libasan", "libubsan", "unrecognized",
                   "unsupported")
        if any(m in proc.stderr for m in missing):
            pytest.skip("toolchain lacks the sanitizer runtime: "
                        + proc.stderr.strip().splitlines()[-1])
        pytest.fail(proc.stderr)
    return exe


def _run(exe, env_extra):
    env = dict(os.environ, **env_extra)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, env=env,
                          timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "json_decode_check OK" in proc.stdout


def test_json_decode_address_and_undefined(tmp_path):
    exe = _build(tmp_path, "check_asan",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                  "-static-libasan", "-static-libubsan"])
    _run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
               "UBSAN_OPTIONS": "print_stacktrace=1"})


def test_json_decode_plain(tmp_path):
    """Same program without instrumentation, optimised as the engine is
    (runs even where the sanitizer runtimes are missing)."""
    exe = _build(tmp_path, "check_plain", ["-O3"])
    _run(exe, {})
