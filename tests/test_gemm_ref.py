"""tests/native/gemm_ref_check.cpp, a stand-alone program over gpuhealth_ref.hpp:
built plain and with ASan + UBSan linked into the program itself, run as a process.
The table it prints holds tests/gemm_model.py, the numpy side of the GPU tests of
the GEMM check, to the native generator and reference; the model's layout of a
stage and its decision rule are tested here too, and every seeded fault case of
tests/test_gpu_gemm_faults.py is held against the rule: none may leave an element
of D undecided."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gemm_model as gm

ROOT = Path(__file__).resolve().parent.parent
CXX = os.environ.get("CXX", "g++")
SANITIZE = ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-static-libasan", "-static-libubsan"]


def _build_and_run(tmp_path, flags):
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
    return run.stdout


@pytest.mark.parametrize("flags", [["-O2"], SANITIZE], ids=["plain", "asan_ubsan"])
def test_gemm_ref_check(tmp_path, flags):
    _build_and_run(tmp_path, flags)


def test_model_matches_the_native_table(tmp_path):
    """Generator values at near and far indices and reference elements, both seeds
    and both data types, as the native header computes them."""
    names = {0: "bf16", 1: "f16"}
    which = {0: "a", 1: "b", 2: "c"}
    gens = refs = 0
    for line in _build_and_run(tmp_path, ["-O2"]).splitlines():
        kind, *fields = line.split()
        if kind == "gen":
            seed, dt, w, r, c, value = (int(f) for f in fields)
            assert gm.operand_matrix(names[dt], seed, which[w], 1, 1, r, c)[0, 0] == value, line
            gens += 1
        elif kind == "ref":
            seed, dt, k, r, c, value = (int(f) for f in fields)
            assert gm.reference_element(names[dt], seed, k, r, c) == value, line
            refs += 1
    assert gens == 2 * 2 * 3 * 8 * 7 and refs == 2 * 2 * 27
    assert {gm.DEFAULT_SEED, gm.SEED2} == {0x5EED1234, 0x0BADC0DE}


def test_operand_matrix_is_the_grid_of_its_elements():
    for dtype in gm.DTYPES:
        whole = gm.operand_matrix(dtype, gm.SEED2, "b", 70, 67, row0=65500, col0=3)
        assert whole.min() == -8 and whole.max() == 8
        for r, c in [(0, 0), (69, 66), (36, 5)]:
            assert whole[r, c] == gm.operand_matrix(dtype, gm.SEED2, "b", 1, 1, 65500 + r, 3 + c)
        assert not np.array_equal(whole[:67, :], whole[:67, :].T)


def test_encode_and_decode():
    ints = np.arange(-8, 9)
    assert list(gm.encode("bf16", [1, 8, -1, 0])) == [0x3F80, 0x4100, 0xBF80, 0]
    assert list(gm.encode("f16", [1, 8, -1, 0])) == [0x3C00, 0x4800, 0xBC00, 0]
    for dtype in gm.DTYPES:
        assert np.array_equal(gm.decode(dtype, gm.encode(dtype, ints)), ints)
        assert gm.flipped(dtype, 1.0, 0x4000) == np.inf and gm.flipped(dtype, -1.0, 0x4000) == -np.inf
        assert gm.flipped(dtype, 3.0, 0x8000) == -3.0
        assert gm.flipped(dtype, 0.0, 0x8000) == 0.0
    assert gm.flipped("bf16", 1.0, 0x0001) == 1 + 2.0 ** -7
    assert gm.flipped("f16", 1.0, 0x0001) == 1 + 2.0 ** -10
    assert np.isnan(gm.flipped("f16", np.inf, 0x0001))


def test_stage_layout_holds_every_element_once():
    """16 KiB of a stage are the 64 x 64 of A and of B, each exactly once; a
    chunk stays whole, and the swizzles are the ones the kernel's comments give."""
    m0, n0, stage = 64, 128, 2
    seen = {"a": set(), "b": set()}
    for offset in range(0, gm.STAGE_BYTES, 2):
        operand, row, col = gm.lds_element(offset, m0, n0, stage)
        assert operand == ("a" if offset < 8192 else "b")
        seen[operand].add((row, col))
    assert seen["a"] == {(m0 + r, 64 * stage + c) for r in range(64) for c in range(64)}
    assert seen["b"] == {(64 * stage + r, n0 + c) for r in range(64) for c in range(64)}
    # row 5 of A: swizzle 2, so slot 0 holds chunk 2; row 10 of B: bits 1 and 3 set, swizzle 6
    assert gm.lds_element(128 * 5 + 2 * 3, 0, 0, 0) == ("a", 5, 16 + 3)
    assert gm.lds_element(8192 + 128 * 10 + 16 * 1, 0, 0, 1) == ("b", 64 + 10, 8 * 7)
    assert [gm.a_swizzle(r) for r in (0, 1, 2, 15, 16, 63)] == [0, 0, 1, 7, 0, 7]
    assert [gm.b_swizzle(r) for r in (0, 2, 8, 10, 13, 63)] == [0, 2, 4, 6, 4, 6]
    assert gm.lds_element(128 * 5, 0, 0, 0, a_shift=2) != gm.lds_element(128 * 5, 0, 0, 0)


def test_decision_rule():
    clean = np.array([100.0, 100.0, 100.0, 100.0, 100.0, 0.0])
    faulted = np.array([100.0, np.inf, np.nan, 101.0, 100.0 + 2.0 ** -20, 2.0 ** -30])
    s = np.array([4000.0, np.inf, np.inf, 4001.0, 4000.0 + 2.0 ** -20, 4000.0])
    verdict, exact = gm.judge(clean, faulted, s, 192, 2.0 ** -30)
    # equal; Inf; NaN; exact and different; below the bound and not exact, twice:
    # 2^-30 and 4000 are both fp32 values, but integers plus 2^-30 do not add exactly
    assert list(verdict) == [gm.MUST_MATCH, gm.MUST_MISMATCH, gm.MUST_MISMATCH, gm.MUST_MISMATCH,
                             gm.UNDECIDED, gm.UNDECIDED]
    assert list(exact) == [False] * 6
    assert list(gm.judge(clean, faulted, s, 192, 2.0 ** -10)[1]) == [True, False, False, True,
                                                                     True, True]
    assert [gm.grid_of(v) for v in (0.0, 8.0, 1 + 2.0 ** -7, 2.0 ** -13, 3 * 2.0 ** 67)] == [
        1.0, 1.0, 2.0 ** -7, 2.0 ** -13, 1.0]
    # the bound itself: 8 K 2^-24 S, strictly above it is a mismatch
    bound = 8 * 65536 * 2.0 ** -24 * 3.0e6
    verdict, _ = gm.judge(np.array([5.0, 5.0]), np.array([5.0 + bound * 0.99, 5.0 + bound * 1.01]),
                          np.array([3.0e6 + 0.3, 3.0e6 + 0.3]), 65536, 2.0 ** -40)
    assert list(verdict) == [gm.UNDECIDED, gm.MUST_MISMATCH]


@pytest.fixture(scope="module", params=gm.DTYPES)
def clean(request):
    return (request.param, *gm.clean_operands(request.param, gm.DEFAULT_SEED, *gm.FAULT_SHAPE))


def test_no_fault_case_leaves_an_element_undecided(clean):
    """The cap: every case of the bit sweep, the zero flips, the position sweep
    and the LDS sweep is decided for every element of D, so the GPU tests can
    assert the mismatch set itself."""
    dtype, a, b, c, d = clean
    memory = (gm.bit_sweep_cases(a, b) + gm.zero_flip_cases(a, b)
              + gm.position_sweep_cases(dtype, a, b, c, d))
    assert len(memory) == 64 + 2 + 128
    undecided = [(case, v.undecided) for case in memory
                 for v in [gm.verdict_of(dtype, a, b, c, d, case)] if v.undecided]
    lds = gm.lds_sweep_cases(dtype, a, b)
    assert len(lds) == 2 * 3 * 64
    undecided += [(case, v.undecided) for case in lds
                  for v in [gm.lds_verdict(dtype, a, b, c, d, case)] if v.undecided]
    assert undecided == []


def test_fault_cases_cover_what_they_claim(clean):
    dtype, a, b, c, d = clean
    sweep = gm.position_sweep_cases(dtype, a, b, c, d)
    for operand, line_at, k_at in (("a", 1, 2), ("b", 2, 1)):
        mine = [case for case in sweep if case[0] == operand]
        assert sorted(case[line_at] % 64 for case in mine) == list(range(64))
        assert sorted(case[k_at] % 64 for case in mine) == list(range(64))  # a permutation
        assert {case[k_at] // 64 for case in mine} == {0, 1, 2}
        assert {case[3] for case in mine} == set(gm.MASKS)
        halves = [case[line_at] // 64 for case in mine]
        assert 16 <= sum(halves) <= 48  # both tile rows / columns, about half each
    for operand, row, col, mask in gm.bit_sweep_cases(a, b):
        assert abs((a if operand == "a" else b)[row, col]) in (1, 8)
    lds = gm.lds_sweep_cases(dtype, a, b)
    assert {case[0] for case in lds} == {0, 1, 2, 3} and {case[1] for case in lds} == {0, 1, 2}
    assert {case[2] < 8192 for case in lds} == {True, False}
    assert {case[2] % 16 // 2 for case in lds} == set(range(8))
    assert all(gm.lds_verdict(dtype, a, b, c, d, case).bad.any() for case in lds)


def test_inf_flip_marks_the_whole_line(clean):
    """1.0 ^ 0x4000 is +Inf in both types: Inf times a non-zero partner is Inf,
    Inf times 0 is NaN, and the whole row of D (A) or column (B) is bad."""
    dtype, a, b, c, d = clean
    for operand, mat in (("a", a), ("b", b)):
        row, col = gm.find_element(mat, 1)
        v = gm.verdict_of(dtype, a, b, c, d, (operand, row, col, 0x4000))
        partners = b[col, :] if operand == "a" else a[:, row]
        assert np.count_nonzero(partners == 0) > 0
        assert v.bad.sum() == 128 and not np.isfinite(v.faulted[v.bad]).any()
        line = v.faulted[row, :] if operand == "a" else v.faulted[:, col]
        assert np.array_equal(np.isnan(line), partners == 0)
        zero = gm.verdict_of(dtype, a, b, c, d, (operand, *gm.find_element(mat, 0), 0x8000))
        assert not zero.bad.any() and np.array_equal(zero.faulted, d)
