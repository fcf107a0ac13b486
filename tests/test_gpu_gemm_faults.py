"""Seeded faults of the burn-in's GEMM check on the device, against the decision
rule of tests/gemm_model.py: which elements of D a changed operand must change
follows from arithmetic, and tests/test_gemm_ref.py holds every case used here
to "no element undecided", so the mismatch set itself is asserted.

* memory side (``inject=``): all 16 one-bit masks at elements of magnitude 1 and
  8 of A and of B, the Inf / NaN line, the sign flip of a 0, and one element per
  tile row / column at every k offset of a stage, in every stage;
* LDS side (``lds_inject=``): one 16-bit word of one workgroup's LDS, after the
  stage has landed; the layout model names the element, only that workgroup's
  tile may change, and the operands in memory stay what they were.

Shape 128 x 128 x 192: four tiles, three stages, both buffers and one reuse. The
faults are xors into data. Every comparison is exact.
"""
import numpy as np
import pytest

import gemm_model as gm

pytestmark = pytest.mark.gpu

M, N, K = gm.FAULT_SHAPE


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


def _unpack(dtype, raw):
    a = gm.decode(dtype, np.frombuffer(raw["a"], np.uint16)).reshape(M, K)
    b = gm.decode(dtype, np.frombuffer(raw["b"], np.uint16)).reshape(K, N)
    c, d = (np.frombuffer(raw[x], np.float32).reshape(M, N).astype(np.float64) for x in "cd")
    return a, b, c, d


@pytest.fixture(scope="module", params=gm.DTYPES)
def clean(native, request):
    """One clean dump per data type, shared and left unchanged: (dtype, A, B, C, D)
    in float64. It is the model's, element for element."""
    dtype = request.param
    a, b, c, d = _unpack(dtype, native.debug_gemm_dump(0, dtype, M, N, K))
    want = gm.clean_operands(dtype, gm.DEFAULT_SEED, M, N, K)
    for got, model in zip((a, b, c, d), want):
        assert np.array_equal(got, model)
    return dtype, a, b, c, d


def _assert_reported(r, v, clean_d):
    """The whole report of one run against the Verdict of its fault."""
    tiles, n_bad = v.tiles(), int(v.bad.sum())
    assert r["ok"] is (n_bad == 0) and r["mismatches"] == n_bad
    assert [f["tile"] for f in r["faulty"]] == sorted(tiles)
    for f in r["faulty"]:
        assert (f["mismatches"], f["first_bad"]) == tiles[f["tile"]]
        assert {"xcc", "se", "sh", "cu"} <= set(f)
    first = v.first_bad()
    if first is None:
        assert r["first_bad"] is None
        return
    row, col, got, expected = r["first_bad"]
    assert (row, col) == first and expected == clean_d[row, col]
    assert v.got_matches(row, col, got), (got, v.faulted[row, col])
    assert not got == expected  # a NaN counts


# ---------------------------------------------------------------------------
# memory side
# ---------------------------------------------------------------------------
def test_bit_sweep(native, clean):
    """Every bit of an operand is seen: the sign, the exponent (up to Inf) and
    the mantissa down to its last bit, whose change of D is exact at this K."""
    dtype, a, b, c, d = clean
    cases = gm.bit_sweep_cases(a, b)
    assert len(cases) == 64
    for case in cases:
        v = gm.verdict_of(dtype, a, b, c, d, case)
        assert v.undecided == 0 and v.bad.any(), case
        r = native.gemm_exact(0, dtype, M, N, K, inject=case)
        _assert_reported(r, v, d)


@pytest.mark.parametrize("operand", ("a", "b"))
def test_inf_marks_the_whole_line(native, clean, operand):
    """1.0 ^ 0x4000 is Inf in bf16 and in f16. Inf times a non-zero partner is
    Inf and Inf times 0 is NaN: all 128 elements of the row (A) or column (B) of
    D are bad, the zero partners included, two tiles of 64 each, and the first of
    them is reported as what it is."""
    dtype, a, b, c, d = clean
    mat = a if operand == "a" else b
    row, col = gm.find_element(mat, 1)
    partners = b[col, :] if operand == "a" else a[:, row]
    assert np.count_nonzero(partners == 0) > 0 and abs(mat[row, col]) == 1
    r = native.gemm_exact(0, dtype, M, N, K, inject=(operand, row, col, 0x4000))
    assert r["ok"] is False and r["mismatches"] == 128
    crossed = [(row // 64, t) for t in range(2)] if operand == "a" else [(t, col // 64) for t in range(2)]
    assert [f["tile"] for f in r["faulty"]] == crossed
    assert [f["mismatches"] for f in r["faulty"]] == [64, 64]
    frow, fcol, got, expected = r["first_bad"]
    assert (frow, fcol) == ((row, 0) if operand == "a" else (0, col))
    assert expected == d[frow, fcol]
    if partners[0] == 0:
        assert np.isnan(got)
    else:
        assert got == np.sign(mat[row, col]) * np.sign(partners[0]) * np.inf
    assert r["faulty"][0]["first_bad"] == (frow, fcol)
    assert r["faulty"][1]["first_bad"] == ((row, 64) if operand == "a" else (64, col))


def test_sign_flip_of_a_zero_is_no_alarm(native, clean):
    dtype, a, b, c, d = clean
    for case in gm.zero_flip_cases(a, b):
        operand, row, col, mask = case
        assert (a if operand == "a" else b)[row, col] == 0 and mask == 0x8000
        r = native.gemm_exact(0, dtype, M, N, K, inject=case)
        assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)


def test_position_sweep(native, clean):
    """Every row of a tile of A and every column of a tile of B, at every k offset
    of a stage, in all three stages, in both tile rows / columns: every lane,
    chunk, k-group and quadrant position of the operand reads, and every row of
    the check kernel's blocks."""
    dtype, a, b, c, d = clean
    cases = gm.position_sweep_cases(dtype, a, b, c, d)
    assert len(cases) == 128
    seen = 0
    for case in cases:
        v = gm.verdict_of(dtype, a, b, c, d, case)
        assert v.undecided == 0, case
        r = native.gemm_exact(0, dtype, M, N, K, inject=case)
        _assert_reported(r, v, d)
        seen += bool(v.bad.any())
    assert seen >= 96  # a 0 whose sign flips or that becomes a denormal changes nothing


def test_dumps_of_faulted_runs(native, clean):
    """D of a faulted run is the float64 product of the operands it dumps, bit
    for bit wherever the rule says the sum is exact, with the product's Inf / NaN
    pattern in the Inf case, and untouched everywhere else."""
    dtype, a, b, c, d = clean
    sweep = gm.position_sweep_cases(dtype, a, b, c, d)
    per_stage = [next(case for case in sweep if case[0] == "a" and case[2] // 64 == st
                      and gm.verdict_of(dtype, a, b, c, d, case).bad.any()) for st in range(3)]
    per_stage += [next(case for case in sweep if case[0] == "b" and case[1] // 64 == st
                       and gm.verdict_of(dtype, a, b, c, d, case).bad.any()) for st in range(3)]
    inf_case = ("b", *gm.find_element(b, 1), 0x4000)
    for case in [inf_case, gm.zero_flip_cases(a, b)[0], *per_stage]:
        operand, row, col, mask = case
        v = gm.verdict_of(dtype, a, b, c, d, case)
        fa, fb, fc, fd = _unpack(dtype, native.debug_gemm_dump(0, dtype, M, N, K, inject=case))
        want_a, want_b = a.copy(), b.copy()
        (want_a if operand == "a" else want_b)[row, col] = gm.flipped(
            dtype, (a if operand == "a" else b)[row, col], mask)
        assert np.array_equal(fa, want_a, equal_nan=True)
        assert np.array_equal(fb, want_b, equal_nan=True) and np.array_equal(fc, c)
        touched = v.faulted != d
        touched |= np.isnan(v.faulted)
        assert np.array_equal(fd[~touched], d[~touched])
        assert np.array_equal(fd[v.exact_map], v.faulted[v.exact_map])
        assert np.array_equal(fd != d, v.bad)
        if case is inf_case:
            assert np.array_equal(np.isnan(fd), np.isnan(v.faulted)) and np.isnan(fd).any()
            inf = np.isinf(v.faulted)
            assert inf.any() and np.array_equal(fd[inf], v.faulted[inf])


# ---------------------------------------------------------------------------
# LDS side
# ---------------------------------------------------------------------------
def test_lds_sweep(native, clean):
    """A and B, every stage (both buffers, one of them reused), every row, the
    slots and the elements of a chunk in turn: the element the layout model names
    changes for that tile, so every staged location is consumed as the swizzle
    comments say, and the check names that tile alone."""
    dtype, a, b, c, d = clean
    cases = gm.lds_sweep_cases(dtype, a, b)
    assert len(cases) == 384
    for case in cases:
        tile = case[0]
        v = gm.lds_verdict(dtype, a, b, c, d, case)
        assert v.undecided == 0 and v.bad.any(), case
        r = native.gemm_exact(0, dtype, M, N, K, lds_inject=case)
        _assert_reported(r, v, d)
        assert [f["tile"] for f in r["faulty"]] == [(tile // 2, tile % 2)], case
        assert r["mismatches"] == r["faulty"][0]["mismatches"] <= 64


def test_lds_fault_dumps(native, clean):
    """The operands in memory are untouched, and D is the clean D with that one
    element changed for that one tile: nothing else of the tile moves, not even
    what stage s + 2 adds out of the same buffer, and no other tile."""
    dtype, a, b, c, d = clean
    cases = gm.lds_sweep_cases(dtype, a, b)
    for case in cases[5::64]:  # A and B, each stage
        v = gm.lds_verdict(dtype, a, b, c, d, case)
        fa, fb, fc, fd = _unpack(dtype, native.debug_gemm_dump(0, dtype, M, N, K, lds_inject=case))
        assert np.array_equal(fa, a) and np.array_equal(fb, b) and np.array_equal(fc, c)
        assert v.exact.all() and v.bad.any()
        assert np.array_equal(fd, v.faulted)
    assert {(case[2] >= 8192, case[1]) for case in cases[5::64]} == {
        (is_b, st) for is_b in (False, True) for st in range(3)}


def test_lds_and_memory_faults_add_up(native, clean):
    """Both hooks in one run: the memory fault marks its line in tile row 1, the
    LDS fault its tile (0, 0), and neither hides the other."""
    dtype, a, b, c, d = clean
    mem = ("a", *gm.find_element(a, 8), 0x8000)
    lds = next(case for case in gm.lds_sweep_cases(dtype, a, b) if case[0] == 0 and case[2] >= 8192)
    v_mem, v_lds = gm.verdict_of(dtype, a, b, c, d, mem), gm.lds_verdict(dtype, a, b, c, d, lds)
    assert not (v_mem.bad & v_lds.bad).any()  # tile row 1 against tile (0, 0)
    r = native.gemm_exact(0, dtype, M, N, K, inject=mem, lds_inject=lds)
    assert r["mismatches"] == int(v_mem.bad.sum() + v_lds.bad.sum())
    assert [f["tile"] for f in r["faulty"]] == sorted({**v_mem.tiles(), **v_lds.tiles()})


@pytest.mark.parametrize("bad", [(4, 0, 0, 1), (0, 3, 0, 1), (0, 0, 16384, 1), (0, 0, 3, 1),
                                 (0, 0, 0, 0), (0, 0, 0, 0x10000), (-1, 0, 0, 1), (0, 0, -2, 1)])
def test_bad_lds_faults_raise(native, bad):
    """Validated like inject=: a tile, stage or offset the GEMM does not have, an
    odd offset and a mask that is no 16-bit value are refused before any launch."""
    with pytest.raises(ValueError):
        native.gemm_exact(0, "bf16", M, N, K, lds_inject=bad)
    with pytest.raises(ValueError):
        native.debug_gemm_dump(0, "f16", M, N, K, lds_inject=bad)
