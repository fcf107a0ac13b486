"""The burn-in's GEMM check on the device against numpy in float64; the operands
are small integers, so every comparison is exact. Shapes: one stage, the first
buffer swap, a reused buffer, several workgroups of a non-square matrix."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 64), (64, 64, 128), (64, 64, 192), (128, 192, 128)]
DTYPES = ("bf16", "f16")


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    return gpuhealth


_dumps = {}


def _dump(native, dtype, shape, inject=None):
    """A, B, C, D of one run and A·B + C in float64; one run per case."""
    key, (m, n, k) = (dtype, shape, inject), shape
    if key not in _dumps:
        raw = native.debug_gemm_dump(0, dtype, m, n, k, inject=inject)

        def operand(name, rows, cols):
            u = np.frombuffer(raw[name], np.uint16).reshape(rows, cols)
            if dtype == "bf16":
                return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
            return u.view(np.float16).astype(np.float64)
        a, b = operand("a", m, k), operand("b", k, n)
        c, d = (np.frombuffer(raw[x], np.float32).reshape(m, n) for x in "cd")
        _dumps[key] = (a, b, c, d, a @ b + c)
    return _dumps[key]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_equals_the_float64_product(native, dtype, shape):
    a, b, c, d, ref = _dump(native, dtype, shape)
    assert np.array_equal(d, ref)
    for which, mat in (("a", a), ("b", b), ("c", c)):
        rows, cols = mat.shape
        for r, col in [(0, 0), (0, 1), (1, 0), (rows - 1, cols - 1), (rows // 2, cols // 3)]:
            assert mat[r, col] == native.gemm_operand(dtype, which, r, col)
    assert np.abs(a).max() == 8 and np.abs(b).max() == 8  # not all zeros


@pytest.mark.parametrize("shape", SHAPES + [(0, 0, 0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_passes_on_a_healthy_device(native, dtype, shape):
    r = native.gemm_exact(0, dtype, *shape)
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)
    if shape == (0, 0, 0):  # the default: the smallest square with two workgroups per CU
        side, want = r["m"] // 64, native.GEMM_WORKGROUPS_PER_CU * r["cu_total"]
        assert r["m"] == r["n"] == 64 * side and r["k"] == native.GEMM_DEFAULT_K
        assert (side - 1) ** 2 < want <= side ** 2 == r["workgroups"]
        assert 1 <= r["cu_seen"] <= r["cu_total"]
    else:
        assert (r["m"], r["n"], r["k"]) == shape


# k of the fault: second MFMA step of the second stage (96..127), which K = 64 has not
@pytest.mark.parametrize("operand", ("a", "b"))
@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_operand_fault(native, dtype, shape, operand):
    m, n, k = shape
    a, b, c, _, clean = _dump(native, dtype, shape)
    line = m - 3 if operand == "a" else n - 3  # the row of A / the column of B
    kk = 96 + int(np.flatnonzero(  # the first non-zero one: a sign flip of 0 changes nothing
        a[line, 96:128] if operand == "a" else b[96:128, line])[0])
    inject = (operand, line, kk, 0x8000) if operand == "a" else (operand, kk, line, 0x8000)

    fa, fb, _, fd, faulted = _dump(native, dtype, shape, inject)
    want_a, want_b = a.copy(), b.copy()
    (want_a if operand == "a" else want_b)[inject[1], inject[2]] *= -1
    assert np.array_equal(fa, want_a) and np.array_equal(fb, want_b)
    assert np.array_equal(fd, faulted)  # D is the product of the faulted operand

    bad = np.argwhere(faulted != clean)
    partners = b[kk, :] if operand == "a" else a[:, kk]
    assert len(bad) == np.count_nonzero(partners) > 0
    assert set(bad[:, 0 if operand == "a" else 1]) == {line}

    r = native.gemm_exact(0, dtype, m, n, k, inject=inject)
    assert r["ok"] is False and r["mismatches"] == len(bad)
    row, col = (int(v) for v in bad[0])
    assert r["first_bad"] == (row, col, faulted[row, col], clean[row, col])
    crossed = ([(line // 64, t) for t in range(n // 64)] if operand == "a"
               else [(t, line // 64) for t in range(m // 64)])
    assert [f["tile"] for f in r["faulty"]] == crossed
    assert crossed == sorted({(int(y) // 64, int(x) // 64) for y, x in bad})
    assert all({"xcc", "se", "sh", "cu"} <= set(f) and f["mismatches"] > 0 for f in r["faulty"])
    assert sum(f["mismatches"] for f in r["faulty"]) == len(bad)


@pytest.mark.parametrize("shape", [(65, 64, 64), (64, 96, 64), (64, 64, 32),
                                   (64, 64, 65536 + 64), (-64, 64, 64)])
def test_bad_shapes_raise(native, shape):
    for dtype, bad in (("bf16", shape), ("fp8", (64, 64, 64))):
        with pytest.raises(ValueError):
            native.gemm_exact(0, dtype, *bad)


def test_transposed_read_lane_map(native):
    """The map in gpuhealth_gemm.hip: word w holds w and lane l points at word 4 l, so
    out[l][e] = in[b + 4 e + (l & 15) / 4][(l & 15) % 4] is word 4 b + 16 e + (l & 15)."""
    got = np.array(native.debug_lds_tr_dump(0))
    lane, e = np.arange(64)[:, None], np.arange(4)[None, :]
    assert np.array_equal(got, 4 * (lane & ~15) + 16 * e + (lane & 15))
