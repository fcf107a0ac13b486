"""The burn-in's narrow GEMM check (fp8, mxfp4) on the device against numpy in
float64. fp8 operands are small integers and mxfp4 sums are multiples of 1/16
below 2^24, so every comparison is exact. Shapes, with S the stage depth: one
stage, the first buffer swap, a reused buffer, several workgroups of a
non-square grid; the default shape; the deepest K."""
import numpy as np
import pytest

import gpuhealth_model as hm

pytestmark = pytest.mark.gpu

DTYPES = ("fp8", "mxfp4")
STAGE = {"fp8": 128, "mxfp4": 256}
MAX_K = {"fp8": 65536, "mxfp4": 4096}
E4M3 = np.array([hm.e4m3_to_f32(b) for b in range(256)])
E2M1 = np.array([hm.e2m1_to_float(c) for c in range(16)])


def _shapes(dtype):
    s = STAGE[dtype]
    return [(64, 64, s), (64, 64, 2 * s), (64, 64, 3 * s), (128, 192, 2 * s)]


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    assert gpuhealth.GEMM_NARROW_STAGE_K == STAGE and gpuhealth.GEMM_NARROW_MAX_K == MAX_K
    return gpuhealth


def _nibbles(raw, rows, cols):
    """Two e2m1 codes per byte along the row, the even element in the low nibble."""
    u = np.frombuffer(raw, np.uint8).reshape(rows, cols // 2)
    return np.stack([u & 15, u >> 4], axis=-1).reshape(rows, cols)


_dumps = {}


def _dump(native, dtype, shape, inject=None):
    """Raw A, B (codes for mxfp4), the scales, decoded A and B, D and A·B + C in
    float64; one run per case."""
    key, (m, n, k) = (dtype, shape, inject), shape
    if key not in _dumps:
        raw = native.debug_gemm_narrow_dump(0, dtype, m, n, k, inject=inject)
        c, d = (np.frombuffer(raw[x], np.float32).reshape(m, n) for x in "cd")
        if dtype == "fp8":
            assert set(raw) == {"a", "b", "c", "d"}
            a = E4M3[np.frombuffer(raw["a"], np.uint8).reshape(m, k)]
            b = E4M3[np.frombuffer(raw["b"], np.uint8).reshape(k, n)]
            codes = {"a": a, "b": b, "c": c}
        else:
            sa = np.frombuffer(raw["sa"], np.uint8).reshape(m, k // 32)
            sb = np.frombuffer(raw["sb"], np.uint8).reshape(k // 32, n)
            codes = {"a": _nibbles(raw["a"], m, k), "b": _nibbles(raw["b"], k, n), "c": c,
                     "sa": sa, "sb": sb}
            a = E2M1[codes["a"]] * np.repeat(2.0 ** (sa.astype(int) - 127), 32, axis=1)
            b = E2M1[codes["b"]] * np.repeat(2.0 ** (sb.astype(int) - 127), 32, axis=0)
        _dumps[key] = (codes, a, b, d, a @ b + c.astype(np.float64))
    return _dumps[key]


@pytest.mark.parametrize("bits", (8, 4))
def test_transposed_read_lane_maps(native, bits):
    """The maps in gpuhealth_gemm_narrow.hip; a source is lane * elements + element.
    tr_b8: byte e of lane l is byte i % 8 of lane b + 2 e + i / 8. tr_b4: nibble e
    of lane l is nibble i of lane b + e."""
    got = np.array(native.debug_lds_tr_dump(0, bits=bits))
    lane, e = np.arange(64)[:, None], np.arange(64 // bits)[None, :]
    b, i = lane & ~15, lane & 15
    want = 8 * (b + 2 * e + i // 8) + i % 8 if bits == 8 else 16 * (b + e) + i
    assert np.array_equal(got, want)
    assert np.array_equal(native.debug_lds_tr_dump(0), native.debug_lds_tr_dump(0, bits=16))


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_equals_the_float64_product(native, dtype, case):
    codes, a, b, d, ref = _dump(native, dtype, _shapes(dtype)[case])
    assert np.abs(ref).max() < 2 ** 24 / (16 if dtype == "mxfp4" else 1)
    assert np.array_equal(d, ref)
    for which, mat in codes.items():
        rows, cols = mat.shape
        for r, col in [(0, 0), (0, 1), (1, 0), (rows - 1, cols - 1), (rows // 2, cols // 3)]:
            assert mat[r, col] == native.gemm_narrow_operand(dtype, which, r, col)
    assert np.abs(a).max() >= 8 and np.abs(b).max() >= 8  # not all zeros
    if dtype == "mxfp4":
        assert set(codes["sa"].ravel()) == set(codes["sb"].ravel()) == {126, 127, 128}
        assert set(codes["a"].ravel()) == set(codes["b"].ravel()) == set(range(16))


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_passes_on_a_healthy_device(native, dtype, case):
    shape = (_shapes(dtype) + [(0, 0, 0)])[case]
    r = native.gemm_narrow_exact(0, dtype, *shape)
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)
    assert r["dtype"] == dtype
    if shape == (0, 0, 0):  # the default: the smallest square with two workgroups per CU
        side, want = r["m"] // 64, native.GEMM_WORKGROUPS_PER_CU * r["cu_total"]
        assert r["m"] == r["n"] == 64 * side and r["k"] == native.GEMM_DEFAULT_K
        assert (side - 1) ** 2 < want <= side ** 2 == r["workgroups"]
        assert 1 <= r["cu_seen"] <= r["cu_total"]
    else:
        assert (r["m"], r["n"], r["k"]) == shape


@pytest.mark.parametrize("dtype", DTYPES)
def test_deepest_k(native, dtype):
    """K at the exactness limit, 64 x 64: the buffer parity all the way and, for
    mxfp4, sums of the size the premise is argued for."""
    shape = (64, 64, MAX_K[dtype])
    assert native.gemm_narrow_exact(0, dtype, *shape)["ok"] is True
    if dtype == "mxfp4":
        _, _, _, d, ref = _dump(native, dtype, shape)
        print(f"mxfp4: max |D| at K = 4096 is {np.abs(ref).max()}")
        assert np.array_equal(d, ref)


# k of the fault: the last MFMA step of the second stage
@pytest.mark.parametrize("case", (1, 3))
@pytest.mark.parametrize("dtype,which", [("fp8", "a"), ("fp8", "b"), ("mxfp4", "a"), ("mxfp4", "b"),
                                         ("mxfp4", "sa"), ("mxfp4", "sb")])
def test_seeded_fault(native, dtype, which, case):
    m, n, k = shape = _shapes(dtype)[case]
    step = 128 if dtype == "mxfp4" else 32
    lo, hi = 2 * STAGE[dtype] - step, 2 * STAGE[dtype]
    codes, a, b, _, clean = _dump(native, dtype, shape)
    on_a = which in ("a", "sa")
    line = m - 3 if on_a else n - 3  # the row of A / the column of B
    if which in ("a", "b"):  # a sign flip of the first non-zero element: of 0 it changes nothing
        kk = lo + int(np.flatnonzero(a[line, lo:hi] if on_a else b[lo:hi, line])[0])
        mask, ks = (0x8 if dtype == "mxfp4" else 0x80), slice(kk, kk + 1)
        want_a, want_b = a.copy(), b.copy()
        (want_a[line, ks] if on_a else want_b[ks, line])[...] *= -1
    else:  # an xor of 1 into the scale of the last block of the stage: 126 <-> 127, 128 -> 129
        kk, mask, ks = hi // 32 - 1, 1, slice(hi - 32, hi)
        old = int(codes[which][(line, kk) if on_a else (kk, line)])
        want_a, want_b = a.copy(), b.copy()
        (want_a[line, ks] if on_a else want_b[ks, line])[...] *= 2.0 ** ((old ^ 1) - old)
    inject = (which, line, kk, mask) if on_a else (which, kk, line, mask)

    _, fa, fb, fd, faulted = _dump(native, dtype, shape, inject)
    assert np.array_equal(fa, want_a) and np.array_equal(fb, want_b)
    assert np.array_equal(fd, faulted)  # D is the product of the faulted operand

    bad = np.argwhere(faulted != clean)
    assert len(bad) > 0 and set(bad[:, 0 if on_a else 1]) == {line}
    r = native.gemm_narrow_exact(0, dtype, m, n, k, inject=inject)
    assert r["ok"] is False and r["mismatches"] == len(bad)
    row, col = (int(v) for v in bad[0])
    assert r["first_bad"] == (row, col, faulted[row, col], clean[row, col])
    crossed = ([(line // 64, t) for t in range(n // 64)] if on_a
               else [(t, line // 64) for t in range(m // 64)])
    assert [f["tile"] for f in r["faulty"]] == crossed
    assert crossed == sorted({(int(y) // 64, int(x) // 64) for y, x in bad})
    assert all({"xcc", "se", "sh", "cu"} <= set(f) and f["mismatches"] > 0 for f in r["faulty"])
    assert sum(f["mismatches"] for f in r["faulty"]) == len(bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_raise(native, dtype):
    s, top = STAGE[dtype], MAX_K[dtype]
    for shape in [(64, 64, s // 2), (64, 64, top + s), (65, 64, s)]:
        with pytest.raises(ValueError):
            native.gemm_narrow_exact(0, dtype, *shape)
    with pytest.raises(ValueError):
        native.gemm_narrow_exact(0, "bf16", 64, 64, 256)
    for inject in [("a", 64, 0, 1), ("b", 0, 64, 1), ("a", 0, s, 1), ("c", 0, 0, 1), ("a", 0, 0, 0x100),
                   ("sa", 0, s // 32, 1)]:
        with pytest.raises(ValueError):
            native.gemm_narrow_exact(0, dtype, 64, 64, s, inject=inject)
