"""The burn-in's GEMM check on the device against numpy in float64; the operands
are small integers, so every comparison is exact. Shapes: one stage, the first
buffer swap, a reused buffer, several workgroups of a non-square matrix; then
the edges, against tests/gemm_model.py: the default shape (every CU, several
workgroups per CU, 16 stages), the deepest K, the widest and the tallest grid
of tiles, a D of 4 GiB, a second seed, and where the faulty tiles ran."""
import numpy as np
import pytest

import gemm_model as gm

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


# ---------------------------------------------------------------------------
# shape and seed edges, against the numpy model of tests/gemm_model.py
# ---------------------------------------------------------------------------
def _unpack(dtype, raw, m, n, k):
    a = gm.decode(dtype, np.frombuffer(raw["a"], np.uint16)).reshape(m, k)
    b = gm.decode(dtype, np.frombuffer(raw["b"], np.uint16)).reshape(k, n)
    c, d = (np.frombuffer(raw[x], np.float32).reshape(m, n) for x in "cd")
    return a, b, c, d


def _assert_model_dump(dtype, seed, raw, m, n, k):
    """A, B and C are the generator's everywhere and D is the float64 product."""
    a, b, c, d = _unpack(dtype, raw, m, n, k)
    for which, mat in (("a", a), ("b", b), ("c", c)):
        assert np.array_equal(mat, gm.operand_matrix(dtype, seed, which, *mat.shape)), which
    ref = a @ b + c
    assert np.abs(ref).max() < 2 ** 24
    assert np.array_equal(d, ref)
    return ref


def _assert_line_fault(native, dtype, m, n, k, case):
    """A memory-side fault at a shape too large to dump: the report against the
    rule, the reference for the one affected line from the generator alone."""
    v = gm.line_verdict(dtype, gm.DEFAULT_SEED, m, n, k, case)
    assert v.undecided == 0 and v.bad.any()
    r = native.gemm_exact(0, dtype, m, n, k, inject=case)
    tiles = v.tiles()
    assert r["ok"] is False and r["mismatches"] == int(v.bad.sum())
    assert [f["tile"] for f in r["faulty"]] == sorted(tiles)
    assert all((f["mismatches"], f["first_bad"]) == tiles[f["tile"]] for f in r["faulty"])
    row, col, got, expected = r["first_bad"]
    assert (row, col) == v.first_bad()
    assert expected == gm.reference_element(dtype, gm.DEFAULT_SEED, k, row, col)
    assert v.got_matches(row, col, got) and got != expected
    return r


def _nonzero_k(dtype, operand, line, lo, hi):
    """The first k in lo..hi - 1 at which A[line][k] / B[k][line] is not 0."""
    if operand == "a":
        values = gm.operand_matrix(dtype, gm.DEFAULT_SEED, "a", 1, hi - lo, line, lo)[0]
    else:
        values = gm.operand_matrix(dtype, gm.DEFAULT_SEED, "b", hi - lo, 1, lo, line)[:, 0]
    return lo + int(np.flatnonzero(values)[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_shape_against_numpy(native, dtype):
    """What the probe runs: two workgroups or more per CU at non-zero LDS bases,
    every CU, 16 stages per workgroup."""
    r = native.gemm_exact(0, dtype)
    m, n, k = r["m"], r["n"], r["k"]
    assert r["ok"] is True and k == 1024 and r["workgroups"] >= 2 * r["cu_total"]
    assert 1 <= r["cu_seen"] <= r["cu_total"]
    _assert_model_dump(dtype, gm.DEFAULT_SEED, native.debug_gemm_dump(0, dtype, m, n, k), m, n, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_deepest_k(native, dtype):
    """K = 65536, the exactness limit: 1024 stages, the buffer parity all the way;
    then a fault in the last stage."""
    m, n, k = 64, 64, 65536
    ref = _assert_model_dump(dtype, gm.DEFAULT_SEED, native.debug_gemm_dump(0, dtype, m, n, k),
                             m, n, k)
    print(f"{dtype}: max |D| at K = 65536 is {np.abs(ref).max():.0f}")
    assert native.gemm_exact(0, dtype, m, n, k)["ok"] is True
    kk = _nonzero_k(dtype, "a", 61, 65472, 65536)
    assert 65472 <= kk < 65536
    r = _assert_line_fault(native, dtype, m, n, k, ("a", 61, kk, 0x8000))
    assert [f["tile"] for f in r["faulty"]] == [(0, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_widest_and_tallest_grid(native, dtype):
    """tiles_n = 1024 and its tall mirror, clean and with a fault in the last tile."""
    wide, tall = (64, 65536, 64), (65536, 64, 64)
    for shape in (wide, tall):
        r = native.gemm_exact(0, dtype, *shape)
        assert (r["ok"], r["mismatches"], r["faulty"], r["workgroups"]) == (True, 0, [], 1024)
    col = 65536 - 3
    r = _assert_line_fault(native, dtype, *wide, ("b", _nonzero_k(dtype, "b", col, 32, 64), col, 0x8000))
    assert [f["tile"] for f in r["faulty"]] == [(0, 1023)]
    row = 65536 - 3
    r = _assert_line_fault(native, dtype, *tall, ("a", row, _nonzero_k(dtype, "a", row, 32, 64), 0x8000))
    assert [f["tile"] for f in r["faulty"]] == [(1023, 0)]


@pytest.mark.parametrize("m", [32768, 65536])
def test_d_of_4_gib_and_beyond(native, m):
    """m x 32768 x 64. At m = 32768 C and D are 4 GiB each: byte offsets into them
    reach 2^32 - 4, past what a signed 32-bit offset holds. At m = 65536 they are
    8 GiB and the byte offsets pass 2^32. (The element indices stay below 2^32 at
    every shape the check accepts, so it is the 64-bit byte addressing that is
    pinned here.) Clean, then a fault in A's last row: the last tile row, all
    512 tile columns."""
    need = 4 * (m // 32768) * 4  # C and D, and as much again to be safe, in GiB
    free = native.device_info(0)["free_mem_gb"]
    if free < need:
        pytest.skip(f"{free:.1f} GiB free on the device; the case wants {need} GiB to be safe")
    n, row = 32768, m - 1
    r = native.gemm_exact(0, "bf16", m, n, 64)
    assert (r["ok"], r["mismatches"], r["faulty"], r["workgroups"]) == (True, 0, [], m // 64 * 512)
    r = _assert_line_fault(native, "bf16", m, n, 64, ("a", row, _nonzero_k("bf16", "a", row, 32, 64), 0x8000))
    assert [f["tile"] for f in r["faulty"]] == [(m // 64 - 1, t) for t in range(512)]
    assert r["first_bad"][0] == row and (row * n * 4 >= 1 << 32) is (m == 65536)


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_seed(native, dtype):
    m, n, k = 128, 192, 128
    _assert_model_dump(dtype, gm.SEED2, native.debug_gemm_dump(0, dtype, m, n, k, seed=gm.SEED2),
                       m, n, k)
    first = _unpack(dtype, native.debug_gemm_dump(0, dtype, m, n, k), m, n, k)[0]
    assert not np.array_equal(first, gm.operand_matrix(dtype, gm.SEED2, "a", m, k))  # another matrix
    for which, (rows, cols) in (("a", (m, k)), ("b", (k, n)), ("c", (m, n))):
        model = gm.operand_matrix(dtype, gm.SEED2, which, rows, cols)
        for r in range(0, rows, 17):
            for col in range(0, cols, 13):
                assert native.gemm_operand(dtype, which, r, col, seed=gm.SEED2) == model[r, col]
        assert native.gemm_operand(dtype, which, 0xFFFFFF03, 0x80000007, seed=gm.SEED2) == \
            gm.operand_matrix(dtype, gm.SEED2, which, 1, 1, 0xFFFFFF03, 0x80000007)[0, 0]
    r = native.gemm_exact(0, dtype, m, n, k, seed=gm.SEED2)
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)


def test_faulty_tiles_ran_where_the_sweep_has_been(native):
    """The location of a faulty tile is a CU of this device: one of the places a
    saturating CU sweep reports in its coverage map."""
    sweep = native.cu_sweep()
    if sweep["cu_covered"] < sweep["cu_total"]:
        sweep = native.cu_sweep(max_rounds=32)
    # an element of A that is 1 or -1 becomes Inf: its whole row of D is bad, three tiles
    row, col = gm.find_element(gm.operand_matrix("f16", gm.DEFAULT_SEED, "a", 128, 128), 1)
    r = native.gemm_exact(0, "f16", 128, 192, 128, inject=("a", row, col, 0x4000))
    assert len(r["faulty"]) == 3 and all(f["mismatches"] == 64 for f in r["faulty"])
    for f in r["faulty"]:
        assert all(isinstance(f[key], int) and f[key] >= 0 for key in ("xcc", "se", "sh", "cu"))
    if sweep["cu_covered"] < sweep["cu_total"]:
        pytest.skip(f"the CU sweep covered {sweep['cu_covered']} of {sweep['cu_total']} CUs: "
                    "its map cannot vouch for every location")
    known = {(l["xcc"], l["se"], l["sh"], l["cu"]) for l in sweep["locations"]}
    assert len(known) == sweep["cu_total"]
    assert all((f["xcc"], f["se"], f["sh"], f["cu"]) in known for f in r["faulty"])
