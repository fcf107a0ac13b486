"""The burn-in's attention check on the device against numpy in float64 from
the dumped raw operands; every sum is a multiple of 2^-8 below 2^15, so == is
the compare. Shapes (M, N): one block, the first rescale and buffer swap, a
reused stage, several workgroups, the exactness bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "f16")
SHAPES = [(64, 64), (64, 128), (64, 192), (128, 256), (64, 4096)]


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    assert (gpuhealth.ATTN_MAX_N, gpuhealth.ATTN_HEAD_DIM) == (4096, 64)
    return gpuhealth


def _decode(raw, dtype, rows):
    u = np.frombuffer(raw, np.uint16).reshape(rows, 64)
    f = u.view(np.float16) if dtype == "f16" else (u.astype(np.uint32) << 16).view(np.float32)
    return f.astype(np.float64)


_dumps = {}


def _dump(native, dtype, shape, inject=None):
    """Decoded Q, K, V, [O~ | m | l] (M x 66) of the device and of numpy, the scores."""
    key, (m, n) = (dtype, shape, inject), shape
    if key not in _dumps:
        raw = native.debug_attn_dump(0, dtype, m, n, inject=inject)
        q, k, v = (_decode(raw[x], dtype, rows) for x, rows in (("q", m), ("k", n), ("v", n)))
        got = np.column_stack([np.frombuffer(raw["o"], np.float32).reshape(m, 64),
                               np.frombuffer(raw["m"], np.float32),
                               np.frombuffer(raw["l"], np.float32)]).astype(np.float64)
        s = q @ k.T
        p = 2.0 ** (s - s.max(1, keepdims=True))
        _dumps[key] = (q, k, v, got, np.column_stack([p @ v, s.max(1), p.sum(1)]), s)
    return _dumps[key]


def test_permlane_swap_lane_maps(native):
    """vdst = lane, vsrc = 64 + lane. The 16-lane swap exchanges rows 1 and 3 of
    vdst with rows 0 and 2 of vsrc, the 32-lane swap their upper and lower halves."""
    got = np.array(native.debug_permlane_dump(0))
    lane = np.arange(64)
    odd = (lane >> 4) & 1 == 1
    assert np.array_equal(got[0], np.where(odd, 64 + lane - 16, lane))
    assert np.array_equal(got[1], np.where(odd, 64 + lane, lane + 16))
    assert np.array_equal(got[2], np.where(lane >= 32, 64 + lane - 32, lane))
    assert np.array_equal(got[3], np.where(lane >= 32, 64 + lane, lane + 32))


def test_exp2_is_exact_on_integers(native):
    """v_exp_f32 on 0, -1, .., -126 and -inf. Production feeds it -8 .. 0 and -inf."""
    got = np.array(native.debug_exp2_dump(0), np.float64)
    want = 2.0 ** -np.arange(127.0)
    print("v_exp_f32 inexact at 2^-n for n =", np.flatnonzero(got[:127] != want).tolist())
    assert np.array_equal(got[:9], want[:9]) and got[127] == 0.0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_equals_the_float64_reference(native, dtype, shape):
    q, k, v, got, ref, s = _dump(native, dtype, shape)
    assert np.array_equal(got, ref)
    for which, mat in (("q", q), ("k", k), ("v", v)):
        for r, c in [(0, 0), (1, 0), (0, 1), (len(mat) - 1, 63), (len(mat) // 2, 21)]:
            assert mat[r, c] == native.attn_operand(dtype, which, r, c)
    assert np.abs(q).max() == 2 and np.abs(v).max() == 8 and np.all(q == np.rint(q))
    assert np.all((k != 0).sum(1) == 2) and set(np.unique(k)) == {-1.0, 0.0, 1.0}
    assert np.all(s.max(1) - s.min(1) <= 8) and np.abs(ref[:, :64]).max() <= 8 * shape[1]
    if shape[1] > 64:  # the rescale path: a maximum that rises after the first block, and p < 1
        assert np.any(s.argmax(1) >= 64) and np.any(s < s.max(1, keepdims=True))


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_passes_at_the_default_shape(native, dtype):
    r = native.attn_exact(0, dtype)
    print(f"attn_exact {dtype}: {r['elapsed_ms']:.3f} ms, cu_seen {r['cu_seen']}/{r['cu_total']}")
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)
    assert (r["dtype"], r["n"], r["head_dim"]) == (dtype, native.ATTN_DEFAULT_N, 64)
    assert r["m"] == 64 * native.GEMM_WORKGROUPS_PER_CU * r["cu_total"] == 64 * r["workgroups"]
    assert 1 <= r["cu_seen"] <= r["cu_total"]


@pytest.mark.parametrize("which", "qkv")
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_fault(native, dtype, which):
    """A sign flip of a non-zero element stays inside the premise."""
    m, n = shape = (128, 256)
    q, k, v, _, clean, _ = _dump(native, dtype, shape)
    mat, row = {"q": (q, m - 3), "k": (k, 64 + 5), "v": (v, 64 + 9)}[which]
    inject = (which, row, int(np.flatnonzero(mat[row])[0]), 0x8000)
    *ops, got, faulted, _ = _dump(native, dtype, shape, inject)
    want = mat.copy()
    want[row, inject[2]] *= -1
    assert np.array_equal(ops["qkv".index(which)], want) and np.array_equal(got, faulted)
    bad = np.argwhere(faulted != clean)
    r = native.attn_exact(0, dtype, m, n, inject=inject)
    assert r["ok"] is False and r["mismatches"] == len(bad) > 0
    y, x = (int(t) for t in bad[0])
    assert r["first_bad"] == (y, x, faulted[y, x], clean[y, x])
    assert [f["tile"] for f in r["faulty"]] == [(int(t), 0) for t in np.unique(bad[:, 0] // 64)]
    assert [f["tile"] for f in r["faulty"]] == ([(1, 0)] if which == "q" else [(0, 0), (1, 0)])
    assert all({"xcc", "se", "sh", "cu"} <= set(f) and f["mismatches"] > 0 for f in r["faulty"])
    assert sum(f["mismatches"] for f in r["faulty"]) == len(bad)


def test_bad_arguments_raise(native):
    for dtype, m, n in [("bf16", 65, 64), ("bf16", 64, 96), ("bf16", 64, 4096 + 64), ("fp8", 64, 64)]:
        with pytest.raises(ValueError):
            native.attn_exact(0, dtype, m, n)
    for inject in [("q", 64, 0, 1), ("k", 128, 0, 1), ("v", 0, 64, 1), ("o", 0, 0, 1), ("q", 0, 0, 0x10000)]:
        with pytest.raises(ValueError):
            native.attn_exact(0, "f16", 64, 128, inject=inject)
