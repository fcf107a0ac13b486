"""The burn-in's MoE check on the device against numpy in float64, with ==: the per-entry
products P and the atomically summed Y, guard rows included, from the dumped operands and the
dumped routing. Cases (T, E, top_k, K, N, route): one entry under 63 masked rows; a full tile,
two stages; a one-row tail; empty experts first and in the middle, two N tiles; trailing empty
experts, idle workgroups; two atomic contributions a row; the bound; the generated routing."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_attn_exact import DTYPES, native  # noqa: F401  (the module-scoped build fixture)

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 64, 64, None), (64, 1, 1, 128, 64, None), (65, 1, 1, 64, 64, None),
         (3, 4, 1, 64, 128, (1, 1, 3)), (2, 4, 1, 64, 64, (0, 0)), (70, 2, 2, 64, 64, None),
         (8, 8, 8, 4096, 64, None), (200, 5, 2, 192, 128, None)]
FAULT_CASE = (70, 4, 2, 128, 128, None)


def _floats(raw, dtype):
    u = np.frombuffer(raw, np.uint16)
    f = u.view(np.float16) if dtype == "f16" else (u.astype(np.uint32) << 16).view(np.float32)
    return f.astype(np.float64)


def _dump(native, dtype, case, inject=None):
    """The device's p and y; numpy's ref_p and ref_y from the dumped operands and routing; x (no
    poison row), w, offsets, and token, weight, expert and row tile of every sorted entry."""
    T, E, top_k, K, N, route = case
    raw = native.debug_moe_dump(0, dtype, T, E, top_k, K, N, route and list(route),
                                inject=inject)
    d = SimpleNamespace(x=_floats(raw["x"], dtype).reshape(T + 1, K),
                        w=_floats(raw["w"], dtype).reshape(E, K, N))
    assert np.all(np.frombuffer(raw["x"], np.uint16)[T * K:] == native.MOE_POISON)
    d.offsets = np.frombuffer(raw["offsets"], np.uint32).astype(np.int64)
    d.token = np.frombuffer(raw["sorted_token"], np.uint32).astype(np.int64)
    d.weight = np.frombuffer(raw["sorted_weight"], np.float32).astype(np.float64)
    d.expert = np.repeat(np.arange(E), np.diff(d.offsets))
    assert d.offsets[0] == 0 and d.offsets[-1] == len(d.token) == len(d.expert) == T * top_k
    d.ref_p = np.zeros((T * top_k + 64, N))
    for e, (a, b) in enumerate(zip(d.offsets, d.offsets[1:])):
        d.ref_p[a:b] = d.x[d.token[a:b]] @ d.w[e]
    d.ref_y = np.zeros((T + 1, N))
    np.add.at(d.ref_y, d.token, d.weight[:, None] * d.ref_p[:T * top_k])
    d.p = np.frombuffer(raw["p"], np.float32).reshape(-1, N).astype(np.float64)
    d.y = np.frombuffer(raw["y"], np.float32).reshape(-1, N).astype(np.float64)
    tiles = -(-np.diff(d.offsets) // 64)  # row tiles of each expert, none for an empty one
    d.tile = (np.cumsum(tiles) - tiles)[d.expert] + (
        np.arange(T * top_k) - d.offsets[d.expert]) // 64
    d.x = d.x[:T]
    return d


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_moe_equals_the_float64_reference(native, dtype, case):
    T, E, top_k, K, N, route = case
    d = _dump(native, dtype, case)
    assert d.p.shape == d.ref_p.shape == (T * top_k + 64, N) and np.array_equal(d.p, d.ref_p)
    assert d.y.shape == d.ref_y.shape == (T + 1, N) and np.array_equal(d.y, d.ref_y)
    assert not d.p[T * top_k:].any() and not d.y[T].any()  # the guards; below, the premise
    assert all(np.all(m == np.rint(m)) and np.abs(m).max() <= 8 for m in (d.x, d.w))
    assert set(d.weight) <= {1.0, 0.5, 0.25} and np.abs(d.ref_y).max() * 4 < 2 ** 24
    pairs = set(zip(d.token.tolist(), d.expert.tolist()))  # distinct experts per token
    assert len(pairs) == T * top_k and np.all(np.bincount(d.token, minlength=T) == top_k)
    assert all(np.all(np.diff(d.token[a:b]) > 0) for a, b in zip(d.offsets, d.offsets[1:]))
    if route is not None:
        assert sorted(pairs) == sorted(enumerate(route))
    assert d.x[T - 1, K - 1] == native.moe_operand(dtype, "x", T - 1, K - 1)
    assert d.w[E - 1, K - 1, N - 1] == native.moe_operand(dtype, "w", E * K - 1, N - 1)
    r = native.moe_exact(0, dtype, T, E, top_k, K, N, route and list(route))
    tiles = int(d.tile.max()) + 1
    assert (r["ok"], r["mismatches"], r["faulty"]) == (True, 0, [])
    assert (r["tiles"], r["workgroups"], r["entries"]) == (tiles, tiles * (N // 64), T * top_k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_passes_at_the_default_shape(native, dtype):
    r = native.moe_exact(0, dtype)
    print(f"moe_exact {dtype}: {r['tokens']} tokens, {r['tiles']} row tiles, "
          f"{r['elapsed_ms']:.3f} ms, {r['tflops']:.0f} TFLOP/s, "
          f"cu_seen {r['cu_seen']}/{r['cu_total']}")
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)
    assert (r["dtype"], r["experts"], r["top_k"], r["k"], r["n"]) == (dtype, 16, 2, 1024, 1024)
    assert r["tokens"] % 64 == 0 and r["entries"] == 2 * r["tokens"]
    assert r["workgroups"] == 16 * r["tiles"] >= native.GEMM_WORKGROUPS_PER_CU * r["cu_total"]
    assert 1 <= r["cu_seen"] <= r["cu_total"]
    offsets = np.frombuffer(native.debug_moe_dump(0, dtype)["offsets"], np.uint32)
    sizes = np.diff(offsets.astype(np.int64))  # an empty expert, a ragged group, unequal loads
    assert sizes.sum() == r["entries"] and (sizes == 0).any() and (sizes % 64 != 0).any() and len(set(sizes[sizes > 0])) > 1
    col = next(c for c in range(1024) if native.moe_operand(dtype, "x", 5, c))
    bad = native.moe_exact(0, dtype, inject=("x", 5, col, 0x8000))  # a tile of where[] is a CU
    assert bad["ok"] is False and bad["faulty"]
    assert all({"xcc", "se", "sh", "cu"} <= set(f) for f in bad["faulty"])
    assert (native.MOE_MAX_K, native.MOE_MAX_TOP_K) == (4096, 8)


@pytest.mark.parametrize("which", ["x", "w", "route"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_fault(native, dtype, which):
    """A sign flip of a non-zero element of X or W, or a sorted entry that names its token's
    neighbour, stays inside the premise."""
    T, E, top_k, K, N, _ = FAULT_CASE
    clean = _dump(native, dtype, FAULT_CASE)
    entry = int(clean.offsets[2]) + 3  # of expert 2, whose group is not the first
    want_x, want_w, want_token = clean.x.copy(), clean.w.copy(), clean.token.copy()
    if which == "x":
        inject = ("x", 14, int(np.flatnonzero(clean.x[14])[0]), 0x8000)
        want_x[14, inject[2]] *= -1
    elif which == "w":
        inject = ("w", 2 * K + 37, int(np.flatnonzero(clean.w[2, 37])[0]), 0x8000)
        want_w[2, 37, inject[2]] *= -1
    else:
        inject = ("route", entry, 0, 1)
        want_token[entry] ^= 1
    bad = _dump(native, dtype, FAULT_CASE, inject)
    assert np.array_equal(bad.x, want_x) and np.array_equal(bad.w, want_w)
    assert np.array_equal(bad.token, want_token)
    assert np.array_equal(bad.p, bad.ref_p) and np.array_equal(bad.y, bad.ref_y)
    bad_y = np.argwhere(bad.ref_y != clean.ref_y)
    assert len(bad_y) > 0 and not bad.ref_y[T].any()
    if which == "route":  # the token that lost a product and the one that got it
        assert {int(clean.token[entry]), int(clean.token[entry]) ^ 1} <= set(bad_y[:, 0].tolist())
    r = native.moe_exact(0, dtype, T, E, top_k, K, N, inject=inject)
    first = tuple(bad_y[0])
    assert r["ok"] is False and r["mismatches"] == len(bad_y)
    assert r["first_bad"] == (*first, bad.ref_y[first], clean.ref_y[first])
    bad_p = np.argwhere(bad.ref_p != clean.ref_p)  # (entry, col): the workgroups
    tiles = sorted({(int(clean.tile[e]), int(c) // 64) for e, c in bad_p})
    assert [f["tile"] for f in r["faulty"]] == tiles and tiles
    assert all({"xcc", "se", "sh", "cu"} <= set(f) for f in r["faulty"])
    assert sum(f["mismatches"] for f in r["faulty"]) == len(bad_p)


@pytest.mark.parametrize("dtype,T,E,top_k,K,N,route", [
    ("fp8", 4, 2, 1, 64, 64, None), ("bf16", 4, 2, 1, 96, 64, None),
    ("bf16", 4, 2, 1, 64, 32, None), ("bf16", 4, 2, 1, -64, 64, None),
    ("bf16", 4, 2, 1, 4160, 64, None), ("bf16", 4, 65, 1, 64, 64, None),
    ("bf16", 4, -1, 1, 64, 64, None), ("bf16", 4, 2, 3, 64, 64, None),
    ("bf16", 4, 16, 9, 64, 64, None), ("bf16", 4, 2, -1, 64, 64, None),
    ("bf16", -1, 2, 1, 64, 64, None), ("bf16", 65537, 2, 1, 64, 64, None),
    ("bf16", 65536, 64, 8, 4096, 65536, None), ("bf16", 4, 2, 1, 64, 64, [0, 1, 0]),
    ("bf16", 2, 2, 1, 64, 64, [0, 2]), ("bf16", 2, 2, 1, 64, 64, [0, -1]),
    ("bf16", 2, 2, 2, 64, 64, [0, 1, 1, 1]), ("bf16", 0, 2, 2, 64, 64, [0]),
    ("bf16", 0, 2, 2, 64, 64, [0, 1, 0])])
def test_bad_arguments_raise(native, dtype, T, E, top_k, K, N, route):
    with pytest.raises(ValueError):
        native.moe_exact(0, dtype, T, E, top_k, K, N, route)


@pytest.mark.parametrize("inject", [
    ("x", 4, 0, 1), ("x", 0, 64, 1), ("w", 128, 0, 1), ("w", 0, 64, 1), ("y", 0, 0, 1),
    ("x", 0, 0, 0), ("x", 0, 0, 0x10000), ("route", 4, 0, 1), ("route", 0, 1, 1),
    ("route", 0, 0, 4), ("route", 0, 0, 0)])
def test_bad_injects_raise(native, inject):
    with pytest.raises(ValueError):
        native.moe_exact(0, "f16", 4, 2, 1, 64, 64, inject=inject)
