"""The burn-in's causal attention check on the device against numpy in float64 from
the dumped operands, with ==. Cases (heads, seq, causal): one workgroup with the mask in
every wave position, stage reuse across a pair, head offsets, no mask, the exactness bound."""
import numpy as np
import pytest

from test_gpu_attn_exact import DTYPES, native  # noqa: F401  (the module-scoped build fixture)

pytestmark = pytest.mark.gpu

CASES = [(1, 128, True), (1, 256, True), (3, 256, True), (1, 256, False), (1, 4096, True)]
_dumps = {}


def _dump(native, dtype, case, inject=None):
    """Decoded Q, K, V, [O~ | m | l] (rows x 130) of the device and of numpy, the masked scores."""
    key, (heads, seq, causal) = (dtype, case, inject), case
    if key not in _dumps:
        raw = native.debug_attn_causal_dump(0, dtype, heads, seq, causal, inject=inject)
        u = {x: np.frombuffer(raw[x], np.uint16).reshape(-1, 128) for x in "qkv"}
        q, k, v = ((u[x].view(np.float16) if dtype == "f16" else
                    (u[x].astype(np.uint32) << 16).view(np.float32)).astype(np.float64) for x in "qkv")
        got = np.column_stack([np.frombuffer(raw["o"], np.float32).reshape(-1, 128)] + [
            np.frombuffer(raw[x], np.float32) for x in "ml"]).astype(np.float64)
        ref, scores = [], []
        for h in range(heads):
            rows = slice(h * seq, (h + 1) * seq)
            s = q[rows] @ k[rows].T
            if causal:
                s[np.triu_indices(seq, 1)] = -np.inf
            p = 2.0 ** (s - s.max(1, keepdims=True))
            ref.append(np.column_stack([p @ v[rows], s.max(1), p.sum(1)]))
            scores.append(s)
        _dumps[key] = (q, k, v, got, np.vstack(ref), np.vstack(scores).astype(np.float32))
    return _dumps[key]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_equals_the_float64_reference(native, dtype, case):
    heads, seq, causal = case
    q, k, v, got, ref, s = _dump(native, dtype, case)
    assert got.shape == ref.shape == (heads * seq, 130) and np.array_equal(got, ref)
    r = heads * seq - 1
    assert [m[r, 85] for m in (q, k, v)] == [native.attn_causal_operand(dtype, x, r, 85) for x in "qkv"]
    seen = np.isfinite(s)  # the premise on the data
    assert np.all(s[seen] == np.rint(s[seen])) and np.abs(ref[:, :128]).max() <= 8 * seq
    assert np.all(s.max(1) - np.where(seen, s, np.inf).min(1) <= 8)
    assert np.abs(q).max() == 2 and np.abs(v).max() == 8 and np.all((k != 0).sum(1) == 2)
    if seq > 128:  # the rescale path: a maximum that rises after the first key block, and p < 1
        assert np.any(s.max(1) > s[:, :64].max(1)) and np.any(seen & (s < s.max(1, keepdims=True)))
    if causal:  # a head's first query sees its first key alone
        first = np.arange(heads) * seq
        assert np.array_equal(got[first, :128], v[first]) and np.all(got[first, 129] == 1)
        assert np.array_equal(got[first, 128], (q[first] * k[first]).sum(1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_passes_at_the_default_shape(native, dtype):
    r = native.attn_causal_exact(0, dtype)
    print(f"attn_causal_exact {dtype}: {r['elapsed_ms']:.3f} ms, cu_seen {r['cu_seen']}/{r['cu_total']}")
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)
    assert (r["dtype"], r["seq"], r["head_dim"], r["causal"]) == (dtype, 1024, 128, True)
    assert (native.ATTN_CAUSAL_DEFAULT_SEQ, native.ATTN_CAUSAL_HEAD_DIM,
            native.ATTN_CAUSAL_MAX_SEQ) == (1024, 128, 4096)
    want = native.GEMM_WORKGROUPS_PER_CU * r["cu_total"]
    assert r["workgroups"] == r["heads"] * 8 and want <= r["workgroups"] < want + 8
    assert 1 <= r["cu_seen"] <= r["cu_total"] and (r["m"], r["n"]) == (r["heads"] * 1024, 1024)


@pytest.mark.parametrize("which", "qkv")
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_fault(native, dtype, which):
    """A sign flip of a non-zero element of head 1 stays inside the premise."""
    heads, seq, _ = case = (2, 256, True)
    q, k, v, _, clean, _ = _dump(native, dtype, case)
    mat, row = {"q": (q, 2 * seq - 3), "k": (k, seq + 64 + 5), "v": (v, seq + 64 + 9)}[which]
    inject = (which, row, int(np.flatnonzero(mat[row])[0]), 0x8000)
    *ops, got, faulted, _ = _dump(native, dtype, case, inject)
    want = mat.copy()
    want[row, inject[2]] *= -1
    assert np.array_equal(ops["qkv".index(which)], want) and np.array_equal(got, faulted)
    bad = np.argwhere(faulted != clean)  # not in head 0, nor in the queries before a key or value
    assert len(bad) > 0 and bad[:, 0].min() >= (row if which != "q" else seq)
    r = native.attn_causal_exact(0, dtype, heads, seq, inject=inject)
    assert r["ok"] is False and r["mismatches"] == len(bad)
    assert r["first_bad"] == (*bad[0], faulted[tuple(bad[0])], clean[tuple(bad[0])])
    qb = bad[:, 0] % seq // 64  # the workgroup of a row: its head's pairs, then its query block's pair
    tiles = np.unique(bad[:, 0] // seq * (seq // 128) + np.minimum(qb, seq // 64 - 1 - qb))
    assert [f["tile"] for f in r["faulty"]] == [(int(t), 0) for t in tiles]
    assert all({"xcc", "se", "sh", "cu"} <= set(f) and f["mismatches"] > 0 for f in r["faulty"])
    assert sum(f["mismatches"] for f in r["faulty"]) == len(bad)


@pytest.mark.parametrize("dtype,heads,seq,inject", [
    ("bf16", 1, 64, None), ("bf16", 1, 192, None), ("bf16", 1, -128, None), ("bf16", 1, 4224, None),
    ("bf16", -1, 128, None), ("bf16", 1025, 128, None), ("f16", 64, 4096, None),
    ("fp8", 1, 128, None), ("mxfp4", 1, 128, None),
    ("f16", 2, 128, ("q", 256, 0, 1)), ("f16", 2, 128, ("k", 256, 0, 1)),
    ("f16", 2, 128, ("v", 0, 128, 1)), ("f16", 2, 128, ("o", 0, 0, 1)),
    ("f16", 2, 128, ("q", 0, 0, 0x10000)), ("f16", 2, 128, ("q", 0, 0, 0))])
def test_bad_arguments_raise(native, dtype, heads, seq, inject):
    with pytest.raises(ValueError):
        native.attn_causal_exact(0, dtype, heads, seq, inject=inject)
