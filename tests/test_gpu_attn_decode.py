"""The burn-in's decode attention check on the device against numpy in float64, with ==:
finals and split partials from the dumped pools gathered through the dumped block table.
Cases (batch, kv_heads, group, splits, ctx): a single key, a full page, tails next to poison
in a wave's first and second page, a whole step, idle waves, empty splits, more splits than
steps, sequence and head offsets with mixed lengths, the exactness bound, group 1. With 600 and 4096 keys a wave's running maximum
rises after its first step (13 to 73 times a case, counted with the host reference)."""
import numpy as np
import pytest

from test_gpu_attn_exact import DTYPES, native  # noqa: F401  (the module-scoped build fixture)

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 1, (1,)), (1, 1, 8, 1, (16,)), (1, 1, 8, 1, (17,)), (1, 1, 8, 1, (33,)),
         (1, 1, 8, 1, (128,)), (1, 1, 8, 1, (129,)), (1, 1, 8, 4, (1,)), (1, 1, 8, 4, (300,)),
         (3, 2, 4, 2, (600, 5, 128)), (1, 1, 16, 4, (4096,)), (1, 1, 1, 2, (257,))]
FAULT_CASE = (2, 2, 4, 2, (300, 200))
_dumps = {}


def _softmax_state(q, k, v):
    """[O~ | m | l] of queries q over keys k, the empty state for no key at all."""
    if len(k) == 0:
        return np.column_stack([np.zeros((len(q), 128)), np.full(len(q), -np.inf), np.zeros(len(q))])
    s = q @ k.T
    p = 2.0 ** (s - s.max(1, keepdims=True))
    return np.column_stack([p @ v, s.max(1), p.sum(1)])


def _dump(native, dtype, case, inject=None):
    """The device's finals [rows, 130] and partials [rows, S, 130], numpy's of both from the
    dumped cache, q, the gathered K and V of every KV row, the table, the scores of every row."""
    key, (batch, kv_heads, group, S, ctx) = (dtype, case, inject), case
    if key not in _dumps:
        raw = native.debug_attn_decode_dump(0, dtype, batch, kv_heads, group, max(ctx), S, list(ctx),
                                            inject=inject)
        u = {x: np.frombuffer(raw[x], np.uint16) for x in ("q", "k_pool", "v_pool")}
        q, kp, vp = ((u[x].view(np.float16) if dtype == "f16" else (u[x].astype(np.uint32) << 16)
                      .view(np.float32)).astype(np.float64) for x in ("q", "k_pool", "v_pool"))
        q, kp, vp = q.reshape(-1, 128), kp.reshape(-1, kv_heads, 16, 128), vp.reshape(-1, kv_heads, 16, 128)
        table = np.frombuffer(raw["table"], np.int32).reshape(batch, -1)
        assert list(np.frombuffer(raw["ctx"], np.uint32)) == list(ctx) and table.max() < len(kp)
        owned = np.zeros((len(kp), 16), bool)
        for b, n in enumerate(ctx):
            owned[table[b, np.arange(n) // 16], np.arange(n) % 16] = True
        # every slot that no sequence owns holds the poison (a faulted table names another owner)
        for pool in ("k_pool", "v_pool") if inject is None or inject[0] != "table" else ():
            assert np.all(u[pool].reshape(-1, kv_heads, 16, 128).transpose(0, 2, 1, 3)[~owned]
                          == native.ATTN_DECODE_POISON)
        got = np.column_stack([np.frombuffer(raw["o"], np.float32).reshape(-1, 128)] + [
            np.frombuffer(raw[x], np.float32) for x in "ml"]).astype(np.float64)
        part = np.frombuffer(raw["partial"], np.float32).reshape(-1, S, 130).astype(np.float64)
        ref, ref_part, ks, vs, scores = [], [], [], [], []
        for kvrow in range(batch * kv_heads):
            b, hk, n = kvrow // kv_heads, kvrow % kv_heads, ctx[kvrow // kv_heads]
            pages = table[b, :-(-n // 16)]
            k, v = kp[pages, hk].reshape(-1, 128)[:n], vp[pages, hk].reshape(-1, 128)[:n]
            qg, ns = q[kvrow * group:(kvrow + 1) * group], -(-n // 128)
            ref.append(_softmax_state(qg, k, v))
            cut = [min(128 * (s * ns // S), n) for s in range(S + 1)]
            ref_part.append(np.stack([_softmax_state(qg, k[a:e], v[a:e]) for a, e in zip(cut, cut[1:])], 1))
            ks.append(k), vs.append(v), scores.append(qg @ k.T)
        _dumps[key] = (got, part, np.vstack(ref), np.vstack(ref_part), q, ks, vs, table, scores)
    return _dumps[key]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_equals_the_float64_reference(native, dtype, case):
    batch, kv_heads, group, S, ctx = case
    got, part, ref, ref_part, q, ks, vs, _, scores = _dump(native, dtype, case)
    assert got.shape == ref.shape == (batch * kv_heads * group, 130) and np.array_equal(got, ref)
    assert part.shape == ref_part.shape and np.array_equal(part, ref_part)
    assert (-np.inf in ref_part[:, :, 128]) == any(S > -(-n // 128) for n in ctx)  # empty splits
    r, j = len(q) - 1, ctx[-1] - 1  # the last query head, the last key of the last KV row
    assert [q[r, 85], ks[-1][j, 85], vs[-1][j, 85]] == [
        native.attn_decode_operand(dtype, x, row, 85) for x, row in
        (("q", r), ("k", (batch * kv_heads - 1) * 4096 + j), ("v", (batch * kv_heads - 1) * 4096 + j))]
    for s, n in zip(scores, np.repeat(ctx, kv_heads)):  # the premise on the data
        assert np.all(s == np.rint(s)) and np.all(s.max(1) - s.min(1) <= 8) and s.shape[1] == n
    assert all(np.abs(ref[kvrow * group:(kvrow + 1) * group, :128]).max() <= 8 * len(k)
               for kvrow, k in enumerate(ks))
    if max(ctx) > 128:  # a p < 1
        assert any(np.any(s < s.max(1, keepdims=True)) for s in scores)
    if case == CASES[7]:  # the merge's rescale: a split whose maximum lies below the row's
        assert np.any(np.isfinite(ref_part[:, :, 128]) & (ref_part[:, :, 128] < ref[:, None, 128]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_passes_at_the_default_shape(native, dtype):
    r = native.attn_decode_exact(0, dtype)
    print(f"attn_decode_exact {dtype}: main {r['elapsed_ms']:.3f} ms, merge {r['merge_ms']:.3f} ms, "
          f"{r['kv_bytes']} bytes, {r['gb_s']:.0f} GB/s, cu_seen {r['cu_seen']}/{r['cu_total']}")
    assert (r["ok"], r["mismatches"], r["faulty"], r["first_bad"]) == (True, 0, [], None)
    assert (r["dtype"], r["kv_heads"], r["group"], r["splits"], r["max_ctx"], r["head_dim"]) == (
        dtype, 8, 8, native.ATTN_DECODE_DEFAULT_SPLITS, native.ATTN_DECODE_DEFAULT_CTX, 128)
    want = native.GEMM_WORKGROUPS_PER_CU * r["cu_total"]
    assert r["workgroups"] == r["batch"] * 8 * r["splits"] and want <= r["workgroups"] < want + 8 * r["splits"]
    assert 1 <= r["cu_seen"] <= r["cu_total"] and r["m"] == r["batch"] * 64
    assert (native.ATTN_DECODE_MAX_CTX, native.ATTN_DECODE_PAGE_TOKENS) == (4096, 16)
    bad = native.attn_decode_exact(0, dtype, inject=("k", 5, 0, 0x4000))  # each tile of where[] is a CU
    assert bad["ok"] is False and bad["faulty"] and all(
        {"xcc", "se", "sh", "cu"} <= set(f) for f in bad["faulty"])


@pytest.mark.parametrize("which", ["q", "k", "v", "table"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_fault(native, dtype, which):
    """A sign flip of a non-zero element of sequence 1, or a table entry of it that points at a
    page of sequence 0, stays inside the premise."""
    batch, kv_heads, group, S, ctx = case = FAULT_CASE
    clean, clean_part, _, _, q, ks, vs, table, _ = _dump(native, dtype, case)
    if which == "table":  # logical page 3 of sequence 1 reads logical page 2 of sequence 0
        inject = ("table", 1, 3, int(table[1, 3] ^ table[0, 2]))
    else:
        mat, row, pos = {"q": (q, 14, 14), "k": (ks[2], 2 * 4096 + 150, 150), "v": (vs[3], 3 * 4096 + 37, 37)}[which]
        inject = (which, row, int(np.flatnonzero(mat[pos])[0]), 0x8000)
    got, part, faulted, faulted_part, fq, fks, fvs, ftable, _ = _dump(native, dtype, case, inject)
    if which == "table":
        assert np.argwhere(ftable != table).tolist() == [[1, 3]] and ftable[1, 3] == table[0, 2]
    else:
        want = mat.copy()
        want[pos, inject[2]] *= -1
        assert np.array_equal({"q": fq, "k": fks[2], "v": fvs[3]}[which], want)
    assert np.array_equal(got, faulted) and np.array_equal(part, faulted_part)
    bad = np.argwhere(faulted != clean)  # in sequence 1 alone
    assert len(bad) > 0 and bad[:, 0].min() >= kv_heads * group
    r = native.attn_decode_exact(0, dtype, batch, kv_heads, group, max(ctx), S, list(ctx), inject=inject)
    assert r["ok"] is False and r["mismatches"] == len(bad)
    assert r["first_bad"] == (*bad[0], faulted[tuple(bad[0])], clean[tuple(bad[0])])
    bad_part = np.argwhere(faulted_part != clean_part)  # (row, split, col): the workgroups
    tiles = sorted({(int(row) // group, int(s)) for row, s, _ in bad_part})
    assert [f["tile"] for f in r["faulty"]] == tiles and tiles
    assert all({"xcc", "se", "sh", "cu"} <= set(f) for f in r["faulty"])
    assert sum(f["mismatches"] for f in r["faulty"]) == len(bad_part)


@pytest.mark.parametrize("dtype,batch,kv_heads,group,max_ctx,splits,ctx,inject", [
    ("bf16", 1, 1, 3, 128, 1, None, None), ("bf16", 1, 1, 32, 128, 1, None, None),
    ("bf16", 1, 1, 8, 4097, 1, None, None), ("bf16", 1, 1, 8, -1, 1, None, None),
    ("bf16", 1, 1, 8, 128, 33, None, None), ("bf16", 1, -1, 8, 128, 1, None, None),
    ("bf16", -1, 1, 8, 128, 1, None, None), ("f16", 64, 64, 8, 4096, 1, None, None),
    ("bf16", 2, 1, 8, 128, 1, [5], None), ("bf16", 1, 1, 8, 128, 1, [0], None),
    ("bf16", 1, 1, 8, 128, 1, [129], None), ("fp8", 1, 1, 8, 128, 1, None, None),
    ("f16", 1, 1, 8, 128, 1, [100], ("q", 8, 0, 1)), ("f16", 1, 1, 8, 128, 1, [100], ("k", 100, 0, 1)),
    ("f16", 1, 1, 8, 128, 1, [100], ("v", 0, 128, 1)), ("f16", 1, 1, 8, 128, 1, [100], ("o", 0, 0, 1)),
    ("f16", 1, 1, 8, 128, 1, [100], ("table", 0, 8, 1)), ("f16", 1, 1, 8, 128, 1, [100], ("table", 0, 0, 8)),
    ("f16", 1, 1, 8, 128, 1, [100], ("table", 1, 0, 1)), ("f16", 1, 1, 8, 128, 1, [100], ("q", 0, 0, 0))])
def test_bad_arguments_raise(native, dtype, batch, kv_heads, group, max_ctx, splits, ctx, inject):
    with pytest.raises(ValueError):
        native.attn_decode_exact(0, dtype, batch, kv_heads, group, max_ctx, splits, ctx, inject=inject)
