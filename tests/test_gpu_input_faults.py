"""Seeded faults that enter the burn-in from the input side.

The other probe tests seed every fault after the work is done: an xor into D,
or into one memory word in one named phase. Here the fault goes in where a real
one would:

* into one operand register of one lane before the MFMA reads it
  (``inject_operand=``), so that the device shows which element of A, B, C or
  of the MX scales each register of each lane is, which registers the MX
  instruction ignores, and that the check flags a fault that came in through
  an operand. The expected D is tests/gpuhealth_model.py's register model with
  the same xor applied, in float64.
* as a stuck-at bit of one HBM word (``stuck=``) or of one LDS word
  (``inject_lds_stuck=``), forced after every fill of every pass and both
  phases. A stuck bit disagrees with the pattern in exactly one of the two
  phases, whichever value the pattern wants there; that is what the moving
  inversion buys, and a sweep that does not invert, or that runs fewer passes
  than it was asked for, gives other counts. Expectations come from
  ``pattern_words`` alone.

The conditions that make the MFMA comparison exact are asserted on the case
table without a GPU. Subnormal operands are out of scope: every finite case
flips a bit of an element whose clean and faulted codes are both normal numbers
of their format. Every comparison is exact. A seeded fault only makes a
comparison fail: each write lands in a live allocation, in the workgroup's own
LDS or in its own registers.
"""
import collections
import functools
import math
import struct

import numpy as np
import pytest

import gpuhealth_model as model
from gpuhealth_model import DTYPES, M32, pattern_words

MIB = 1 << 20
SEED = 0x5EED1234            # gh::kDefaultSeed; the GPU tests check that it is
SEED2 = 0x0BADC0DE
WORKGROUPS = 1024
TILES = (0, WORKGROUPS - 1)


@pytest.fixture(scope="module")
def native():
    from kuberay_amd._native.build import build_gpuhealth
    build_gpuhealth()
    from kuberay_amd._native import gpuhealth
    assert gpuhealth.DEFAULT_SEED == SEED
    return gpuhealth


# ---------------------------------------------------------------------------
# the operand-fault case table
# ---------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name dtype wg lane operand reg mask kind what")
# kind: finite | control | nonfinite; what: the bit or byte that is flipped

ELEMENT_BITS = {"bf16": 16, "f16": 16, "fp8": 8, "mxfp4": 4}
DATA_DWORDS = {"bf16": 4, "f16": 4, "fp8": 2, "mxfp4": 4}
# sign, the lowest bit the generators toggle, and a third: bit 0, which the
# generators never set in bf16 / f16 / e4m3 (e2m1 has no such bit: its bit 0 is
# the lowest toggled one and the third is the high exponent bit)
ELEMENT_FLIPS = {"bf16": (("sign", 15), ("toggled", 5), ("bit0", 0)),
                 "f16": (("sign", 15), ("toggled", 8), ("bit0", 0)),
                 "fp8": (("sign", 7), ("toggled", 1), ("bit0", 0)),
                 "mxfp4": (("sign", 3), ("toggled", 0), ("exp", 2))}
CORNER_LANES = [16 * g + i for g in range(4) for i in (0, 15)]


def _is_normal(dtype, code):
    """The element code is a normal, finite, non-zero number of its format."""
    if dtype == "bf16":
        return 0 < (code >> 7) & 0xFF < 0xFF
    if dtype == "f16":
        return 0 < (code >> 10) & 0x1F < 0x1F
    if dtype == "fp8":
        return (code >> 3) & 0xF > 0 and code & 0x7F != 0x7F
    return code & 7 >= 2          # e2m1: 1, 1.5, 2, 3, 4, 6


def _element_code(dtype, regs, operand, lane, pos):
    if dtype == "mxfp4":
        return (regs[operand][lane][pos // 2] >> (4 * (pos % 2))) & 15
    return regs[operand][lane][pos]


@functools.lru_cache(maxsize=None)
def _regs(dtype, wg):
    return model.pack_registers(dtype, SEED, wg)


@functools.lru_cache(maxsize=None)
def _clean_tile(dtype, wg):
    tile = model.tile_from_registers(dtype, _regs(dtype, wg))
    tile.setflags(write=False)
    return tile


def _faulted_regs(case):
    return model.xor_register(case.dtype, _regs(case.dtype, case.wg), case.lane, case.operand,
                              case.reg, case.mask)


def _faulted_tile(case):
    return model.tile_from_registers(case.dtype, _faulted_regs(case))


def _differs(a, b):
    """Elementwise: not the same value; a NaN differs from everything."""
    return ~(a == b)


def _changed(case):
    return np.argwhere(_differs(_faulted_tile(case), _clean_tile(case.dtype, case.wg)))


def _element_case(dtype, wg, operand, lane, flip, bit, start):
    """One A or B case at that lane: the first of the four corner positions
    (first and last register, low and high element of the dword), tried from
    `start` on and then the lane's other elements, whose element is a normal
    number before and after the flip and whose fault reaches at least 8
    elements of D."""
    width = ELEMENT_BITS[dtype]
    per_dword = 32 // width
    last = DATA_DWORDS[dtype] * per_dword - 1
    corners = [0, per_dword - 1, last - per_dword + 1, last]
    corners = corners[start % 4:] + corners[:start % 4]
    for pos in corners + [p for p in range(last + 1) if p not in corners]:
        code = _element_code(dtype, _regs(dtype, wg), operand, lane, pos)
        if not (_is_normal(dtype, code) and _is_normal(dtype, code ^ (1 << bit))):
            continue
        case = Case(f"{operand}-lane{lane}-el{pos}-{flip}", dtype, wg, lane, operand,
                    pos // per_dword, 1 << (width * (pos % per_dword) + bit), "finite",
                    (flip, pos))
        if len(_changed(case)) >= 8:
            return case
    raise AssertionError(f"{dtype} tile {wg} {operand} lane {lane} {flip}: no usable element")


def _c_cases(dtype, wg):
    """Sign and one high mantissa bit, first and last register, at the first
    lane from a spread of starts whose C there is not zero."""
    out = []
    for n, (reg, flip, bit) in enumerate(((0, "sign", 31), (3, "sign", 31),
                                          (0, "mantissa", 22), (3, "mantissa", 22))):
        lane = next(l % 64 for l in range(21 * n, 21 * n + 64)
                    if _regs(dtype, wg)["c"][l % 64][reg] != 0.0)
        out.append(Case(f"c-lane{lane}-reg{reg}-{flip}", dtype, wg, lane, "c", reg, 1 << bit,
                        "finite", (flip, reg)))
    return out


def _scale_cases(wg):
    out = []
    for n, (operand, bit) in enumerate((("sa", 0), ("sa", 1), ("sb", 0), ("sb", 1))):
        for lane in CORNER_LANES[2 * n + 1:] + CORNER_LANES[:2 * n + 1]:
            case = Case(f"{operand}-lane{lane}-bit{bit}", "mxfp4", wg, lane, operand, 0, 1 << bit,
                        "finite", ("scale", bit))
            if len(_changed(case)) >= 8:
                out.append(case)
                break
        else:
            raise AssertionError(f"mxfp4 tile {wg} {operand} bit {bit}: no usable lane")
    # what the instruction is documented to ignore: bytes 1..3 of a scale
    # register (opsel 0) and VGPRs 4..7 of the eight-VGPR FP4 operand
    for lane, operand, reg, mask in ((5, "sa", 0, 1 << 8), (58, "sb", 0, 1 << 15),
                                     (21, "sa", 0, 0xFFFFFF00), (0, "a", 4, 1),
                                     (63, "a", 7, 1 << 31), (17, "b", 4, M32),
                                     (46, "b", 7, 0x00010000)):
        out.append(Case(f"control-{operand}-lane{lane}-reg{reg}-{mask:#x}", "mxfp4", wg, lane,
                        operand, reg, mask, "control", ("ignored", reg)))
    return out


def _nonfinite_case(dtype, wg):
    """bf16 / f16: an exponent flip that turns a 1.0 into +inf (0x3F80 ^ 0x4000,
    0x3C00 ^ 0x4000); e4m3: the flips that turn a non-zero element into 0x7F,
    the NaN. In A on the first tile, in B on the last."""
    operand = "a" if wg == 0 else "b"
    regs = _regs(dtype, wg)
    width = ELEMENT_BITS[dtype]
    per_dword = 32 // width
    one = {"bf16": 0x3F80, "f16": 0x3C00}.get(dtype)
    for lane in range(7, 64 + 7):
        lane %= 64
        for pos in range(8):
            code = regs[operand][lane][pos]
            if dtype == "fp8" and code & 0x7F != 0:
                flip = code ^ 0x7F
            elif code == one:
                flip = 0x4000
            else:
                continue
            return Case(f"nonfinite-{operand}-lane{lane}-el{pos}", dtype, wg, lane, operand,
                        pos // per_dword, flip << (width * (pos % per_dword)), "nonfinite",
                        ("nonfinite", pos))
    raise AssertionError(f"{dtype} tile {wg}: no element to make non-finite")


@functools.lru_cache(maxsize=None)
def operand_cases(dtype, wg):
    cases = []
    for operand in ("a", "b"):
        for li, lane in enumerate(CORNER_LANES):
            for fi, (flip, bit) in enumerate(ELEMENT_FLIPS[dtype]):
                cases.append(_element_case(dtype, wg, operand, lane, flip, bit, li + fi))
    cases += _c_cases(dtype, wg)
    if dtype == "mxfp4":
        cases += _scale_cases(wg)
    else:
        cases.append(_nonfinite_case(dtype, wg))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


TABLE = [(dtype, wg) for dtype in DTYPES for wg in TILES]


# ---------------------------------------------------------------------------
# CPU: the model's xor, and the conditions on the case table
# ---------------------------------------------------------------------------
def test_xor_register_is_little_endian():
    """Dword reg of a 16-bit operand is elements 2 reg (low half) and
    2 reg + 1; of a byte operand bytes 4 reg .. 4 reg + 3; of C the fp32 bits.
    The registers handed in stay as they were."""
    regs = _regs("bf16", 0)
    out = model.xor_register("bf16", regs, 37, "a", 3, 0x80000001)
    assert out["a"][37][6] == regs["a"][37][6] ^ 1
    assert out["a"][37][7] == regs["a"][37][7] ^ 0x8000
    assert out["a"][37][:6] == regs["a"][37][:6] and out["b"] == regs["b"]
    assert out["a"][36] == regs["a"][36] and regs == model.pack_registers("bf16", SEED, 0)
    fp8 = model.xor_register("fp8", _regs("fp8", 0), 2, "b", 1, 0x7F000100)
    assert fp8["b"][2][5] == _regs("fp8", 0)["b"][2][5] ^ 1
    assert fp8["b"][2][7] == _regs("fp8", 0)["b"][2][7] ^ 0x7F
    fp4 = model.xor_register("mxfp4", _regs("mxfp4", 0), 9, "a", 3, 0xF0000000)
    assert fp4["a"][9][15] == _regs("mxfp4", 0)["a"][9][15] ^ 0xF0
    hi = model.xor_register("mxfp4", _regs("mxfp4", 0), 9, "a", 7, 0xF0000000)
    assert hi["a"][9][31] == 0xF0 and hi["a"][9][:16] == _regs("mxfp4", 0)["a"][9][:16]
    c = model.xor_register("f16", _regs("f16", 0), 0, "c", 2, 1 << 31)
    assert c["c"][0][2] == -_regs("f16", 0)["c"][0][2]
    sa = model.xor_register("mxfp4", _regs("mxfp4", 0), 63, "sb", 0, 0x102)
    assert sa["sb"][63] == _regs("mxfp4", 0)["sb"][63] ^ 0x102


def test_nonfinite_products_are_placed_element_by_element():
    """inf x 0 is NaN, inf x negative is -inf, and only that row is touched."""
    A = np.zeros((2, 3))
    B = np.array([[1.0, 0.0], [2.0, 2.0], [-1.0, 5.0]])
    C_ = np.ones((2, 2))
    A[0] = (math.inf, 1.0, 1.0)
    A[1] = (1.0, 1.0, 1.0)
    D = model._matmul_add(A, B, C_)
    assert D[0, 0] == math.inf and math.isnan(D[0, 1]) and list(D[1]) == [3.0, 8.0]
    A[0, 0] = -math.inf
    assert model._matmul_add(A, B, C_)[0, 0] == -math.inf
    A[0, 0] = 4.0
    assert np.array_equal(model._matmul_add(A, B, C_), A @ B + C_)


@pytest.mark.parametrize("dtype,wg", TABLE)
def test_case_table_covers_what_it_should(dtype, wg):
    cases = operand_cases(dtype, wg)
    per_dword = 32 // ELEMENT_BITS[dtype]
    for operand in ("a", "b"):
        mine = [c for c in cases if c.operand == operand and c.kind == "finite"]
        assert len(mine) == 24
        assert {c.lane for c in mine} == set(CORNER_LANES)     # every k-group, i = 0 and 15
        assert {c.reg for c in mine} >= {0, DATA_DWORDS[dtype] - 1}
        assert {c.what[1] % per_dword for c in mine} >= {0, per_dword - 1}   # both halves
        # the first and the last element: bytes 0 and 7 of fp8, nibbles 0 and 31 of FP4
        assert {0, DATA_DWORDS[dtype] * per_dword - 1} <= {c.what[1] for c in mine}
        for flip, bit in ELEMENT_FLIPS[dtype]:
            lanes = {c.lane for c in mine if c.what[0] == flip}
            assert lanes == set(CORNER_LANES), (operand, flip)
        for c in mine:
            assert bin(c.mask).count("1") == 1
    c_cases = [c for c in cases if c.operand == "c"]
    assert sorted((c.reg, c.mask) for c in c_cases) == [(0, 1 << 22), (0, 1 << 31),
                                                         (3, 1 << 22), (3, 1 << 31)]
    scale = [(c.operand, c.mask) for c in cases
             if c.operand in ("sa", "sb") and c.kind == "finite"]
    controls = [c for c in cases if c.kind == "control"]
    nonfinite = [c for c in cases if c.kind == "nonfinite"]
    if dtype == "mxfp4":
        assert sorted(scale) == [("sa", 1), ("sa", 2), ("sb", 1), ("sb", 2)]
        assert {(c.operand, c.reg) for c in controls} == {("sa", 0), ("sb", 0), ("a", 4), ("a", 7),
                                                          ("b", 4), ("b", 7)}
        assert all(c.mask & 0xFF == 0 for c in controls if c.operand in ("sa", "sb"))
        assert nonfinite == []
    else:
        assert scale == [] and controls == [] and len(nonfinite) == 1
    print(f"{dtype} tile {wg}: {len(cases)} cases")


def _assert_exact_in_any_order(case, A, B, C_, changed):
    """There is a q with every product and C a multiple of 2^-q and, for every
    affected element, the sum of the absolute values of its terms below
    2^(24-q): every partial sum in any order is then an fp32 number."""
    products = A[:, :, None] * B[None, :, :]                   # [row, k, col], exact in float64
    terms = np.concatenate([products, C_[:, None, :]], axis=1)
    q = 0
    while not np.array_equal(np.ldexp(terms, q), np.rint(np.ldexp(terms, q))):
        q += 1
        assert q <= 24, case.name
    total = np.abs(terms).sum(axis=1)
    for row, col in changed:
        assert total[row, col] < 2.0 ** (24 - q), (case.name, row, col, q, total[row, col])
    return q


@pytest.mark.parametrize("dtype,wg", TABLE)
def test_case_conditions(dtype, wg):
    """What makes the GPU comparison exact, and the structure of each fault:
    an A or sa fault in lane 16 g + i stays in row i, a B or sb fault in column
    i, a C fault at register r is D[4 g + r][i] alone, the controls change
    nothing, every A / B / scale case reaches at least 8 elements."""
    clean = _clean_tile(dtype, wg)
    assert np.isfinite(clean).all()
    worst_q = 0
    for case in operand_cases(dtype, wg):
        i, g = case.lane & 15, case.lane >> 4
        regs = _faulted_regs(case)
        A, B, C_ = model.matrices_from_registers(dtype, regs)
        faulted = model.tile_from_registers(dtype, regs)
        changed = np.argwhere(_differs(faulted, clean))
        rows, cols = set(changed[:, 0].tolist()), set(changed[:, 1].tolist())
        if case.kind == "control":
            assert len(changed) == 0 and np.array_equal(faulted, clean), case.name
            continue
        if case.operand in ("a", "sa"):
            assert rows == {i} and len(changed) >= 8, (case.name, changed.tolist())
        elif case.operand in ("b", "sb"):
            assert cols == {i} and len(changed) >= 8, (case.name, changed.tolist())
        else:
            assert changed.tolist() == [[4 * g + case.reg, i]], (case.name, changed.tolist())
        if case.kind == "nonfinite":
            assert not np.isfinite(faulted[tuple(changed.T)]).any(), case.name
            assert len(changed) == 16, case.name
            untouched = np.ones((16, 16), bool)
            untouched[tuple(changed.T)] = False
            assert np.array_equal(faulted[untouched], clean[untouched])
            continue
        # finite: the faulted operand is a normal number ...
        if case.operand in ("a", "b"):
            pos = case.what[1]
            code = _element_code(dtype, regs, case.operand, case.lane, pos)
            was = _element_code(dtype, _regs(dtype, wg), case.operand, case.lane, pos)
            assert code != was and _is_normal(dtype, code) and _is_normal(dtype, was), case.name
        elif case.operand == "c":
            value = regs["c"][case.lane][case.reg]
            assert math.isfinite(value) and abs(value) >= 2.0 ** -126, case.name
        else:
            assert 0 < regs[case.operand][case.lane] & 0xFF < 0xFF, case.name
        # ... and the sum is exact whatever the order
        assert np.isfinite(faulted).all()
        worst_q = max(worst_q, _assert_exact_in_any_order(case, A, B, C_, changed))
        assert np.array_equal(faulted.astype(np.float32).astype(np.float64), faulted), case.name
    print(f"{dtype} tile {wg}: largest q {worst_q}")


# ---------------------------------------------------------------------------
# GPU: operand-side faults through the MFMA
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_tiles(native):
    """Host reference of tiles 0..1023, float32 [1024, 16, 16], computed once
    per data type, shared and left unchanged."""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            ref = np.array([native.reference_tile(dtype, SEED, wg) for wg in range(WORKGROUPS)],
                           dtype=np.float32)
            ref.setflags(write=False)
            cache[dtype] = ref
        return cache[dtype]
    return get


def _inject(case):
    return (case.wg, case.lane, case.operand, case.reg, case.mask)


def _same_bits(got, want):
    """Bit for bit, a NaN compared as a NaN."""
    nan = np.isnan(want)
    return (np.isnan(got[nan]).all()
            and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,wg", TABLE)
def test_operand_fault_reaches_d_as_the_model_says(native, reference_tiles, dtype, wg):
    """The faulted tile equals the register model's D bit for bit and every
    other tile the host reference. Would fail on an operand fragment packed in
    another element or k-group order than documented (even one that both
    operands share, which a clean run cannot see), a scale taken from another
    byte or lane, an FP4 operand read from VGPRs 4..7."""
    ref = reference_tiles(dtype)
    assert np.array_equal(_clean_tile(dtype, wg), ref[wg].astype(np.float64))
    failures = []
    for case in operand_cases(dtype, wg):
        raw = native.debug_mfma_dump(0, dtype, WORKGROUPS, SEED, inject_operand=_inject(case))
        D = np.frombuffer(raw, dtype="<f4").reshape(WORKGROUPS, 16, 16)
        want = _faulted_tile(case).astype(np.float32)
        others = np.arange(WORKGROUPS) != wg
        ok_tile = _same_bits(D[wg], want)
        ok_rest = np.array_equal(D[others].view(np.uint32), ref[others].view(np.uint32))
        if not (ok_tile and ok_rest):
            bad = np.argwhere(~(D[wg] == want) & ~(np.isnan(D[wg]) & np.isnan(want)))
            print(f"{case.name}: tile differs at {bad[:6].tolist()} got "
                  f"{[float(D[wg][tuple(b)]) for b in bad[:6]]} want "
                  f"{[float(want[tuple(b)]) for b in bad[:6]]}; other tiles ok: {ok_rest}")
            failures.append(case.name)
    assert failures == []


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,wg", TABLE)
def test_check_flags_an_operand_fault(native, reference_tiles, dtype, wg):
    """The check kernel counts exactly the elements where the model's faulted
    D differs from the reference (a NaN differs), names the smallest with the
    model's value as `got`, and stays silent for the negative controls."""
    ref = reference_tiles(dtype)[wg]
    failures = []
    for case in operand_cases(dtype, wg):
        want = _faulted_tile(case).astype(np.float32)
        bad = np.argwhere(_differs(want, ref))
        r = native.mfma_verify(0, dtype, workgroups=WORKGROUPS, seed=SEED,
                               inject_operand=_inject(case))
        ok = r["tiles"] == WORKGROUPS and r["mismatches"] == len(bad)
        if len(bad) == 0:
            ok = ok and case.kind == "control" and r["first_bad"] is None
        else:
            row, col = bad[0].tolist()
            ok = ok and case.kind != "control" and r["first_bad"] is not None
            if ok:
                tile, r_row, r_col, got, expected = r["first_bad"]
                ok = (tile, r_row, r_col) == (wg, row, col)
                ok = ok and _bits(expected) == _bits(float(ref[row, col]))
                model_got = float(want[row, col])
                ok = ok and (math.isnan(got) if math.isnan(model_got)
                             else _bits(got) == _bits(model_got))
        if not ok:
            print(f"{case.name}: {r}; model: {len(bad)} mismatches, first {bad[:1].tolist()}")
            failures.append(case.name)
    assert failures == []


@pytest.mark.gpu
def test_operand_fault_with_another_seed_and_an_output_fault(native):
    """The hook takes the seed it is given, and combines with an xor into D."""
    regs = model.pack_registers("f16", SEED2, 3)
    lane, pos = next((l, p) for l in range(64) for p in range(8)
                     if _is_normal("f16", regs["b"][l][p]))
    mask = 0x8000 << (16 * (pos % 2))
    want = model.tile_from_registers(
        "f16", model.xor_register("f16", regs, lane, "b", pos // 2, mask)).astype(np.float32)
    raw = native.debug_mfma_dump(0, "f16", 4, SEED2, inject_operand=(3, lane, "b", pos // 2, mask))
    D = np.frombuffer(raw, dtype="<f4").reshape(4, 16, 16)
    assert _same_bits(D[3], want)
    ref = np.array(native.reference_tile("f16", SEED2, 3), dtype=np.float32)
    n_bad = int(_differs(want, ref).sum())
    assert n_bad >= 8
    r = native.mfma_verify(0, "f16", workgroups=4, seed=SEED2, corruptions=[(5, 1 << 20)],
                           inject_operand=(3, lane, "b", pos // 2, mask))
    assert r["mismatches"] == n_bad + 1 and r["first_bad"][:3] == (0, 0, 5)


@pytest.mark.gpu
def test_operand_injection_arguments_are_checked(native):
    bad = [
        ("bf16", (0, 64, "a", 0, 1)), ("bf16", (0, -1, "a", 0, 1)),
        ("bf16", (0, 0, "a", 4, 1)), ("f16", (0, 0, "b", 4, 1)), ("fp8", (0, 0, "a", 2, 1)),
        ("mxfp4", (0, 0, "b", 8, 1)), ("bf16", (0, 0, "c", 4, 1)), ("mxfp4", (0, 0, "sa", 1, 1)),
        ("bf16", (0, 0, "a", -1, 1)),
        ("bf16", (0, 0, "sa", 0, 1)), ("fp8", (0, 0, "sb", 0, 1)),
        ("bf16", (0, 0, "a", 0, 0)), ("bf16", (0, 0, "a", 0, 1 << 32)),
        ("bf16", (0, 0, "a", 0, -1)),
        ("bf16", (4, 0, "a", 0, 1)), ("bf16", (-1, 0, "a", 0, 1)),
        ("bf16", (0, 0, "d", 0, 1)), ("bf16", (0, 0, "A", 0, 1)),
    ]
    for dtype, inject in bad:
        with pytest.raises(ValueError):
            native.debug_mfma_dump(0, dtype, 4, SEED, inject_operand=inject)
            pytest.fail(f"dump accepted {dtype} {inject}")
        with pytest.raises(ValueError):
            native.mfma_verify(0, dtype, workgroups=4, inject_operand=inject)
            pytest.fail(f"verify accepted {dtype} {inject}")
    # None is the default, and the device is as usable as before
    assert native.debug_mfma_dump(0, "bf16", 4, SEED, inject_operand=None) == \
        native.debug_mfma_dump(0, "bf16", 4, SEED)
    assert native.mfma_verify(0, "mxfp4", workgroups=4, inject_operand=None)["mismatches"] == 0


# ---------------------------------------------------------------------------
# GPU: stuck-at faults in the HBM sweep
# ---------------------------------------------------------------------------
def _force(x, mask, value):
    return x | mask if value else x & ~mask & M32


def _hbm_expect(nbytes, passes, stuck, corruptions=(), corrupt_at=(0, 0), seed=SEED, base=0):
    """The sweep's four counters from pattern_words alone: per word, pass and
    phase the difference between what the verify wants and what the xor and
    then the stuck bits leave of it."""
    words = {}
    for word, mask in corruptions:
        words.setdefault(word, {})["xor"] = mask
    for word, mask, value in stuck:
        words.setdefault(word, {})["stuck"] = (mask, value)
    want = {"mismatched_words": 0, "flipped_bits": 0, "bad_bit_mask": 0, "first_bad_offset": -1,
            "bytes_checked": nbytes}
    for word in sorted(words):
        pattern = int(pattern_words(seed, base + word, 1)[0])
        for at in ((p, ph) for p in range(passes) for ph in (0, 1)):
            wanted = pattern ^ (M32 if at[1] else 0)
            got = wanted ^ (words[word].get("xor", 0) if at == tuple(corrupt_at) else 0)
            if "stuck" in words[word]:
                got = _force(got, *words[word]["stuck"])
            diff = got ^ wanted
            if diff:
                want["mismatched_words"] += 1
                want["flipped_bits"] += bin(diff).count("1")
                want["bad_bit_mask"] |= diff
                if want["first_bad_offset"] < 0:
                    want["first_bad_offset"] = 4 * word
    return want


def _counters(r):
    return {k: r[k] for k in ("mismatched_words", "flipped_bits", "bad_bit_mask",
                              "first_bad_offset", "bytes_checked")}


def test_hbm_expectation_follows_the_issue_formula():
    """For one stuck word the difference in a phase is
    (pattern ^ inv ^ forced) & mask."""
    for word, mask, value in ((0, 1, 0), (7, 1 << 31, 1), (1027, M32, 1), (5, 0x00F0F000, 0)):
        pattern = int(pattern_words(SEED, word, 1)[0])
        diffs = [(pattern ^ inv ^ (mask if value else 0)) & mask for inv in (0, M32)]
        want = _hbm_expect(8192, 3, [(word, mask, value)])
        assert want["mismatched_words"] == 3 * sum(d != 0 for d in diffs)
        assert want["flipped_bits"] == 3 * sum(bin(d).count("1") for d in diffs)
        assert want["flipped_bits"] == 3 * bin(mask).count("1")
        assert want["bad_bit_mask"] == diffs[0] | diffs[1] == mask


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("nbytes", [16, 4096 + 16, MIB + 16])
def test_hbm_stuck_bit_is_caught_in_exactly_one_phase(native, nbytes, passes):
    """First word, last word and one in the last, partial block of the grid.
    A single stuck bit disagrees with the pattern in one phase of each pass
    whichever value it is stuck at: a sweep that does not invert gives 0 or
    2 x passes, one that ignores passes gives 1."""
    n_words = nbytes // 4
    for word in sorted({0, n_words - 1, max(n_words - 3, 1)}):
        for value in (0, 1):
            for mask in (1, 1 << 31):
                r = native.hbm_pattern_check(0, bytes=nbytes, passes=passes,
                                             stuck=[(word, mask, value)])
                print(word, mask, value, _counters(r))
                assert r["mismatched_words"] == passes
                assert _counters(r) == _hbm_expect(nbytes, passes, [(word, mask, value)])
                assert r["flipped_bits"] == passes and r["bad_bit_mask"] == mask
                assert r["first_bad_offset"] == 4 * word
            r = native.hbm_pattern_check(0, bytes=nbytes, passes=passes,
                                         stuck=[(word, M32, value)])
            print(word, "full", value, _counters(r))
            assert r["flipped_bits"] == 32 * passes and r["bad_bit_mask"] == M32
            assert _counters(r) == _hbm_expect(nbytes, passes, [(word, M32, value)])


@pytest.mark.gpu
def test_hbm_stuck_word_in_the_second_chunk(native):
    nbytes = MIB + 16
    stuck = [(MIB // 4 + 2, 1 << 17, 1), (MIB // 4 - 1, 0x0000FF00, 0)]
    r = native.hbm_pattern_check(0, bytes=nbytes, max_chunk_mib=1, passes=2, stuck=stuck,
                                 seed=SEED2, base_word=(1 << 32) - 8)
    assert r["chunks"] == 2
    want = _hbm_expect(nbytes, 2, stuck, seed=SEED2, base=(1 << 32) - 8)
    assert _counters(r) == want
    assert want["mismatched_words"] == 2 + 4 and want["flipped_bits"] == 2 * (1 + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("at", [(0, 0), (1, 1)])
def test_hbm_stuck_and_xor_combine(native, at):
    """On different words both count; on one word the stuck bits are forced
    after the xor, as a stuck cell would hold them."""
    nbytes = 4096 + 16
    stuck = [(9, 0x0000FFFF, 1), (1027, 1 << 4, 0)]
    corruptions = [(9, 0x00FF00FF), (100, 0x3)]
    r = native.hbm_pattern_check(0, bytes=nbytes, passes=2, stuck=stuck, corruptions=corruptions,
                                 corrupt_at=at)
    want = _hbm_expect(nbytes, 2, stuck, corruptions, at)
    print(_counters(r), want)
    assert _counters(r) == want
    assert want["bad_bit_mask"] == 0x00FFFFFF | 0x10 | 0x3


# ---------------------------------------------------------------------------
# GPU: stuck-at faults in the LDS march
# ---------------------------------------------------------------------------
CLEAN_LDS = {"bad_words": 0, "flipped_bits": 0, "bad_bit_mask": 0, "first_bad_word": -1}


def _lds_expect(visit, word, mask, value, passes, seed=SEED):
    """Two verifies per phase, times the phases that differ, times passes."""
    pattern = int(pattern_words(seed, (visit << 32) + word, 1)[0])
    diffs = [(pattern ^ inv ^ (mask if value else 0)) & mask for inv in (0, M32)]
    differing = [d for d in diffs if d]
    if not differing:
        return dict(CLEAN_LDS)
    return {"bad_words": 2 * passes * len(differing),
            "flipped_bits": 2 * passes * sum(bin(d).count("1") for d in differing),
            "bad_bit_mask": diffs[0] | diffs[1], "first_bad_word": word}


def _where(d):
    return (d["xcc"], d["se"], d["sh"], d["cu"])


def _assert_one_lds_fault(r, want):
    rec = r["record"]
    assert rec is not None
    assert len(r["faulty"]) == 1, r["faulty"]
    f = r["faulty"][0]
    assert _where(f) == _where(rec)
    assert f["lds"] == want and f["mfma"] == []
    assert rec["lds"] == want


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2, 3])
@pytest.mark.parametrize("size", ["one_vector", "stride_plus_one", "device_max"])
def test_lds_stuck_bit_is_caught_in_every_pass(native, size, passes):
    """The bits are forced after every fill, so each pass reports them again:
    a kernel that ran one pass whatever it was told, or that did not invert,
    gives other counts."""
    lds_bytes = {"one_vector": 16, "stride_plus_one": 4096 + 16, "device_max": 0}[size]
    blocks, visit = 3, 2
    n_words = len(native.debug_cu_lds_dump(0, lds_bytes)) // 4
    # a 16-byte LDS has no word 1025
    for word in sorted({0, n_words - 1, 1025} - set(range(n_words, 1026))):
        for value in (0, 1):
            for mask in (1, 1 << 31, M32):
                r = native.cu_sweep(lds_bytes=lds_bytes, passes=passes, blocks_per_round=blocks,
                                    max_rounds=1, inject_lds_stuck=(visit, word, mask, value))
                want = _lds_expect(visit, word, mask, value, passes)
                print(word, hex(mask), value, r["faulty"])
                _assert_one_lds_fault(r, want)
                if mask == M32:
                    assert want["flipped_bits"] == 64 * passes and want["bad_bit_mask"] == M32
                else:
                    assert want["bad_words"] == 2 * passes and want["bad_bit_mask"] == mask
                assert sum(l["visits"] for l in r["locations"]) == blocks


@pytest.mark.gpu
def test_lds_stuck_bit_in_a_full_round(native):
    """The last visit of one full round at the device's LDS maximum: the fault
    is at the place that workgroup recorded and every other slot is clean."""
    cus = native.device_info(0)["multi_processor_count"]
    blocks = 4 * cus
    word, mask, value, passes = 1025, 1 << 13, 0, 2
    r = native.cu_sweep(seed=SEED2, passes=passes, blocks_per_round=0, max_rounds=1,
                        inject_lds_stuck=(blocks - 1, word, mask, value))
    assert r["blocks_per_round"] == blocks and r["rounds"] == 1
    want = _lds_expect(blocks - 1, word, mask, value, passes, seed=SEED2)
    assert want["bad_words"] == 2 * passes
    _assert_one_lds_fault(r, want)           # exactly one faulty slot: all others are clean
    assert sum(l["visits"] for l in r["locations"]) == blocks


@pytest.mark.gpu
def test_lds_stuck_and_mfma_fault_together(native):
    r = native.cu_sweep(blocks_per_round=4, max_rounds=1, passes=2,
                        inject_lds_stuck=(2, 77, 0x0F, 1),
                        inject_mfma=(2, 1, "fp8", 17, 1 << 20))
    rec = r["record"]
    assert len(r["faulty"]) == 1
    f = r["faulty"][0]
    assert _where(f) == _where(rec)
    assert f["mfma"] == [(rec["simd"][1], "fp8")]
    want = _lds_expect(2, 77, 0x0F, 1, 2)
    assert f["lds"] == want == rec["lds"]
    assert want["flipped_bits"] == 2 * 2 * 4 and want["bad_bit_mask"] == 0x0F
