"""Numpy model of the burn-in's GEMM check (kuberay_amd/_native/gpuhealth_gemm.hip
over gpuhealth_ref.hpp): the independent side of tests/test_gpu_gemm_exact.py and
tests/test_gpu_gemm_faults.py. Nothing here imports the extension.

* the matrix generator, written from the description in gpuhealth_ref.hpp (hash
  the seed with the data type and the matrix, then the row, then the column
  into that result; an integer in [-8, 8]), vectorised over a whole matrix;
* bf16 / f16 bits <-> float64;
* where an element lies in the LDS of a stage, from the layout and the two
  swizzles the comments of gpuhealth_gemm.hip state;
* the rule that says which elements of D a faulted operand must change, must
  leave alone, and where neither can be promised;
* the seeded fault cases of tests/test_gpu_gemm_faults.py, so that the CPU suite
  (tests/test_gemm_ref.py) can hold every one of them against the rule.
"""
import numpy as np

from gpuhealth_model import DT_INDEX, GEN_A, GEN_B, GEN_C, M32, _mix32_np, mix32

DEFAULT_SEED = 0x5EED1234
SEED2 = 0x0BADC0DE
DTYPES = ("bf16", "f16")
WHICH = {"a": GEN_A, "b": GEN_B, "c": GEN_C}
TILE = 64                      # a workgroup's tile of D and the K depth of a stage
ROW_BYTES = 2 * TILE           # 128: eight 16-byte chunks
OPERAND_BYTES = TILE * ROW_BYTES
STAGE_BYTES = 2 * OPERAND_BYTES  # A's 8 KiB, then B's


# ---------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------
def gemm_matrix_hash(seed, dtype, which):
    return mix32(seed ^ (((DT_INDEX[dtype] * 8 + which + 1) * 0x9E3779B9) & M32))


def gemm_int_of(matrix_hash, rows, cols):
    """The integers at rows x cols (1-D index arrays, 32-bit values) as int64."""
    m = np.uint64(M32)
    rows = np.asarray(rows, dtype=np.uint64)[:, None]
    cols = np.asarray(cols, dtype=np.uint64)[None, :]
    h = (_mix32_np(np.uint64(matrix_hash) ^ rows) + cols) & m
    return ((_mix32_np(h) >> np.uint64(8)) % np.uint64(17)).astype(np.int64) - 8


def operand_matrix(dtype, seed, which, rows, cols, row0=0, col0=0):
    """rows x cols of A, B or C (which: 'a', 'b', 'c') from (row0, col0), int64."""
    h = gemm_matrix_hash(seed, dtype, WHICH[which])
    return gemm_int_of(h, row0 + np.arange(rows, dtype=np.uint64),
                       col0 + np.arange(cols, dtype=np.uint64))


def reference_element(dtype, seed, k, row, col):
    a = operand_matrix(dtype, seed, "a", 1, k, row0=row)
    b = operand_matrix(dtype, seed, "b", k, 1, col0=col)
    return int((a @ b)[0, 0] + operand_matrix(dtype, seed, "c", 1, 1, row, col)[0, 0])


# ---------------------------------------------------------------------------
# bf16 / f16 bits <-> float64
# ---------------------------------------------------------------------------
def decode(dtype, bits):
    u = np.asarray(bits, dtype=np.uint16)
    if dtype == "bf16":
        return (u.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return u.view(np.float16).astype(np.float64)


def encode(dtype, values):
    """Round to nearest even; the GEMM's integers are exact in both types."""
    f = np.asarray(values, dtype=np.float64).astype(np.float32)
    if dtype == "f16":
        return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))
            >> np.uint32(16)).astype(np.uint16)


def flipped(dtype, value, mask):
    """The float64 value of an operand element after its 16 bits were xored."""
    return float(decode(dtype, encode(dtype, [value]) ^ np.uint16(mask))[0])


# ---------------------------------------------------------------------------
# layout of one stage in LDS
#
# A stage is A's 64 x 64 tile, then B's, 8 KiB each, rows of 128 bytes = eight
# 16-byte slots. Chunk c (eight elements) of row r lies in slot c ^ swizzle(r):
#   A: swizzle(r) = (r >> 1) & 7
#   B: swizzle(r) = bit 1 of r moved to bit 1, bit 3 of r moved to bit 2
# A's rows are rows of the tile and its columns the stage's 64 k; B's rows are
# the stage's 64 k and its columns the tile's columns.
# ---------------------------------------------------------------------------
def a_swizzle(row, shift=1):
    return (row >> shift) & 7


def b_swizzle(row):
    return ((row >> 1) & 1) << 1 | ((row >> 3) & 1) << 2


def lds_offset(operand, row, slot, e):
    return (OPERAND_BYTES if operand == "b" else 0) + ROW_BYTES * row + 16 * slot + 2 * e


def lds_element(offset, m0, n0, stage, a_shift=1):
    """(operand, row, col) of the element of A or B that lies at that even byte
    offset of stage `stage` in the workgroup of the tile at (m0, n0). a_shift
    other than 1 is a deliberately wrong model, for showing that the tests bite."""
    assert 0 <= offset < STAGE_BYTES and offset % 2 == 0
    operand = "a" if offset < OPERAND_BYTES else "b"
    row = offset % OPERAND_BYTES // ROW_BYTES
    slot, e = offset % ROW_BYTES // 16, offset % 16 // 2
    if operand == "a":
        return "a", m0 + row, TILE * stage + 8 * (slot ^ a_swizzle(row, a_shift)) + e
    return "b", TILE * stage + row, n0 + 8 * (slot ^ b_swizzle(row)) + e


# ---------------------------------------------------------------------------
# decision rule for a faulted product
#
# The kernel adds K products and C in fp32, in an order the MFMA and the tiling
# choose. A product of two 16-bit operands has at most 22 significant bits and
# is exact in fp32, so the only error is that of the sum. For a sum of n terms
# t_i in any order, each addition rounding by at most u relative,
#   |fl(sum) - sum| <= ((1 + u)^(n - 1) - 1) * sum |t_i| <= 1.01 n u S
# for n u < 0.01 (Higham, Accuracy and Stability, section 4.2), with u = 2^-24
# for round to nearest, n = K + 1 and S = sum |a'||b| + |c|. The matrix pipe may
# truncate where an adder would round, and may align a block of products to its
# largest exponent before adding; both stay within a few u per term, and the
# factor 8 takes them in. So when the float64 value of the faulted product
# differs from the clean one, an integer that fp32 holds exactly, by more than
# 8 K 2^-24 S, no fp32 evaluation of the faulted sum can land on the clean
# value: the element must mismatch. A float64 value that is not finite in fp32
# (Inf from an exponent flip, NaN from Inf * 0) must mismatch as well, the
# check counts a NaN as bad. Equal float64 values must match. When every term is
# a multiple of one power of two q and S < 2^24 q, every partial sum in every
# order is such a multiple below 2^24 q, fp32 holds it, and D is the float64
# value bit for bit. This is the sound form of "the value and S are both exact
# in fp32": that alone would also take 2^-30 + 4000, which fp32 cannot add. All
# operands but one are integers, so q is the lowest set bit of that one. What
# none of these decides is undecided: nothing can be promised there.
# ---------------------------------------------------------------------------
MUST_MATCH, MUST_MISMATCH, UNDECIDED = 0, 1, 2


def _line_sum(x, y, c):
    """sum_k x[k] * y[k, :] + c without a BLAS, NaN and Inf by IEEE rules."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (x[:, None] * y).sum(axis=0) + c


def grid_of(value):
    """The largest power of two, 1 at the most, that divides a finite value."""
    q = 1.0
    while value != 0.0 and (value / q) % 1.0 != 0.0:
        q /= 2.0
    return q


def judge(clean, faulted, s, k, q=1.0):
    """Per element: (verdict, exact). clean, faulted: float64 values of D;
    s: sum |a'||b| + |c|; q: the power of two every term is a multiple of;
    exact: D must equal `faulted` bit for bit."""
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(faulted.astype(np.float32)) & np.isfinite(s.astype(np.float32))
        exact = finite & (s < 2.0 ** 24 * q) & (q >= 2.0 ** -126)
        far = np.abs(faulted - clean) > 8.0 * k * 2.0 ** -24 * s
    verdict = np.full(clean.shape, UNDECIDED)
    verdict[finite & (faulted == clean)] = MUST_MATCH
    verdict[exact & (faulted != clean)] = MUST_MISMATCH
    verdict[finite & far] = MUST_MISMATCH
    verdict[~finite] = MUST_MISMATCH
    return verdict, exact


class Verdict:
    """What one changed element of A or B does to D. line: the row of D (fault
    in A) or the column (fault in B); cols / rows restrict it to one tile for an
    LDS-side fault. faulted is the float64 D of the whole matrix."""

    def __init__(self, a, b, c, clean, operand, row, col, value, span=None, origin=(0, 0)):
        k = a.shape[1]
        self.operand, self.k, self.origin = operand, k, origin  # origin: of clean in D
        lo, hi = span if span else (0, b.shape[1] if operand == "a" else a.shape[0])
        if operand == "a":
            x = a[row].copy()
            x[col] = value
            y, cc, self.line = b[:, lo:hi], c[row, lo:hi], row
            where = (row, slice(lo, hi))
        else:
            x = b[:, col].copy()
            x[row] = value
            y, cc, self.line = a[lo:hi].T, c[lo:hi, col], col
            where = (slice(lo, hi), col)
        new = _line_sum(x, y, cc)
        s = _line_sum(np.abs(x), np.abs(y), np.abs(cc))
        q = grid_of(value) if np.isfinite(value) else 1.0
        self.verdict, self.exact = judge(clean[where], new, s, k, q)
        self.s = s
        self.faulted = clean.copy()
        self.faulted[where] = new
        self.bad = np.zeros(clean.shape, dtype=bool)
        self.bad[where] = self.verdict == MUST_MISMATCH
        self.exact_map = np.zeros(clean.shape, dtype=bool)
        self.exact_map[where] = self.exact
        self.s_map = np.zeros(clean.shape)
        self.s_map[where] = s

    @property
    def undecided(self):
        return int(np.count_nonzero(self.verdict == UNDECIDED))

    def first_bad(self):
        """(row, col) in D of the first mismatch in row-major order, or None."""
        idx = np.flatnonzero(self.bad)
        if idx.size == 0:
            return None
        r, c = np.unravel_index(idx[0], self.bad.shape)
        return int(r) + self.origin[0], int(c) + self.origin[1]

    def tiles(self):
        """{(tile_row, tile_col): (mismatches, first_bad)} of the tiles with any."""
        out = {}
        for r, c in np.argwhere(self.bad):
            r, c = int(r) + self.origin[0], int(c) + self.origin[1]
            n, first = out.get((r // TILE, c // TILE), (0, (r, c)))
            out[(r // TILE, c // TILE)] = (n + 1, first)
        return out

    def got_matches(self, row, col, got):
        """Whether the D the device reports at a mismatch is what the rule allows:
        bit for bit where exact, the same NaN / Inf where not finite, else within
        the forward error bound."""
        row, col = row - self.origin[0], col - self.origin[1]
        want = self.faulted[row, col]
        with np.errstate(over="ignore", invalid="ignore"):
            want32 = np.float32(want)
        if self.exact_map[row, col] or not np.isfinite(want32):
            return bool(np.array_equal(np.float32(got), want32, equal_nan=True))
        return abs(float(got) - want) <= 8.0 * self.k * 2.0 ** -24 * self.s_map[row, col]


def line_verdict(dtype, seed, m, n, k, case):
    """The Verdict of a memory-side fault from the generator alone, for shapes
    too large to hold whole: only the row of A, C and D (fault in A) or the
    column of B, C and D (fault in B) that the element touches is built."""
    operand, row, col, mask = case
    if operand == "a":
        a = operand_matrix(dtype, seed, "a", 1, k, row0=row).astype(np.float64)
        b = operand_matrix(dtype, seed, "b", k, n).astype(np.float64)
        c = operand_matrix(dtype, seed, "c", 1, n, row0=row).astype(np.float64)
        return Verdict(a, b, c, a @ b + c, "a", 0, col, flipped(dtype, a[0, col], mask),
                       origin=(row, 0))
    a = operand_matrix(dtype, seed, "a", m, k).astype(np.float64)
    b = operand_matrix(dtype, seed, "b", k, 1, col0=col).astype(np.float64)
    c = operand_matrix(dtype, seed, "c", m, 1, col0=col).astype(np.float64)
    return Verdict(a, b, c, a @ b + c, "b", row, 0, flipped(dtype, b[row, 0], mask),
                   origin=(0, col))


def clean_operands(dtype, seed, m, n, k):
    """A, B, C as float64 and the clean D = A·B + C (integers, exact)."""
    a = operand_matrix(dtype, seed, "a", m, k)
    b = operand_matrix(dtype, seed, "b", k, n)
    c = operand_matrix(dtype, seed, "c", m, n)
    return a.astype(np.float64), b.astype(np.float64), c.astype(np.float64), \
        (a @ b + c).astype(np.float64)


# ---------------------------------------------------------------------------
# the seeded fault cases of tests/test_gpu_gemm_faults.py at 128 x 128 x 192:
# four tiles, three stages, both buffers and one reuse
# ---------------------------------------------------------------------------
FAULT_SHAPE = (128, 128, 192)
MASKS = tuple(1 << bit for bit in range(16))


def find_element(mat, magnitude, skip=0):
    """(row, col) of an element of that magnitude, the skip-th in row-major order
    that is not in the first tile row / column or the first stage."""
    hits = [(int(r), int(c)) for r, c in np.argwhere(np.abs(mat) == magnitude)
            if r >= TILE and c >= TILE]
    return hits[skip]


def bit_sweep_cases(a, b):
    """(operand, row, col, mask): all 16 one-bit masks at one element of
    magnitude 1 and one of magnitude 8, of A and of B."""
    cases = []
    for operand, mat in (("a", a), ("b", b)):
        for magnitude in (1, 8):
            row, col = find_element(mat, magnitude)
            cases += [(operand, row, col, mask) for mask in MASKS]
    return cases


def zero_flip_cases(a, b):
    """A sign flip of an element that is 0: nothing may change."""
    return [(operand, *find_element(mat, 0), 0x8000) for operand, mat in (("a", a), ("b", b))]


def position_case(operand, r, half, stage):
    """Tile row (A) or tile column (B) r = 0..63 in the first or second tile row
    / column; k = 64 stage + (37 r + 5) % 64 hits every k offset of a stage once,
    and the mask cycles over the 16 bits."""
    kk = TILE * stage + (37 * r + 5) % TILE
    line = TILE * half + r
    mask = MASKS[r % 16]
    return (operand, line, kk, mask) if operand == "a" else (operand, kk, line, mask)


def position_sweep_cases(dtype, a, b, c, clean):
    """One case per operand and r. The half alternates with r and the stage
    cycles over 0, 1, 2; where the rule leaves an element of that case undecided
    (a mantissa flip of a 0 makes a denormal no bound speaks for), the position
    moves: to the other half, then to the next stage."""
    cases = []
    for operand in ("a", "b"):
        for r in range(TILE):
            tries = [position_case(operand, r, (r + h) % 2, (r + st) % 3)
                     for st in range(3) for h in range(2)]
            decided = [case for case in tries
                       if verdict_of(dtype, a, b, c, clean, case).undecided == 0]
            cases.append((decided or tries)[0])
    return cases


def verdict_of(dtype, a, b, c, clean, case, span=None):
    operand, row, col, mask = case
    mat = a if operand == "a" else b
    return Verdict(a, b, c, clean, operand, row, col, flipped(dtype, mat[row, col], mask), span)


LDS_MASKS = {"bf16": (0x8000, 0x0100), "f16": (0x8000, 0x0800)}  # the sign, one exponent bit


def lds_sweep_cases(dtype, a, b, tiles_n=2):
    """(tile, stage, offset, mask): A and B, stages 0..2, every row, slot
    (5 row + 3) % 8; the element within the chunk, the mask and the tile cycle.
    The element is the first from its turn in the cycle that is not 0, so that
    every case changes D (the chunk read is the same one)."""
    cases, n = [], 0
    for operand in ("a", "b"):
        for stage in range(3):
            for row in range(TILE):
                tile, slot = n % 4, (5 * row + 3) % 8
                m0, n0 = TILE * (tile // tiles_n), TILE * (tile % tiles_n)
                for e in ((n + step) % 8 for step in range(8)):
                    offset = lds_offset(operand, row, slot, e)
                    _, r, col = lds_element(offset, m0, n0, stage)
                    if (a if operand == "a" else b)[r, col] != 0:
                        break
                cases.append((tile, stage, offset, LDS_MASKS[dtype][(n // 4) % 2]))
                n += 1
    return cases


def lds_verdict(dtype, a, b, c, clean, case, tiles_n=2, a_shift=1):
    """The Verdict of an LDS-side fault: the element the layout names changes
    for that one tile only, its 64 columns (A) or rows (B) of D."""
    tile, stage, offset, mask = case
    m0, n0 = TILE * (tile // tiles_n), TILE * (tile % tiles_n)
    operand, row, col = lds_element(offset, m0, n0, stage, a_shift)
    lo = n0 if operand == "a" else m0
    return verdict_of(dtype, a, b, c, clean, (operand, row, col, mask), (lo, lo + TILE))
