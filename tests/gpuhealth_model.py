"""Python model of kuberay_amd/_native/gpuhealth_ref.hpp and of the operand
lane maps documented above ``mfma_exact_tile`` in gpuhealth.hip.

It is the independent side of the burn-in tests: the HBM sweep pattern (scalar
and numpy-vectorised), the operand generators, the bf16 / f16 / e4m3 / e2m1 /
E8M0 encoders and decoders, and a register-level model of one MFMA tile that
can unpack the registers through a deliberately wrong lane map. Nothing here
imports the extension.
"""
import struct

import numpy as np

M32 = 0xFFFFFFFF
DTYPES = ("bf16", "f16", "fp8", "mxfp4")
DT_INDEX = {"bf16": 0, "f16": 1, "fp8": 2, "mxfp4": 3}
GEN_A, GEN_B, GEN_C, GEN_SA, GEN_SB = range(5)
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def k_of(dtype):
    return 128 if dtype == "mxfp4" else 32


# ---------------------------------------------------------------------------
# hash and HBM sweep pattern
# ---------------------------------------------------------------------------
def mix32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def pattern_word(seed, index):
    lo, hi = index & M32, index >> 32
    x = (lo + seed * 0x9E3779B9) & M32
    x ^= (hi * 0x85EBCA6B) & M32
    return mix32(x)


def _mix32_np(x):
    """mix32 over a uint64 array that holds 32-bit values."""
    m = np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def pattern_words(seed, start, n):
    """pattern_word(seed, start + j) for j in range(n), as a uint32 array."""
    assert 0 <= start and start + n <= 1 << 64
    m = np.uint64(M32)
    idx = np.uint64(start) + np.arange(n, dtype=np.uint64)
    lo, hi = idx & m, idx >> np.uint64(32)
    x = (lo + np.uint64((seed * 0x9E3779B9) & M32)) & m
    x = x ^ ((hi * np.uint64(0x85EBCA6B)) & m)
    return _mix32_np(x).astype(np.uint32)


# ---------------------------------------------------------------------------
# operand generators
# ---------------------------------------------------------------------------
def elem_hash(seed, wg, dtype, which, i, k):
    h = mix32(seed ^ (((wg + 1) * 0x9E3779B9) & M32))
    return mix32(h ^ (((DT_INDEX[dtype] * 8 + which) << 24) & M32) ^ (i << 8) ^ k)


def elem_hash_grid(seed, wg, dtype, which, n_i, n_k):
    """elem_hash for i in range(n_i), k in range(n_k), as a uint64 [n_i, n_k]."""
    h = mix32(seed ^ (((wg + 1) * 0x9E3779B9) & M32))
    h ^= ((DT_INDEX[dtype] * 8 + which) << 24) & M32
    i = np.arange(n_i, dtype=np.uint64)[:, None] << np.uint64(8)
    k = np.arange(n_k, dtype=np.uint64)[None, :]
    return _mix32_np(np.uint64(h) ^ i ^ k)


def gen_int(seed, wg, dtype, which, i, k):
    return ((elem_hash(seed, wg, dtype, which, i, k) >> 8) % 17) - 8


def gen_fp4_code(seed, wg, which, i, k):
    return (elem_hash(seed, wg, "mxfp4", which, i, k) >> 8) & 15


def gen_fp4(seed, wg, which, i, k):
    return e2m1_to_float(gen_fp4_code(seed, wg, which, i, k))


def gen_scale_code(seed, wg, which, i, block):
    return 126 + ((elem_hash(seed, wg, "mxfp4", which, i, block) >> 8) % 3)


def gen_scale(seed, wg, which, i, block):
    return e8m0_to_float(gen_scale_code(seed, wg, which, i, block))


def operands(dtype, seed, wg):
    """Logical A (16 x K), B (K x 16) and C (16 x 16) of one tile, float64."""
    K = k_of(dtype)
    A = np.zeros((16, K))
    B = np.zeros((K, 16))
    C_ = np.zeros((16, 16))
    for i in range(16):
        for k in range(K):
            if dtype == "mxfp4":
                A[i, k] = gen_fp4(seed, wg, GEN_A, i, k) * gen_scale(seed, wg, GEN_SA, i, k // 32)
                B[k, i] = gen_fp4(seed, wg, GEN_B, i, k) * gen_scale(seed, wg, GEN_SB, i, k // 32)
            else:
                A[i, k] = gen_int(seed, wg, dtype, GEN_A, i, k)
                B[k, i] = gen_int(seed, wg, dtype, GEN_B, i, k)
        for c in range(16):
            C_[i, c] = gen_int(seed, wg, dtype, GEN_C, i, c)
    return A, B, C_


# ---------------------------------------------------------------------------
# encoders / decoders (bit patterns as ints)
# ---------------------------------------------------------------------------
def f32_bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def bits_f32(u):
    return struct.unpack("<f", struct.pack("<I", u & M32))[0]


def f32_to_bf16(f):
    u = f32_bits(f)
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return ((u >> 16) | 0x40) & 0xFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & M32
    return u >> 16


def bf16_to_f32(b):
    return bits_f32(b << 16)


def f32_to_f16(f):
    u = f32_bits(f)
    sign = (u >> 16) & 0x8000
    e = ((u >> 23) & 0xFF) - 127 + 15
    m = u & 0x7FFFFF
    if e <= 0:
        return sign
    if e >= 31:
        return sign | 0x7C00
    h = (e << 10) | (m >> 13)
    rem = m & 0x1FFF
    if rem > 0x1000 or (rem == 0x1000 and (h & 1)):
        h += 1
    return sign | h


def f16_to_f32(h):
    return float(np.array([h], dtype=np.uint16).view(np.float16)[0])


def f32_to_e4m3(f):
    u = f32_bits(f)
    sign = (u >> 24) & 0x80
    e = ((u >> 23) & 0xFF) - 127 + 7
    m = u & 0x7FFFFF
    if e <= 0:
        return sign
    if e >= 16:
        return sign | 0x7E
    h = (e << 3) | (m >> 20)
    rem = m & 0xFFFFF
    if rem > 0x80000 or (rem == 0x80000 and (h & 1)):
        h += 1
    return sign | min(h, 0x7E)


def e4m3_to_f32(b):
    """OCP e4m3fn from its definition: bias 7, subnormals, one NaN, no inf."""
    sign = -1.0 if b & 0x80 else 1.0
    e, m = (b >> 3) & 15, b & 7
    if e == 0:
        return sign * m * 2.0 ** -9
    if e == 15 and m == 7:
        return float("nan")
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


def e2m1_to_float(code):
    v = E2M1[code & 7]
    return -v if code & 8 else v


def e8m0_to_float(s):
    return 2.0 ** (s - 127)


ENCODE = {"bf16": f32_to_bf16, "f16": f32_to_f16, "fp8": f32_to_e4m3}
DECODE = {"bf16": bf16_to_f32, "f16": f16_to_f32, "fp8": e4m3_to_f32}


# ---------------------------------------------------------------------------
# register-level model of one tile
#
# Lane l holds, with i = l & 15 and g = l >> 4:
#   bf16 / f16 / fp8 : element j (0..7) of the A operand = A[i][8g + j], of the
#                      B operand = B[8g + j][i]
#   mxfp4            : 16 operand bytes; nibble j (0..31) is k = 32g + j, the
#                      even element in the low nibble of byte j // 2; scale
#                      byte sa = E8M0(row i, block g), sb = E8M0(col i, block g).
#                      The operand is eight VGPRs wide and the scale register
#                      four bytes: bytes 16..31 of the one and bytes 1..3 of
#                      the other are ignored
#   C / D            : register r (0..3) = [4g + r][i]
# xor_register applies a seeded operand fault to these registers, dword by
# dword as the kernel's inject_operand hook does.
# ---------------------------------------------------------------------------
FAULTS_ALL = ("swap_k_groups", "swap_rows", "reverse_j", "reverse_c", "reverse_d",
              "transpose_d")
FAULTS_MXFP4 = ("swap_nibbles", "scale_other_block", "swap_scales")


def pack_registers(dtype, seed, wg):
    """Per-lane registers as the kernel builds them: 'a' and 'b' are
    [64][8] element codes (bf16 / f16 / fp8) or [64][32] bytes (mxfp4: the
    eight VGPRs of the operand, FP4 data in the first 16 bytes and zeros in
    VGPRs 4..7), 'sa' and 'sb' [64] 32-bit scale registers with the E8M0 in
    byte 0 (mxfp4 only), 'c' [64][4] values."""
    regs = {"a": [], "b": [], "sa": [], "sb": [], "c": []}
    for lane in range(64):
        i, g = lane & 15, lane >> 4
        if dtype == "mxfp4":
            for name, which in (("a", GEN_A), ("b", GEN_B)):
                codes = [gen_fp4_code(seed, wg, which, i, 32 * g + j) for j in range(32)]
                regs[name].append([codes[2 * n] | (codes[2 * n + 1] << 4) for n in range(16)]
                                  + [0] * 16)
            regs["sa"].append(gen_scale_code(seed, wg, GEN_SA, i, g))
            regs["sb"].append(gen_scale_code(seed, wg, GEN_SB, i, g))
        else:
            enc = ENCODE[dtype]
            for name, which in (("a", GEN_A), ("b", GEN_B)):
                regs[name].append([enc(float(gen_int(seed, wg, dtype, which, i, 8 * g + j)))
                                   for j in range(8)])
        regs["c"].append([float(gen_int(seed, wg, dtype, GEN_C, 4 * g + r, i))
                          for r in range(4)])
    return regs


OPERANDS = ("a", "b", "c", "sa", "sb")


def operand_dwords(dtype, operand):
    """32-bit registers one lane holds of that operand."""
    if operand in ("sa", "sb"):
        return 1
    if operand == "c":
        return 4
    return {"bf16": 4, "f16": 4, "fp8": 2, "mxfp4": 8}[dtype]


def xor_register(dtype, regs, lane, operand, reg, mask):
    """A copy of regs with the 32-bit mask xored into dword reg of that lane's
    operand, little-endian: a 16-bit element 2 reg in the low half, bytes
    4 reg .. 4 reg + 3 from the low byte up."""
    assert operand in OPERANDS and 0 <= lane < 64 and 0 < mask <= M32
    assert 0 <= reg < operand_dwords(dtype, operand)
    assert dtype == "mxfp4" or operand not in ("sa", "sb")
    out = {name: [list(v) if isinstance(v, list) else v for v in per_lane]
           for name, per_lane in regs.items()}
    if operand in ("sa", "sb"):
        out[operand][lane] ^= mask
    elif operand == "c":
        out["c"][lane][reg] = bits_f32(f32_bits(out["c"][lane][reg]) ^ mask)
    elif dtype in ("bf16", "f16"):
        out[operand][lane][2 * reg] ^= mask & 0xFFFF
        out[operand][lane][2 * reg + 1] ^= mask >> 16
    else:
        for n in range(4):
            out[operand][lane][4 * reg + n] ^= (mask >> (8 * n)) & 0xFF
    return out


def _matmul_add(A, B, C_):
    """A·B + C. Finite operands: numpy. A non-finite operand: products and
    sums element by element in k order, so that where a NaN or an infinity
    lands does not depend on a BLAS."""
    if np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C_).all():
        return A @ B + C_
    D = np.zeros((A.shape[0], B.shape[1]))
    for r in range(A.shape[0]):
        for c in range(B.shape[1]):
            acc = float(C_[r, c])
            for k in range(A.shape[1]):
                acc += float(A[r, k]) * float(B[k, c])
            D[r, c] = acc
    return D


def _lane_values(dtype, reg, swap_nibbles=False):
    """The k-ordered element values one lane's operand register decodes to.
    Of the eight-VGPR FP4 operand only VGPRs 0..3 hold data: the instruction
    ignores the rest."""
    if dtype != "mxfp4":
        return [DECODE[dtype](code) for code in reg]
    out = []
    for byte in reg[:16]:
        even, odd = byte & 15, byte >> 4
        if swap_nibbles:
            even, odd = odd, even
        out += [e2m1_to_float(even), e2m1_to_float(odd)]
    return out


def matrices_from_registers(dtype, regs, fault=None):
    """Logical A (16 x K), B (K x 16) and C (16 x 16), float64, unpacked from
    the registers; fault as in tile_from_registers (the D-side faults do not
    act here)."""
    assert fault is None or fault in FAULTS_ALL + FAULTS_MXFP4
    K = k_of(dtype)
    per = K // 4
    swap01 = {0: 1, 1: 0}
    A = np.zeros((16, K))
    B = np.zeros((K, 16))
    C_ = np.zeros((16, 16))
    for lane in range(64):
        i, g = lane & 15, lane >> 4
        ga = swap01.get(g, g) if fault == "swap_k_groups" else g
        ia = swap01.get(i, i) if fault == "swap_rows" else i
        va = _lane_values(dtype, regs["a"][16 * ga + ia], fault == "swap_nibbles")
        vb = _lane_values(dtype, regs["b"][lane])
        if fault == "reverse_j":
            va = va[::-1]
        if dtype == "mxfp4":
            sa = regs["sa"][16 * (g ^ 1) + i if fault == "scale_other_block" else lane]
            sb = regs["sb"][lane]
            if fault == "swap_scales":
                sa, sb = sb, sa
            # opsel 0: the E8M0 is byte 0 of the scale register, the rest is ignored
            va = [v * e8m0_to_float(sa & 0xFF) for v in va]
            vb = [v * e8m0_to_float(sb & 0xFF) for v in vb]
        A[i, per * g:per * g + per] = va
        B[per * g:per * g + per, i] = vb
        c = regs["c"][lane]
        C_[4 * g:4 * g + 4, i] = c[::-1] if fault == "reverse_c" else c
    return A, B, C_


def tile_from_registers(dtype, regs, fault=None):
    """D (16 x 16, row-major as the kernel stores it) computed from the packed
    registers. fault=None unpacks by the documented lane maps; a fault name
    gets exactly one thing wrong, on the A side where a side has to be chosen
    (the same mistake on both A and B would cancel in the dot product)."""
    D = _matmul_add(*matrices_from_registers(dtype, regs, fault))
    out = np.zeros((16, 16))
    for lane in range(64):
        i, g = lane & 15, lane >> 4
        d_reg = [D[4 * g + r, i] for r in range(4)]
        if fault == "reverse_d":
            d_reg = d_reg[::-1]
        for r in range(4):
            out[4 * g + r, i] = d_reg[r]
    return out.T.copy() if fault == "transpose_d" else out
