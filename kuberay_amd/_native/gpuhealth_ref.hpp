// gpuhealth_ref — Python-free, device-free core of the GPU burn-in probe.
//
// Everything that has to agree bit-for-bit between the host and the gfx950
// kernels in gpuhealth.hip lives here as plain functions that compile for both
// sides (GH_HD): the HBM sweep pattern, the operand generators of the exact
// MFMA check, the encoders to bf16 / f16 / OCP e4m3 / e2m1 bit patterns, the
// exact reference product, the matrix generator and reference of the GEMM
// checks, and the generators, the premise, the integer reference and the LDS
// address functions of the attention check, of the causal one at head
// dimension 128 and of the paged decode one, and the generators, the routing
// builder, the tile lookup and the reference of the MoE check. No HIP, no
// pybind11 — the programs under tests/native/ (gpuhealth_ref_check.cpp,
// gemm_ref_check.cpp, gemm_narrow_ref_check.cpp, attn_ref_check.cpp,
// attn128_ref_check.cpp, attn_decode_ref_check.cpp, moe_ref_check.cpp) drive it
// as stand-alone g++ programs.
//
// Exactness premise: bf16 / f16 / fp8 operands are integers in [-8, 8], so a
// K=32 dot product plus C is an integer below 2^12; MXFP4 operands are e2m1
// codes times a block scale of 0.5, 1 or 2, so a K=128 dot product plus C is
// a multiple of 1/16 below 2^15. Both fit the 24-bit fp32 significand, hence
// every accumulation order gives the same fp32 result and the device's D can
// be compared with == against integer arithmetic.
//
// What the premise costs: integers in [-8, 8] leave the low mantissa bits of
// every bf16 (bits 4..0), f16 (bits 7..0) and e4m3 (bit 0) operand at 0, so a
// stuck-at-0 fault on those operand bits is outside what the data can show.
// Every other operand bit, every e2m1 bit and every E8M0 scale bit takes both
// values (tests/test_gpu_probe_kernels.py).
//
// Shown on the device with seeded faults that enter on the input side
// (tests/test_gpu_input_faults.py): an xor into one operand register of one
// lane before the MFMA changes D exactly as the operand lane maps say, for A,
// B, C and the MX scales, the low mantissa bits and a non-finite operand
// included, and the check flags it; the MX instruction ignores bytes 1..3 of a
// scale register and VGPRs 4..7 of the eight-VGPR FP4 operand; a stuck-at bit
// in the HBM sweep and in the LDS march is reported in exactly one of the two
// phases of every pass, whichever value it is stuck at. Still not shown:
// subnormal operands, and a stuck-at-0 on the low mantissa bits: the test
// flips them, the production data never sets them.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GH_HD __host__ __device__
#else
#define GH_HD
#endif

namespace gh {

enum Dtype : int { BF16 = 0, F16 = 1, FP8 = 2, MXFP4 = 3 };
constexpr int kNumDtypes = 4;
constexpr int kTile = 16;               // D is 16x16 for every data path
constexpr uint32_t kDefaultSeed = 0x5EED1234u;

GH_HD inline int k_of(int dtype) { return dtype == MXFP4 ? 128 : 32; }

// lowbias32 (two multiply-xorshift rounds, a bijection of 32 bits)
GH_HD inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// ---------------------------------------------------------------------------
// HBM sweep pattern: a function of the full 64-bit word index. For a fixed
// high half it is a bijection of the low half, and the high half selects the
// bijection, so an address line dropped above bit 32 cannot alias to the same
// data.
// ---------------------------------------------------------------------------
GH_HD inline uint32_t pattern_word(uint32_t seed, uint64_t word_index) {
  const uint32_t lo = (uint32_t)word_index;
  const uint32_t hi = (uint32_t)(word_index >> 32);
  uint32_t x = lo + seed * 0x9E3779B9u;
  x ^= hi * 0x85EBCA6Bu;
  return mix32(x);
}

// ---------------------------------------------------------------------------
// CU sweep: where a wave runs, and the LDS march pattern
//
// decode_location takes the raw values of the XCC_ID and HW_ID hardware
// registers. The masks below are the only place the register layout is written
// down. They follow the GCN/CDNA HW_ID layout as the HIP headers document it
// for the gfx942 family (SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 14:13: four
// shader engines per XCC; bit 15 belongs to SE_ID only on the single-die
// gfx908/gfx90a) and XCC_ID 3:0 of its own register. The layout is right
// exactly when a saturating sweep observes as many distinct location keys as
// the device has CUs (tests/test_gpu_cu_sweep.py): a field that is too narrow
// merges CUs and gives too few, a mask that takes in bits of a neighbouring
// field (wave slot, pipe, thread-group id) splits CUs and gives too many.
// ---------------------------------------------------------------------------
struct CuLocation {
  uint32_t xcc, se, sh, cu, simd;
};

constexpr uint32_t kXccShift = 0, kXccBits = 4;    // XCC_ID register
constexpr uint32_t kSimdShift = 4, kSimdBits = 2;  // HW_ID register from here on
constexpr uint32_t kCuShift = 8, kCuBits = 4;
constexpr uint32_t kShShift = 12, kShBits = 1;
constexpr uint32_t kSeShift = 13, kSeBits = 2;
constexpr uint32_t kNumSimds = 1u << kSimdBits;
// one slot per (xcc, se, sh, cu) the fields can name
constexpr uint32_t kCuSlots = 1u << (kXccBits + kSeBits + kShBits + kCuBits);

GH_HD inline uint32_t reg_field(uint32_t reg, uint32_t shift, uint32_t bits) {
  return (reg >> shift) & ((1u << bits) - 1u);
}

GH_HD inline CuLocation decode_location(uint32_t xcc_id_reg, uint32_t hw_id_reg) {
  CuLocation loc;
  loc.xcc = reg_field(xcc_id_reg, kXccShift, kXccBits);
  loc.se = reg_field(hw_id_reg, kSeShift, kSeBits);
  loc.sh = reg_field(hw_id_reg, kShShift, kShBits);
  loc.cu = reg_field(hw_id_reg, kCuShift, kCuBits);
  loc.simd = reg_field(hw_id_reg, kSimdShift, kSimdBits);
  return loc;
}

// dense index over (xcc, se, sh, cu), below kCuSlots; the SIMD is not part of it
GH_HD inline uint32_t location_key(const CuLocation& loc) {
  return (((loc.xcc << kSeBits | loc.se) << kShBits | loc.sh) << kCuBits) | loc.cu;
}

// inverse of location_key (simd = 0)
GH_HD inline CuLocation location_of_key(uint32_t key) {
  CuLocation loc;
  loc.cu = key & ((1u << kCuBits) - 1u);
  key >>= kCuBits;
  loc.sh = key & ((1u << kShBits) - 1u);
  key >>= kShBits;
  loc.se = key & ((1u << kSeBits) - 1u);
  key >>= kSeBits;
  loc.xcc = key & ((1u << kXccBits) - 1u);
  loc.simd = 0;
  return loc;
}

// LDS word `word` of workgroup visit `visit` holds
// pattern_word(seed, lds_pattern_index(visit, word)) ^ invert: the visit is the
// high half of the index and so selects the bijection, every visit of a CU
// sees different data.
GH_HD inline uint64_t lds_pattern_index(uint32_t visit, uint32_t word) {
  return (uint64_t)visit << 32 | word;
}

// ---------------------------------------------------------------------------
// operand generators
// ---------------------------------------------------------------------------
enum Which : uint32_t { GEN_A = 0, GEN_B = 1, GEN_C = 2, GEN_SA = 3, GEN_SB = 4 };

// i: row of A / column of B / row of C (0..15); k: k of A and B, column of C,
// scale block of SA / SB (0..127)
GH_HD inline uint32_t elem_hash(uint32_t seed, uint32_t wg, int dtype,
                                uint32_t which, uint32_t i, uint32_t k) {
  uint32_t h = mix32(seed ^ ((wg + 1u) * 0x9E3779B9u));
  return mix32(h ^ (((uint32_t)dtype * 8u + which) << 24) ^ (i << 8) ^ k);
}

// integer operand in [-8, 8] (bf16 / f16 / fp8 A and B, and C of every path)
GH_HD inline int gen_int(uint32_t seed, uint32_t wg, int dtype, uint32_t which,
                         uint32_t i, uint32_t k) {
  return (int)((elem_hash(seed, wg, dtype, which, i, k) >> 8) % 17u) - 8;
}

// e2m1 code 0..15 (MXFP4 A and B): all codes, -0 and the half-steps included
GH_HD inline uint32_t gen_fp4(uint32_t seed, uint32_t wg, uint32_t which,
                              uint32_t i, uint32_t k) {
  return (elem_hash(seed, wg, MXFP4, which, i, k) >> 8) & 15u;
}

// E8M0 scale of one 32-element block: 126, 127 or 128 (x0.5, x1, x2).
// which is GEN_SA (i = row of A) or GEN_SB (i = column of B).
GH_HD inline uint32_t gen_scale(uint32_t seed, uint32_t wg, uint32_t which,
                                uint32_t i, uint32_t block) {
  return 126u + (elem_hash(seed, wg, MXFP4, which, i, block) >> 8) % 3u;
}

GH_HD inline int gen_c(uint32_t seed, uint32_t wg, int dtype, uint32_t row,
                       uint32_t col) {
  return gen_int(seed, wg, dtype, GEN_C, row, col);
}

// ---------------------------------------------------------------------------
// encoders / decoders
// ---------------------------------------------------------------------------
GH_HD inline uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
GH_HD inline float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// round-to-nearest-even; NaN stays NaN
GH_HD inline uint16_t f32_to_bf16(float f) {
  uint32_t u = f32_bits(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
GH_HD inline float bf16_to_f32(uint16_t b) { return bits_f32((uint32_t)b << 16); }

// normal range and zero, round-to-nearest-even; magnitudes below 2^-14 flush
// to zero and overflow gives infinity (the generators emit small integers)
GH_HD inline uint16_t f32_to_f16(float f) {
  const uint32_t u = f32_bits(f);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const int e = (int)((u >> 23) & 0xFFu) - 127 + 15;
  const uint32_t m = u & 0x7FFFFFu;
  if (e <= 0) return (uint16_t)sign;
  if (e >= 31) return (uint16_t)(sign | 0x7C00u);
  uint32_t h = ((uint32_t)e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
  return (uint16_t)(sign | h);
}
GH_HD inline float f16_to_f32(uint16_t h) {
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 0x1Fu;
  const uint32_t m = h & 0x3FFu;
  if (e == 0) {  // zero / subnormal: m * 2^-24
    const float v = (float)m * (1.0f / 16777216.0f);
    return sign ? -v : v;
  }
  if (e == 31) return bits_f32(sign | 0x7F800000u | (m << 13));
  return bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}

// OCP e4m3fn (bias 7, no infinity, max 448): normal range and zero,
// round-to-nearest-even, saturating; magnitudes below 2^-6 flush to zero
GH_HD inline uint8_t f32_to_e4m3(float f) {
  const uint32_t u = f32_bits(f);
  const uint32_t sign = (u >> 24) & 0x80u;
  const int e = (int)((u >> 23) & 0xFFu) - 127 + 7;
  const uint32_t m = u & 0x7FFFFFu;
  if (e <= 0) return (uint8_t)sign;
  if (e >= 16) return (uint8_t)(sign | 0x7Eu);
  uint32_t h = ((uint32_t)e << 3) | (m >> 20);
  const uint32_t rem = m & 0xFFFFFu;
  if (rem > 0x80000u || (rem == 0x80000u && (h & 1u))) ++h;
  if (h > 0x7Eu) h = 0x7Eu;
  return (uint8_t)(sign | h);
}
GH_HD inline float e4m3_to_f32(uint8_t b) {
  const uint32_t sign = ((uint32_t)b & 0x80u) << 24;
  const uint32_t e = (b >> 3) & 0xFu;
  const uint32_t m = b & 7u;
  if (e == 0) {  // zero / subnormal: m * 2^-9
    const float v = (float)m * (1.0f / 512.0f);
    return sign ? -v : v;
  }
  if (e == 15 && m == 7) return bits_f32(sign | 0x7FC00000u);
  return bits_f32(sign | ((e + 120u) << 23) | (m << 20));
}

// e2m1: code = sign<<3 | magnitude index; magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6.
// Value in half units (exact integers), sign applied; -0 decodes to 0.
GH_HD inline int e2m1_half_units(uint32_t code) {
  const uint32_t mag = code & 7u;
  const int h = mag < 4u ? (int)mag : (mag < 6u ? (int)(2u * mag - 4u) : (int)(4u * mag - 16u));
  return (code & 8u) ? -h : h;
}
GH_HD inline float e2m1_to_f32(uint32_t code) {
  const float v = 0.5f * (float)e2m1_half_units(code & 7u);
  return (code & 8u) ? -v : v;  // keeps the sign of -0
}
// exact values only (a multiple of 0.5 that e2m1 has); anything else -> 0xFF
GH_HD inline uint8_t f32_to_e2m1(float f) {
  const uint32_t sign = (f32_bits(f) >> 28) & 8u;
  const float a = f < 0.0f ? -f : f;
  for (uint32_t mag = 0; mag < 8u; ++mag) {
    if (0.5f * (float)e2m1_half_units(mag) == a) return (uint8_t)(sign | mag);
  }
  return 0xFFu;
}
// two codes per byte, the even element in the low nibble
GH_HD inline uint8_t pack_fp4(uint32_t even_code, uint32_t odd_code) {
  return (uint8_t)((even_code & 15u) | ((odd_code & 15u) << 4));
}
GH_HD inline float e8m0_to_f32(uint32_t s) { return bits_f32((s & 0xFFu) << 23); }

// ---------------------------------------------------------------------------
// logical operand values (MX scales applied) and the exact reference
// ---------------------------------------------------------------------------
GH_HD inline float logical_a(int dtype, uint32_t seed, uint32_t wg, uint32_t row, uint32_t k) {
  if (dtype == MXFP4) {
    return e2m1_to_f32(gen_fp4(seed, wg, GEN_A, row, k)) *
           e8m0_to_f32(gen_scale(seed, wg, GEN_SA, row, k >> 5));
  }
  return (float)gen_int(seed, wg, dtype, GEN_A, row, k);
}
GH_HD inline float logical_b(int dtype, uint32_t seed, uint32_t wg, uint32_t k, uint32_t col) {
  if (dtype == MXFP4) {
    return e2m1_to_f32(gen_fp4(seed, wg, GEN_B, col, k)) *
           e8m0_to_f32(gen_scale(seed, wg, GEN_SB, col, k >> 5));
  }
  return (float)gen_int(seed, wg, dtype, GEN_B, col, k);
}

// D[row][col] in units of 1/16, in integer arithmetic only
GH_HD inline int64_t reference_element_x16(int dtype, uint32_t seed, uint32_t wg,
                                           uint32_t row, uint32_t col) {
  int64_t acc = 16 * (int64_t)gen_c(seed, wg, dtype, row, col);
  if (dtype == MXFP4) {
    for (uint32_t blk = 0; blk < 4u; ++blk) {
      // (a/2 * 2^(sa-127)) * (b/2 * 2^(sb-127)) * 16 = a*b * 2^(sa+sb-252)
      const int shift = (int)gen_scale(seed, wg, GEN_SA, row, blk) +
                        (int)gen_scale(seed, wg, GEN_SB, col, blk) - 252;
      int64_t part = 0;
      for (uint32_t k = 32u * blk; k < 32u * blk + 32u; ++k) {
        part += (int64_t)e2m1_half_units(gen_fp4(seed, wg, GEN_A, row, k)) *
                e2m1_half_units(gen_fp4(seed, wg, GEN_B, col, k));
      }
      acc += part * ((int64_t)1 << shift);
    }
  } else {
    int64_t dot = 0;
    for (uint32_t k = 0; k < 32u; ++k) {
      dot += (int64_t)gen_int(seed, wg, dtype, GEN_A, row, k) *
             gen_int(seed, wg, dtype, GEN_B, col, k);
    }
    acc += 16 * dot;
  }
  return acc;
}

GH_HD inline float reference_element(int dtype, uint32_t seed, uint32_t wg,
                                     uint32_t row, uint32_t col) {
  // |x16| < 2^24, so the conversion and the division by 16 are both exact
  return (float)reference_element_x16(dtype, seed, wg, row, col) * 0.0625f;
}

inline void reference_tile(int dtype, uint32_t seed, uint32_t wg, float D[16][16]) {
  for (uint32_t r = 0; r < 16u; ++r)
    for (uint32_t c = 0; c < 16u; ++c)
      D[r][c] = reference_element(dtype, seed, wg, r, c);
}

// ---------------------------------------------------------------------------
// MFMA load: a chain of MFMAs on one exact tile that stays exactly checkable
//
// Alternating-sign premise: a wave holds A, B and C of an exact tile and issues
// acc = mfma(A, B, acc), acc = mfma(-A, B, acc), ... starting from acc = C,
// where -A is A with the sign bit of every element flipped (negate_mask). Every
// partial sum is C plus a signed subset of the K products of one A·B: for
// bf16 / f16 / fp8 an integer below 2^13, for MXFP4 a multiple of 1/16 below
// 2^16. Both fit the fp32 significand, so every accumulation order gives the
// same bits, as in the premise at the top, and after n MFMAs acc is
// reference_element (n odd) or C (n even), whatever n is. A chain of any
// length on hashed data can be compared with == against integer arithmetic.
//
// Its one real limit: an error that enters the accumulator is carried to the
// next check only if it is at least one unit of the data (1 for the integer
// paths, 1/16 for MXFP4). An error below the ulp of a later partial sum can be
// rounded away before the check sees it; the check interval (check_every
// MFMAs) bounds how long that window is.
// ---------------------------------------------------------------------------
constexpr uint32_t kLoadWaves = 4;  // waves of one load workgroup, one per SIMD
constexpr uint32_t kLoadTiles = 4;  // independent exact tiles one wave keeps going

// the per-dword xor that negates every element of a packed A or B operand; MX
// scales are not touched
GH_HD inline uint32_t negate_mask(int dtype) {
  return dtype == MXFP4 ? 0x88888888u : (dtype == FP8 ? 0x80808080u : 0x80008000u);
}

GH_HD inline uint64_t flop_per_mfma(int dtype) {
  return 2ull * kTile * kTile * (uint64_t)k_of(dtype);
}

// Which exact tile (the wg of the generators) tile `tile` of wave `wave` of
// workgroup visit `visit` works on: different for every wave of every launch.
// One operand set serves all chunks of a visit: building a set is integer
// hashing (the expectation is computed off the matrix pipe) and was measured at
// about 40 us a wave, 330 us for MXFP4, against 7 to 9 us for a chunk of 239
// MFMAs per tile (docs/benchmarks.md, "MFMA load"). It is paid once per launch
// and not once per check.
GH_HD inline uint32_t load_tile_index(uint32_t visit, uint32_t wave, uint32_t tile) {
  return (visit * kLoadWaves + wave) * kLoadTiles + tile;
}

// acc[row][col] of tile wg after n_mfmas MFMAs of the alternating chain
GH_HD inline float expected_after(int dtype, uint32_t seed, uint32_t wg, uint32_t row,
                                  uint32_t col, uint64_t n_mfmas) {
  return (n_mfmas & 1u) ? reference_element(dtype, seed, wg, row, col)
                        : (float)gen_c(seed, wg, dtype, row, col);
}

// ---------------------------------------------------------------------------
// GEMM check: D = A·B + C on whole matrices in device memory
//
// elem_hash packs i << 8 ^ k and so cannot index a matrix; this generator
// hashes the full 32-bit row and column, the row first and the column into its
// result, so (r, c) and (c, r) are unrelated. Exactness premise: A (M x K) and
// B (K x N) hold integers in [-8, 8] as bf16 or f16 and C integers in [-8, 8]
// as fp32, so every partial sum is an integer and |D| <= 64 K + 8 < 2^24 for
// K <= kGemmMaxK = 65536. Every accumulation order, whatever the tiling and
// the split of K, gives the same fp32 value, and == is the compare. The cost is
// that of the premise at the top: the low mantissa bits of every operand are 0.
// ---------------------------------------------------------------------------
constexpr uint32_t kGemmTile = 64;     // a workgroup's tile of D, and the K step of a stage
constexpr uint32_t kGemmMaxK = 65536;  // 64 K + 8 < 2^24
constexpr uint32_t kGemmMaxMN = 65536;  // not needed for exactness: bounds what one call allocates

// the per-matrix part of the hash; which is GEN_A, GEN_B or GEN_C
GH_HD inline uint32_t gemm_matrix_hash(uint32_t seed, int dtype, uint32_t which) {
  return mix32(seed ^ (((uint32_t)dtype * 8u + which + 1u) * 0x9E3779B9u));
}
GH_HD inline int gemm_int_of(uint32_t matrix_hash, uint32_t row, uint32_t col) {
  return (int)((mix32(mix32(matrix_hash ^ row) + col) >> 8) % 17u) - 8;
}
// A[row][col] (row of M, col of K), B[row][col] (row of K, col of N) or
// C[row][col]: an integer in [-8, 8]
GH_HD inline int gen_gemm_int(uint32_t seed, int dtype, uint32_t which, uint32_t row,
                              uint32_t col) {
  return gemm_int_of(gemm_matrix_hash(seed, dtype, which), row, col);
}

// D[row][col] of the K-deep product, in integer arithmetic only
GH_HD inline int32_t gemm_reference_element(uint32_t seed, int dtype, uint32_t K, uint32_t row,
                                            uint32_t col) {
  const uint32_t ha = mix32(gemm_matrix_hash(seed, dtype, GEN_A) ^ row);
  const uint32_t hb = gemm_matrix_hash(seed, dtype, GEN_B);
  int32_t acc = gen_gemm_int(seed, dtype, GEN_C, row, col);
  for (uint32_t k = 0; k < K; ++k) {
    const int a = (int)((mix32(ha + k) >> 8) % 17u) - 8;  // gemm_int_of, the row hoisted
    acc += a * gemm_int_of(hb, k, col);
  }
  return acc;
}

// a 16-bit operand of the GEMM as it lies in memory
GH_HD inline uint16_t gemm_encode(int dtype, int value) {
  return dtype == F16 ? f32_to_f16((float)value) : f32_to_bf16((float)value);
}

// ---------------------------------------------------------------------------
// Narrow GEMM check: the same D = A·B + C for fp8 (OCP e4m3) and MXFP4
//
// Layouts, all row-major: A is M x K and B is K x N; fp8 is a byte per
// element, mxfp4 two e2m1 codes per byte along the row (along K for A, along N
// for B), the even element in the low nibble as pack_fp4 has it. The MX scales
// are bytes, SA[M][K / 32] and SB[K / 32][N]; block kb covers k = 32 kb .. + 31.
// C and D are fp32. The generator is the matrix hash above (full 32-bit row
// and column); gemm_matrix_hash takes GEN_SA and GEN_SB as well.
//
// Exactness premise. fp8: A, B and C are integers in [-8, 8] (e4m3 holds them
// exactly, bit 0 of every operand stays 0), so |D| <= 64 K + 8 < 2^24 for
// K <= 65536, as for bf16. mxfp4: A and B take all 16 e2m1 codes, at most 12
// half units, and the scales are 126, 127 or 128 (x0.5, x1, x2); in units of
// 1/16 one product is at most 12 · 12 · 2^4 = 2304 and C adds at most 128, so
// 2304 K + 128 < 2^24 holds up to K = 7168 and K is capped at 4096. Every
// partial sum is then a multiple of 1/16 below 2^20 and every accumulation
// order gives the same fp32 value. That the scaled MFMA keeps sums of this
// size exact is shown on the device for the hashed data at K = 4096 (and for
// fp8 at K = 65536) by tests/test_gpu_gemm_narrow.py; for other data of the
// same range it is argued from the bound and not shown. The data never holds
// a subnormal or a non-finite fp8 operand.
// ---------------------------------------------------------------------------
constexpr uint32_t kNarrowMaxKFp8 = 65536;   // 64 K + 8 < 2^24
constexpr uint32_t kNarrowMaxKMxfp4 = 4096;  // 2304 K + 128 < 2^24 up to 7168
constexpr uint32_t kNarrowMaxProductX16 = 12 * 12 * 16;  // mxfp4, in sixteenths

GH_HD constexpr uint32_t narrow_stage_k(int dtype) { return dtype == MXFP4 ? 256u : 128u; }
GH_HD constexpr uint32_t narrow_max_k(int dtype) {
  return dtype == MXFP4 ? kNarrowMaxKMxfp4 : kNarrowMaxKFp8;
}
// elements of A or B that one byte holds
GH_HD constexpr uint32_t narrow_per_byte(int dtype) { return dtype == MXFP4 ? 2u : 1u; }

// e2m1 code 0..15 of an mxfp4 A[row][col] or B[row][col]
GH_HD inline uint32_t gemm_fp4_of(uint32_t matrix_hash, uint32_t row, uint32_t col) {
  return (mix32(mix32(matrix_hash ^ row) + col) >> 8) & 15u;
}
// E8M0 byte of SA[row][block] or SB[block][col]: 126, 127 or 128
GH_HD inline uint32_t gemm_scale_of(uint32_t matrix_hash, uint32_t row, uint32_t col) {
  return 126u + (mix32(mix32(matrix_hash ^ row) + col) >> 8) % 3u;
}

// What the generator puts at [row][col] of a matrix of the narrow check: the
// integer for fp8 A and B and for every C, the e2m1 code for mxfp4 A and B, the
// E8M0 byte for SA and SB.
GH_HD inline int gen_narrow(uint32_t seed, int dtype, uint32_t which, uint32_t row, uint32_t col) {
  const uint32_t h = gemm_matrix_hash(seed, dtype, which);
  if (which == GEN_SA || which == GEN_SB) return (int)gemm_scale_of(h, row, col);
  if (dtype == MXFP4 && which != GEN_C) return (int)gemm_fp4_of(h, row, col);
  return gemm_int_of(h, row, col);
}

// the byte of A or B that holds elements [row][col ..] (col a multiple of
// narrow_per_byte), as it lies in memory
GH_HD inline uint8_t narrow_operand_byte(uint32_t matrix_hash, int dtype, uint32_t row,
                                         uint32_t col) {
  if (dtype == MXFP4)
    return pack_fp4(gemm_fp4_of(matrix_hash, row, col), gemm_fp4_of(matrix_hash, row, col + 1));
  return f32_to_e4m3((float)gemm_int_of(matrix_hash, row, col));
}

// D[row][col] of the K-deep product in units of 1/16, in integer arithmetic only
GH_HD inline int64_t gemm_narrow_reference_x16(uint32_t seed, int dtype, uint32_t K, uint32_t row,
                                               uint32_t col) {
  if (dtype != MXFP4) return 16 * (int64_t)gemm_reference_element(seed, dtype, K, row, col);
  const uint32_t ha = mix32(gemm_matrix_hash(seed, dtype, GEN_A) ^ row);  // the row hoisted
  const uint32_t hsa = mix32(gemm_matrix_hash(seed, dtype, GEN_SA) ^ row);
  const uint32_t hb = gemm_matrix_hash(seed, dtype, GEN_B);
  const uint32_t hsb = gemm_matrix_hash(seed, dtype, GEN_SB);
  int64_t acc = 16 * (int64_t)gen_narrow(seed, dtype, GEN_C, row, col);
  for (uint32_t kb = 0; kb < K / 32u; ++kb) {
    // (a/2 · 2^(sa-127)) · (b/2 · 2^(sb-127)) · 16 = a·b · 2^(sa+sb-252)
    const int shift = (int)(126u + (mix32(hsa + kb) >> 8) % 3u) +
                      (int)gemm_scale_of(hsb, kb, col) - 252;
    int32_t part = 0;
    for (uint32_t k = 32u * kb; k < 32u * kb + 32u; ++k)
      part += e2m1_half_units((mix32(ha + k) >> 8) & 15u) *
              e2m1_half_units(gemm_fp4_of(hb, k, col));
    acc += (int64_t)part * ((int64_t)1 << shift);
  }
  return acc;
}
GH_HD inline float gemm_narrow_reference(uint32_t seed, int dtype, uint32_t K, uint32_t row,
                                         uint32_t col) {
  // |x16| < 2^24, so the conversion and the division by 16 are both exact
  return (float)gemm_narrow_reference_x16(seed, dtype, K, row, col) * 0.0625f;
}

// ---------------------------------------------------------------------------
// Narrow GEMM check: where a stage lies in LDS, shared by the kernel and by
// tests/native/gemm_narrow_ref_check.cpp, which shows every address in bounds
// and the placement complete before the kernel runs at all.
//
// A stage is 8 KiB of A and 8 KiB of B of one 64 x 64 tile of D, 512 slots of
// 16 bytes per operand. A: 64 rows of 128 bytes for both types (128 fp8 or 256
// e2m1 of K), eight chunks per row. B: fp8 128 k-rows of 64 bytes, four chunks
// per row; mxfp4 256 k-rows of 32 bytes, two chunks per row. Slot s of an
// operand holds chunk (s % per_row) ^ swizzle(row) of row s / per_row.
//
// Swizzles (correctness does not depend on them):
//   A: (row >> 1) & 7, as in the 16-bit check: the 16 rows that 16 lanes read
//      at one chunk fall into 16 different places of the 64 banks.
//   B fp8: (row >> 2) & 3. A transposed read of 16 lanes touches 8 consecutive
//      k-rows at one chunk and the four lane groups 32 of them; rows 64 bytes
//      apart repeat their banks every 4 rows, the xor moves rows 4 .. 15 of
//      every 16 onto the other three chunks, so 16 rows cover the 64 banks once.
//   B mxfp4: (row >> 3) & 1. A transposed read of 16 lanes touches 16
//      consecutive k-rows, 8 bytes each; rows 32 bytes apart repeat every 8
//      rows and there is one bit of chunk to give: rows 8 .. 15 go to the other
//      chunk. The four lane groups are 32 rows apart and still share banks.
// ---------------------------------------------------------------------------
constexpr uint32_t kNarrowOperandBytes = 8192;
constexpr uint32_t kNarrowSlots = kNarrowOperandBytes / 16;

struct NarrowChunk {
  uint32_t row, byte;  // row of the tile (of M for A, of the stage's K for B), byte within it
};

GH_HD constexpr uint32_t narrow_b_row_bytes(int dtype) { return dtype == MXFP4 ? 32u : 64u; }
GH_HD inline uint32_t narrow_a_swizzle(uint32_t row) { return (row >> 1) & 7u; }
GH_HD inline uint32_t narrow_b_swizzle(int dtype, uint32_t row) {
  return dtype == MXFP4 ? (row >> 3) & 1u : (row >> 2) & 3u;
}

// what belongs into 16-byte slot `slot` (0..511) of A's and of B's part of a stage
GH_HD inline NarrowChunk narrow_a_source(uint32_t slot) {
  const uint32_t row = slot >> 3;
  return {row, 16u * ((slot & 7u) ^ narrow_a_swizzle(row))};
}
GH_HD inline NarrowChunk narrow_b_source(int dtype, uint32_t slot) {
  const uint32_t per_row = narrow_b_row_bytes(dtype) / 16u, row = slot / per_row;
  return {row, 16u * ((slot % per_row) ^ narrow_b_swizzle(dtype, row))};
}

// Byte offset within A's 8 KiB of the A fragment of lane (i, g) for tile row
// `row` at MFMA step t of the stage. fp8: 8 bytes, k = 32 t + 8 g + j. mxfp4:
// 16 bytes, k = 128 t + 32 g + j, two to a byte.
GH_HD inline uint32_t narrow_a_read(int dtype, uint32_t row, uint32_t t, uint32_t g) {
  const uint32_t byte = dtype == MXFP4 ? 64u * t + 16u * g : 32u * t + 8u * g;
  return row * 128u + 16u * ((byte >> 4) ^ narrow_a_swizzle(row)) + (byte & 15u);
}

// Lane maps of the two transposed reads, as debug_lds_tr_dump(bits=8 / 4)
// measures them (tests/test_gpu_gemm_narrow.py); both stay within a group of 16
// lanes, b = l & ~15, i = l & 15. Lane l hands in the address of 8 bytes.
//   ds_read_b64_tr_b8: byte e (0..7) of lane l's result is byte i % 8 of what
//     lane b + 2 e + i / 8 pointed at. Read as a matrix whose row e is the 16
//     bytes of lanes b + 2 e and b + 2 e + 1, lane l receives column i.
//   ds_read_b64_tr_b4: nibble e (0..15) of lane l's result is nibble i of what
//     lane b + e pointed at: row e is the 16 nibbles of lane b + e, lane l
//     receives column i.
// The value is the source as lane * elements-per-lane + element.
GH_HD inline uint32_t narrow_tr8_source(uint32_t lane, uint32_t e) {
  const uint32_t b = lane & ~15u, i = lane & 15u;
  return 8u * (b + 2u * e + i / 8u) + i % 8u;
}
GH_HD inline uint32_t narrow_tr4_source(uint32_t lane, uint32_t e) {
  return 16u * ((lane & ~15u) + e) + (lane & 15u);
}

// Byte offset within B's 8 KiB that lane (i, g) hands to the transposed read
// for the 16 columns from tile column `col` (a multiple of 16) at MFMA step t.
// fp8: one ds_read_b64_tr_b8; the lane points at k-row 32 t + 8 g + i / 2,
// bytes col + 8 (i % 2) .. + 7, and receives B[32 t + 8 g + e][col + i].
// mxfp4: two ds_read_b64_tr_b4, half h; the lane points at k-row 128 t + 32 g +
// 16 h + i, the 16 nibbles from column col, and receives in nibble e
// B[128 t + 32 g + 16 h + e][col + i]. k runs along the register, as MFMA wants.
GH_HD inline uint32_t narrow_b_read(int dtype, uint32_t col, uint32_t t, uint32_t g, uint32_t h,
                                    uint32_t i) {
  const uint32_t row = dtype == MXFP4 ? 128u * t + 32u * g + 16u * h + i
                                      : 32u * t + 8u * g + i / 2u;
  const uint32_t byte = dtype == MXFP4 ? col / 2u : col + 8u * (i % 2u);
  return row * narrow_b_row_bytes(dtype) +
         16u * ((byte >> 4) ^ narrow_b_swizzle(dtype, row)) + (byte & 15u);
}

// ---------------------------------------------------------------------------
// Attention check: unnormalised single-head attention forward, base 2, scale 1
//
//   s = Q·Kᵀ,  m[i] = max_j s_ij,  l[i] = Σ_j 2^(s_ij - m_i),
//   O~[i][d] = Σ_j 2^(s_ij - m_i) · V[j][d]
//
// Q is M x 64, K and V are N x 64, row-major bf16 or f16; O~, m and l are fp32.
// No mask and no final division. The generators hash (row, col, seed) through
// gemm_matrix_hash with GEN_Q, GEN_KEY and GEN_V:
//   Q: dense integers in [-2, 2].
//   K: two-hot. Row j is zero but for ±1 at two distinct columns d1(j) != d2(j)
//      (attn_key_of), so s_ij = ±Q[i][d1] ± Q[i][d2] is an integer in [-4, 4]
//      that costs two lookups to recompute.
//   V: dense integers in [-8, 8].
//
// Exactness premise. Every s is an integer in [-4, 4], so for every row
// max_j s - min_j s <= 8 by construction. A running maximum m_run of an online
// softmax is the maximum over the keys seen so far, so 0 <= m_run - s <= 8 for
// every s among them and every p = 2^(s - m_run) is a power of two in
// [2^-8, 1]: exact in fp32, in bf16 and in f16 (normal down to 2^-14). Every partial l is a sum of at most N such
// powers: a multiple of 2^-8 and at most N. Every partial O~ is a sum of at
// most N products p·v with |v| <= 8: a multiple of 2^-8 of magnitude at most
// 8 N <= 2^15 for N <= kAttnMaxN = 4096, at most 15 + 8 = 23 significant bits,
// so it is exact in fp32 in any summation order. A rescale by
// 2^(m_old - m_new) is exact because its result is again such a sum, under the
// new maximum. Hence the device's O~, m and l can be compared with == against
// integer arithmetic: Σ_j 2^(8 + s - m) · v is an int32 of magnitude at most
// 2^23, scaled by 2^-8. That the MFMA keeps sums of this size exact is shown on
// the device for the hashed data at N = 4096 (tests/test_gpu_attn_exact.py);
// for other data of the same range it is argued from the bound.
//
// What the premise costs, beyond the zero low mantissa bits of every operand:
// v_exp_f32 only ever sees the integers -8 .. 0 and -inf.
// ---------------------------------------------------------------------------
constexpr uint32_t GEN_Q = 5, GEN_KEY = 6, GEN_V = 7;  // after Which, for gemm_matrix_hash
constexpr uint32_t kAttnHeadDim = 64;
constexpr uint32_t kAttnBlock = 64;     // queries of a workgroup, and keys of a stage
constexpr uint32_t kAttnMaxN = 4096;    // 8 N * 2^8 <= 2^23
constexpr uint32_t kAttnMaxM = 65536;   // not needed for exactness: bounds what one call allocates
constexpr uint32_t kAttnOutCols = kAttnHeadDim + 2;  // a row of the result: O~, then m, then l

GH_HD inline int attn_q_of(uint32_t matrix_hash, uint32_t row, uint32_t col) {
  return (int)((mix32(mix32(matrix_hash ^ row) + col) >> 8) % 5u) - 2;
}

struct AttnKey {
  uint32_t d1, d2;  // distinct columns
  int s1, s2;       // +1 or -1
};
GH_HD inline AttnKey attn_key_of(uint32_t matrix_hash, uint32_t row) {
  const uint32_t h = mix32(matrix_hash ^ row);
  AttnKey k;
  k.d1 = (h >> 8) & 63u;
  k.d2 = (k.d1 + 1u + (h >> 14) % 63u) & 63u;  // d1 + 1 .. d1 + 63 mod 64: never d1
  k.s1 = (h >> 24) & 1u ? -1 : 1;
  k.s2 = (h >> 25) & 1u ? -1 : 1;
  return k;
}
GH_HD inline int attn_k_of(uint32_t matrix_hash, uint32_t row, uint32_t col) {
  const AttnKey k = attn_key_of(matrix_hash, row);
  return col == k.d1 ? k.s1 : col == k.d2 ? k.s2 : 0;
}

// Q[row][col], K[row][col] or V[row][col] of the attention check; which is
// GEN_Q, GEN_KEY or GEN_V
GH_HD inline int gen_attn(uint32_t seed, int dtype, uint32_t which, uint32_t row, uint32_t col) {
  const uint32_t h = gemm_matrix_hash(seed, dtype, which);
  return which == GEN_Q ? attn_q_of(h, row, col)
                        : which == GEN_KEY ? attn_k_of(h, row, col) : gemm_int_of(h, row, col);
}

struct AttnExpected {
  float o, m, l;
};

// O~[row][d], m[row] and l[row] over N keys, in integer arithmetic only and in
// one pass: 2^(8 + s - m) = 2^(s + 4) · 2^(4 - m), so the sums are taken with
// the weights 2^(s + 4) in [1, 256] and shifted once the maximum is known. The
// shifted sums are the true ones times 2^8, below 2^23 and 2^20.
GH_HD inline AttnExpected attn_reference(uint32_t seed, int dtype, uint32_t N, uint32_t row,
                                         uint32_t d) {
  const uint32_t hq = mix32(gemm_matrix_hash(seed, dtype, GEN_Q) ^ row);  // the row hoisted
  const uint32_t hk = gemm_matrix_hash(seed, dtype, GEN_KEY);
  const uint32_t hv = gemm_matrix_hash(seed, dtype, GEN_V);
  int m = -4;
  int64_t o = 0, l = 0;
  for (uint32_t j = 0; j < N; ++j) {
    const AttnKey k = attn_key_of(hk, j);
    const int s = k.s1 * ((int)((mix32(hq + k.d1) >> 8) % 5u) - 2) +
                  k.s2 * ((int)((mix32(hq + k.d2) >> 8) % 5u) - 2);
    m = s > m ? s : m;
    l += (int64_t)1 << (s + 4);
    o += ((int64_t)1 << (s + 4)) * gemm_int_of(hv, j, d);
  }
  // |o| << (4 - m) < 2^24 and a multiple of 1: the conversion and the scaling
  // by 2^-8 are both exact
  AttnExpected e;
  e.o = (float)(int32_t)(o * ((int64_t)1 << (4 - m))) * (1.0f / 256.0f);
  e.m = (float)m;
  e.l = (float)(int32_t)(l * ((int64_t)1 << (4 - m))) * (1.0f / 256.0f);
  return e;
}

// ---------------------------------------------------------------------------
// Attention check: where a stage lies in LDS, shared by the kernel
// (gpuhealth_attn.hip) and by tests/native/attn_ref_check.cpp, which shows every
// address in bounds and every register position the element the MFMA wants.
//
// A stage is a block of 64 keys: 8 KiB of K and 8 KiB of V, 64 rows of 128
// bytes = eight 16-byte chunks, 512 slots per operand. Slot s holds chunk
// (s % 8) ^ swizzle(row) of row s / 8; the global side fetches what belongs
// into its slot, as in the GEMM checks.
//
// Reads (lane l, i = l & 15, g = l >> 4):
//   K is the A operand of Sᵀ = K·Qᵀ: lane (i, g) reads K[key][32 ds + 8 g .. + 7]
//   of key 16 kt + i with one ds_read_b128, the A-read of the GEMM check, and
//   its swizzle: (row >> 1) & 7 spreads the 16 rows of a read over the banks.
//   V is the A operand of O~ᵀ += Vᵀ·Pᵀ. The B operand Pᵀ is what the lane holds
//   of Sᵀ, in register order: k-slot t (0..7) of lane group g in the 32-key
//   chunk c is key attn_v_key(c, g, t) = 32 c + 16 (t / 4) + 4 g + t % 4, so
//   Vᵀ has to bring the same keys to the same slots. Half h (slots 4 h .. + 3)
//   of a fragment is one ds_read_b64_tr_b16 in which lane (i, g) points at
//   V[32 c + 16 h + 4 g + i / 4][16 dt + 4 (i % 4) .. + 3]; by the lane map of
//   the read (attn_tr16_source, measured by debug_lds_tr_dump) it receives
//   V[32 c + 16 h + 4 g + e][16 dt + i], e = 0..3.
//   V's swizzle, for this pattern and not the GEMM's: one read touches the 16
//   consecutive rows 32 c + 16 h .. + 15 at one pair of chunks (32 bytes), the
//   first 32 lanes rows .. + 7. Rows are 128 bytes, half of the 64 banks, so
//   unswizzled every second row repeats its banks. Bit 0 of the row picks the
//   half of the banks already; bits 2..1 of the row are xored into the pair
//   index (bits 2..1 of the chunk), which keeps a pair together and puts the 8
//   rows of 32 lanes on 8 different pairs of the 64 banks.
// Correctness does not depend on either swizzle.
// ---------------------------------------------------------------------------
constexpr uint32_t kAttnOperandBytes = kAttnBlock * kAttnHeadDim * 2;  // 8 KiB
constexpr uint32_t kAttnRowBytes = kAttnHeadDim * 2;                   // 128

GH_HD inline uint32_t attn_k_swizzle(uint32_t row) { return (row >> 1) & 7u; }
GH_HD inline uint32_t attn_v_swizzle(uint32_t row) { return ((row >> 1) & 3u) << 1; }

// what belongs into 16-byte slot `slot` (0..511) of K's and of V's part of a
// stage: the row of the block and the byte within the row
GH_HD inline NarrowChunk attn_k_source(uint32_t slot) {
  const uint32_t row = slot >> 3;
  return {row, 16u * ((slot & 7u) ^ attn_k_swizzle(row))};
}
GH_HD inline NarrowChunk attn_v_source(uint32_t slot) {
  const uint32_t row = slot >> 3;
  return {row, 16u * ((slot & 7u) ^ attn_v_swizzle(row))};
}
// element offset into K or V (N x 64) of what slot `slot` of key block `block` holds
GH_HD inline uint64_t attn_global_offset(uint32_t block, NarrowChunk c) {
  return ((uint64_t)block * kAttnBlock + c.row) * kAttnHeadDim + c.byte / 2u;
}

// byte offset within K's 8 KiB of the 16 bytes K[row][32 ds + 8 g .. + 7]
GH_HD inline uint32_t attn_k_read(uint32_t row, uint32_t ds, uint32_t g) {
  return row * kAttnRowBytes + 16u * ((4u * ds + g) ^ attn_k_swizzle(row));
}

// the key, within the block, of k-slot t of lane group g in 32-key chunk c
GH_HD inline uint32_t attn_v_key(uint32_t c, uint32_t g, uint32_t t) {
  return 32u * c + 16u * (t / 4u) + 4u * g + t % 4u;
}

// lane map of ds_read_b64_tr_b16: word e (0..3) of lane l's result is word
// (l & 15) % 4 of what lane (l & ~15) + 4 e + (l & 15) / 4 pointed at; the value
// is the source as lane * 4 + word
GH_HD inline uint32_t attn_tr16_source(uint32_t lane, uint32_t e) {
  const uint32_t i = lane & 15u;
  return 4u * ((lane & ~15u) + 4u * e + i / 4u) + i % 4u;
}

// byte offset within V's 8 KiB that lane (i, g) hands to the transposed read
// for half h of the fragment of chunk c and d-tile dt
GH_HD inline uint32_t attn_v_read(uint32_t c, uint32_t h, uint32_t dt, uint32_t g, uint32_t i) {
  const uint32_t row = 32u * c + 16u * h + 4u * g + (i >> 2);
  const uint32_t col = 16u * dt + 4u * (i & 3u);
  return row * kAttnRowBytes + 16u * ((col >> 3) ^ attn_v_swizzle(row)) + 2u * (col & 7u);
}

// ---------------------------------------------------------------------------
// Causal attention check: H heads of sequence length L at head dimension 128
//
// Q, K and V are [H·L, 128] row-major bf16 or f16, head h in rows h·L .. h·L +
// L - 1; O~ [H·L, 128], m and l [H·L] are fp32. With i and j the positions of a
// query and a key within their head,
//   s_ij = Q[hL + i]·K[hL + j],  visible(i, j) = !causal || j <= i,
//   m[i] = max over visible j of s_ij,  l[i] = Σ over visible j of 2^(s_ij - m_i),
//   O~[i][d] = Σ over visible j of 2^(s_ij - m_i) · V[hL + j][d]
// Scale 1, base 2, no final division. The generators are those of the check
// above over 128 columns, hashed from the flat row h·L + i, so heads differ:
// Q dense in [-2, 2] (attn_q_of), V dense in [-8, 8] (gemm_int_of), K two-hot
// with ±1 at two distinct columns of 128 (attn128_key_of), under the same
// GEN_Q, GEN_KEY and GEN_V.
//
// Exactness premise, restated for the mask. A masked key contributes exactly 0
// to l and to O~ and does not take part in m: on the device its score is -inf,
// v_max_f32 ignores it next to a finite value and v_exp_f32 turns it into +0
// (measured by debug_exp2_dump), which bf16 and f16 hold exactly. Every visible
// s is an integer in [-4, 4], so the argument of the check above holds for the
// visible keys alone: a running maximum is the maximum of the visible keys seen
// so far, every p is 0 or a power of two in [2^-8, 1], every partial l and O~
// is a multiple of 2^-8 of magnitude at most L and 8 L <= 2^15 for L <=
// kAttn128MaxL = 4096: at most 23 significant bits, exact in fp32 in any
// order, and a rescale is exact because its result is such a sum again. Key 0
// of a head is visible to every query of it, so the visible set is never empty,
// m is finite and the first key block of a row always raises m_run from -inf
// to a finite value: -inf - -inf does not occur. Shown on the device for the
// hashed data at L = 4096 (tests/test_gpu_attn_causal.py); for other data of
// the same range it is argued from the bound.
// ---------------------------------------------------------------------------
constexpr uint32_t kAttn128HeadDim = 128;
constexpr uint32_t kAttn128Block = 64;    // queries of a query block, and keys of a stage
constexpr uint32_t kAttn128MaxL = 4096;   // 8 L * 2^8 <= 2^23
// heads · L at most; not needed for exactness: bounds what one call allocates,
// 1288 bytes a row of Q, K, V, O~, m and l together, 161 MiB at the cap
constexpr uint32_t kAttn128MaxRows = 1u << 17;
constexpr uint32_t kAttn128OutCols = kAttn128HeadDim + 2;  // O~, then m, then l

GH_HD inline AttnKey attn128_key_of(uint32_t matrix_hash, uint32_t row) {
  const uint32_t h = mix32(matrix_hash ^ row);
  AttnKey k;
  k.d1 = (h >> 8) & 127u;
  k.d2 = (k.d1 + 1u + (h >> 15) % 127u) & 127u;  // d1 + 1 .. d1 + 127 mod 128: never d1
  k.s1 = (h >> 24) & 1u ? -1 : 1;
  k.s2 = (h >> 25) & 1u ? -1 : 1;
  return k;
}
GH_HD inline int attn128_k_of(uint32_t matrix_hash, uint32_t row, uint32_t col) {
  const AttnKey k = attn128_key_of(matrix_hash, row);
  return col == k.d1 ? k.s1 : col == k.d2 ? k.s2 : 0;
}

// Q, K or V of the causal check at flat row h·L + i; which is GEN_Q, GEN_KEY or GEN_V
GH_HD inline int gen_attn128(uint32_t seed, int dtype, uint32_t which, uint32_t row, uint32_t col) {
  const uint32_t h = gemm_matrix_hash(seed, dtype, which);
  return which == GEN_Q ? attn_q_of(h, row, col)
                        : which == GEN_KEY ? attn128_k_of(h, row, col) : gemm_int_of(h, row, col);
}

// O~[row][d], m[row] and l[row] of flat row `row` = h·L + i over the visible
// keys of head h, in integer arithmetic and one pass, as attn_reference
GH_HD inline AttnExpected attn128_reference(uint32_t seed, int dtype, uint32_t L, bool causal,
                                            uint32_t row, uint32_t d) {
  const uint32_t hq = mix32(gemm_matrix_hash(seed, dtype, GEN_Q) ^ row);  // the row hoisted
  const uint32_t hk = gemm_matrix_hash(seed, dtype, GEN_KEY);
  const uint32_t hv = gemm_matrix_hash(seed, dtype, GEN_V);
  const uint32_t first = row - row % L, keys = causal ? row % L + 1u : L;
  int m = -4;
  int64_t o = 0, l = 0;
  for (uint32_t j = first; j < first + keys; ++j) {
    const AttnKey k = attn128_key_of(hk, j);
    const int s = k.s1 * ((int)((mix32(hq + k.d1) >> 8) % 5u) - 2) +
                  k.s2 * ((int)((mix32(hq + k.d2) >> 8) % 5u) - 2);
    m = s > m ? s : m;
    l += (int64_t)1 << (s + 4);
    o += ((int64_t)1 << (s + 4)) * gemm_int_of(hv, j, d);
  }
  AttnExpected e;
  e.o = (float)(int32_t)(o * ((int64_t)1 << (4 - m))) * (1.0f / 256.0f);
  e.m = (float)m;
  e.l = (float)(int32_t)(l * ((int64_t)1 << (4 - m))) * (1.0f / 256.0f);
  return e;
}

// ---------------------------------------------------------------------------
// Causal attention check: where a stage lies in LDS, shared by the kernel
// (gpuhealth_attn128.hip) and by tests/native/attn128_ref_check.cpp.
//
// A stage is a block of 64 keys: 16 KiB of K and 16 KiB of V, 64 rows of 256
// bytes = sixteen 16-byte chunks, 1024 slots per operand. Slot s holds chunk
// (s % 16) ^ swizzle(row) of row s / 16; the global side fetches what belongs
// into its slot. A wave's load of 64 slots is four whole rows, so the global
// side still reads whole 256-byte lines whatever the swizzle.
//
// A 256-byte row is all 64 banks once, so unswizzled every row repeats the
// banks of the row above and the swizzles for 128-byte rows, which count on
// bit 0 of the row to pick a half of the banks, do not carry over.
//
// Reads (lane l, i = l & 15, g = l >> 4):
//   K is the A operand of Sᵀ = K·Qᵀ: lane (i, g) reads K[key][32 ds + 8 g .. + 7]
//   of key 16 kt + i with one ds_read_b128, ds = 0..3: chunk 4 ds + g. The 16
//   lanes of a group g read one chunk index in 16 consecutive rows, 256 bytes
//   in all; xoring the low four bits of the row into the chunk index sends the
//   16 rows to 16 different chunks, which are the 64 banks once.
//   V is the A operand of O~ᵀ += Vᵀ·Pᵀ in P's register order (attn_v_key): half
//   h of the fragment of 32-key chunk c and d-tile dt (0..7) is one
//   ds_read_b64_tr_b16 in which lane (i, g) points at
//   V[32 c + 16 h + 4 g + i / 4][16 dt + 4 (i % 4) .. + 3] and by the lane map
//   (attn_tr16_source) receives V[32 c + 16 h + 4 g + e][16 dt + i]. One read
//   touches the 16 consecutive rows 32 c + 16 h .. + 15 at one pair of chunks
//   (chunks 2 dt and 2 dt + 1, 32 bytes), the first 32 lanes rows .. + 7. A row
//   has 8 such pairs; xoring the low three bits of the row into the pair index
//   (bits 3..1 of the chunk) keeps a pair together and puts the 8 rows of 32
//   lanes on the 8 different pairs, the 64 banks once.
// That the reads are conflict-free is argued here, not measured. Correctness
// does not depend on either swizzle: staging and reads go through the same
// function, and any function into 0..15 gives the same data.
// ---------------------------------------------------------------------------
constexpr uint32_t kAttn128RowBytes = kAttn128HeadDim * 2;                     // 256
constexpr uint32_t kAttn128OperandBytes = kAttn128Block * kAttn128RowBytes;    // 16 KiB
constexpr uint32_t kAttn128Slots = kAttn128OperandBytes / 16;                  // 1024

GH_HD inline uint32_t attn128_k_swizzle(uint32_t row) { return row & 15u; }
GH_HD inline uint32_t attn128_v_swizzle(uint32_t row) { return (row & 7u) << 1; }

// what belongs into 16-byte slot `slot` (0..1023) of K's and of V's part of a
// stage: the row of the key block and the byte within the row
GH_HD inline NarrowChunk attn128_k_source(uint32_t slot) {
  const uint32_t row = slot >> 4;
  return {row, 16u * ((slot & 15u) ^ attn128_k_swizzle(row))};
}
GH_HD inline NarrowChunk attn128_v_source(uint32_t slot) {
  const uint32_t row = slot >> 4;
  return {row, 16u * ((slot & 15u) ^ attn128_v_swizzle(row))};
}
// element offset into K or V ([H·L, 128]) of chunk c of the key block that
// starts at flat row `first_row`
GH_HD inline uint64_t attn128_global_offset(uint32_t first_row, NarrowChunk c) {
  return ((uint64_t)first_row + c.row) * kAttn128HeadDim + c.byte / 2u;
}

// byte offset within K's 16 KiB of the 16 bytes K[row][32 ds + 8 g .. + 7]
GH_HD inline uint32_t attn128_k_read(uint32_t row, uint32_t ds, uint32_t g) {
  return row * kAttn128RowBytes + 16u * ((4u * ds + g) ^ attn128_k_swizzle(row));
}

// byte offset within V's 16 KiB that lane (i, g) hands to the transposed read
// for half h of the fragment of chunk c and d-tile dt (0..7)
GH_HD inline uint32_t attn128_v_read(uint32_t c, uint32_t h, uint32_t dt, uint32_t g, uint32_t i) {
  const uint32_t row = 32u * c + 16u * h + 4u * g + (i >> 2);
  const uint32_t col = 16u * dt + 4u * (i & 3u);
  return row * kAttn128RowBytes + 16u * ((col >> 3) ^ attn128_v_swizzle(row)) + 2u * (col & 7u);
}

// The work split of the causal check: workgroup `pair` (0 .. nb / 2 - 1) of a
// head takes query blocks pair and nb - 1 - pair, nb = L / 64, one after the
// other. Query block qb walks key blocks 0 .. qb under the mask and all nb
// without: nb + 1 or 2 nb key-block steps a workgroup.
GH_HD inline uint32_t attn128_query_block(uint32_t nb, uint32_t pair, uint32_t phase) {
  return phase ? nb - 1u - pair : pair;
}
GH_HD inline uint32_t attn128_key_blocks(uint32_t nb, uint32_t qb, bool causal) {
  return causal ? qb + 1u : nb;
}
// the workgroup, counted over all heads, that computes flat row `row`
GH_HD inline uint32_t attn128_workgroup_of(uint32_t L, uint32_t row) {
  const uint32_t nb = L / kAttn128Block, qb = row % L / kAttn128Block;
  return row / L * (nb / 2u) + (qb < nb - 1u - qb ? qb : nb - 1u - qb);
}

// ---------------------------------------------------------------------------
// Decode attention check: one query token a sequence over a paged KV cache,
// grouped-query heads, the context split over workgroups (split-KV)
//
// For sequence b, KV head hk and query head hq = hk·G + g, flat Q row
// (b·kv_heads + hk)·G + g:
//   keys j = 0 .. ctx[b] - 1 of (b, hk), found through the block table
//   s_j = Q[row]·K[b][hk][j],  m = max_j s_j,  l = Σ_j 2^(s_j - m),
//   O~[d] = Σ_j 2^(s_j - m) · V[b][hk][j][d]
// Scale 1, base 2, head dimension 128, no final division.
//
// Cache: pages of kDecodePageTokens = 16 tokens. The pools are [pages,
// kv_heads, 16, 128] 16-bit for K and for V, so a (page, head) tile is 16
// contiguous rows of 256 bytes, 4 KiB. The block table is [batch, max_pages]
// int32, max_pages = ceil(max_ctx / 16). The pool has decode_pool_pages =
// the power of two at or above batch · max_pages pages, and logical page
// b · max_pages + p lies at decode_page_of: an affine map modulo the pool with
// an odd multiplier from the seed (5 modulo 16), a bijection of the pool that
// never puts neighbouring logical pages next to each other.
//
// Generators: Q dense in [-2, 2] (attn_q_of at the flat Q row), K two-hot ±1
// (attn128_key_of) and V dense in [-8, 8] (gemm_int_of), both at logical row
// (b · kv_heads + hk) · kDecodeMaxCtx + position, under GEN_Q, GEN_KEY, GEN_V:
// the data does not depend on where the table put it, and the check needs no
// table to recompute it.
//
// Exactness premise, restated. Every token slot that no sequence owns (the
// tail of a sequence's last page, and every page beyond it or mapped to no
// sequence) holds kDecodePoison = 0x7700: 28672 as f16 and 2^111 as bf16, a
// large finite number in both, small enough that a 128-term dot product with
// |q| <= 2 stays finite in fp32. A kernel that forgets the mask takes poison
// into m, l or O~ and fails loudly. A correct kernel overwrites the score of
// such a key with -inf before the maximum (a select, no arithmetic on the
// poisoned score), p = exp2(-inf - finite) = +0, and 0 · poison = 0 exactly:
// the poisoned V row adds nothing. Pages wholly past ctx are not read at all.
// Every visible s is an integer in [-4, 4], so what the checks above argue
// holds for any subset of a row's keys under that subset's own maximum: a
// per-wave partial (the keys of one wave of one workgroup) and a split partial
// (the steps of one workgroup) are sums of powers of two in [2^-8, 1] times
// integers in [-8, 8], multiples of 2^-8 of magnitude at most 8·ctx <= 2^15.
// A rescale by 2^(m_part - m) with m the maximum of a superset keeps it a
// multiple of 2^-8 of at most that magnitude, because the whole row's score
// range is at most 8: at most 23 significant bits, exact in fp32 in any order.
// An empty part (a wave or a split that saw no key) has m = -inf, l = 0, O~ =
// 0 and is merged with exp2(-inf - finite) = 0. Hence finals and split
// partials compare with == against integer arithmetic for ctx <=
// kDecodeMaxCtx = 4096. Shown on the device for the hashed data at ctx = 4096
// (tests/test_gpu_attn_decode.py); for other data argued from the bound.
// ---------------------------------------------------------------------------
constexpr uint32_t kDecodePageTokens = 16;
constexpr uint32_t kDecodeMaxCtx = 4096;     // 8 N * 2^8 <= 2^23
constexpr uint32_t kDecodeStepKeys = 128;    // a workgroup's step: 8 pages, 2 a wave
constexpr uint32_t kDecodeStepPages = kDecodeStepKeys / kDecodePageTokens;
constexpr uint32_t kDecodeMaxGroup = 16;     // the N side of one 16x16x32 MFMA
constexpr uint32_t kDecodeMaxSplits = kDecodeMaxCtx / kDecodeStepKeys;  // 32: a step a split
constexpr uint32_t kDecodePoison = 0x7700u;
constexpr uint32_t kDecodePageElems = kDecodePageTokens * kAttn128HeadDim;  // of one head
// K and V pools together at most; not needed for exactness: bounds what one call allocates
constexpr uint64_t kDecodeMaxPoolBytes = 1ull << 30;
// batch · kv_heads at most: the logical K / V row fits 32 bits and a grid dimension holds it
constexpr uint32_t kDecodeMaxKvRows = 1u << 15;

GH_HD inline uint32_t decode_pages(uint32_t ctx) {
  return (ctx + kDecodePageTokens - 1u) / kDecodePageTokens;
}
GH_HD inline uint32_t decode_pool_pages(uint32_t batch, uint32_t max_pages) {
  uint32_t pool = 1;
  while (pool < batch * max_pages) pool <<= 1;
  return pool;
}
// physical page of logical page `logical` = b · max_pages + p; pool_pages a power of two
GH_HD inline uint32_t decode_page_of(uint32_t seed, uint32_t pool_pages, uint32_t logical) {
  // 5 modulo 16: odd, and two neighbours are never fewer than 5 pages apart
  const uint32_t mult = (mix32(seed ^ 0x50A6E5u) & ~15u) | 5u, add = mix32(seed ^ 0x0FF5E7u);
  return (mult * logical + add) & (pool_pages - 1u);
}
// ctx[b] when the caller gives none: sequence 0 the full max_ctx, the rest
// hashed into [1, max_ctx], not rounded to a page
GH_HD inline uint32_t decode_default_ctx(uint32_t seed, uint32_t b, uint32_t max_ctx) {
  return b == 0 ? max_ctx : 1u + mix32(mix32(seed ^ 0xC7C7C7u) + b) % max_ctx;
}
// the logical K / V row of position `pos` of KV row kvrow = b · kv_heads + hk
GH_HD inline uint32_t decode_kv_row(uint32_t kvrow, uint32_t pos) {
  return kvrow * kDecodeMaxCtx + pos;
}
// Q[row][col] at the flat Q row, K or V[kvrow][pos][col] at row = decode_kv_row
GH_HD inline int gen_decode(uint32_t seed, int dtype, uint32_t which, uint32_t row, uint32_t col) {
  return gen_attn128(seed, dtype, which, row, col);
}

// The work split: a sequence has ns = decode_steps(ctx) steps of 128 keys, and
// split s of S takes steps decode_split_first(ns, S, s) .. (ns, S, s + 1) - 1,
// none at all where S > ns.
GH_HD inline uint32_t decode_steps(uint32_t ctx) {
  return (ctx + kDecodeStepKeys - 1u) / kDecodeStepKeys;
}
GH_HD inline uint32_t decode_split_first(uint32_t ns, uint32_t S, uint32_t s) { return s * ns / S; }
// the keys of split s of S of a sequence of ctx keys: [first, end), empty when first == end
GH_HD inline uint32_t decode_split_key(uint32_t ctx, uint32_t S, uint32_t s) {
  const uint32_t key = decode_split_first(decode_steps(ctx), S, s) * kDecodeStepKeys;
  return key < ctx ? key : ctx;
}

// O~[row][d], m[row] and l[row] of flat Q row `row` over keys key_first ..
// key_end - 1 of its KV row, in integer arithmetic and one pass, as
// attn_reference: the whole context for a final, a split's keys for a partial.
// No key at all gives m = -inf, l = 0, O~ = 0.
GH_HD inline AttnExpected decode_reference(uint32_t seed, int dtype, uint32_t group, uint32_t row,
                                           uint32_t d, uint32_t key_first, uint32_t key_end) {
  AttnExpected e;
  if (key_first >= key_end) {
    e.o = 0.f, e.m = -__builtin_inff(), e.l = 0.f;
    return e;
  }
  const uint32_t hq = mix32(gemm_matrix_hash(seed, dtype, GEN_Q) ^ row);  // the row hoisted
  const uint32_t hk = gemm_matrix_hash(seed, dtype, GEN_KEY);
  const uint32_t hv = gemm_matrix_hash(seed, dtype, GEN_V);
  const uint32_t base = decode_kv_row(row / group, 0);
  int m = -4;
  int64_t o = 0, l = 0;
  for (uint32_t j = base + key_first; j < base + key_end; ++j) {
    const AttnKey k = attn128_key_of(hk, j);
    const int s = k.s1 * ((int)((mix32(hq + k.d1) >> 8) % 5u) - 2) +
                  k.s2 * ((int)((mix32(hq + k.d2) >> 8) % 5u) - 2);
    m = s > m ? s : m;
    l += (int64_t)1 << (s + 4);
    o += ((int64_t)1 << (s + 4)) * gemm_int_of(hv, j, d);
  }
  e.o = (float)(int32_t)(o * ((int64_t)1 << (4 - m))) * (1.0f / 256.0f);
  e.m = (float)m;
  e.l = (float)(int32_t)(l * ((int64_t)1 << (4 - m))) * (1.0f / 256.0f);
  return e;
}

// ---------------------------------------------------------------------------
// Decode attention check: LDS addresses, shared by the kernel
// (gpuhealth_attn_decode.hip) and by tests/native/attn_decode_ref_check.cpp.
//
// A workgroup is four waves and 64 KiB of LDS: wave w owns bytes 16384 w ..
// + 16383, two stages of 8 KiB. A stage is the wave's two pages of V of one
// step, 32 rows (row 16 t + token of page t) of 256 bytes, 512 slots of 16
// bytes; slot s holds chunk (s % 16) ^ swizzle(row) of row s / 16, and the
// global side fetches what belongs into its slot. K does not pass through LDS.
//
// The V read is that of the causal check with one 32-key chunk: rows of 256
// bytes, half h of a fragment one ds_read_b64_tr_b16 over the 16 consecutive
// rows 16 h .. + 15 (page h) at one pair of chunks. The derivation of
// attn128_v_swizzle speaks of exactly that and carries over unchanged, so the
// functions below are attn128_v_source and attn128_v_read at chunk 0. Argued,
// not measured, and correctness does not depend on it.
//
// Epilogue: the stages are free, and wave w lays its partial into its own
// 16 KiB: O~ᵀ[d][query i] as fp32 at 4 (16 d + i), 8 KiB, then m[i] and l[i].
// The stores of the four lane groups fall on the same banks four at a time;
// it is one pass a workgroup and left so.
// ---------------------------------------------------------------------------
constexpr uint32_t kDecodeWaves = 4;
constexpr uint32_t kDecodeStageBytes = 2 * kDecodePageTokens * kAttn128RowBytes;  // 8 KiB
constexpr uint32_t kDecodeStageSlots = kDecodeStageBytes / 16;                    // 512
constexpr uint32_t kDecodeWaveBytes = 2 * kDecodeStageBytes;                      // 16 KiB
constexpr uint32_t kDecodeLdsBytes = kDecodeWaves * kDecodeWaveBytes;             // 64 KiB

GH_HD inline uint32_t decode_stage_base(uint32_t wave, uint32_t buf) {
  return wave * kDecodeWaveBytes + buf * kDecodeStageBytes;
}
// what belongs into slot `slot` (0..511) of a stage: row = 16 · page of the wave + token
GH_HD inline NarrowChunk decode_v_source(uint32_t slot) { return attn128_v_source(slot); }
// element offset into a pool of [token][col] of head hk of physical page `page`
GH_HD inline uint64_t decode_pool_offset(uint32_t page, uint32_t kv_heads, uint32_t hk,
                                         uint32_t token, uint32_t col) {
  return (((uint64_t)page * kv_heads + hk) * kDecodePageTokens + token) * kAttn128HeadDim + col;
}
// byte offset within a stage that lane (i, g) hands to the transposed read for
// half h (page h of the wave) of the fragment of d-tile dt
GH_HD inline uint32_t decode_v_read(uint32_t h, uint32_t dt, uint32_t g, uint32_t i) {
  return attn128_v_read(0, h, dt, g, i);
}
// the epilogue's places, byte offsets into the workgroup's LDS
GH_HD inline uint32_t decode_epi_o(uint32_t wave, uint32_t d, uint32_t i) {
  return wave * kDecodeWaveBytes + 4u * (16u * d + i);
}
GH_HD inline uint32_t decode_epi_ml(uint32_t wave, uint32_t which, uint32_t i) {  // 0: m, 1: l
  return wave * kDecodeWaveBytes + kDecodeStageBytes + 64u * which + 4u * i;
}

// ---------------------------------------------------------------------------
// MoE check: a routed grouped GEMM with a top-k combine by fp32 atomics
//
// Tokens X are [T + 1, K] and expert weights W are [E, K, N], 16-bit, each
// expert row-major K x N. Token t goes to top_k distinct experts route[t][j],
// j = 0 .. top_k - 1, with the router weight moe_weight_of(seed, t, j) in
// {1, 1/2, 1/4}. The routing the kernel reads is sorted by expert
// (moe_build_routing): offsets[E + 1], and for entry p = offsets[e] .. of
// expert e, tokens ascending, sorted_token[p] and sorted_weight[p]. It is input
// data that the host builds and uploads, as the decode check's block table is.
//   P[p][n] = Σ_k X[sorted_token[p]][k] · W[e][k][n]      (plain stores)
//   Y[t][n] = Σ_j weight(t, j) · P[entry of (t, j)][n]    (fp32 atomics onto zero)
//
// Generators: X[t][k] = gemm_int_of under GEN_A at (t, k), W[e][k][n] =
// gemm_int_of under GEN_B at (e·K + k, n): integers in [-8, 8]. Row T of X is
// the poison row, kMoePoison = 0x7700 in every element (28672 as f16, 2^111 as
// bf16: finite, and a K <= 4096 dot product with |w| <= 8 stays finite). The
// tail rows of a group's last tile gather it and are masked out of P and Y, so
// a mask that is off shows as a mismatch; row T of Y and the kMoeGuardRows rows
// of P after the last entry are guards that must stay zero, which is where a
// row that escapes the mask lands instead of out of bounds.
//
// Exactness premise. |P| <= 64 K, an integer. Every partial sum of a row of Y
// is a multiple of 1/4 of magnitude at most top_k · 64 K; with top_k <=
// kMoeMaxTopK = 8 and K <= kMoeMaxK = 4096 that is at most 2^21, below 2^23
// quarters: it fits the fp32 significand, the products weight · P are exact
// (a power of two times an integer), and the atomics give the same value in
// every order. Shown on the device for the hashed data at the bound
// (tests/test_gpu_moe.py); for other data argued from the bound.
// ---------------------------------------------------------------------------
constexpr uint32_t kMoeMaxK = 4096;      // 8 · 64 K · 4 <= 2^23
constexpr uint32_t kMoeMaxTopK = 8;
constexpr uint32_t kMoeMaxExperts = 64;  // one lane an expert in the tile lookup
constexpr uint32_t kMoePoison = 0x7700u;
constexpr uint32_t kMoeGuardRows = kGemmTile;
// not needed for exactness: bound what one call allocates
constexpr uint32_t kMoeMaxTokens = 1u << 16;
constexpr uint64_t kMoeMaxBytes = 1ull << 31;  // X, W, P and Y together
// where[] of a workgroup past the last tile; a key never written stays ~0
constexpr uint32_t kMoeIdleKey = 0xFFFFFFFEu;

// X[row][col] at row = token, W[e][k][col] at row = e·K + k; which is GEN_A or GEN_B
GH_HD inline int gen_moe(uint32_t seed, int dtype, uint32_t which, uint32_t row, uint32_t col) {
  return gen_gemm_int(seed, dtype, which, row, col);
}
// log2 of 1 / weight: 0, 1 or 2
GH_HD inline uint32_t moe_weight_shift(uint32_t seed, uint32_t token, uint32_t j) {
  return mix32(mix32(seed ^ 0x30E30Eu) + token * kMoeMaxTopK + j) % 3u;
}
GH_HD inline float moe_weight_of(uint32_t seed, uint32_t token, uint32_t j) {
  return 1.0f / (float)(1u << moe_weight_shift(seed, token, j));
}

// The generated routing. Experts e with e % 4 == 1 get no token where the
// others are enough for top_k (at E = 16: 1, 5, 9 and 13 are empty, first,
// middle and near the end); active expert a is a + (a + 2) / 3. A token's
// first choice is the smaller of two hashed draws, so low experts carry more
// load, and choice j is the j-th active expert after it, cyclically: distinct.
GH_HD inline uint32_t moe_active_experts(uint32_t E, uint32_t top_k) {
  const uint32_t na = E - (E + 2u) / 4u;
  return na >= top_k ? na : E;
}
GH_HD inline uint32_t moe_default_expert(uint32_t seed, uint32_t E, uint32_t top_k, uint32_t token,
                                         uint32_t j) {
  const uint32_t na = moe_active_experts(E, top_k);
  const uint32_t h = mix32(mix32(seed ^ 0x0E7E27u) + token);
  const uint32_t d0 = (h & 0xFFFFu) % na, d1 = (h >> 16) % na;
  const uint32_t a = ((d0 < d1 ? d0 : d1) + j) % na;
  return na == E ? a : a + (a + 2u) / 3u;
}

// Sorts route[T · top_k] (expert of (t, j) at t · top_k + j) by expert, tokens
// ascending within one: offsets[E + 1], sorted_token, sorted_weight and
// entry_of[T · top_k], the entry of (t, j). The caller has checked the ids.
inline void moe_build_routing(uint32_t seed, uint32_t T, uint32_t E, uint32_t top_k,
                              const uint32_t* route, uint32_t* offsets, uint32_t* sorted_token,
                              float* sorted_weight, uint32_t* entry_of) {
  for (uint32_t e = 0; e <= E; ++e) offsets[e] = 0;
  for (uint32_t p = 0; p < T * top_k; ++p) offsets[route[p] + 1] += 1;
  for (uint32_t e = 0; e < E; ++e) offsets[e + 1] += offsets[e];
  for (uint32_t p = 0; p < T * top_k; ++p) {  // offsets[e] is the cursor of group e
    const uint32_t at = offsets[route[p]]++;
    sorted_token[at] = p / top_k;
    sorted_weight[at] = moe_weight_of(seed, p / top_k, p % top_k);
    entry_of[p] = at;
  }
  // every cursor stands at its group's end, the start of the next one
  for (uint32_t e = E; e > 0; --e) offsets[e] = offsets[e - 1];
  offsets[0] = 0;
}

// The tile lookup, as the kernel does it with one lane an expert: row tile rt
// of the grid belongs to the expert whose running count of ceil(size / 64)
// first exceeds rt; empty experts count nothing. false past the last tile.
GH_HD inline uint32_t moe_tiles_of(uint32_t count) { return (count + kGemmTile - 1u) / kGemmTile; }
GH_HD inline bool moe_tile_lookup(const uint32_t* offsets, uint32_t E, uint32_t rt,
                                  uint32_t* expert, uint32_t* first_row) {
  uint32_t before = 0;
  for (uint32_t e = 0; e < E; ++e) {
    const uint32_t mine = moe_tiles_of(offsets[e + 1] - offsets[e]);
    if (rt < before + mine) {
      *expert = e, *first_row = offsets[e] + (rt - before) * kGemmTile;
      return true;
    }
    before += mine;
  }
  return false;
}
// its inverse for an entry of expert e, and the number of non-idle row tiles
GH_HD inline uint32_t moe_tile_of_entry(const uint32_t* offsets, uint32_t e, uint32_t entry) {
  uint32_t before = 0;
  for (uint32_t x = 0; x < e; ++x) before += moe_tiles_of(offsets[x + 1] - offsets[x]);
  return before + (entry - offsets[e]) / kGemmTile;
}
GH_HD inline uint32_t moe_row_tiles(const uint32_t* offsets, uint32_t E) {
  return moe_tile_of_entry(offsets, E, offsets[E]);
}
// what the grid is sized by: it depends on T, top_k and E alone
GH_HD inline uint32_t moe_max_row_tiles(uint32_t T, uint32_t top_k, uint32_t E) {
  return moe_tiles_of(T * top_k) + E;
}

// P of (token, expert) at column col, in integer arithmetic only
GH_HD inline int32_t moe_product_element(uint32_t seed, int dtype, uint32_t K, uint32_t token,
                                         uint32_t expert, uint32_t col) {
  const uint32_t hx = mix32(gemm_matrix_hash(seed, dtype, GEN_A) ^ token);  // the row hoisted
  const uint32_t hw = gemm_matrix_hash(seed, dtype, GEN_B);
  int32_t acc = 0;
  for (uint32_t k = 0; k < K; ++k)
    acc += ((int)((mix32(hx + k) >> 8) % 17u) - 8) * gemm_int_of(hw, expert * K + k, col);
  return acc;
}
// Y[token][col] in quarters; experts is route + token · top_k
GH_HD inline int32_t moe_y_quarters(uint32_t seed, int dtype, uint32_t K, uint32_t top_k,
                                    const uint32_t* experts, uint32_t token, uint32_t col) {
  int32_t quarters = 0;
  for (uint32_t j = 0; j < top_k; ++j)
    quarters += moe_product_element(seed, dtype, K, token, experts[j], col) *
                (int32_t)(4u >> moe_weight_shift(seed, token, j));
  return quarters;
}

}  // namespace gh
