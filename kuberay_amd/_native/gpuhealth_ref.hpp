// gpuhealth_ref — Python-free, device-free core of the GPU burn-in probe.
//
// Everything that has to agree bit-for-bit between the host and the gfx950
// kernels in gpuhealth.hip lives here as plain functions that compile for both
// sides (GH_HD): the HBM sweep pattern, the operand generators of the exact
// MFMA check, the encoders to bf16 / f16 / OCP e4m3 / e2m1 bit patterns, and
// the exact reference product. No HIP, no pybind11 — tests/native/
// gpuhealth_ref_check.cpp drives it as a stand-alone g++ program.
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

}  // namespace gh
