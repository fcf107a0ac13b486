// The narrow GEMM check's core in gpuhealth_ref.hpp: generators, encoders, the
// exactness bounds, the integer reference against a double-precision triple
// loop, and the stage placement and LDS read addresses composed with the maps
// of the two transposed reads: every address in bounds before the kernel runs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "gpuhealth_ref.hpp"

#define CHECK(cond) \
  if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }

static const uint32_t kSeed = gh::kDefaultSeed;

static double decoded(int dt, uint32_t which, uint32_t row, uint32_t col) {
  const int v = gh::gen_narrow(kSeed, dt, which, row, col);
  if (dt != gh::MXFP4) return gh::e4m3_to_f32(gh::f32_to_e4m3((float)v));
  const uint32_t scale = which == gh::GEN_A ? gh::gen_narrow(kSeed, dt, gh::GEN_SA, row, col / 32)
                                            : gh::gen_narrow(kSeed, dt, gh::GEN_SB, row / 32, col);
  return (double)gh::e2m1_to_f32((uint32_t)v) * gh::e8m0_to_f32(scale);
}

static void check_generators_and_reference(int dt) {
  const uint32_t K = gh::narrow_stage_k(dt);
  unsigned codes = 0, scales = 0, ints = 0;
  for (uint32_t which : {(uint32_t)gh::GEN_A, (uint32_t)gh::GEN_B})
    for (uint32_t r = 0; r < 64; ++r)
      for (uint32_t c = 0; c < 64; ++c) {
        const int v = gh::gen_narrow(kSeed, dt, which, r, c);
        if (dt == gh::MXFP4) {
          CHECK(v >= 0 && v < 16 && gh::f32_to_e2m1(gh::e2m1_to_f32(v)) == (uint32_t)v);
          codes |= 1u << v;
          const int s = gh::gen_narrow(kSeed, dt, which == gh::GEN_A ? gh::GEN_SA : gh::GEN_SB, r, c);
          CHECK(s >= 126 && s <= 128 && gh::e8m0_to_f32(s) == (s == 126 ? 0.5f : s == 127 ? 1.f : 2.f));
          scales |= 1u << (s - 126);
        } else {
          CHECK(v >= -8 && v <= 8 && gh::e4m3_to_f32(gh::f32_to_e4m3((float)v)) == (float)v);
          ints |= 1u << (v + 8);
        }
        // the byte in memory holds the element where the layout says
        const uint8_t byte = gh::narrow_operand_byte(gh::gemm_matrix_hash(kSeed, dt, which), dt, r,
                                                     c & ~(gh::narrow_per_byte(dt) - 1u));
        CHECK(dt == gh::MXFP4 ? ((byte >> (4 * (c & 1u))) & 15u) == (uint32_t)v
                              : byte == gh::f32_to_e4m3((float)v));
      }
  CHECK(dt == gh::MXFP4 ? codes == 0xFFFFu && scales == 7u : ints == (1u << 17) - 1u);
  for (uint32_t r = 0; r < 64; ++r)
    for (uint32_t c = 0; c < 64; ++c) {
      double sum = gh::gen_narrow(kSeed, dt, gh::GEN_C, r, c);
      for (uint32_t k = 0; k < K; ++k) sum += decoded(dt, gh::GEN_A, r, k) * decoded(dt, gh::GEN_B, k, c);
      CHECK(sum * 16.0 == (double)gh::gemm_narrow_reference_x16(kSeed, dt, K, r, c));
      CHECK((double)gh::gemm_narrow_reference(kSeed, dt, K, r, c) == sum);
    }
}

// One stage whose A and B tiles hold, per byte, the byte's index within the tile:
// placed by the staging functions, read back through the read addresses and the
// tr maps, compared with what the MFMA lane maps want.
static void check_addresses(int dt) {
  const bool mx = dt == gh::MXFP4;
  const uint32_t b_row = gh::narrow_b_row_bytes(dt), b_rows = gh::kNarrowOperandBytes / b_row;
  CHECK(b_rows == gh::narrow_stage_k(dt) && 128u * gh::narrow_per_byte(dt) == gh::narrow_stage_k(dt));
  std::vector<uint32_t> a_lds(gh::kNarrowOperandBytes, ~0u), b_lds(gh::kNarrowOperandBytes, ~0u);
  std::vector<int> a_seen(gh::kNarrowSlots, 0), b_seen(gh::kNarrowSlots, 0);
  for (uint32_t slot = 0; slot < gh::kNarrowSlots; ++slot) {  // slot 64 q + lane lands at 16 slot
    const gh::NarrowChunk ca = gh::narrow_a_source(slot), cb = gh::narrow_b_source(dt, slot);
    CHECK(ca.row < 64 && ca.byte % 16 == 0 && ca.byte + 16 <= 128);
    CHECK(cb.row < b_rows && cb.byte % 16 == 0 && cb.byte + 16 <= b_row);
    ++a_seen[(ca.row * 128 + ca.byte) / 16];
    ++b_seen[(cb.row * b_row + cb.byte) / 16];
    for (uint32_t j = 0; j < 16; ++j) {
      a_lds[16 * slot + j] = ca.row * 128 + ca.byte + j;
      b_lds[16 * slot + j] = cb.row * b_row + cb.byte + j;
    }
  }
  for (uint32_t chunk = 0; chunk < gh::kNarrowSlots; ++chunk)  // every chunk exactly once
    CHECK(a_seen[chunk] == 1 && b_seen[chunk] == 1);

  const uint32_t steps = mx ? 2 : 4, a_bytes = mx ? 16 : 8;
  for (uint32_t t = 0; t < steps; ++t)
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t i = lane & 15u, g = lane >> 4;
      for (uint32_t row = i; row < 64; row += 16) {  // the A fragment: k along the bytes
        const uint32_t at = gh::narrow_a_read(dt, row, t, g);
        CHECK(at % a_bytes == 0 && at + a_bytes <= gh::kNarrowOperandBytes);
        for (uint32_t j = 0; j < a_bytes; ++j)
          CHECK(a_lds[at + j] == row * 128 + (mx ? 64 * t + 16 * g : 32 * t + 8 * g) + j);
      }
      for (uint32_t col = 0; col < 64; col += 16)
        for (uint32_t h = 0; h < (mx ? 2u : 1u); ++h) {
          const uint32_t mine = gh::narrow_b_read(dt, col, t, g, h, i);
          CHECK(mine % 8 == 0 && mine + 8 <= gh::kNarrowOperandBytes);
          for (uint32_t e = 0; e < (mx ? 16u : 8u); ++e) {
            // the element of the result comes from element `from` of what lane `src` handed in
            const uint32_t source = mx ? gh::narrow_tr4_source(lane, e) : gh::narrow_tr8_source(lane, e);
            const uint32_t src = source / (mx ? 16 : 8), from = source % (mx ? 16 : 8);
            CHECK(src / 16 == lane / 16);
            const uint32_t at = gh::narrow_b_read(dt, col, t, g, h, src & 15u);
            if (mx) {  // nibble `from` of the 8 bytes: B[k][col + i], two columns to a byte
              const uint32_t k = 128 * t + 32 * g + 16 * h + e;
              CHECK(b_lds[at + from / 2] == k * b_row + (col + i) / 2 && from % 2 == (col + i) % 2);
            } else {
              CHECK(b_lds[at + from] == (32 * t + 8 * g + e) * b_row + col + i);
            }
          }
        }
    }
}

int main() {
  static_assert(64ull * gh::kNarrowMaxKFp8 + 8 < (1ull << 24), "fp8: every sum is exact in fp32");
  static_assert((uint64_t)gh::kNarrowMaxProductX16 * gh::kNarrowMaxKMxfp4 + 128 < (1ull << 24),
                "mxfp4: every sum is exact in fp32");
  int widest = 0;  // the largest |half units| an e2m1 code decodes to
  for (uint32_t code = 0; code < 16; ++code) widest = std::max(widest, std::abs(gh::e2m1_half_units(code)));
  CHECK(widest * widest * 16 == (int)gh::kNarrowMaxProductX16);
  for (int dt : {(int)gh::FP8, (int)gh::MXFP4}) {
    check_generators_and_reference(dt);
    check_addresses(dt);
  }
  std::printf("gemm_narrow_ref_check OK\n");
}
