// The GEMM check's core in gpuhealth_ref.hpp: range, spread and asymmetry of
// gen_gemm_int, gemm_encode, and gemm_reference_element against the plain sum.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "gpuhealth_ref.hpp"

#define CHECK(cond) \
  if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }

int main() {
  for (uint32_t seed : {gh::kDefaultSeed, 0x0BADC0DEu})
    for (int dt : {(int)gh::BF16, (int)gh::F16}) {
      for (uint32_t which : {(uint32_t)gh::GEN_A, (uint32_t)gh::GEN_B, (uint32_t)gh::GEN_C}) {
        unsigned seen = 0, asymmetric = 0;
        for (uint32_t r = 0; r < 96; ++r)
          for (uint32_t c = 0; c < 96; ++c) {
            const int v = gh::gen_gemm_int(seed, dt, which, r, c);
            const int far = gh::gen_gemm_int(seed, dt, which, 0xFFFFFF00u + r, 0x80000000u + c);
            CHECK(v >= -8 && v <= 8 && far >= -8 && far <= 8);
            seen |= 1u << (v + 8);
            asymmetric += v != gh::gen_gemm_int(seed, dt, which, c, r);
            const uint16_t bits = gh::gemm_encode(dt, v);
            CHECK((dt == gh::F16 ? gh::f16_to_f32(bits) : gh::bf16_to_f32(bits)) == (float)v &&
                  (bits & (dt == gh::F16 ? 0xFFu : 0x1Fu)) == 0);  // low mantissa bits clear
          }
        CHECK(seen == (1u << 17) - 1u && asymmetric > 96 * 96 / 2);
      }
      for (uint32_t k : {64u, 192u, 1024u})
        for (uint32_t r : {0u, 63u, 130u})
          for (uint32_t c : {0u, 65u, 191u}) {
            int64_t sum = gh::gen_gemm_int(seed, dt, gh::GEN_C, r, c);
            for (uint32_t kk = 0; kk < k; ++kk)
              sum += (int64_t)gh::gen_gemm_int(seed, dt, gh::GEN_A, r, kk) *
                     gh::gen_gemm_int(seed, dt, gh::GEN_B, kk, c);
            CHECK(sum == gh::gemm_reference_element(seed, dt, k, r, c));
          }
      // the table tests/test_gemm_ref.py holds tests/gemm_model.py against:
      // generator values at near and far indices, reference elements
      for (uint32_t which : {(uint32_t)gh::GEN_A, (uint32_t)gh::GEN_B, (uint32_t)gh::GEN_C})
        for (uint32_t r : {0u, 1u, 63u, 64u, 1471u, 32767u, 65535u, 0xFFFFFF03u})
          for (uint32_t c : {0u, 1u, 65u, 1023u, 65472u, 65535u, 0x80000007u})
            std::printf("gen %u %d %u %u %u %d\n", seed, dt, which, r, c,
                        gh::gen_gemm_int(seed, dt, which, r, c));
      for (uint32_t k : {64u, 192u, 1024u})
        for (uint32_t r : {0u, 127u, 32767u})
          for (uint32_t c : {0u, 191u, 65535u})
            std::printf("ref %u %d %u %u %u %d\n", seed, dt, k, r, c,
                        gh::gemm_reference_element(seed, dt, k, r, c));
    }
  static_assert(64ull * gh::kGemmMaxK + 8 < (1ull << 24), "every sum is exact in fp32");
  std::printf("gemm_ref_check OK\n");
}
