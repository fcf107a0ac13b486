// Stand-alone check of kuberay_amd/_native/gpuhealth_ref.hpp (no HIP, no
// Python): the HBM sweep pattern, the operand encoders and the exact MFMA
// reference. Built by tests/test_gpuhealth_ref.py plain, at -O0 and under
// AddressSanitizer + UBSan, and run as its own process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpuhealth_ref.hpp"

static int failures = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      if (++failures > 20) std::exit(1);                  \
    }                                                     \
  } while (0)

static const uint32_t kSeeds[] = {gh::kDefaultSeed, 0u, 1u, 0xFFFFFFFFu};

static void check_pattern() {
  const uint64_t N = 1ull << 20;
  for (uint32_t seed : kSeeds) {
    // the high half of the index matters
    const uint64_t starts[] = {0, 1, 2, 3, 255, 4096, 123456789, 0xFFFFFFFFull};
    for (uint64_t i : starts) {
      const uint32_t a = gh::pattern_word(seed, i);
      const uint32_t b = gh::pattern_word(seed, i + (1ull << 32));
      const uint32_t c = gh::pattern_word(seed, i + (1ull << 33));
      CHECK(a != b, "seed %u i %llu", seed, (unsigned long long)i);
      CHECK(b != c, "seed %u i %llu", seed, (unsigned long long)i);
    }
    std::vector<uint32_t> w(N);
    for (uint64_t i = 0; i < N; ++i) w[i] = gh::pattern_word(seed, i);
    // not periodic: no period p < N maps the sequence onto itself. A period
    // would have to repeat word 0 at p, so only those p need the full compare.
    for (uint64_t p = 1; p < N; ++p) {
      if (w[p] != w[0]) continue;
      bool periodic = true;
      for (uint64_t i = 0; i + p < N && periodic; ++i) periodic = w[i] == w[i + p];
      CHECK(!periodic, "seed %u period %llu", seed, (unsigned long long)p);
    }
    // every bit position is set in 45%..55% of the words
    for (int bit = 0; bit < 32; ++bit) {
      uint64_t ones = 0;
      for (uint64_t i = 0; i < N; ++i) ones += (w[i] >> bit) & 1u;
      CHECK(ones * 100 >= N * 45 && ones * 100 <= N * 55, "seed %u bit %d ones %llu",
            seed, bit, (unsigned long long)ones);
    }
    // same band in a window above 2^32
    for (int bit = 0; bit < 32; ++bit) {
      uint64_t ones = 0;
      for (uint64_t i = 0; i < N; ++i)
        ones += (gh::pattern_word(seed, (5ull << 32) + i) >> bit) & 1u;
      CHECK(ones * 100 >= N * 45 && ones * 100 <= N * 55, "seed %u high bit %d", seed, bit);
    }
  }
}

static void check_encoders() {
  // e4m3fn byte codes of the integers the generators emit
  const uint8_t e4m3_pos[9] = {0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50};
  for (int v = -8; v <= 8; ++v) {
    const float f = (float)v;
    const uint8_t e = gh::f32_to_e4m3(f);
    const uint8_t want = v < 0 ? (uint8_t)(e4m3_pos[-v] | 0x80) : e4m3_pos[v];
    CHECK(e == want, "e4m3(%d) = 0x%02X, want 0x%02X", v, e, want);
    CHECK(gh::e4m3_to_f32(e) == f, "e4m3 round trip %d", v);
    CHECK(gh::bf16_to_f32(gh::f32_to_bf16(f)) == f, "bf16 round trip %d", v);
    CHECK(gh::f16_to_f32(gh::f32_to_f16(f)) == f, "f16 round trip %d", v);
  }
  CHECK(gh::f32_to_bf16(1.0f) == 0x3F80, "bf16(1)");
  CHECK(gh::f32_to_bf16(-8.0f) == 0xC100, "bf16(-8)");
  CHECK(gh::f32_to_f16(1.0f) == 0x3C00, "f16(1)");
  CHECK(gh::f32_to_f16(-8.0f) == 0xC800, "f16(-8)");
  CHECK(gh::f32_to_f16(7.0f) == 0x4700, "f16(7)");
  // rounding to nearest even where the value is not representable
  CHECK(gh::f32_to_bf16(1.00390625f) == 0x3F80, "bf16 tie to even");
  CHECK(gh::f32_to_bf16(1.01171875f) == 0x3F82, "bf16 tie to even (odd)");
  CHECK(gh::f32_to_e4m3(448.0f) == 0x7E && gh::f32_to_e4m3(1e9f) == 0x7E, "e4m3 saturates");

  // e2m1: all 16 codes
  const float e2m1_val[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  for (uint32_t code = 0; code < 16; ++code) {
    const float v = gh::e2m1_to_f32(code);
    const float want = (code & 8) ? -e2m1_val[code & 7] : e2m1_val[code & 7];
    CHECK(v == want && std::signbit(v) == ((code & 8) != 0), "e2m1 decode %u", code);
    CHECK(gh::f32_to_e2m1(v) == code, "e2m1 round trip %u", code);
    CHECK(gh::e2m1_half_units(code) == (int)(2.0f * want), "e2m1 half units %u", code);
  }
  CHECK(gh::f32_to_e2m1(5.0f) == 0xFF, "e2m1 rejects 5");
  for (uint32_t lo = 0; lo < 16; ++lo)
    for (uint32_t hi = 0; hi < 16; ++hi)
      CHECK(gh::pack_fp4(lo, hi) == (lo | (hi << 4)), "pack %u %u", lo, hi);
  CHECK(gh::e8m0_to_f32(126) == 0.5f && gh::e8m0_to_f32(127) == 1.0f &&
            gh::e8m0_to_f32(128) == 2.0f, "e8m0");
}

static void check_generators_and_reference() {
  for (int dt = 0; dt < gh::kNumDtypes; ++dt) {
    const uint32_t K = (uint32_t)gh::k_of(dt);
    unsigned codes_seen = 0, scales_seen = 0;
    for (uint32_t wg = 0; wg < 64; ++wg) {
      const uint32_t seed = kSeeds[wg & 1];
      std::vector<double> A(16 * K), B(K * 16);
      for (uint32_t i = 0; i < 16; ++i) {
        for (uint32_t k = 0; k < K; ++k) {
          const float a = gh::logical_a(dt, seed, wg, i, k);
          const float b = gh::logical_b(dt, seed, wg, k, i);
          A[i * K + k] = a;
          B[k * 16 + i] = b;
          if (dt == gh::MXFP4) {
            const uint32_t ca = gh::gen_fp4(seed, wg, gh::GEN_A, i, k);
            const uint32_t s = gh::gen_scale(seed, wg, gh::GEN_SA, i, k >> 5);
            CHECK(ca < 16 && s >= 126 && s <= 128, "mxfp4 generator range");
            codes_seen |= 1u << ca;
            scales_seen |= 1u << (s - 126);
          } else {
            CHECK(a >= -8 && a <= 8 && a == std::floor(a), "A range %g", a);
            CHECK(b >= -8 && b <= 8 && b == std::floor(b), "B range %g", b);
          }
        }
      }
      // no constant row of A / column of B (as encoded: codes or integers)
      for (uint32_t i = 0; i < 16; ++i) {
        bool a_const = true, b_const = true;
        for (uint32_t k = 1; k < K; ++k) {
          a_const = a_const && A[i * K + k] == A[i * K];
          b_const = b_const && B[k * 16 + i] == B[i];
        }
        CHECK(!a_const && !b_const, "constant row/col dt %d wg %u i %u", dt, wg, i);
      }
      float D[16][16];
      gh::reference_tile(dt, seed, wg, D);
      double P[16][16];
      for (uint32_t r = 0; r < 16; ++r) {
        for (uint32_t c = 0; c < 16; ++c) {
          const int cin = gh::gen_c(seed, wg, dt, r, c);
          CHECK(cin >= -8 && cin <= 8, "C range");
          double acc = 0.0;
          for (uint32_t k = 0; k < K; ++k) acc += A[r * K + k] * B[k * 16 + c];
          P[r][c] = acc;
          acc += cin;
          CHECK((double)D[r][c] == acc, "reference dt %d wg %u [%u][%u] %g vs %g", dt,
                wg, r, c, (double)D[r][c], acc);
          // exactness premise: a multiple of 1/16 that needs at most 24 bits
          const double x16 = acc * 16.0;
          CHECK(x16 == std::floor(x16) && std::fabs(x16) < 16777216.0, "24 bits: %g", acc);
          CHECK((double)(float)acc == acc, "fp32 exact: %g", acc);
          CHECK(gh::reference_element_x16(dt, seed, wg, r, c) == (int64_t)x16, "x16");
        }
      }
      bool d_sym = true, p_sym = true;
      for (uint32_t r = 0; r < 16; ++r)
        for (uint32_t c = 0; c < 16; ++c) {
          d_sym = d_sym && D[r][c] == D[c][r];
          p_sym = p_sym && P[r][c] == P[c][r];
        }
      CHECK(!d_sym && !p_sym, "symmetric tile dt %d wg %u", dt, wg);
    }
    if (dt == gh::MXFP4) {
      CHECK(codes_seen == 0xFFFFu, "e2m1 codes seen 0x%X", codes_seen);
      CHECK(scales_seen == 7u, "scales seen 0x%X", scales_seen);
    }
  }
  // worst case of the premise, independent of the hash: |a*b| <= 144 per
  // element pair in quarter units, x16 for two x2 scales, K = 128, plus C
  const long long worst = 144LL * 16 * 128 + 16 * 8;
  CHECK(worst < (1LL << 24), "worst case %lld", worst);
  CHECK(worst / 16 < (1LL << 15), "worst case magnitude %lld", worst / 16);
}

int main() {
  check_pattern();
  check_encoders();
  check_generators_and_reference();
  if (failures) {
    std::printf("gpuhealth_ref_check FAILED (%d)\n", failures);
    return 1;
  }
  std::printf("gpuhealth_ref_check OK\n");
  return 0;
}
