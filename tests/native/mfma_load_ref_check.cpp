// Stand-alone check of the MFMA load section of
// kuberay_amd/_native/gpuhealth_ref.hpp (no HIP, no Python): negate_mask
// negates every element of every code, the alternating-sign chain accumulated
// in fp32 equals expected_after bit for bit in any k order, flop_per_mfma, and
// the tile index. Built by tests/test_mfma_load_ref.py plain, at -O0 and under
// AddressSanitizer + UBSan, and run as its own process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
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

static const int kDtypes[] = {gh::BF16, gh::F16, gh::FP8, gh::MXFP4};
static const uint32_t kSeeds[] = {gh::kDefaultSeed, 0u, 0xFFFFFFFFu};
constexpr uint32_t kSign = 0x80000000u;

// the value element `pos` of a packed operand dword decodes to
static float decode_element(int dtype, uint32_t dword, uint32_t pos) {
  switch (dtype) {
    case gh::BF16: return gh::bf16_to_f32((uint16_t)(dword >> (16 * pos)));
    case gh::F16: return gh::f16_to_f32((uint16_t)(dword >> (16 * pos)));
    case gh::FP8: return gh::e4m3_to_f32((uint8_t)(dword >> (8 * pos)));
    default: return gh::e2m1_to_f32((dword >> (4 * pos)) & 15u);
  }
}

static uint32_t elements_per_dword(int dtype) {
  return dtype == gh::MXFP4 ? 8u : (dtype == gh::FP8 ? 4u : 2u);
}

// Every code at every position of the dword, the other positions holding
// another code: the masked dword decodes to the negation, bit for bit (so -0
// for 0, and a NaN stays a NaN with the other sign), at that position and at
// the others.
static void check_negate_mask() {
  CHECK(gh::negate_mask(gh::BF16) == 0x80008000u, "bf16");
  CHECK(gh::negate_mask(gh::F16) == 0x80008000u, "f16");
  CHECK(gh::negate_mask(gh::FP8) == 0x80808080u, "fp8");
  CHECK(gh::negate_mask(gh::MXFP4) == 0x88888888u, "mxfp4");
  for (int dtype : kDtypes) {
    const uint32_t per = elements_per_dword(dtype), bits = 32u / per;
    const uint32_t codes = 1u << bits, mask = gh::negate_mask(dtype);
    for (uint32_t pos = 0; pos < per; ++pos) {
      for (uint32_t code = 0; code < codes; ++code) {
        uint32_t dword = 0;
        for (uint32_t q = 0; q < per; ++q)
          dword |= ((q == pos ? code : (code * 2654435761u >> 7)) & (codes - 1u)) << (bits * q);
        for (uint32_t q = 0; q < per; ++q) {
          const uint32_t plain = gh::f32_bits(decode_element(dtype, dword, q));
          const uint32_t negated = gh::f32_bits(decode_element(dtype, dword ^ mask, q));
          CHECK(negated == (plain ^ kSign), "dtype %d pos %u code %#x element %u: %#x vs %#x",
                dtype, pos, code, q, negated, plain);
        }
      }
    }
  }
  // the cases the issue names, spelled out
  CHECK(gh::f32_bits(gh::e4m3_to_f32(0x7F ^ 0x80)) == 0xFFC00000u, "e4m3 NaN");
  CHECK(gh::f32_bits(gh::e4m3_to_f32(0xFF ^ 0x80)) == 0x7FC00000u, "e4m3 -NaN");
  CHECK(gh::f32_bits(gh::e2m1_to_f32(0u ^ 8u)) == kSign, "e2m1 0 -> -0");
  CHECK(gh::f32_bits(gh::e2m1_to_f32(8u ^ 8u)) == 0u, "e2m1 -0 -> 0");
  CHECK(gh::e2m1_to_f32(1u ^ 8u) == -0.5f && gh::e2m1_to_f32(3u ^ 8u) == -1.5f, "half-steps");
  CHECK(gh::f32_bits(gh::bf16_to_f32(0x0000 ^ 0x8000)) == kSign, "bf16 0 -> -0");
  CHECK(gh::f32_bits(gh::f16_to_f32(0x8000 ^ 0x8000)) == 0u, "f16 -0 -> 0");
}

// A[row][k] as the MFMA reads it: the encoded element, its sign bit flipped by
// the mask when negated, decoded, times the scale (which the mask leaves alone)
static float a_as_issued(int dtype, uint32_t seed, uint32_t wg, uint32_t row, uint32_t k,
                         bool negated) {
  const uint32_t per = elements_per_dword(dtype), pos = k % per;
  const uint32_t flip = negated ? gh::negate_mask(dtype) : 0u;
  uint32_t dword;
  float scale = 1.0f;
  if (dtype == gh::MXFP4) {
    dword = gh::gen_fp4(seed, wg, gh::GEN_A, row, k) << (4 * pos);
    scale = gh::e8m0_to_f32(gh::gen_scale(seed, wg, gh::GEN_SA, row, k >> 5));
  } else {
    const float v = (float)gh::gen_int(seed, wg, dtype, gh::GEN_A, row, k);
    const uint32_t code = dtype == gh::BF16  ? gh::f32_to_bf16(v)
                          : dtype == gh::F16 ? gh::f32_to_f16(v)
                                             : gh::f32_to_e4m3(v);
    dword = code << ((32u / per) * pos);
  }
  return decode_element(dtype, dword ^ flip, pos) * scale;
}

enum Order { FORWARD, REVERSE, SHUFFLED };

static std::vector<uint32_t> k_order(uint32_t K, Order order, uint32_t salt) {
  std::vector<uint32_t> ks(K);
  for (uint32_t k = 0; k < K; ++k) ks[k] = order == REVERSE ? K - 1 - k : k;
  if (order == SHUFFLED)
    for (uint32_t k = K - 1; k > 0; --k) std::swap(ks[k], ks[gh::mix32(salt + k) % (k + 1)]);
  return ks;
}

static void check_chain() {
  const uint32_t counts[] = {1, 2, 3, 31, 32};
  const uint32_t visits[] = {0, 1, 4097};
  for (int dtype : kDtypes) {
    const uint32_t K = (uint32_t)gh::k_of(dtype);
    // bound of the premise, in units of 1/16
    const double bound = dtype == gh::MXFP4 ? 16.0 * 65536.0 : 16.0 * 8192.0;
    for (uint32_t seed : kSeeds) {
      for (uint32_t visit : visits) {
        const uint32_t wg = gh::load_tile_index(visit, visit % gh::kLoadWaves,
                                                (visit + 1) % gh::kLoadTiles);
        for (int order = FORWARD; order <= SHUFFLED; ++order) {
          for (uint32_t row = 0; row < 16; ++row) {
            for (uint32_t col = 0; col < 16; ++col) {
              volatile float acc = (float)gh::gen_c(seed, wg, dtype, row, col);
              CHECK(gh::f32_bits(acc) ==
                        gh::f32_bits(gh::expected_after(dtype, seed, wg, row, col, 0)),
                    "dtype %d n 0", dtype);
              uint32_t next = 0;
              for (uint32_t n = 1; n <= 32; ++n) {
                const bool negated = (n - 1) % 2 == 1;
                for (uint32_t k : k_order(K, (Order)order, seed ^ (n * 977u + row * 16u + col))) {
                  const float a = a_as_issued(dtype, seed, wg, row, k, negated);
                  const float b = gh::logical_b(dtype, seed, wg, k, col);
                  volatile float product = a * b;  // no contraction into an fma
                  acc = acc + product;
                  CHECK(std::fabs((double)acc) * 16.0 < bound, "dtype %d partial %g", dtype,
                        (double)acc);
                  CHECK((double)acc * 16.0 == std::floor((double)acc * 16.0), "unit %g",
                        (double)acc);
                }
                if (n != counts[next]) continue;
                ++next;
                const float want = gh::expected_after(dtype, seed, wg, row, col, n);
                CHECK(gh::f32_bits(acc) == gh::f32_bits(want),
                      "dtype %d seed %u wg %u order %d [%u][%u] n %u: %g vs %g", dtype, seed, wg,
                      order, row, col, n, (double)acc, (double)want);
              }
              CHECK(next == 5, "every count was checked");
            }
          }
        }
        // an odd count is the reference, an even one C, and the two differ somewhere
        bool differ = false;
        for (uint32_t row = 0; row < 16; ++row)
          for (uint32_t col = 0; col < 16; ++col) {
            CHECK(gh::expected_after(dtype, seed, wg, row, col, 4095) ==
                      gh::reference_element(dtype, seed, wg, row, col), "odd");
            CHECK(gh::expected_after(dtype, seed, wg, row, col, 1ull << 40) ==
                      (float)gh::gen_c(seed, wg, dtype, row, col), "even");
            differ = differ || gh::expected_after(dtype, seed, wg, row, col, 1) !=
                                   gh::expected_after(dtype, seed, wg, row, col, 2);
          }
        CHECK(differ, "dtype %d wg %u: A·B is zero everywhere", dtype, wg);
      }
    }
  }
}

static void check_flop_and_index() {
  CHECK(gh::flop_per_mfma(gh::BF16) == 16384u, "bf16");
  CHECK(gh::flop_per_mfma(gh::F16) == 16384u, "f16");
  CHECK(gh::flop_per_mfma(gh::FP8) == 16384u, "fp8");
  CHECK(gh::flop_per_mfma(gh::MXFP4) == 65536u, "mxfp4");
  for (int dtype : kDtypes)
    CHECK(gh::flop_per_mfma(dtype) == 2ull * 16 * 16 * (uint64_t)gh::k_of(dtype), "2 M N K");
  std::set<uint32_t> seen;
  for (uint32_t visit = 0; visit < 64; ++visit)
    for (uint32_t wave = 0; wave < gh::kLoadWaves; ++wave)
      for (uint32_t tile = 0; tile < gh::kLoadTiles; ++tile)
        seen.insert(gh::load_tile_index(visit, wave, tile));
  CHECK(seen.size() == 64u * gh::kLoadWaves * gh::kLoadTiles, "tile indices collide");
  CHECK(*seen.rbegin() == 64u * gh::kLoadWaves * gh::kLoadTiles - 1u, "tile indices are dense");
}

int main() {
  check_negate_mask();
  check_chain();
  check_flop_and_index();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("mfma_load_ref_check OK\n");
  return 0;
}
