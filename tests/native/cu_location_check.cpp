// Stand-alone check of the CU sweep's device-free core in
// kuberay_amd/_native/gpuhealth_ref.hpp (no HIP, no Python): the decode of the
// XCC_ID / HW_ID registers, the dense location key and the LDS march's pattern
// index. Built by tests/test_cu_location_ref.py plain, at -O0 and under
// AddressSanitizer + UBSan, and run as its own process.
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

// The documented layout, written out a second time on purpose: XCC_ID 3:0 of
// its own register; HW_ID SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 14:13.
struct Field {
  const char* name;
  bool in_xcc_reg;
  uint32_t shift, bits;
  uint32_t gh::CuLocation::*member;
};
static const Field kFields[] = {
    {"xcc", true, 0, 4, &gh::CuLocation::xcc},
    {"simd", false, 4, 2, &gh::CuLocation::simd},
    {"cu", false, 8, 4, &gh::CuLocation::cu},
    {"sh", false, 12, 1, &gh::CuLocation::sh},
    {"se", false, 13, 2, &gh::CuLocation::se},
};

static void check_decode() {
  for (const Field& f : kFields) {
    for (uint32_t value = 0; value < (1u << f.bits); ++value) {
      const uint32_t field = value << f.shift;
      const uint32_t mask = ((1u << f.bits) - 1u) << f.shift;
      // only that field set, then every other bit of both registers set too
      for (int others = 0; others < 2; ++others) {
        uint32_t xcc_reg = others ? 0xFFFFFFFFu : 0u, hw_reg = xcc_reg;
        uint32_t& reg = f.in_xcc_reg ? xcc_reg : hw_reg;
        reg = (reg & ~mask) | field;
        const gh::CuLocation loc = gh::decode_location(xcc_reg, hw_reg);
        CHECK(loc.*(f.member) == value, "%s value %u others %d got %u", f.name, value,
              others, loc.*(f.member));
        for (const Field& g : kFields) {
          if (&g == &f) continue;
          const uint32_t expect = others ? (1u << g.bits) - 1u : 0u;
          CHECK(loc.*(g.member) == expect, "%s leaks into %s: value %u others %d got %u",
                f.name, g.name, value, others, loc.*(g.member));
        }
      }
    }
  }
  // bits no field owns (wave slot, pipe, thread group and above) change nothing
  const uint32_t owned = 0x7F30u;
  const gh::CuLocation base = gh::decode_location(5u, 0x2A10u);
  for (int bit = 0; bit < 32; ++bit) {
    if (owned >> bit & 1u) continue;
    const gh::CuLocation loc = gh::decode_location(5u, 0x2A10u ^ (1u << bit));
    CHECK(gh::location_key(loc) == gh::location_key(base) && loc.simd == base.simd,
          "HW_ID bit %d", bit);
  }
  for (int bit = 4; bit < 32; ++bit) {
    const gh::CuLocation loc = gh::decode_location(5u ^ (1u << bit), 0x2A10u);
    CHECK(gh::location_key(loc) == gh::location_key(base), "XCC_ID bit %d", bit);
  }
}

static void check_key() {
  CHECK(gh::kCuSlots == 16u * 4u * 2u * 16u, "kCuSlots %u", gh::kCuSlots);
  CHECK(gh::kNumSimds == 4u, "kNumSimds %u", gh::kNumSimds);
  std::vector<int> seen(gh::kCuSlots, 0);
  for (uint32_t xcc = 0; xcc < 16; ++xcc)
    for (uint32_t se = 0; se < 4; ++se)
      for (uint32_t sh = 0; sh < 2; ++sh)
        for (uint32_t cu = 0; cu < 16; ++cu) {
          uint32_t first_key = 0;
          for (uint32_t simd = 0; simd < 4; ++simd) {
            const gh::CuLocation loc{xcc, se, sh, cu, simd};
            const uint32_t key = gh::location_key(loc);
            CHECK(key < gh::kCuSlots, "key %u", key);
            if (key >= gh::kCuSlots) return;
            if (simd == 0) {
              first_key = key;
              ++seen[key];
            }
            CHECK(key == first_key, "simd %u changes the key", simd);
            // through the registers too
            const gh::CuLocation back = gh::decode_location(
                xcc, simd << 4 | cu << 8 | sh << 12 | se << 13);
            CHECK(gh::location_key(back) == key && back.simd == simd, "round trip");
            const gh::CuLocation inv = gh::location_of_key(key);
            CHECK(inv.xcc == xcc && inv.se == se && inv.sh == sh && inv.cu == cu &&
                      inv.simd == 0, "location_of_key(%u)", key);
          }
        }
  for (uint32_t key = 0; key < gh::kCuSlots; ++key)
    CHECK(seen[key] == 1, "key %u named %d times", key, seen[key]);
}

static void check_lds_pattern() {
  CHECK(gh::lds_pattern_index(0, 0) == 0, "origin");
  CHECK(gh::lds_pattern_index(0, 0xFFFFFFFFu) == 0xFFFFFFFFull, "low half");
  CHECK(gh::lds_pattern_index(1, 0) == 1ull << 32, "high half");
  CHECK(gh::lds_pattern_index(0xFFFFFFFFu, 0xFFFFFFFFu) == ~0ull, "both");
  CHECK(gh::lds_pattern_index(0x12345678u, 0x9ABCDEF0u) == 0x123456789ABCDEF0ull, "mixed");
  // 160 KiB of LDS is 40960 words: no word repeats between two visits
  const uint32_t kWords = 40960;
  const uint32_t pairs[][2] = {{0, 1}, {1, 2}, {0, 1023}, {1023, 1024}, {7, 0x80000007u}};
  const uint32_t seeds[] = {gh::kDefaultSeed, 0u, 0xFFFFFFFFu};
  for (uint32_t seed : seeds)
    for (const auto& p : pairs) {
      uint32_t same = 0;
      for (uint32_t w = 0; w < kWords; ++w)
        same += gh::pattern_word(seed, gh::lds_pattern_index(p[0], w)) ==
                gh::pattern_word(seed, gh::lds_pattern_index(p[1], w));
      CHECK(same == 0, "seed %u visits %u and %u share %u words", seed, p[0], p[1], same);
    }
}

int main() {
  check_decode();
  check_key();
  check_lds_pattern();
  if (failures) {
    std::printf("cu_location_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("cu_location_check OK\n");
  return 0;
}
