// The decode attention check's core in gpuhealth_ref.hpp: generators and poison, the page
// map, the split ranges, the integer reference over key ranges against a double-precision
// merge of split partials, and the wave-private staging and read addresses with the tr16 map.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpuhealth_ref.hpp"

#define CHECK(cond) \
  if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }

static const uint32_t kSeed = gh::kDefaultSeed, kD = gh::kAttn128HeadDim;

static int gen(int dt, uint32_t which, uint32_t row, uint32_t d) { return gh::gen_decode(kSeed, dt, which, row, d); }

// the map is a bijection of the pool, neighbours lie apart, the poison is finite and large in both formats
static void check_pages_and_poison() {
  for (uint32_t seed : {kSeed, 1u, 0xFFFFFFFFu})
    for (uint32_t batch : {1u, 3u, 16u}) {
      const uint32_t max_pages = gh::decode_pages(batch == 3 ? 600 : gh::kDecodeMaxCtx);
      const uint32_t pool = gh::decode_pool_pages(batch, max_pages);
      CHECK((pool & (pool - 1)) == 0 && pool >= batch * max_pages && pool < 2 * batch * max_pages);
      std::vector<int> hit(pool, 0);
      for (uint32_t p = 0; p < pool; ++p) hit.at(gh::decode_page_of(seed, pool, p)) += 1;
      for (int n : hit) CHECK(n == 1);
      if (pool >= 64)
        for (uint32_t p = 0; p + 1 < pool; ++p) {
          const uint32_t a = gh::decode_page_of(seed, pool, p), b = gh::decode_page_of(seed, pool, p + 1);
          CHECK(((b - a) & 15u) == 5u);  // never the streamed order
        }
    }
  const float f16 = gh::f16_to_f32((uint16_t)gh::kDecodePoison), bf16 = gh::bf16_to_f32((uint16_t)gh::kDecodePoison);
  CHECK(std::isfinite(f16) && f16 > 1e4f && std::isfinite(bf16) && bf16 > 1e30f);
  CHECK(std::isfinite(2.f * kD * bf16) && 0.f * bf16 == 0.f && 0.f * f16 == 0.f);  // a score stays finite
  bool off_page = gh::decode_default_ctx(kSeed, 0, 2048) != 2048;  // sequence 0 is full
  CHECK(!off_page);
  for (uint32_t b = 1; b < 64; ++b) {
    const uint32_t c = gh::decode_default_ctx(kSeed, b, 2048);
    CHECK(c >= 1 && c <= 2048);
    off_page |= c % gh::kDecodePageTokens != 0;
  }
  CHECK(off_page && gh::decode_kv_row(gh::kDecodeMaxKvRows - 1, gh::kDecodeMaxCtx - 1) == (1u << 27) - 1);
}

// the split ranges tile [0, ns); the keys of the splits tile [0, ctx)
static void check_splits() {
  for (uint32_t ctx : {1u, 16u, 17u, 128u, 129u, 300u, 600u, 4095u, 4096u})
    for (uint32_t S = 1; S <= gh::kDecodeMaxSplits; ++S) {
      const uint32_t ns = gh::decode_steps(ctx);
      CHECK(gh::decode_split_first(ns, S, 0) == 0 && gh::decode_split_first(ns, S, S) == ns);
      CHECK(gh::decode_split_key(ctx, S, 0) == 0 && gh::decode_split_key(ctx, S, S) == ctx);
      for (uint32_t s = 0; s < S; ++s) {
        CHECK(gh::decode_split_key(ctx, S, s) <= gh::decode_split_key(ctx, S, s + 1));
        CHECK(gh::decode_split_first(ns, S, s) + (S <= ns) <= gh::decode_split_first(ns, S, s + 1));
      }
    }
}

// partials over the split ranges merge, in double, to the reference over the whole context,
// which is a double-precision softmax over the generated operands; empty splits take part
static void check_reference(int dt, uint32_t kvrow, uint32_t group, uint32_t ctx, uint32_t S) {
  std::vector<double> s(ctx);
  for (uint32_t g = 0; g < group; g += (group > 4 ? 5 : 1)) {
    const uint32_t row = kvrow * group + g;
    double m = -INFINITY, lo = 1e9;
    for (uint32_t j = 0; j < ctx; ++j) {
      s[j] = 0;
      for (uint32_t d = 0; d < kD; ++d) s[j] += (double)gen(dt, gh::GEN_Q, row, d) * gen(dt, gh::GEN_KEY, gh::decode_kv_row(kvrow, j), d);
      m = std::fmax(m, s[j]), lo = std::fmin(lo, s[j]);
    }
    CHECK(m - lo <= 8 && lo >= -4 && m <= 4);  // the spread of the premise
    for (uint32_t d = 0; d < kD; d += (ctx > 300 ? 41 : 1)) {
      double l = 0, o = 0, mm = -INFINITY, ml = 0, mo = 0;
      for (uint32_t j = 0; j < ctx; ++j) {
        const double p = std::exp2(s[j] - m);
        l += p, o += p * gen(dt, gh::GEN_V, gh::decode_kv_row(kvrow, j), d);
      }
      const gh::AttnExpected e = gh::decode_reference(kSeed, dt, group, row, d, 0, ctx);
      CHECK((double)e.o == o && (double)e.m == m && (double)e.l == l && std::fabs(o) <= 8.0 * ctx);
      bool empty = false;
      std::vector<gh::AttnExpected> parts;
      for (uint32_t sp = 0; sp < S; ++sp) {  // the merge kernel's arithmetic
        parts.push_back(gh::decode_reference(kSeed, dt, group, row, d, gh::decode_split_key(ctx, S, sp),
                                             gh::decode_split_key(ctx, S, sp + 1)));
        if (parts[sp].m == -INFINITY) CHECK(parts[sp].l == 0 && parts[sp].o == 0 && (empty = true));
        mm = std::fmax(mm, (double)parts[sp].m);
      }
      for (const gh::AttnExpected& part : parts) {
        const double scale = std::exp2((double)part.m - mm);
        CHECK(std::fabs(part.o * scale) <= 8.0 * ctx && part.o * scale * 256 == std::rint(part.o * scale * 256));
        ml += part.l * scale, mo += part.o * scale;
      }
      CHECK(mm == m && ml == l && mo == o && empty == (S > gh::decode_steps(ctx)));
    }
  }
}

// a wave's stage whose words hold row * 128 + column, placed by the staging function as the
// kernel issues it (page t = slots 256 t .., four loads of 64 lanes) and read back through
// decode_v_read and the tr map; K's direct loads and every pool offset are in bounds
static void check_addresses() {
  const uint32_t kv_heads = 3, pool = 8;
  std::vector<uint16_t> pool_mem((size_t)pool * kv_heads * gh::kDecodePageElems);
  std::vector<uint32_t> lds(gh::kDecodeLdsBytes / 2, ~0u);
  for (uint32_t wave = 0; wave < gh::kDecodeWaves; ++wave)
    for (uint32_t buf = 0; buf < 2; ++buf) {
      const uint32_t base = gh::decode_stage_base(wave, buf);
      CHECK(base % 1024 == 0 && base + gh::kDecodeStageBytes <= gh::kDecodeLdsBytes);
      for (uint32_t t = 0; t < 2; ++t)
        for (uint32_t u = 0; u < 4; ++u)
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const gh::NarrowChunk c = gh::decode_v_source(256 * t + 64 * u + lane);
            CHECK(c.row / gh::kDecodePageTokens == t && c.byte % 16 == 0 && c.byte < 256);
            for (uint32_t w = 0; w < 8; ++w) {
              pool_mem.at(gh::decode_pool_offset(pool - 1, kv_heads, kv_heads - 1, c.row % 16, c.byte / 2) + w) = 0;
              CHECK(lds.at((base + 1024 * (4 * t + u) + 16 * lane) / 2 + w) == ~0u);  // nothing twice
              lds.at((base + 1024 * (4 * t + u) + 16 * lane) / 2 + w) = c.row * kD + c.byte / 2 + w;
            }
          }
    }
  for (uint32_t w : lds) CHECK(w != ~0u);  // the eight stages are the 64 KiB, complete
  for (uint32_t wave = 0; wave < gh::kDecodeWaves; ++wave)
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t i = lane & 15u, g = lane >> 4, base = gh::decode_stage_base(wave, 1);
      for (uint32_t ds = 0; ds < 4; ++ds)  // K, the A operand of the scores: K[token i][32 ds + 8 g .. + 7]
        pool_mem.at(gh::decode_pool_offset(pool - 1, kv_heads, kv_heads - 1, i, 32 * ds + 8 * g) + 7) = 0;
      // V, the A operand of the second product: V[attn_v_key(0, g, 4 h + e)][16 dt + i], page h
      for (uint32_t t = 0; t < 64; ++t) {
        const uint32_t h = t / 32, dt = t / 4 % 8, e = t % 4;
        const uint32_t src = gh::attn_tr16_source(lane, e), from = src / 4;
        const uint32_t at = gh::decode_v_read(h, dt, from >> 4, from & 15u);
        CHECK(at % 8 == 0 && at + 8 <= gh::kDecodeStageBytes && (from >> 4) == g);
        CHECK(gh::attn_v_key(0, g, 4 * h + e) / gh::kDecodePageTokens == h);
        CHECK(lds.at((base + at) / 2 + src % 4) == gh::attn_v_key(0, g, 4 * h + e) * kD + 16 * dt + i);
      }
    }
  // the epilogue: every wave's O~ᵀ, m and l have places of their own inside its 16 KiB
  std::vector<int> used(gh::kDecodeLdsBytes / 4, 0);
  for (uint32_t wave = 0; wave < gh::kDecodeWaves; ++wave)
    for (uint32_t i = 0; i < 16; ++i) {
      for (uint32_t d = 0; d < kD; ++d) used.at(gh::decode_epi_o(wave, d, i) / 4) += 1;
      for (uint32_t which = 0; which < 2; ++which) used.at(gh::decode_epi_ml(wave, which, i) / 4) += 1;
      CHECK(gh::decode_epi_o(wave, 0, i) / gh::kDecodeWaveBytes == wave && gh::decode_epi_ml(wave, 1, i) / gh::kDecodeWaveBytes == wave);
    }
  for (int n : used) CHECK(n <= 1);
}

int main() {
  CHECK(kD == 128 && gh::kDecodeMaxCtx == 4096 && gh::kDecodeStepPages == 8 && gh::kDecodeLdsBytes == 65536);
  check_pages_and_poison();
  check_splits();
  for (int dt : {(int)gh::BF16, (int)gh::F16}) {
    for (uint32_t ctx : {1u, 17u, 129u}) check_reference(dt, 0, 8, ctx, ctx == 129 ? 2 : 1);
    check_reference(dt, 5, 4, 600, 2), check_reference(dt, 1, 8, 300, 4), check_reference(dt, 0, 8, 1, 4);
    check_reference(dt, 2, 16, 4096, 4), check_reference(dt, 7, 1, 257, 2);
  }
  check_addresses();
  std::printf("attn_decode_ref_check OK\n");
  return 0;
}
