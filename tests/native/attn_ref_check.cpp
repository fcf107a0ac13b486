// The attention check's core in gpuhealth_ref.hpp: generators, the premise, the
// integer reference against an online softmax in double precision, and staging
// and LDS read addresses composed with the map of ds_read_b64_tr_b16: every
// address in bounds and every register position the element the MFMA wants.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpuhealth_ref.hpp"

#define CHECK(cond) \
  if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }

static const uint32_t kSeed = gh::kDefaultSeed;

static void check_generators(int dt) {
  const uint32_t hk = gh::gemm_matrix_hash(kSeed, dt, gh::GEN_KEY);
  unsigned q_seen = 0, v_seen = 0;
  for (uint32_t j = 0; j < gh::kAttnMaxN; ++j) {
    const gh::AttnKey key = gh::attn_key_of(hk, j);
    CHECK(key.d1 < 64 && key.d2 < 64 && key.d1 != key.d2 && key.s1 * key.s1 == 1 && key.s2 * key.s2 == 1);
    int nonzero = 0;
    for (uint32_t d = 0; d < 64; ++d) {
      const int k = gh::gen_attn(kSeed, dt, gh::GEN_KEY, j, d);
      CHECK(k == (d == key.d1 ? key.s1 : d == key.d2 ? key.s2 : 0));
      nonzero += k != 0;
      const int q = gh::gen_attn(kSeed, dt, gh::GEN_Q, j, d), v = gh::gen_attn(kSeed, dt, gh::GEN_V, j, d);
      CHECK(q >= -2 && q <= 2 && v >= -8 && v <= 8);
      q_seen |= 1u << (q + 2), v_seen |= 1u << (v + 8);
    }
    CHECK(nonzero == 2);
  }
  CHECK(q_seen == 31u && v_seen == (1u << 17) - 1u);
}

static void check_reference(int dt, uint32_t M, uint32_t N) {
  std::vector<double> s(N);
  for (uint32_t row = 0; row < M; ++row) {
    double lo = 1e9, hi = -1e9;
    for (uint32_t j = 0; j < N; ++j) {
      s[j] = 0;
      for (uint32_t d = 0; d < 64; ++d)
        s[j] += (double)gh::gen_attn(kSeed, dt, gh::GEN_Q, row, d) * gh::gen_attn(kSeed, dt, gh::GEN_KEY, j, d);
      lo = std::fmin(lo, s[j]), hi = std::fmax(hi, s[j]);
    }
    CHECK(hi - lo <= 8 && lo >= -4 && hi <= 4);  // the spread of the premise
    for (uint32_t d = 0; d < 64; d += (M > 64 ? 21 : 1)) {  // every column at the small shapes
      double m = -INFINITY, l = 0, o = 0;
      for (uint32_t b = 0; b < N; b += 64) {
        double bm = m;
        for (uint32_t j = b; j < b + 64; ++j) bm = std::fmax(bm, s[j]);
        const double alpha = std::exp2(m - bm);
        l *= alpha, o *= alpha, m = bm;
        for (uint32_t j = b; j < b + 64; ++j) {
          l += std::exp2(s[j] - m);
          o += std::exp2(s[j] - m) * gh::gen_attn(kSeed, dt, gh::GEN_V, j, d);
        }
      }
      const gh::AttnExpected e = gh::attn_reference(kSeed, dt, N, row, d);
      CHECK((double)e.o == o && (double)e.m == m && (double)e.l == l);
    }
  }
}

// K and V tiles whose 16-bit words hold their index within the tile, placed by
// the staging functions, read back through the read addresses and the tr map.
// N rows of 64 words stand for K and V in device memory, first and last block.
static void check_addresses(uint32_t N) {
  std::vector<uint16_t> global(N * 64);
  std::vector<uint32_t> k_lds(gh::kAttnOperandBytes / 2, ~0u), v_lds(gh::kAttnOperandBytes / 2, ~0u);
  for (uint32_t block : {0u, N / 64 - 1}) {
    for (uint32_t slot = 0; slot < 512; ++slot) {  // slot 64 q + lane lands at byte 16 slot
      const gh::NarrowChunk ck = gh::attn_k_source(slot), cv = gh::attn_v_source(slot);
      CHECK(ck.row < 64 && ck.byte % 16 == 0 && ck.byte + 16 <= 128 && cv.row < 64 &&
            cv.byte % 16 == 0 && cv.byte + 16 <= 128);
      for (uint32_t w = 0; w < 8; ++w) {
        global.at(gh::attn_global_offset(block, ck) + w) = 0;  // the 16 bytes fetched, in bounds
        global.at(gh::attn_global_offset(block, cv) + w) = 0;
        k_lds.at(8 * slot + w) = ck.row * 64 + ck.byte / 2 + w;
        v_lds.at(8 * slot + w) = cv.row * 64 + cv.byte / 2 + w;
      }
    }
  }
  std::vector<int> seen(64 * 64, 0);
  for (uint32_t w : k_lds) seen.at(w) += 1;
  for (uint32_t w : v_lds) seen.at(w) += 2;
  for (int n : seen) CHECK(n == 3);  // both placements complete, nothing twice

  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t i = lane & 15u, g = lane >> 4;
    for (uint32_t kt = 0; kt < 4; ++kt)
      for (uint32_t ds = 0; ds < 2; ++ds) {
        const uint32_t at = gh::attn_k_read(16 * kt + i, ds, g);
        CHECK(at % 16 == 0);
        for (uint32_t j = 0; j < 8; ++j)
          CHECK(k_lds.at(at / 2 + j) == (16 * kt + i) * 64 + 32 * ds + 8 * g + j);
      }
    // V, the A operand of the second product: V[attn_v_key(c, g, 4 h + e)][16 dt + i]
    for (uint32_t c = 0; c < 2; ++c)
      for (uint32_t h = 0; h < 2; ++h)
        for (uint32_t dt = 0; dt < 4; ++dt)
          for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t src = gh::attn_tr16_source(lane, e), from = src / 4;
            const uint32_t at = gh::attn_v_read(c, h, dt, from >> 4, from & 15u);
            CHECK(at % 8 == 0 && (from >> 4) == g);
            CHECK(v_lds.at(at / 2 + src % 4) == gh::attn_v_key(c, g, 4 * h + e) * 64 + 16 * dt + i);
            CHECK(gh::attn_v_key(c, g, 4 * h + e) == 16 * (2 * c + h) + 4 * g + e);
          }
  }
}

int main() {
  for (int dt : {(int)gh::BF16, (int)gh::F16}) {
    check_generators(dt);
    check_reference(dt, 64, 64), check_reference(dt, 64, 192), check_reference(dt, 128, 4096);
  }
  check_addresses(64), check_addresses(gh::kAttnMaxN);
  std::printf("attn_ref_check OK\n");
  return 0;
}
