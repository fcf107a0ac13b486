// The causal attention check's core in gpuhealth_ref.hpp: generators, the masked
// reference against a double-precision online softmax, the work split, and the
// 256-byte-row staging and read addresses composed with the tr16 lane map.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpuhealth_ref.hpp"

#define CHECK(cond) \
  if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }

static const uint32_t kSeed = gh::kDefaultSeed, kD = gh::kAttn128HeadDim;

static int gen(int dt, uint32_t which, uint32_t row, uint32_t d) { return gh::gen_attn128(kSeed, dt, which, row, d); }

static void check_generators(int dt) {
  unsigned q_seen = 0, v_seen = 0, upper = 0;
  for (uint32_t j = 0; j < gh::kAttn128MaxL; ++j) {
    int nonzero = 0;
    for (uint32_t d = 0; d < kD; ++d) {
      const int k = gen(dt, gh::GEN_KEY, j, d), q = gen(dt, gh::GEN_Q, j, d), v = gen(dt, gh::GEN_V, j, d);
      CHECK(k * k <= 1 && q >= -2 && q <= 2 && v >= -8 && v <= 8);
      nonzero += k != 0, upper += k != 0 && d >= 64;
      q_seen |= 1u << (q + 2), v_seen |= 1u << (v + 8);
    }
    CHECK(nonzero == 2);  // two distinct columns
  }
  CHECK(q_seen == 31u && v_seen == (1u << 17) - 1u && upper > gh::kAttn128MaxL / 2);  // all 128 columns in use
}

static void check_reference(int dt, uint32_t heads, uint32_t L, bool causal, uint32_t row_step) {
  std::vector<double> s(L);
  for (uint32_t row = 0; row < heads * L; row += row_step) {
    const uint32_t first = row / L * L, keys = causal ? row % L + 1 : L;
    double lo = 1e9, hi = -1e9;
    for (uint32_t j = 0; j < keys; ++j) {
      s[j] = 0;
      for (uint32_t d = 0; d < kD; ++d) s[j] += (double)gen(dt, gh::GEN_Q, row, d) * gen(dt, gh::GEN_KEY, first + j, d);
      lo = std::fmin(lo, s[j]), hi = std::fmax(hi, s[j]);
    }
    CHECK(hi - lo <= 8 && lo >= -4 && hi <= 4);  // the spread of the premise
    for (uint32_t d = 0; d < kD; d += (row_step > 1 ? 37 : 1)) {  // every column at the small shapes
      double m = -INFINITY, l = 0, o = 0;
      for (uint32_t b = 0; b < keys; b += 64) {  // key blocks up to the diagonal one, masked inside
        double bm = m;
        for (uint32_t j = b; j < b + 64; ++j) bm = std::fmax(bm, j < keys ? s[j] : -INFINITY);
        CHECK(std::isfinite(bm));  // key 0 is visible: no -inf - -inf
        const double alpha = std::exp2(m - bm);
        l *= alpha, o *= alpha, m = bm;
        for (uint32_t j = b; j < b + 64; ++j) {
          const double p = std::exp2((j < keys ? s[j] : -INFINITY) - m);
          l += p, o += p * gen(dt, gh::GEN_V, first + j, d);
        }
      }
      const gh::AttnExpected e = gh::attn128_reference(kSeed, dt, L, causal, row, d);
      CHECK((double)e.o == o && (double)e.m == m && (double)e.l == l && std::fabs(o) <= 8.0 * L);
    }
  }
}

// every query block of a head is taken once, and a workgroup's steps are nb + 1
static void check_work_split(uint32_t L) {
  const uint32_t nb = L / 64;
  std::vector<int> taken(nb, 0);
  for (uint32_t pair = 0; pair < nb / 2; ++pair) {
    const uint32_t qb0 = gh::attn128_query_block(nb, pair, 0), qb1 = gh::attn128_query_block(nb, pair, 1);
    CHECK(qb0 < nb && qb1 < nb);
    taken[qb0] += 1, taken[qb1] += 1;
    CHECK(gh::attn128_key_blocks(nb, qb0, true) + gh::attn128_key_blocks(nb, qb1, true) == nb + 1);
    for (uint32_t qb : {qb0, qb1}) CHECK(gh::attn128_workgroup_of(L, 2 * L + 64 * qb + 63) == nb + pair);
  }
  for (int n : taken) CHECK(n == 1);
}

// K and V stages whose words hold their index within the key block, placed by the staging
// functions and read back through the read addresses and the tr map, as attn_ref_check does
static void check_addresses(uint32_t rows) {
  std::vector<uint16_t> global((size_t)rows * kD);
  std::vector<uint32_t> k_lds(gh::kAttn128OperandBytes / 2, ~0u), v_lds(k_lds);
  for (uint32_t first_row : {0u, rows - 64})
    for (uint32_t slot = 0; slot < gh::kAttn128Slots; ++slot) {  // slot 64 q + lane lands at byte 16 slot
      const gh::NarrowChunk ck = gh::attn128_k_source(slot), cv = gh::attn128_v_source(slot);
      CHECK(ck.row < 64 && ck.byte % 16 == 0 && ck.byte < 256 && cv.row < 64 && cv.byte % 16 == 0 && cv.byte < 256);
      for (uint32_t w = 0; w < 8; ++w) {
        global.at(gh::attn128_global_offset(first_row, ck) + w) = 0;  // the 16 bytes fetched, in bounds
        global.at(gh::attn128_global_offset(first_row, cv) + w) = 0;
        k_lds.at(8 * slot + w) = ck.row * kD + ck.byte / 2 + w;
        v_lds.at(8 * slot + w) = cv.row * kD + cv.byte / 2 + w;
      }
    }
  std::vector<int> seen(64 * kD, 0);
  for (uint32_t w : k_lds) seen.at(w) += 1;
  for (uint32_t w : v_lds) seen.at(w) += 2;
  for (int n : seen) CHECK(n == 3);  // both placements complete, nothing twice

  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t i = lane & 15u, g = lane >> 4;
    for (uint32_t t = 0; t < 16; ++t) {  // key tile kt, d-step ds
      const uint32_t kt = t / 4, ds = t % 4, at = gh::attn128_k_read(16 * kt + i, ds, g);
      CHECK(at % 16 == 0);
      for (uint32_t j = 0; j < 8; ++j) CHECK(k_lds.at(at / 2 + j) == (16 * kt + i) * kD + 32 * ds + 8 * g + j);
    }
    // V, the A operand of the second product: V[attn_v_key(c, g, 4 h + e)][16 dt + i]
    for (uint32_t t = 0; t < 128; ++t) {
      const uint32_t c = t / 64, h = t / 32 % 2, dt = t / 4 % 8, e = t % 4;
      const uint32_t src = gh::attn_tr16_source(lane, e), from = src / 4;
      const uint32_t at = gh::attn128_v_read(c, h, dt, from >> 4, from & 15u);
      CHECK(at % 8 == 0 && (from >> 4) == g);
      CHECK(v_lds.at(at / 2 + src % 4) == gh::attn_v_key(c, g, 4 * h + e) * kD + 16 * dt + i);
    }
  }
}

int main() {
  CHECK(kD == 128 && gh::kAttn128OutCols == 130 && gh::kAttn128MaxL == 4096);
  for (int dt : {(int)gh::BF16, (int)gh::F16}) {
    check_generators(dt);
    check_reference(dt, 1, 128, true, 1), check_reference(dt, 1, 256, false, 1);
    check_reference(dt, 3, 256, true, 7), check_reference(dt, 1, 4096, true, 211);
  }
  for (uint32_t L : {128u, 256u, 4096u}) check_work_split(L);
  check_addresses(128), check_addresses(3 * 256);
  std::printf("attn128_ref_check OK\n");
  return 0;
}
