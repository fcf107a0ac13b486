// The MoE check's core in gpuhealth_ref.hpp at the cases of tests/test_gpu_moe.py: the routing and its
// builder, the tile lookup the kernel mirrors, the integer reference against a naive loop in double.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gpuhealth_ref.hpp"

#define CHECK(cond) \
  if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }

static const uint32_t kSeed = gh::kDefaultSeed;

struct Case {
  uint32_t T, E, top_k, K, N;
  std::vector<uint32_t> route;  // empty: the generated one
};

static void check_case(int dt, const Case& c) {
  const uint32_t entries = c.T * c.top_k;
  std::vector<uint32_t> route(entries), offsets(c.E + 1), token(entries), entry_of(entries);
  std::vector<float> weight(entries);
  for (uint32_t p = 0; p < entries; ++p)
    route[p] = c.route.empty() ? gh::moe_default_expert(kSeed, c.E, c.top_k, p / c.top_k, p % c.top_k)
                               : c.route.at(p);
  for (uint32_t p = 0; p < entries; ++p) {  // in range, distinct within a token
    CHECK(route[p] < c.E);
    for (uint32_t q = p - p % c.top_k; q < p; ++q) CHECK(route[q] != route[p]);
  }
  gh::moe_build_routing(kSeed, c.T, c.E, c.top_k, route.data(), offsets.data(), token.data(),
                        weight.data(), entry_of.data());
  // offsets monotone from 0 to entries; every (token, choice) once, in its expert's group,
  // tokens ascending within a group; explicit routes honoured; weights in {1, 1/2, 1/4}
  CHECK(offsets[0] == 0 && offsets[c.E] == entries);
  std::vector<int> hit(entries, 0);
  for (uint32_t e = 0; e < c.E; ++e)
    for (uint32_t p = offsets[e]; p + 1 < offsets[e + 1]; ++p) CHECK(token[p] < token[p + 1]);
  for (uint32_t e = 0; e < c.E; ++e) CHECK(offsets[e] <= offsets[e + 1]);
  for (uint32_t p = 0; p < entries; ++p) {
    const uint32_t at = entry_of[p], e = route[p];
    CHECK(at < entries && at >= offsets[e] && at < offsets[e + 1] && token[at] == p / c.top_k);
    CHECK(weight[at] == gh::moe_weight_of(kSeed, p / c.top_k, p % c.top_k));
    CHECK(weight[at] == 1.f || weight[at] == .5f || weight[at] == .25f);
    hit[at] += 1;
  }
  for (int n : hit) CHECK(n == 1);

  // the lookup: the row tiles of the grid are the groups' tiles in order, empty experts own
  // none, every entry lies in the tile its inverse names, and what lies past is idle
  const uint32_t tiles = gh::moe_row_tiles(offsets.data(), c.E), grid = gh::moe_max_row_tiles(c.T, c.top_k, c.E);
  CHECK(tiles >= 1 && tiles <= grid);
  std::vector<int> covered(entries, 0);
  for (uint32_t rt = 0; rt < grid; ++rt) {
    uint32_t e = ~0u, row0 = ~0u;
    CHECK(gh::moe_tile_lookup(offsets.data(), c.E, rt, &e, &row0) == (rt < tiles));
    if (rt >= tiles) continue;
    CHECK(e < c.E && row0 >= offsets[e] && row0 < offsets[e + 1] && (row0 - offsets[e]) % 64 == 0);
    CHECK(gh::moe_tile_of_entry(offsets.data(), e, row0) == rt);
    for (uint32_t r = 0; r < 64 && row0 + r < offsets[e + 1]; ++r) covered.at(row0 + r) += 1;
    CHECK(row0 + 63 < entries + gh::kMoeGuardRows);  // a row that escapes the mask stays inside P
  }
  for (int n : covered) CHECK(n == 1);

  // the reference against a naive loop in double; the bound of the premise
  const uint32_t step_t = c.T > 16 ? c.T / 5 : 1, step_n = c.N / 4 + 1;
  for (uint32_t t = 0; t < c.T; t += step_t)
    for (uint32_t n = 0; n < c.N; n += step_n) {
      double y = 0;
      for (uint32_t j = 0; j < c.top_k; ++j) {
        const uint32_t e = route[t * c.top_k + j];
        double p = 0;
        for (uint32_t k = 0; k < c.K; ++k)
          p += (double)gh::gen_moe(kSeed, dt, gh::GEN_A, t, k) * gh::gen_moe(kSeed, dt, gh::GEN_B, e * c.K + k, n);
        CHECK((double)gh::moe_product_element(kSeed, dt, c.K, t, e, n) == p && std::fabs(p) <= 64.0 * c.K);
        y += p * weight[entry_of[t * c.top_k + j]];
      }
      const int32_t q = gh::moe_y_quarters(kSeed, dt, c.K, c.top_k, route.data() + t * c.top_k, t, n);
      CHECK(0.25 * q == y && std::abs(q) < (1 << 23) && (double)(0.25f * (float)q) == y);
    }
}

int main() {
  CHECK(gh::kMoeMaxTopK * 64u * gh::kMoeMaxK * 4u <= (1u << 23) && gh::kMoeMaxExperts == 64);
  const float f16 = gh::f16_to_f32((uint16_t)gh::kMoePoison), bf16 = gh::bf16_to_f32((uint16_t)gh::kMoePoison);
  CHECK(std::isfinite(f16) && f16 > 1e4f && std::isfinite(bf16 * 8.f * gh::kMoeMaxK) && bf16 > 1e30f);
  const std::vector<Case> cases = {
      {1, 1, 1, 64, 64, {}},       {64, 1, 1, 128, 64, {}},  {65, 1, 1, 64, 64, {}},
      {3, 4, 1, 64, 128, {1, 1, 3}}, {2, 4, 1, 64, 64, {0, 0}}, {70, 2, 2, 64, 64, {}},
      {8, 8, 8, 4096, 64, {}},     {200, 5, 2, 192, 128, {}}, {832, 16, 2, 1024, 1024, {}}};
  for (int dt : {(int)gh::BF16, (int)gh::F16})
    for (const Case& c : cases) check_case(dt, c);
  // the generated routing at the default shape: empty experts, a ragged group, unequal loads
  std::vector<uint32_t> load(16, 0);
  for (uint32_t p = 0; p < 832 * 2; ++p) load[gh::moe_default_expert(kSeed, 16, 2, p / 2, p % 2)] += 1;
  CHECK(load[1] == 0 && load[13] == 0 && load[0] % 64 != 0 && load[0] != load[2] && load[2] != 0);
  std::printf("moe_ref_check OK\n");
  return 0;
}
