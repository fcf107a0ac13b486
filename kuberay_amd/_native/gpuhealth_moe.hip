// gpuhealth_moe — the MoE check of the MI355X (gfx950) burn-in: kernels and
// their host code. Bound to Python by gpuhealth.hip through gpuhealth_gemm.hpp;
// generators, the routing builder, the tile lookup, the reference and the
// exactness premise are in gpuhealth_ref.hpp.
//
// Built like gpuhealth_gemm.hip, with packed fp32 arithmetic disabled for the
// device code (build.py; the reason is at the top of that file). Unlike the
// GEMM kernels this one does fp32 arithmetic outside the MFMA: one multiply by
// the router weight an element, a plain v_mul_f32 under that switch.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpuhealth_gemm.hpp"
#include "gpuhealth_gemm_device.hpp"
#include "gpuhealth_ref.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "gpuhealth targets gfx950 (MI355X) only"
#endif

namespace ghgemm {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 frag_ab_t;
typedef __attribute__((ext_vector_type(8))) _Float16 frag_f16_t;
typedef __attribute__((ext_vector_type(4))) float frag_cd_t;
typedef __attribute__((ext_vector_type(4))) uint32_t frag_u32x4_t;
typedef __attribute__((ext_vector_type(4))) short frag_i16x4_t;

// ---------------------------------------------------------------------------
// Burn-in, part 10: MoE check — the routed expert GEMM of a mixture-of-experts
// layer and its top-k combine; exact, single-shot
//
//   P[p][n]  = X[sorted_token[p]] · W[expert of p]         plain stores
//   Y[t][n] += sorted_weight[p] · P[p][n], t = sorted_token[p]   fp32 atomics
//
// What it runs that no other check does: operand rows whose global address
// comes from a loaded index, tiles whose place in the problem is found on the
// device from data and whose tails are masked, weights picked by a value from
// memory, and global_atomic_add_f32 from several workgroups onto one row.
//
// Work split: a workgroup of four waves owns 64 consecutive sorted entries of
// one expert by 64 columns, a wave a 32 x 32 quadrant, as in gemm_exact
// (gpuhealth_gemm.hip: the MFMA tiling, the 32 KiB double-buffered stage, the
// lane maps of ds_read_b128 and ds_read_b64_tr_b16 and the two swizzles are
// that kernel's; its comments derive them and they are repeated here because
// that file's are private to its translation unit, whose device code must not
// change). The grid is (N / 64, ceil(T · top_k / 64) + E): an upper bound on
// the row tiles that needs no count from the device.
//
// Tile lookup, every wave for itself and wave-uniform in its result: lane e <
// E reads offsets[e] and offsets[e + 1], an inclusive prefix sum of ceil(count
// / 64) runs over the wave with six shuffles, a ballot of (row tile < prefix)
// names the owner as its first set lane, and the owner's first row and end
// come back by readlane. An empty expert adds nothing to the sum and owns no
// tile. No lane set: the workgroup is past the last tile, wave 0 writes
// kMoeIdleKey to where[] and all four waves leave before any barrier.
//
// Routing in registers: lane l of every wave holds token id and weight of tile
// row l, or (T, 0) for a row past the group's end, so a tail row gathers the
// poison row. A token id is clamped to T: whatever the list holds, no address
// leaves X or Y. The lanes that stage row r of A fetch its token by a shuffle
// once, before the loop, and keep the row's global address; each stage adds
// the K offset. B is W + expert · K · N. The epilogue fetches token, weight
// and validity of an accumulator's row by shuffle, stores P and adds weight ·
// P onto Y with a no-return agent-scope atomic, both under the mask. A row
// that escapes the mask lands in the next group's rows of P, in P's guard rows
// or in Y's guard row T, all of which are compared. No workgroup waits on
// another.
// ---------------------------------------------------------------------------
constexpr int kMoeThreads = 256;
constexpr uint32_t kRowBytes = gh::kGemmTile * 2;            // 128
constexpr uint32_t kOperandBytes = gh::kGemmTile * kRowBytes;  // 8 KiB
constexpr uint32_t kStageBytes = 2 * kOperandBytes;           // A then B
constexpr uint32_t kLdsBytes = 2 * kStageBytes;               // 32 KiB

// gemm_a_swizzle and gemm_b_swizzle of gpuhealth_gemm.hip
__device__ inline uint32_t a_swizzle(uint32_t row) { return (row >> 1) & 7u; }
__device__ inline uint32_t b_swizzle(uint32_t row) {
  return ((row >> 1) & 1u) << 1 | ((row >> 3) & 1u) << 2;
}

struct MoeArgs {
  const uint16_t* x;
  const uint16_t* w;
  const uint32_t* offsets;
  const uint32_t* sorted_token;
  const float* sorted_weight;
  float* p;
  float* y;
  uint32_t* where;  // one location key per workgroup, kMoeIdleKey for one without a tile
  uint32_t n, k, tokens, experts, entries;
};

template <int DT> struct MoeFrag { typedef frag_ab_t type; };
template <> struct MoeFrag<gh::F16> { typedef frag_f16_t type; };

template <int DT>
__global__ __launch_bounds__(kMoeThreads) void moe_kernel(MoeArgs g) {
  static_assert(DT == gh::BF16 || DT == gh::F16, "the 16-bit paths only");
  typedef typename MoeFrag<DT>::type frag_t;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kLdsBytes];
  GH_LDS unsigned char* lds = (GH_LDS unsigned char*)lds_raw;

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = lane & 15u, grp = lane >> 4;
  const uint32_t rt = blockIdx.y, n0 = blockIdx.x * gh::kGemmTile;
  const uint32_t wg = rt * gridDim.x + blockIdx.x;

  // the tile lookup (gh::moe_tile_lookup is the same arithmetic on the host)
  uint32_t start = 0, count = 0;
  if (lane < g.experts) {
    start = g.offsets[lane];
    count = g.offsets[lane + 1] - start;
  }
  const uint32_t mine = gh::moe_tiles_of(count);
  uint32_t upto = mine;  // inclusive prefix sum over the lanes
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t below = (uint32_t)__shfl_up((int)upto, d);
    if (lane >= d) upto += below;
  }
  const unsigned long long owners = __ballot(rt < upto);
  if (owners == 0) {
    if (threadIdx.x == 0) g.where[wg] = gh::kMoeIdleKey;
    return;
  }
  const uint32_t expert = __builtin_amdgcn_readfirstlane((uint32_t)__ffsll(owners) - 1u);
  const uint32_t row0 = (uint32_t)__builtin_amdgcn_readlane(
      (int)(start + (rt - (upto - mine)) * gh::kGemmTile), (int)expert);
  uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)(start + count), (int)expert);
  end = end < g.entries ? end : g.entries;

  // tile row `lane`: its token and weight, the poison row and 0 past the end
  const bool valid = row0 + lane < end;
  uint32_t token = valid ? g.sorted_token[row0 + lane] : g.tokens;
  token = token < g.tokens ? token : g.tokens;
  const float weight = valid ? g.sorted_weight[row0 + lane] : 0.f;

  // this wave's four 1 KiB loads of a stage: rows 8 q + lane / 8, q = 2 wave + t
  const uint16_t* src_a[2];
  const uint16_t* src_b[2];
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t row = 8 * (2 * wave + t) + (lane >> 3), slot = lane & 7u;
    const uint32_t row_token = (uint32_t)__shfl((int)token, (int)row);
    src_a[t] = g.x + (size_t)row_token * g.k + 8 * (slot ^ a_swizzle(row));
    src_b[t] = g.w + ((size_t)expert * g.k + row) * g.n + n0 + 8 * (slot ^ b_swizzle(row));
  }
  auto issue_stage = [&](uint32_t kt, GH_LDS unsigned char* stage) {
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
      const uint32_t q = 2 * wave + t;
      __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)(src_a[t] + kt),
                                       (GH_LDS void*)(stage + 1024 * q), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)(src_b[t] + (size_t)kt * g.n),
                                       (GH_LDS void*)(stage + kOperandBytes + 1024 * q), 16, 0,
                                       0);
    }
  };

  const uint32_t wrow = 32 * (wave >> 1), wcol = 32 * (wave & 1u);  // the wave's quadrant
  frag_cd_t acc[2][2];
#pragma unroll
  for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
    for (uint32_t tn = 0; tn < 2; ++tn) acc[tm][tn] = frag_cd_t{0.f, 0.f, 0.f, 0.f};

  const uint32_t stages = g.k / gh::kGemmTile;
  issue_stage(0, lds);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (uint32_t s = 0; s < stages; ++s) {
    GH_LDS unsigned char* a_lds = lds + (s & 1u) * kStageBytes;
    GH_LDS unsigned char* b_lds = a_lds + kOperandBytes;
    if (s + 1 < stages)
      issue_stage((s + 1) * gh::kGemmTile, lds + ((s + 1) & 1u) * kStageBytes);
#pragma unroll
    for (uint32_t kk = 0; kk < 2; ++kk) {
      frag_t a[2], b[2];
#pragma unroll
      for (uint32_t tm = 0; tm < 2; ++tm) {
        const uint32_t row = wrow + 16 * tm + i;
        const uint32_t slot = (4 * kk + grp) ^ a_swizzle(row);
        a[tm] = __builtin_bit_cast(
            frag_t, *(const GH_LDS frag_u32x4_t*)(a_lds + row * kRowBytes + 16 * slot));
      }
#pragma unroll
      for (uint32_t tn = 0; tn < 2; ++tn) {
        const uint32_t col = wcol + 16 * tn + 4 * (i & 3u);
        frag_i16x4_t half[2];
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          const uint32_t row = 32 * kk + 8 * grp + 4 * h + (i >> 2);
          const uint32_t slot = (col >> 3) ^ b_swizzle(row);
          half[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (GH_LDS frag_i16x4_t*)(b_lds + row * kRowBytes + 16 * slot + 2 * (col & 7u)));
        }
        b[tn] = __builtin_bit_cast(
            frag_t, __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
        for (uint32_t tn = 0; tn < 2; ++tn) {
          if constexpr (DT == gh::BF16)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
          else
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
        }
    }
    // stage s + 1 has landed and stage s is no longer read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // register r of a tile is row 4 grp + r, column i: the row's routing by shuffle
#pragma unroll
  for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t row = wrow + 16 * tm + 4 * grp + r;
      const uint32_t row_token = (uint32_t)__shfl((int)token, (int)row);
      const float row_weight = __shfl(weight, (int)row);
      if (row0 + row < end) {
#pragma unroll
        for (uint32_t tn = 0; tn < 2; ++tn) {
          const uint32_t col = n0 + wcol + 16 * tn + i;
          g.p[(size_t)(row0 + row) * g.n + col] = acc[tm][tn][r];
          (void)__hip_atomic_fetch_add(g.y + (size_t)row_token * g.n + col,
                                       row_weight * acc[tm][tn][r], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  if (threadIdx.x == 0)
    g.where[wg] = gh::location_key(gh::decode_location(read_xcc_id_reg(), read_hw_id_reg()));
}

// X (the poison row included) and W, two 16-bit elements per store
__global__ void moe_fill_kernel(uint32_t* __restrict__ x, uint32_t* __restrict__ w, int dtype,
                                uint32_t seed, uint32_t tokens, uint32_t experts, uint32_t n,
                                uint32_t k) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t hx = gh::gemm_matrix_hash(seed, dtype, gh::GEN_A);
  const uint32_t hw = gh::gemm_matrix_hash(seed, dtype, gh::GEN_B);
  for (uint64_t p = first; p < (uint64_t)(tokens + 1) * k / 2; p += stride) {
    const uint32_t row = (uint32_t)(2 * p / k), col = (uint32_t)(2 * p % k);
    x[p] = row == tokens
               ? gh::kMoePoison | gh::kMoePoison << 16
               : (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hx, row, col)) |
                     (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hx, row, col + 1)) << 16;
  }
  for (uint64_t p = first; p < (uint64_t)experts * k * n / 2; p += stride) {
    const uint32_t row = (uint32_t)(2 * p / n), col = (uint32_t)(2 * p % n);  // row = e · K + k
    w[p] = (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hw, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hw, row, col + 1)) << 16;
  }
}

// A wave is one token row by 64 columns, a block four rows; grid (N / 64,
// ceil((T + 1) / 4)). It recomputes the top_k products of its row from the
// generators in integer arithmetic, off the matrix pipe, through the clean
// routing (route, entry_of: never the list the kernel read), compares each
// with its row of P and their weighted sum in quarters with Y. stats is
// [row tiles][column tiles] for P, first_bad = entry · N + col, then one slot
// for Y, first_bad = row · N + col. Row T is Y's guard row and expects 0.
__global__ void moe_check_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                 const uint32_t* __restrict__ offsets,
                                 const uint32_t* __restrict__ route,
                                 const uint32_t* __restrict__ entry_of, int dtype, uint32_t seed,
                                 uint32_t tokens, uint32_t top_k, uint32_t n, uint32_t k,
                                 TileStats* __restrict__ stats, uint32_t y_slot) {
  const uint32_t t = 4 * blockIdx.y + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (t > tokens) return;
  const uint32_t col0 = blockIdx.x * gh::kGemmTile, col = col0 + lane;
  int32_t quarters = 0;
  for (uint32_t j = 0; j < (t < tokens ? top_k : 0u); ++j) {
    const uint32_t e = route[t * top_k + j], entry = entry_of[t * top_k + j];
    const int32_t product = gh::moe_product_element(seed, dtype, k, t, e, col);
    quarters += product * (int32_t)(4u >> gh::moe_weight_shift(seed, t, j));
    const unsigned long long bad = __ballot(!(p[(size_t)entry * n + col] == (float)product));
    if (bad != 0 && lane == 0) {
      TileStats* mine = stats + (size_t)gh::moe_tile_of_entry(offsets, e, entry) * gridDim.x +
                        blockIdx.x;
      atomicAdd(&mine->mismatches, (unsigned long long)__popcll(bad));
      atomicMin(&mine->first_bad,
                (unsigned long long)entry * n + col0 + (unsigned long long)(__ffsll(bad) - 1));
    }
  }
  const unsigned long long bad = __ballot(!(y[(size_t)t * n + col] == 0.25f * (float)quarters));
  if (bad == 0 || lane != 0) return;
  atomicAdd(&stats[y_slot].mismatches, (unsigned long long)__popcll(bad));
  atomicMin(&stats[y_slot].first_bad,
            (unsigned long long)t * n + col0 + (unsigned long long)(__ffsll(bad) - 1));
}

// the guard rows of P: any bit set in them counts; first_bad = row of P · N + col,
// `first` being that of the guard's first word
__global__ void moe_guard_kernel(const uint32_t* __restrict__ guard, uint32_t words,
                                 unsigned long long first, TileStats* __restrict__ stats) {
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long bad = __ballot(at < words && guard[at] != 0);
  if (bad == 0 || (threadIdx.x & 63u) != 0) return;
  atomicAdd(&stats->mismatches, (unsigned long long)__popcll(bad));
  atomicMin(&stats->first_bad, first + at + (unsigned long long)(__ffsll(bad) - 1));
}

struct Routing {
  std::vector<uint32_t> route, offsets, sorted_token, entry_of;
  std::vector<float> sorted_weight;
};

Routing build_routing(uint32_t seed, uint32_t T, uint32_t E, uint32_t top_k,
                      const std::vector<int64_t>& given) {
  Routing r;
  r.route.resize((size_t)T * top_k);
  for (uint32_t p = 0; p < T * top_k; ++p)
    r.route[p] = given.empty() ? gh::moe_default_expert(seed, E, top_k, p / top_k, p % top_k)
                               : (uint32_t)given[p];
  r.offsets.resize(E + 1);
  r.sorted_token.resize(r.route.size());
  r.sorted_weight.resize(r.route.size());
  r.entry_of.resize(r.route.size());
  gh::moe_build_routing(seed, T, E, top_k, r.route.data(), r.offsets.data(),
                        r.sorted_token.data(), r.sorted_weight.data(), r.entry_of.data());
  return r;
}

template <typename V> void upload(void* dst, const std::vector<V>& src) {
  HIP_CHECK(hipMemcpy(dst, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
}

}  // namespace

MoeResult run_moe_exact(int dtype, int64_t tokens_in, int64_t experts_in, int64_t top_k_in,
                        int64_t k_in, int64_t n_in, const std::vector<int64_t>& route_in,
                        uint32_t seed, const MoeInject* inject, MoeDump* dump) {
  if (dtype != gh::BF16 && dtype != gh::F16)
    throw std::invalid_argument("the MoE check runs bf16 and f16 only");
  int device = 0, cu_total = 0;
  HIP_CHECK(hipGetDevice(&device));
  HIP_CHECK(hipDeviceGetAttribute(&cu_total, hipDeviceAttributeMultiprocessorCount, device));
  if (experts_in == 0) experts_in = kMoeDefaultExperts;
  if (top_k_in == 0) top_k_in = kMoeDefaultTopK;
  if (k_in == 0) k_in = kDefaultK;
  if (n_in == 0) n_in = kDefaultK;
  if (k_in < 0 || n_in < 0 || k_in % gh::kGemmTile || n_in % gh::kGemmTile)
    throw std::invalid_argument("k and n must be positive multiples of 64");
  if (k_in > gh::kMoeMaxK)
    throw std::invalid_argument("k must be at most 4096: beyond it the sums are not exact in fp32");
  if (n_in > gh::kGemmMaxMN) throw std::invalid_argument("n must be at most 65536");
  if (experts_in < 1 || experts_in > gh::kMoeMaxExperts)
    throw std::invalid_argument("experts must be in [1, 64]");
  if (top_k_in < 1 || top_k_in > std::min<int64_t>(gh::kMoeMaxTopK, experts_in))
    throw std::invalid_argument("top_k must be in [1, min(8, experts)]");
  const uint32_t E = (uint32_t)experts_in, top_k = (uint32_t)top_k_in;
  const uint32_t k = (uint32_t)k_in, n = (uint32_t)n_in, tiles_n = n / gh::kGemmTile;
  if (!route_in.empty() && route_in.size() % top_k != 0)
    throw std::invalid_argument("route must have tokens * top_k entries");
  if (tokens_in == 0 && !route_in.empty()) tokens_in = (int64_t)(route_in.size() / top_k);
  if (tokens_in == 0) {
    // No route either: the generated one, grown by 64 tokens at a time until
    // every CU gets kWorkgroupsPerCu workgroups that find a tile. Only the
    // group sizes are needed for that, and each token is counted once.
    const uint32_t want = kWorkgroupsPerCu * (uint32_t)std::max(cu_total, 1);
    std::vector<uint32_t> ends(E + 1, 0);  // moe_row_tiles reads sizes as differences
    uint32_t T = 0;
    while (T < gh::kMoeMaxTokens && gh::moe_row_tiles(ends.data(), E) * tiles_n < want) {
      for (uint32_t t = T; t < T + gh::kGemmTile; ++t)
        for (uint32_t j = 0; j < top_k; ++j)
          for (uint32_t e = gh::moe_default_expert(seed, E, top_k, t, j) + 1; e <= E; ++e)
            ends[e] += 1;
      T += gh::kGemmTile;
    }
    if (gh::moe_row_tiles(ends.data(), E) * tiles_n < want)
      throw std::invalid_argument(
          "no default tokens for this shape: it cannot give every CU its workgroups; give tokens");
    tokens_in = T;
  }
  if (tokens_in < 1 || tokens_in > gh::kMoeMaxTokens)
    throw std::invalid_argument("tokens must be in [1, 65536]");
  const uint32_t T = (uint32_t)tokens_in, entries = T * top_k;
  const size_t x_bytes = (size_t)(T + 1) * k * 2, w_bytes = (size_t)E * k * n * 2;
  const size_t p_bytes = (size_t)(entries + gh::kMoeGuardRows) * n * sizeof(float);
  const size_t y_bytes = (size_t)(T + 1) * n * sizeof(float);
  if (x_bytes + w_bytes + p_bytes + y_bytes > gh::kMoeMaxBytes)
    throw std::invalid_argument("X, W, P and Y together must be at most 2 GiB");
  if (!route_in.empty()) {
    if (route_in.size() != entries)
      throw std::invalid_argument("route must have tokens * top_k entries");
    for (uint32_t p = 0; p < entries; ++p) {
      if (route_in[p] < 0 || route_in[p] >= (int64_t)E)
        throw std::invalid_argument("every route entry must be an expert id below experts");
      for (uint32_t q = p - p % top_k; q < p; ++q)
        if (route_in[q] == route_in[p])
          throw std::invalid_argument("a token's experts must be distinct");
    }
  }
  const Routing r = build_routing(seed, T, E, top_k, route_in);
  if (inject) {
    bool inside = false;
    if (inject->which == MOE_X) inside = inject->row < T && inject->col < k;
    else if (inject->which == MOE_W) inside = inject->row < E * k && inject->col < n;
    else if (inject->which == MOE_ROUTE)
      inside = inject->row < entries && inject->col == 0 &&
               (r.sorted_token[inject->row] ^ inject->mask) < T;
    if (!inside) throw std::invalid_argument("injected element is outside its target");
    if (inject->mask == 0 || inject->mask > 0xFFFFu)
      throw std::invalid_argument("xor mask must be a non-zero 16-bit value");
  }
  const uint32_t max_rt = gh::moe_max_row_tiles(T, top_k, E), workgroups = max_rt * tiles_n;
  const uint32_t y_slot = workgroups, guard_slot = workgroups + 1, n_stats = workgroups + 2;

  DeviceScope scope;
  uint16_t* d_x = (uint16_t*)scope.alloc(x_bytes);
  uint16_t* d_w = (uint16_t*)scope.alloc(w_bytes);
  float* d_p = (float*)scope.alloc(p_bytes);
  float* d_y = (float*)scope.alloc(y_bytes);
  uint32_t* d_offsets = (uint32_t*)scope.alloc((E + 1) * sizeof(uint32_t));
  uint32_t* d_token = (uint32_t*)scope.alloc(entries * sizeof(uint32_t));
  float* d_weight = (float*)scope.alloc(entries * sizeof(float));
  uint32_t* d_route = (uint32_t*)scope.alloc(entries * sizeof(uint32_t));
  uint32_t* d_entry_of = (uint32_t*)scope.alloc(entries * sizeof(uint32_t));
  uint32_t* d_where = (uint32_t*)scope.alloc((size_t)workgroups * sizeof(uint32_t));
  TileStats* d_stats = (TileStats*)scope.alloc((size_t)n_stats * sizeof(TileStats));
  std::vector<TileStats> stats(n_stats, TileStats{0, kNoBadWord});
  upload(d_stats, stats);
  upload(d_offsets, r.offsets);
  upload(d_token, r.sorted_token);
  upload(d_weight, r.sorted_weight);
  upload(d_route, r.route);
  upload(d_entry_of, r.entry_of);
  // a row of P or a key the kernel did not write fails the compare / names no
  // CU; Y and P's guard rows start as zero
  const size_t guard_bytes = (size_t)gh::kMoeGuardRows * n * sizeof(float);
  HIP_CHECK(hipMemset(d_p, 0xFF, p_bytes - guard_bytes));
  HIP_CHECK(hipMemset((char*)d_p + p_bytes - guard_bytes, 0, guard_bytes));
  HIP_CHECK(hipMemset(d_y, 0, y_bytes));
  HIP_CHECK(hipMemset(d_where, 0xFF, (size_t)workgroups * sizeof(uint32_t)));

  const uint64_t fill_items = std::max<uint64_t>((uint64_t)(T + 1) * k, (uint64_t)E * k * n) / 2;
  hipLaunchKernelGGL(moe_fill_kernel,
                     dim3((unsigned)std::min<uint64_t>((fill_items + 255) / 256, 4096)), dim3(256),
                     0, 0, (uint32_t*)d_x, (uint32_t*)d_w, dtype, seed, T, E, n, k);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (inject && inject->which == MOE_ROUTE) {
    const uint32_t token = r.sorted_token[inject->row] ^ inject->mask;  // below T: checked
    HIP_CHECK(hipMemcpy(d_token + inject->row, &token, 4, hipMemcpyHostToDevice));
  } else if (inject) {
    const bool is_x = inject->which == MOE_X;
    const size_t element = (size_t)inject->row * (is_x ? k : n) + inject->col;
    // host read-xor-write of the dword that holds the element
    uint32_t* addr = (uint32_t*)(is_x ? d_x : d_w) + element / 2;
    uint32_t word = 0;
    HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
    word ^= inject->mask << (16 * (element & 1u));
    HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
  }

  const MoeArgs args{d_x, d_w, d_offsets, d_token, d_weight, d_p, d_y, d_where,
                     n,   k,   T,         E,       entries};
  const dim3 grid(tiles_n, max_rt);
  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  if (dtype == gh::BF16)
    hipLaunchKernelGGL((moe_kernel<gh::BF16>), grid, dim3(kMoeThreads), 0, 0, args);
  else
    hipLaunchKernelGGL((moe_kernel<gh::F16>), grid, dim3(kMoeThreads), 0, 0, args);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, 0));
  hipLaunchKernelGGL(moe_check_kernel, dim3(tiles_n, (T + 1 + 3) / 4), dim3(256), 0, 0, d_p, d_y,
                     d_offsets, d_route, d_entry_of, dtype, seed, T, top_k, n, k, d_stats, y_slot);
  HIP_CHECK(hipGetLastError());
  const uint32_t guard_words = gh::kMoeGuardRows * n;
  hipLaunchKernelGGL(moe_guard_kernel, dim3((guard_words + 255) / 256), dim3(256), 0, 0,
                     (const uint32_t*)(d_p + (size_t)entries * n), guard_words,
                     (unsigned long long)entries * n, d_stats + guard_slot);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));

  std::vector<uint32_t> where(workgroups);
  HIP_CHECK(hipMemcpy(stats.data(), d_stats, n_stats * sizeof(TileStats), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(where.data(), d_where, workgroups * sizeof(uint32_t), hipMemcpyDeviceToHost));

  MoeResult res;
  res.dtype = dtype;
  res.m = T, res.n = n, res.k = k;
  res.tokens = T, res.experts = E, res.top_k = top_k, res.entries = entries;
  res.cu_total = cu_total;
  res.elapsed_ms = ms;
  std::vector<uint32_t> seen;
  for (uint32_t key : where)
    if (key != gh::kMoeIdleKey) seen.push_back(key);
  res.workgroups = (int)seen.size();
  res.tiles = (uint32_t)seen.size() / tiles_n;
  std::sort(seen.begin(), seen.end());
  res.cu_seen = (int)(std::unique(seen.begin(), seen.end()) - seen.begin());
  for (uint32_t t = 0; t < workgroups; ++t)  // a bad product names its workgroup
    if (stats[t].mismatches != 0)
      res.faulty.push_back({t / tiles_n, t % tiles_n, where[t], stats[t]});
  const bool products_clean = res.faulty.empty();
  if (stats[guard_slot].mismatches != 0)  // P's guard rows: a place of its own, no CU
    res.faulty.push_back({max_rt, 0, kMoeGuardKey, stats[guard_slot]});
  res.mismatches = stats[y_slot].mismatches + stats[guard_slot].mismatches;
  if (stats[y_slot].mismatches != 0) {
    if (products_clean) res.faulty.push_back({0, 0, kMoeNoCu, stats[y_slot]});  // the scatter
    const unsigned long long first = stats[y_slot].first_bad;
    const uint32_t row = (uint32_t)(first / n), col = (uint32_t)(first % n);
    res.first_bad = (int64_t)first;
    HIP_CHECK(hipMemcpy(&res.got, d_y + first, 4, hipMemcpyDeviceToHost));
    res.expected = row == T ? 0.f
                            : 0.25f * (float)gh::moe_y_quarters(seed, dtype, k, top_k,
                                                                r.route.data() + (size_t)row * top_k,
                                                                row, col);
  }
  if (dump) {
    dump->x = device_bytes(d_x, x_bytes);
    dump->w = device_bytes(d_w, w_bytes);
    dump->offsets = device_bytes(d_offsets, (E + 1) * sizeof(uint32_t));
    dump->sorted_token = device_bytes(d_token, entries * sizeof(uint32_t));
    dump->sorted_weight = device_bytes(d_weight, entries * sizeof(float));
    dump->p = device_bytes(d_p, p_bytes);
    dump->y = device_bytes(d_y, y_bytes);
  }
  return res;
}

}  // namespace ghgemm
