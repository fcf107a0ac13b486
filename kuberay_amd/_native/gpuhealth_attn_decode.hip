// gpuhealth_attn_decode — the decode attention check of the MI355X (gfx950)
// burn-in: exact unnormalised attention of one query token a sequence over a
// paged KV cache, grouped-query heads, the context split over workgroups and
// merged by a second kernel, base 2, for bf16 and f16. Bound to Python by
// gpuhealth.hip through gpuhealth_gemm.hpp; generators, the page map, the
// exactness premise with poison, tails and partials, the reference, the work
// split and every LDS address function are in gpuhealth_ref.hpp. Built with
// the switches of gpuhealth_attn128.hip (build.py): packed fp32 arithmetic is
// disabled for the device code.
//
// Burn-in, part 9. What the attention checks of parts 7 and 8 do not execute
// and an LLM replica's decode attention does: dependent loads (a page index
// read from memory, then an address built from it, in front of every tile),
// gathered 4 KiB pages, a key tail that ends inside a page next to slots that
// were never written, waves that run decoupled with no barrier in the main
// loop, an accumulator reduction across waves through LDS, and a second kernel
// that merges partial softmax states, empty ones included.
//
//   keys j = 0 .. ctx[b] - 1 of (b, hk), found through the block table
//   s_j = Q[row]·K[b][hk][j],  m = max_j s_j,  l = Σ_j 2^(s_j - m),
//   O~[d] = Σ_j 2^(s_j - m) · V[b][hk][j][d],   row = (b·kv_heads + hk)·G + g
//
// Main kernel: grid (splits, kv_heads, batch), four waves. The workgroup's
// query tile is the G query heads of one KV head as the N side of
// mfma_f32_16x16x32: lane (i = l & 15, g = l >> 4) carries query head i, lanes
// with i >= G carry zero Q and store nothing. Scores are Sᵀ = K·Qᵀ as in parts
// 7 and 8, so a lane's scores belong to one query and P is the B operand of
// the second product as it stands. A step is 128 keys = 8 pages; split s of S
// takes steps [s·ns/S, (s+1)·ns/S) of the sequence's own ns = ceil(ctx/128).
// An empty split writes m = -inf, l = 0, O~ = 0 and never enters the loop.
//
// Inside a step the waves split the keys: wave w owns pages 2w and 2w + 1, one
// 32-key chunk, and keeps a private m_run, l and 32 accumulator registers of
// O~ᵀ. The main loop has no __syncthreads(), only s_waitcnt: everything a wave
// reads in it, it loaded itself.
//   K: lane (i, g) takes K[token i][32 ds + 8 g .. + 7] of a page with 16-byte
//     loads straight into the A operand's registers, no LDS.
//   V: the wave stages its two pages with global_load_lds_dwordx4 into its own
//     double-buffered 8 KiB stage (gh::decode_v_source puts the swizzle on the
//     global side) and reads Vᵀ with ds_read_b64_tr_b16 at gh::decode_v_read:
//     half h of a fragment is page h of the wave.
//   Page indices are wave-uniform and read in plain C++ one step ahead of the
//     loads that need them: during step n the wave issues the loads of step
//     n + 1 from the indices it read during step n - 1, then reads those of
//     step n + 2. An index is masked to the pool before it becomes an address,
//     so a corrupt table entry gives a wrong page, never one outside the pool.
// Masking: a page wholly past ctx is neither loaded nor computed (wave-uniform:
// its scores are -inf and its half of the V fragment is zero, the stage behind
// it was never written); the page that straddles ctx gets -inf per key before
// the maximum. A page that is processed holds a visible key, and every query
// sees it, so a block maximum is finite and -inf - -inf cannot occur inside a
// wave. A wave that saw no key keeps m = -inf.
//
// Epilogue: each wave lays (O~ᵀ, m, l) into its own 16 KiB of LDS (its stages
// are free), one barrier, then wave w merges d-tiles 2w and 2w + 1 of the four
// partials with exp2(m_w - m), a power of two or 0, and stores them to the
// workspace [rows, S, 130] with plain vector stores; wave 0 stores m and l.
// Wave 0's first page of a non-empty split always holds a key, so m is finite.
// Lane 0 of wave 0 stores the location key. No workgroup waits on another.
//
// Merge kernel: one block a row, a thread a column; m = max_s m_s, O~ = Σ_s
// O~_s · exp2(m_s - m), l likewise. ctx >= 1, so some split holds a key and m
// is finite.
//
// The fill uses dword stores: poison over both pools, then the owned slots
// through the table. The check recomputes finals and split partials from the
// generators in integer arithmetic (gh::decode_reference), a thread an element.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <limits>
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

typedef __attribute__((ext_vector_type(8))) __bf16 frag_bf16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 frag_f16_t;
typedef __attribute__((ext_vector_type(4))) float frag_cd_t;
typedef __attribute__((ext_vector_type(4))) uint32_t frag_u32x4_t;
typedef __attribute__((ext_vector_type(4))) short frag_i16x4_t;

constexpr int kDecodeThreads = 64 * gh::kDecodeWaves;
constexpr uint32_t kCols = gh::kAttn128OutCols;        // 130: O~, then m, then l
constexpr uint32_t kHeadDim = gh::kAttn128HeadDim;     // 128
constexpr uint32_t kDTiles = kHeadDim / 16;            // 8 d-tiles of O~ᵀ
constexpr uint32_t kDSteps = kHeadDim / 32;            // 4 d-steps of a score
constexpr uint32_t kNoPage = ~0u;                      // a page wholly past ctx, or past the split

struct DecodeArgs {
  const uint16_t* q;
  const uint16_t* k_pool;
  const uint16_t* v_pool;
  float* partial;        // [rows, S, 130]
  uint32_t* where;       // one location key per workgroup
  uint32_t kv_heads, group, max_pages, pool_mask;
};

template <int DT> struct DecodeFrag { typedef frag_bf16_t type; typedef __bf16 elem; };
template <> struct DecodeFrag<gh::F16> { typedef frag_f16_t type; typedef _Float16 elem; };

template <int DT>
__device__ inline frag_cd_t decode_mfma(typename DecodeFrag<DT>::type a,
                                        typename DecodeFrag<DT>::type b, frag_cd_t c) {
  if constexpr (DT == gh::BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// as in gpuhealth_attn128.hip: after the pair of swaps every lane has combined
// the x of lanes i, i + 16, i + 32 and i + 48
__device__ inline float decode_max_over_groups(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
  u = __builtin_bit_cast(uint32_t, x);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
}
__device__ inline float decode_sum_over_groups(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
  u = __builtin_bit_cast(uint32_t, x);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
}

// the physical pages of this wave's two pages of step `step`, kNoPage for one
// that lies past the split or wholly past ctx; wave-uniform
__device__ __forceinline__ void decode_read_pages(const int32_t* __restrict__ tab, uint32_t step,
                                         uint32_t end, uint32_t pages, uint32_t wave,
                                         uint32_t pool_mask, uint32_t pg[2]) {
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t p = gh::kDecodeStepPages * step + 2 * wave + t;
    pg[t] = step < end && p < pages ? (uint32_t)tab[p] & pool_mask : kNoPage;
  }
}

// this wave's loads of one step: K of page t into kf[t], V of both pages into
// the stage at `stage`, four 1 KiB loads a page
__device__ __forceinline__ void decode_issue(const DecodeArgs& a, uint32_t hk, const uint32_t pg[2],
                                    GH_LDS unsigned char* stage, frag_u32x4_t kf[2][kDSteps],
                                    uint32_t lane) {
  const uint32_t i = lane & 15u, grp = lane >> 4;
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    if (pg[t] == kNoPage) continue;
#pragma unroll
    for (uint32_t ds = 0; ds < kDSteps; ++ds)
      kf[t][ds] = *(const frag_u32x4_t*)(a.k_pool + gh::decode_pool_offset(pg[t], a.kv_heads, hk, i,
                                                                           32 * ds + 8 * grp));
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      const gh::NarrowChunk c = gh::decode_v_source(256 * t + 64 * u + lane);  // rows 16 t .. + 15
      const uint16_t* src = a.v_pool + gh::decode_pool_offset(pg[t], a.kv_heads, hk,
                                                              c.row % gh::kDecodePageTokens,
                                                              c.byte / 2u);
      __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src,
                                       (GH_LDS void*)(stage + 1024 * (4 * t + u)), 16, 0, 0);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kDecodeThreads) void decode_kernel(
    DecodeArgs a, const int32_t* __restrict__ table /* [batch, max_pages] */,
    const uint32_t* __restrict__ ctx_of /* [batch] */) {
  static_assert(DT == gh::BF16 || DT == gh::F16, "the 16-bit paths only");
  typedef typename DecodeFrag<DT>::type frag_t;
  typedef typename DecodeFrag<DT>::elem elem_t;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[gh::kDecodeLdsBytes];
  GH_LDS unsigned char* lds = (GH_LDS unsigned char*)lds_raw;
  constexpr float kNegInf = -std::numeric_limits<float>::infinity();

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = lane & 15u, grp = lane >> 4;
  const uint32_t S = gridDim.x, split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const uint32_t kvrow = b * a.kv_heads + hk, row0 = kvrow * a.group;  // first flat Q row
  const uint32_t ctx = ctx_of[b], ns = gh::decode_steps(ctx), pages = gh::decode_pages(ctx);
  const uint32_t first = gh::decode_split_first(ns, S, split);
  const uint32_t end = gh::decode_split_first(ns, S, split + 1);
  const int32_t* __restrict__ tab = table + (size_t)b * a.max_pages;
  const bool mine = i < a.group;  // this lane's query head exists
  float* out = a.partial + ((size_t)(row0 + (mine ? i : 0)) * S + split) * kCols;

  if (threadIdx.x == 0)
    a.where[kvrow * S + split] =
        gh::location_key(gh::decode_location(read_xcc_id_reg(), read_hw_id_reg()));
  if (first == end) {  // an empty split: S > ns
    for (uint32_t e = threadIdx.x; e < a.group * kCols; e += kDecodeThreads)
      a.partial[((size_t)(row0 + e / kCols) * S + split) * kCols + e % kCols] =
          e % kCols == kHeadDim ? kNegInf : 0.f;
    return;
  }

  frag_t qf[kDSteps];
#pragma unroll
  for (uint32_t ds = 0; ds < kDSteps; ++ds) {
    frag_u32x4_t raw{0u, 0u, 0u, 0u};
    if (mine) raw = *(const frag_u32x4_t*)(a.q + (size_t)(row0 + i) * kHeadDim + 32 * ds + 8 * grp);
    qf[ds] = __builtin_bit_cast(frag_t, raw);
  }

  frag_cd_t acc[kDTiles];  // O~ᵀ of this wave's keys, d-tile dt: [d = 16 dt + 4 grp + r][query i]
#pragma unroll
  for (uint32_t dt = 0; dt < kDTiles; ++dt) acc[dt] = frag_cd_t{0.f, 0.f, 0.f, 0.f};
  float m_run = kNegInf, l_run = 0.f;

  uint32_t pg[2];
  frag_u32x4_t kf_next[2][kDSteps] = {};
  decode_read_pages(tab, first, end, pages, wave, a.pool_mask, pg);
  decode_issue(a, hk, pg, lds + gh::decode_stage_base(wave, 0), kf_next, lane);
  decode_read_pages(tab, first + 1, end, pages, wave, a.pool_mask, pg);
  for (uint32_t step = first; step < end; ++step) {
    const uint32_t buf = (step - first) & 1u;
    GH_LDS unsigned char* v_lds = lds + gh::decode_stage_base(wave, buf);
    // this step's stage and K have landed: this wave issued them itself
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    frag_u32x4_t kf[2][kDSteps];
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
      for (uint32_t ds = 0; ds < kDSteps; ++ds) kf[t][ds] = kf_next[t][ds];
    // step + 1 from the indices read a step ago, then the indices of step + 2
    decode_issue(a, hk, pg, lds + gh::decode_stage_base(wave, buf ^ 1u), kf_next, lane);
    decode_read_pages(tab, step + 2, end, pages, wave, a.pool_mask, pg);

    const uint32_t page0 = gh::kDecodeStepPages * step + 2 * wave;  // logical, of the sequence
    if (page0 >= pages) continue;  // both pages wholly past ctx: nothing was loaded
    const bool second = page0 + 1 < pages;

    // Sᵀ = K·Qᵀ: s[t][r] = Sᵀ[token 4 grp + r of page page0 + t][query i]
    frag_cd_t s[2];
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
      if (t == 1 && !second) {
        s[t] = frag_cd_t{kNegInf, kNegInf, kNegInf, kNegInf};
        continue;
      }
      s[t] = frag_cd_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (uint32_t ds = 0; ds < kDSteps; ++ds)
        s[t] = decode_mfma<DT>(__builtin_bit_cast(frag_t, kf[t][ds]), qf[ds], s[t]);
      const uint32_t key0 = (page0 + t) * gh::kDecodePageTokens;
      if (key0 + gh::kDecodePageTokens > ctx) {  // the page that straddles ctx
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
          if (key0 + 4 * grp + r >= ctx) s[t][r] = kNegInf;
      }
    }

    float block_max = s[0][0];
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) block_max = fmaxf(block_max, s[t][r]);
    block_max = decode_max_over_groups(block_max);  // finite: token 0 of page0 is a key
    const float m_new = fmaxf(m_run, block_max);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;

    float p_sum = 0.f;
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) {
        s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - m_new);  // p from here on; 0 where masked
        p_sum += s[t][r];
      }
    l_run = l_run * alpha + p_sum;
#pragma unroll
    for (uint32_t dt = 0; dt < kDTiles; ++dt)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) acc[dt][r] *= alpha;

    // O~ᵀ += Vᵀ·Pᵀ: k-slot t of lane group grp is key gh::attn_v_key(0, grp, t) of the chunk
    frag_t pf;
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) pf[t] = (elem_t)s[t / 4][t % 4];
#pragma unroll
    for (uint32_t dt = 0; dt < kDTiles; ++dt) {
      frag_i16x4_t half[2];
      half[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (GH_LDS frag_i16x4_t*)(v_lds + gh::decode_v_read(0, dt, grp, i)));
      half[1] = frag_i16x4_t{0, 0, 0, 0};  // an unloaded page: its part of the stage is stale
      if (second)
        half[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (GH_LDS frag_i16x4_t*)(v_lds + gh::decode_v_read(1, dt, grp, i)));
      const frag_t vf = __builtin_bit_cast(
          frag_t, __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7));
      acc[dt] = decode_mfma<DT>(vf, pf, acc[dt]);
    }
  }

  // the wave's partial into its own part of LDS: no load is in flight (the last
  // step issued none) and its reads of the stages have returned
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const float l_wave = decode_sum_over_groups(l_run);
#pragma unroll
  for (uint32_t dt = 0; dt < kDTiles; ++dt)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
      *(GH_LDS float*)(lds + gh::decode_epi_o(wave, 16 * dt + 4 * grp + r, i)) = acc[dt][r];
  if (grp == 0) {
    *(GH_LDS float*)(lds + gh::decode_epi_ml(wave, 0, i)) = m_run;
    *(GH_LDS float*)(lds + gh::decode_epi_ml(wave, 1, i)) = l_wave;
  }
  __syncthreads();

  float scale[gh::kDecodeWaves], m_all = kNegInf;
#pragma unroll
  for (uint32_t w = 0; w < gh::kDecodeWaves; ++w) {
    scale[w] = *(const GH_LDS float*)(lds + gh::decode_epi_ml(w, 0, i));
    m_all = fmaxf(m_all, scale[w]);
  }
#pragma unroll
  for (uint32_t w = 0; w < gh::kDecodeWaves; ++w)  // wave 0 saw a key: m_all is finite
    scale[w] = __builtin_amdgcn_exp2f(scale[w] - m_all);
#pragma unroll
  for (uint32_t h = 0; h < 2; ++h)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t d = 16 * (2 * wave + h) + 4 * grp + r;
      float o = 0.f;
#pragma unroll
      for (uint32_t w = 0; w < gh::kDecodeWaves; ++w)
        o += *(const GH_LDS float*)(lds + gh::decode_epi_o(w, d, i)) * scale[w];
      if (mine) out[d] = o;
    }
  if (wave == 0 && grp == 0 && mine) {
    float l = 0.f;
#pragma unroll
    for (uint32_t w = 0; w < gh::kDecodeWaves; ++w)
      l += *(const GH_LDS float*)(lds + gh::decode_epi_ml(w, 1, i)) * scale[w];
    out[kHeadDim] = m_all;
    out[kHeadDim + 1] = l;
  }
}

// block = one flat Q row, thread = one of the 130 columns
__global__ void decode_merge_kernel(const float* __restrict__ partial, uint32_t S,
                                    float* __restrict__ o, float* __restrict__ m,
                                    float* __restrict__ l) {
  const uint32_t row = blockIdx.x, col = threadIdx.x;
  if (col >= kCols) return;
  const float* mine = partial + (size_t)row * S * kCols;
  float m_all = -std::numeric_limits<float>::infinity();
  for (uint32_t s = 0; s < S; ++s) m_all = fmaxf(m_all, mine[s * kCols + kHeadDim]);
  if (col == kHeadDim) {
    m[row] = m_all;
    return;
  }
  float sum = 0.f;  // some split holds a key: m_all is finite, an empty split scales by 0
  for (uint32_t s = 0; s < S; ++s)
    sum += mine[s * kCols + col] * __builtin_amdgcn_exp2f(mine[s * kCols + kHeadDim] - m_all);
  if (col < kHeadDim) o[(size_t)row * kHeadDim + col] = sum;
  else l[row] = sum;
}

// poison over `words` dwords of a pool; the table, whole: every logical page of
// every sequence has its place, owned or not
__global__ void decode_poison_kernel(uint32_t* __restrict__ k, uint32_t* __restrict__ v,
                                     uint64_t words, int32_t* __restrict__ table,
                                     uint32_t entries, uint32_t pool_pages, uint32_t seed) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t p = first; p < words; p += stride)
    k[p] = v[p] = gh::kDecodePoison | gh::kDecodePoison << 16;
  for (uint64_t p = first; p < entries; p += stride)
    table[p] = (int32_t)gh::decode_page_of(seed, pool_pages, (uint32_t)p);
}

// Q whole, and the slots of K and V that a sequence owns, through the table;
// two 16-bit elements per store. grid.y is the KV row b · kv_heads + hk.
__global__ void decode_fill_kernel(uint32_t* __restrict__ q, uint32_t* __restrict__ k,
                                   uint32_t* __restrict__ v, const int32_t* __restrict__ table,
                                   const uint32_t* __restrict__ ctx, int dtype, uint32_t seed,
                                   uint32_t kv_heads, uint32_t group, uint32_t max_pages) {
  const uint32_t kvrow = blockIdx.y, b = kvrow / kv_heads, hk = kvrow % kv_heads;
  const uint32_t hq = gh::gemm_matrix_hash(seed, dtype, gh::GEN_Q);
  const uint32_t hkey = gh::gemm_matrix_hash(seed, dtype, gh::GEN_KEY);
  const uint32_t hv = gh::gemm_matrix_hash(seed, dtype, gh::GEN_V);
  constexpr uint32_t per_row = kHeadDim / 2;
  const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (uint32_t p = first; p < group * per_row; p += stride) {
    const uint32_t row = kvrow * group + p / per_row, col = 2 * (p % per_row);
    q[(size_t)row * per_row + col / 2] =
        (uint32_t)gh::gemm_encode(dtype, gh::attn_q_of(hq, row, col)) |
        (uint32_t)gh::gemm_encode(dtype, gh::attn_q_of(hq, row, col + 1)) << 16;
  }
  for (uint32_t p = first; p < ctx[b] * per_row; p += stride) {
    const uint32_t pos = p / per_row, col = 2 * (p % per_row);
    const uint32_t row = gh::decode_kv_row(kvrow, pos);
    const uint32_t page = (uint32_t)table[b * max_pages + pos / gh::kDecodePageTokens];
    const uint64_t at =
        gh::decode_pool_offset(page, kv_heads, hk, pos % gh::kDecodePageTokens, col) / 2;
    k[at] = (uint32_t)gh::gemm_encode(dtype, gh::attn128_k_of(hkey, row, col)) |
            (uint32_t)gh::gemm_encode(dtype, gh::attn128_k_of(hkey, row, col + 1)) << 16;
    v[at] = (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hv, row, col)) |
            (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hv, row, col + 1)) << 16;
  }
}

// One thread per element recomputes it from the generators in integer
// arithmetic. grid (rows, S + 1): y < S checks the partial of split y, y == S
// the final; a block is the 128 columns of O~ of one row, the threads of
// columns 0 and 1 also compare m and l. stats is [kv rows][S + 1]: slot
// (kvrow, s) is workgroup (kvrow, s) of the main kernel, slot (kvrow, S) the
// finals of that KV row. One atomic pair per wave that saw a mismatch.
__global__ void decode_check_kernel(const float* __restrict__ partial, const float* __restrict__ o,
                                    const float* __restrict__ m, const float* __restrict__ l,
                                    const uint32_t* __restrict__ ctx, int dtype, uint32_t seed,
                                    uint32_t kv_heads, uint32_t group, uint32_t S,
                                    TileStats* __restrict__ stats) {
  const uint32_t row = blockIdx.x, s = blockIdx.y, d = threadIdx.x, lane = threadIdx.x & 63u;
  const uint32_t kvrow = row / group, n = ctx[kvrow / kv_heads];
  const bool final_row = s == S;
  const gh::AttnExpected e = gh::decode_reference(
      seed, dtype, group, row, d, final_row ? 0u : gh::decode_split_key(n, S, s),
      final_row ? n : gh::decode_split_key(n, S, s + 1));
  const float* part = partial + ((size_t)row * S + s) * kCols;
  const float got_o = final_row ? o[(size_t)row * kHeadDim + d] : part[d];
  const float got_m = final_row ? m[row] : part[kHeadDim];
  const float got_l = final_row ? l[row] : part[kHeadDim + 1];
  const unsigned long long bad = __ballot(!(got_o == e.o));
  const unsigned long long bad_ml =
      __ballot((d == 0 && !(got_m == e.m)) || (d == 1 && !(got_l == e.l)));
  if ((bad | bad_ml) == 0 || lane != 0) return;
  TileStats* mine = stats + (size_t)kvrow * (S + 1) + s;
  atomicAdd(&mine->mismatches, (unsigned long long)(__popcll(bad) + __popcll(bad_ml)));
  const uint32_t col = bad ? d + (uint32_t)(__ffsll(bad) - 1)
                           : kHeadDim + (uint32_t)(__ffsll(bad_ml) - 1);
  atomicMin(&mine->first_bad, (unsigned long long)row * kCols + col);
}

}  // namespace

DecodeResult run_attn_decode_exact(int dtype, int64_t batch_in, int64_t kv_heads_in,
                                   int64_t group_in, int64_t max_ctx_in, int64_t splits_in,
                                   const std::vector<int64_t>& ctx_in, uint32_t seed,
                                   const AttnInject* inject, DecodeDump* dump) {
  if (dtype != gh::BF16 && dtype != gh::F16)
    throw std::invalid_argument("the decode attention check runs bf16 and f16 only");
  int device = 0, cu_total = 0;
  HIP_CHECK(hipGetDevice(&device));
  HIP_CHECK(hipDeviceGetAttribute(&cu_total, hipDeviceAttributeMultiprocessorCount, device));
  if (group_in == 0) group_in = kDecodeDefaultGroup;
  if (kv_heads_in == 0) kv_heads_in = kDecodeDefaultKvHeads;
  if (max_ctx_in == 0) max_ctx_in = kDecodeDefaultCtx;
  if (group_in != 1 && group_in != 2 && group_in != 4 && group_in != 8 && group_in != 16)
    throw std::invalid_argument("group must be 1, 2, 4, 8 or 16");
  if (max_ctx_in < 1 || max_ctx_in > gh::kDecodeMaxCtx)
    throw std::invalid_argument(
        "max_ctx must be in [1, 4096]: beyond it the sums are not exact in fp32");
  if (kv_heads_in < 1 || kv_heads_in > gh::kDecodeMaxKvRows)
    throw std::invalid_argument("kv_heads must be in [1, 32768]");
  if (splits_in == 0) splits_in = kDecodeDefaultSplits;
  if (splits_in < 1 || splits_in > gh::kDecodeMaxSplits)
    throw std::invalid_argument("splits must be in [1, 32]");
  if (batch_in == 0) {  // every CU gets kWorkgroupsPerCu workgroups
    const int64_t per_seq = splits_in * kv_heads_in;
    batch_in = ctx_in.empty()
                   ? ((int64_t)kWorkgroupsPerCu * std::max(cu_total, 1) + per_seq - 1) / per_seq
                   : (int64_t)ctx_in.size();
  }
  if (batch_in < 1 || batch_in * kv_heads_in > gh::kDecodeMaxKvRows)
    throw std::invalid_argument("batch must be at least 1 and batch * kv_heads at most 32768");
  const uint32_t batch = (uint32_t)batch_in, kv_heads = (uint32_t)kv_heads_in;
  const uint32_t group = (uint32_t)group_in, max_ctx = (uint32_t)max_ctx_in;
  const uint32_t S = (uint32_t)splits_in, max_pages = gh::decode_pages(max_ctx);
  const uint32_t pool_pages = gh::decode_pool_pages(batch, max_pages);
  const uint64_t pool_elems = (uint64_t)pool_pages * kv_heads * gh::kDecodePageElems;
  if (4 * pool_elems > gh::kDecodeMaxPoolBytes)
    throw std::invalid_argument("the K and V pools together must be at most 1 GiB");
  if (!ctx_in.empty() && ctx_in.size() != batch)
    throw std::invalid_argument("ctx must have one entry a sequence");
  std::vector<uint32_t> ctx(batch);
  uint64_t keys = 0;
  for (uint32_t b = 0; b < batch; ++b) {
    if (!ctx_in.empty() && (ctx_in[b] < 1 || ctx_in[b] > max_ctx))
      throw std::invalid_argument("every ctx must be in [1, max_ctx]");
    ctx[b] = ctx_in.empty() ? gh::decode_default_ctx(seed, b, max_ctx) : (uint32_t)ctx_in[b];
    keys += ctx[b];
  }
  const uint32_t kvrows = batch * kv_heads, rows = kvrows * group, workgroups = kvrows * S;
  if (inject) {
    if (inject->which < ATTN_Q || inject->which > ATTN_TABLE)
      throw std::invalid_argument("injected matrix must be q, k, v or table");
    bool inside;
    if (inject->which == ATTN_Q)
      inside = inject->row < rows && inject->col < kHeadDim;
    else if (inject->which == ATTN_TABLE)  // (sequence, logical page), mask below the pool
      inside = inject->row < batch && inject->col < max_pages && inject->mask < pool_pages;
    else  // the logical row of gh::decode_kv_row: an owned position
      inside = inject->row / gh::kDecodeMaxCtx < kvrows &&
               inject->row % gh::kDecodeMaxCtx < ctx[inject->row / gh::kDecodeMaxCtx / kv_heads] &&
               inject->col < kHeadDim;
    if (!inside) throw std::invalid_argument("injected element is outside what the check owns");
    if (inject->mask == 0 || inject->mask > 0xFFFFu)
      throw std::invalid_argument("xor mask must be a non-zero 16-bit value");
  }

  DeviceScope scope;
  const size_t q_bytes = (size_t)rows * kHeadDim * 2, pool_bytes = (size_t)pool_elems * 2;
  const size_t table_bytes = (size_t)batch * max_pages * sizeof(int32_t);
  const size_t partial_bytes = (size_t)rows * S * kCols * sizeof(float);
  const size_t o_bytes = (size_t)rows * kHeadDim * sizeof(float), ml_bytes = rows * sizeof(float);
  const size_t n_stats = (size_t)kvrows * (S + 1);
  uint16_t* d_q = (uint16_t*)scope.alloc(q_bytes);
  uint16_t* d_k = (uint16_t*)scope.alloc(pool_bytes);
  uint16_t* d_v = (uint16_t*)scope.alloc(pool_bytes);
  int32_t* d_table = (int32_t*)scope.alloc(table_bytes);
  uint32_t* d_ctx = (uint32_t*)scope.alloc(batch * sizeof(uint32_t));
  float* d_partial = (float*)scope.alloc(partial_bytes);
  float* d_o = (float*)scope.alloc(o_bytes);
  float* d_m = (float*)scope.alloc(ml_bytes);
  float* d_l = (float*)scope.alloc(ml_bytes);
  uint32_t* d_where = (uint32_t*)scope.alloc((size_t)workgroups * sizeof(uint32_t));
  TileStats* d_stats = (TileStats*)scope.alloc(n_stats * sizeof(TileStats));
  std::vector<TileStats> stats(n_stats, TileStats{0, kNoBadWord});
  HIP_CHECK(hipMemcpy(d_stats, stats.data(), n_stats * sizeof(TileStats), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_ctx, ctx.data(), batch * sizeof(uint32_t), hipMemcpyHostToDevice));
  // an element or a key the kernels did not write fails the compare / names no CU
  HIP_CHECK(hipMemset(d_partial, 0xFF, partial_bytes));
  HIP_CHECK(hipMemset(d_o, 0xFF, o_bytes));
  HIP_CHECK(hipMemset(d_m, 0xFF, ml_bytes));
  HIP_CHECK(hipMemset(d_l, 0xFF, ml_bytes));
  HIP_CHECK(hipMemset(d_where, 0xFF, (size_t)workgroups * sizeof(uint32_t)));

  hipLaunchKernelGGL(decode_poison_kernel,
                     dim3((unsigned)std::min<uint64_t>((pool_elems / 2 + 255) / 256, 4096)),
                     dim3(256), 0, 0, (uint32_t*)d_k, (uint32_t*)d_v, pool_elems / 2, d_table,
                     batch * max_pages, pool_pages, seed);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(decode_fill_kernel, dim3(16, kvrows), dim3(256), 0, 0, (uint32_t*)d_q,
                     (uint32_t*)d_k, (uint32_t*)d_v, d_table, d_ctx, dtype, seed, kv_heads, group,
                     max_pages);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (inject && inject->which == ATTN_TABLE) {
    int32_t* addr = d_table + (size_t)inject->row * max_pages + inject->col;
    int32_t entry = 0;
    HIP_CHECK(hipMemcpy(&entry, addr, 4, hipMemcpyDeviceToHost));
    entry ^= (int32_t)inject->mask;  // stays below the pool: the mask is
    HIP_CHECK(hipMemcpy(addr, &entry, 4, hipMemcpyHostToDevice));
  } else if (inject) {
    size_t element = (size_t)inject->row * kHeadDim + inject->col;  // of Q
    if (inject->which != ATTN_Q) {  // through the clean table
      const uint32_t kvrow = inject->row / gh::kDecodeMaxCtx, pos = inject->row % gh::kDecodeMaxCtx;
      const uint32_t page = gh::decode_page_of(
          seed, pool_pages, kvrow / kv_heads * max_pages + pos / gh::kDecodePageTokens);
      element = (size_t)gh::decode_pool_offset(page, kv_heads, kvrow % kv_heads,
                                               pos % gh::kDecodePageTokens, inject->col);
    }
    uint16_t* const base[3] = {d_q, d_k, d_v};
    // host read-xor-write of the dword that holds the element
    uint32_t* addr = (uint32_t*)base[inject->which] + element / 2;
    uint32_t word = 0;
    HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
    word ^= inject->mask << (16 * (element & 1u));
    HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
  }

  const DecodeArgs args{d_q, d_k, d_v, d_partial, d_where, kv_heads, group, max_pages,
                        pool_pages - 1u};
  const dim3 grid(S, kv_heads, batch);
  hipEvent_t t0 = scope.event(), t1 = scope.event(), t2 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  if (dtype == gh::BF16)
    hipLaunchKernelGGL((decode_kernel<gh::BF16>), grid, dim3(kDecodeThreads), 0, 0, args,
                       d_table, d_ctx);
  else
    hipLaunchKernelGGL((decode_kernel<gh::F16>), grid, dim3(kDecodeThreads), 0, 0, args,
                       d_table, d_ctx);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, 0));
  hipLaunchKernelGGL(decode_merge_kernel, dim3(rows), dim3(192), 0, 0, d_partial, S, d_o, d_m, d_l);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t2, 0));
  hipLaunchKernelGGL(decode_check_kernel, dim3(rows, S + 1), dim3(kHeadDim), 0, 0, d_partial, d_o,
                     d_m, d_l, d_ctx, dtype, seed, kv_heads, group, S, d_stats);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  float ms = 0.f, merge_ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventElapsedTime(&merge_ms, t1, t2));

  std::vector<uint32_t> where(workgroups);
  HIP_CHECK(hipMemcpy(stats.data(), d_stats, n_stats * sizeof(TileStats), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(where.data(), d_where, workgroups * sizeof(uint32_t), hipMemcpyDeviceToHost));

  DecodeResult res;
  res.dtype = dtype;
  res.m = rows, res.n = max_ctx, res.k = kHeadDim;
  res.batch = batch, res.kv_heads = kv_heads, res.group = group, res.splits = S;
  res.max_ctx = max_ctx;
  res.kv_bytes = 2 * keys * kv_heads * gh::kAttn128RowBytes;  // K and V rows a launch reads
  res.workgroups = (int)workgroups;
  res.cu_total = cu_total;
  res.elapsed_ms = ms;
  res.merge_ms = merge_ms;
  std::vector<uint32_t> seen(where);
  std::sort(seen.begin(), seen.end());
  res.cu_seen = (int)(std::unique(seen.begin(), seen.end()) - seen.begin());
  unsigned long long first = kNoBadWord;
  for (uint32_t kvrow = 0; kvrow < kvrows; ++kvrow) {
    const TileStats* mine = stats.data() + (size_t)kvrow * (S + 1);
    bool named = false;  // a bad partial names its workgroup and where it ran
    for (uint32_t s = 0; s < S; ++s) {
      if (mine[s].mismatches == 0) continue;
      res.faulty.push_back({kvrow, s, where[kvrow * S + s], mine[s]});
      named = true;
    }
    if (mine[S].mismatches == 0) continue;
    res.mismatches += mine[S].mismatches;  // the finals decide
    first = std::min(first, mine[S].first_bad);
    if (!named) res.faulty.push_back({kvrow, S, kDecodeNoCu, mine[S]});  // the merge: no CU
  }
  if (first < (unsigned long long)rows * kCols) {
    res.first_bad = (int64_t)first;
    const uint32_t row = (uint32_t)(first / kCols), col = (uint32_t)(first % kCols);
    const gh::AttnExpected e = gh::decode_reference(seed, dtype, group, row,
                                                    col < kHeadDim ? col : 0, 0,
                                                    ctx[row / group / kv_heads]);
    const float* src = col < kHeadDim ? d_o + (size_t)row * kHeadDim + col
                                      : (col == kHeadDim ? d_m : d_l) + row;
    HIP_CHECK(hipMemcpy(&res.got, src, 4, hipMemcpyDeviceToHost));
    res.expected = col < kHeadDim ? e.o : col == kHeadDim ? e.m : e.l;
  }
  if (dump) {
    dump->q = device_bytes(d_q, q_bytes);
    dump->k_pool = device_bytes(d_k, pool_bytes);
    dump->v_pool = device_bytes(d_v, pool_bytes);
    dump->table = device_bytes(d_table, table_bytes);
    dump->ctx = device_bytes(d_ctx, batch * sizeof(uint32_t));
    dump->partial = device_bytes(d_partial, partial_bytes);
    dump->o = device_bytes(d_o, o_bytes);
    dump->m = device_bytes(d_m, ml_bytes);
    dump->l = device_bytes(d_l, ml_bytes);
  }
  return res;
}

}  // namespace ghgemm
