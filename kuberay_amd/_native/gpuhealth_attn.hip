// gpuhealth_attn — the attention check of the MI355X (gfx950) burn-in: exact
// unnormalised single-head attention forward with online softmax, base 2, for
// bf16 and f16 on matrices in device memory. Bound to Python by gpuhealth.hip
// through gpuhealth_gemm.hpp; generators, the exactness premise, the reference
// and every LDS address function are in gpuhealth_ref.hpp. Built with the
// switches of gpuhealth_gemm.hip (build.py): packed fp32 arithmetic is disabled
// for the device code. Unlike the GEMM units this kernel does fp32 VALU
// arithmetic on accumulators, so here the switch is more than a guard.
//
// Burn-in, part 7. What the GEMM checks do not execute and an attention kernel
// does between its two matrix products: fp32 max / subtract / multiply / add on
// accumulators, the transcendental unit (v_exp_f32), a cross-lane exchange of
// accumulator rows (v_permlane16_swap / v_permlane32_swap), the packed
// down-conversion fp32 -> bf16 / f16, and the hand-over of one MFMA's
// accumulator registers as the next MFMA's operand without leaving the
// register file.
//
//   s = Q·Kᵀ,  m[i] = max_j s_ij,  l[i] = Σ_j 2^(s_ij - m_i),
//   O~[i][d] = Σ_j 2^(s_ij - m_i) · V[j][d]
//
// Q is M x 64, K and V are N x 64, row-major 16-bit; O~ (M x 64), m and l (M)
// are fp32, the form a flash-decoding split writes. Scale 1, base 2, no mask,
// no final division, head dimension 64 only.
//
// Work split: a workgroup of four waves owns 64 queries, a wave 16 of them, and
// walks K and V in blocks of 64 keys. The transposed-score form: the wave
// computes Sᵀ = K·Qᵀ, so that a lane's scores all belong to one query and P
// needs no LDS round trip on its way into the second product.
//
// Staging: a block is 8 KiB of K and 8 KiB of V; two stages make 32 KiB of LDS.
// global_load_lds_dwordx4 lays a wave's 1 KiB down contiguously, lane l at
// + 16 l, and the lane fetches the chunk that gh::attn_k_source /
// attn_v_source say belongs into its slot; wave w issues loads 2 w and 2 w + 1
// of K and of V. Loads of block b + 1 are issued, block b is computed, then
// s_waitcnt vmcnt(0) and one __syncthreads(), as in gpuhealth_gemm.hip. Each
// wave loads its Q fragments once, from device memory into registers: lane
// (i = l & 15, g = l >> 4) holds Q[q0 + i][32 ds + 8 g .. + 7] for ds = 0, 1.
//
// Scores: mfma_f32_16x16x32 with K rows as the A operand (ds_read_b128, the
// A-read of the GEMM check) and Q as the B operand, two d-steps for each of
// the four key tiles. Lane l then holds Sᵀ[key 16 kt + 4 g + r][query i],
// r = 0..3, kt = 0..3: 16 scores of query i; the query's other scores sit in
// lanes i + 16, i + 32 and i + 48.
//
// Softmax: the block maximum in-lane over the 16 scores, then across the four
// lane groups with v_permlane16_swap and v_permlane32_swap, both called with
// vdst = vsrc = x. Their lane maps, as debug_permlane_dump measures them
// (tests/test_gpu_attn_exact.py): the 16-lane swap exchanges rows 1 and 3 of
// vdst (lanes 16..31, 48..63) with rows 0 and 2 of vsrc, the 32-lane swap the
// upper half of vdst with the lower half of vsrc. With vdst = vsrc = x the two
// results of the first are (x of rows 0, 0, 2, 2) and (x of rows 1, 1, 3, 3),
// their maximum is that of rows 0 | 1 and of rows 2 | 3; the second swap does
// the same for the halves. The maps suit, so DPP is not used. Then
//   m_new = max(m_run, block max),  alpha = exp2(m_run - m_new),
//   p = exp2(s - m_new),  l = l·alpha + Σ p,  acc *= alpha
// with exp2 = __builtin_amdgcn_exp2f (v_exp_f32). m_run starts at -inf, for
// which the first alpha is exp2(-inf) = 0 and multiplies zeros. v_exp_f32 on
// the integers 0 .. -126 and on -inf is measured by debug_exp2_dump and is
// exact there (2^n, and 0), so production uses the exp unit and v_ldexp_f32 is
// not needed. l is kept per lane (the lane's own 16 keys of every block) and
// summed across the lane groups once, in the epilogue.
//
// Hand-over: p is converted to bf16 / f16 in registers (v_cvt_pk_bf16_f32 /
// v_cvt_f16_f32); the 8 values a lane holds for a 32-key chunk c, key tiles 2 c
// and 2 c + 1 times four registers, are the B operand Pᵀ of the second product
// as they stand: k-slot t of lane group g is key gh::attn_v_key(c, g, t).
//
// Second product: O~ᵀ += Vᵀ·Pᵀ, four d-tiles times two chunks a block. Vᵀ is
// the A operand, two ds_read_b64_tr_b16 per fragment from the row-major V
// stage at gh::attn_v_read, whose rows follow P's register order (not the
// GEMM's 8 g + 4 h + e); the V swizzle is derived for that in gpuhealth_ref.hpp.
//
// Epilogue: lane l holds O~ᵀ[d = 16 dt + 4 g + r][query i] and stores O~, lane
// group 0 stores m and l, all plain vector stores; lane 0 of wave 0 stores the
// location key. No workgroup waits on another.
//
// The fill uses dword stores only. The check recomputes every element of O~, m
// and l from the generators in integer arithmetic (gh::attn_reference), one
// thread per element of O~, and compares with ==.

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

constexpr int kAttnThreads = 256;
constexpr uint32_t kAttnStageBytes = 2 * gh::kAttnOperandBytes;  // K then V
constexpr uint32_t kAttnLdsBytes = 2 * kAttnStageBytes;          // 32 KiB

struct AttnArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  float* o;
  float* m;
  float* l;
  uint32_t* where;  // one location key per workgroup
  uint32_t n;
};

template <int DT> struct AttnFrag { typedef frag_bf16_t type; typedef __bf16 elem; };
template <> struct AttnFrag<gh::F16> { typedef frag_f16_t type; typedef _Float16 elem; };

template <int DT>
__device__ inline frag_cd_t attn_mfma(typename AttnFrag<DT>::type a, typename AttnFrag<DT>::type b,
                                      frag_cd_t c) {
  if constexpr (DT == gh::BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// this wave's four 1 KiB loads of key block `block`
__device__ inline void attn_issue_stage(const AttnArgs& a, uint32_t block,
                                        GH_LDS unsigned char* stage, uint32_t wave,
                                        uint32_t lane) {
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t q = 2 * wave + t;
    const uint16_t* src_k = a.k + gh::attn_global_offset(block, gh::attn_k_source(64 * q + lane));
    const uint16_t* src_v = a.v + gh::attn_global_offset(block, gh::attn_v_source(64 * q + lane));
    __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src_k,
                                     (GH_LDS void*)(stage + 1024 * q), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src_v,
                                     (GH_LDS void*)(stage + gh::kAttnOperandBytes + 1024 * q),
                                     16, 0, 0);
  }
}

// Both swaps with vdst = vsrc = x: element 0 and 1 of the result are the new
// vdst and vsrc. After the pair of them every lane has combined the x of lanes
// i, i + 16, i + 32 and i + 48 (the maps are in the comment at the top).
__device__ inline float attn_max_over_groups(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
  u = __builtin_bit_cast(uint32_t, x);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
}
__device__ inline float attn_sum_over_groups(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
  u = __builtin_bit_cast(uint32_t, x);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
}

template <int DT>
__global__ __launch_bounds__(kAttnThreads) void attn_exact_kernel(AttnArgs a) {
  static_assert(DT == gh::BF16 || DT == gh::F16, "the 16-bit paths only");
  typedef typename AttnFrag<DT>::type frag_t;
  typedef typename AttnFrag<DT>::elem elem_t;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kAttnLdsBytes];
  GH_LDS unsigned char* lds = (GH_LDS unsigned char*)lds_raw;

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = lane & 15u, grp = lane >> 4;
  const uint32_t query = blockIdx.x * gh::kAttnBlock + 16 * wave + i;  // this lane's

  frag_t qf[2];
#pragma unroll
  for (uint32_t ds = 0; ds < 2; ++ds)
    qf[ds] = __builtin_bit_cast(
        frag_t, *(const frag_u32x4_t*)(a.q + (size_t)query * gh::kAttnHeadDim + 32 * ds + 8 * grp));

  frag_cd_t acc[4];  // O~ᵀ, d-tile dt: [d = 16 dt + 4 grp + r][query]
#pragma unroll
  for (uint32_t dt = 0; dt < 4; ++dt) acc[dt] = frag_cd_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -std::numeric_limits<float>::infinity(), l_run = 0.f;

  const uint32_t blocks = a.n / gh::kAttnBlock;
  attn_issue_stage(a, 0, lds, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (uint32_t b = 0; b < blocks; ++b) {
    GH_LDS unsigned char* k_lds = lds + (b & 1u) * kAttnStageBytes;
    GH_LDS unsigned char* v_lds = k_lds + gh::kAttnOperandBytes;
    if (b + 1 < blocks)
      attn_issue_stage(a, b + 1, lds + ((b + 1) & 1u) * kAttnStageBytes, wave, lane);

    // Sᵀ = K·Qᵀ: s[kt][r] = Sᵀ[key 16 kt + 4 grp + r][query]
    frag_cd_t s[4];
#pragma unroll
    for (uint32_t kt = 0; kt < 4; ++kt) {
      s[kt] = frag_cd_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (uint32_t ds = 0; ds < 2; ++ds) {
        const frag_t kf = __builtin_bit_cast(
            frag_t, *(const GH_LDS frag_u32x4_t*)(k_lds + gh::attn_k_read(16 * kt + i, ds, grp)));
        s[kt] = attn_mfma<DT>(kf, qf[ds], s[kt]);
      }
    }

    float block_max = s[0][0];
#pragma unroll
    for (uint32_t kt = 0; kt < 4; ++kt)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) block_max = fmaxf(block_max, s[kt][r]);
    block_max = attn_max_over_groups(block_max);
    const float m_new = fmaxf(m_run, block_max);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;

    float p_sum = 0.f;
#pragma unroll
    for (uint32_t kt = 0; kt < 4; ++kt)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) {
        s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - m_new);  // p from here on
        p_sum += s[kt][r];
      }
    l_run = l_run * alpha + p_sum;
#pragma unroll
    for (uint32_t dt = 0; dt < 4; ++dt)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) acc[dt][r] *= alpha;

    // O~ᵀ += Vᵀ·Pᵀ: the lane's p of key tiles 2 c and 2 c + 1 are the B operand
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c) {
      frag_t pf;
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) pf[t] = (elem_t)s[2 * c + t / 4][t % 4];
#pragma unroll
      for (uint32_t dt = 0; dt < 4; ++dt) {
        frag_i16x4_t half[2];
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h)
          half[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (GH_LDS frag_i16x4_t*)(v_lds + gh::attn_v_read(c, h, dt, grp, i)));
        const frag_t vf = __builtin_bit_cast(
            frag_t, __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7));
        acc[dt] = attn_mfma<DT>(vf, pf, acc[dt]);
      }
    }
    // block b + 1 has landed (this wave's part, then everybody's) and block b
    // is no longer read: its buffer is the target of the next issue
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  const float l_row = attn_sum_over_groups(l_run);
#pragma unroll
  for (uint32_t dt = 0; dt < 4; ++dt)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
      a.o[(size_t)query * gh::kAttnHeadDim + 16 * dt + 4 * grp + r] = acc[dt][r];
  if (grp == 0) {
    a.m[query] = m_run;
    a.l[query] = l_row;
  }
  if (threadIdx.x == 0)
    a.where[blockIdx.x] =
        gh::location_key(gh::decode_location(read_xcc_id_reg(), read_hw_id_reg()));
}

// Q, K and V two 16-bit elements per store (rows are 64 elements)
__global__ void attn_fill_kernel(uint32_t* __restrict__ q, uint32_t* __restrict__ k,
                                 uint32_t* __restrict__ v, int dtype, uint32_t seed, uint32_t m,
                                 uint32_t n) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t hq = gh::gemm_matrix_hash(seed, dtype, gh::GEN_Q);
  const uint32_t hk = gh::gemm_matrix_hash(seed, dtype, gh::GEN_KEY);
  const uint32_t hv = gh::gemm_matrix_hash(seed, dtype, gh::GEN_V);
  constexpr uint32_t per_row = gh::kAttnHeadDim / 2;
  for (uint64_t p = first; p < (uint64_t)m * per_row; p += stride) {
    const uint32_t row = (uint32_t)(p / per_row), col = 2 * (uint32_t)(p % per_row);
    q[p] = (uint32_t)gh::gemm_encode(dtype, gh::attn_q_of(hq, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::attn_q_of(hq, row, col + 1)) << 16;
  }
  for (uint64_t p = first; p < (uint64_t)n * per_row; p += stride) {
    const uint32_t row = (uint32_t)(p / per_row), col = 2 * (uint32_t)(p % per_row);
    k[p] = (uint32_t)gh::gemm_encode(dtype, gh::attn_k_of(hk, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::attn_k_of(hk, row, col + 1)) << 16;
    v[p] = (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hv, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hv, row, col + 1)) << 16;
  }
}

// One thread per element of O~ recomputes it, and with it m and l of its row,
// from the generators in integer arithmetic, off the matrix pipe. A block is
// four queries of one 64-query tile, a wave one query: lane d compares
// O~[row][d], lanes 0 and 1 also m[row] and l[row]. One atomic pair per wave
// that saw a mismatch, none on a clean result.
__global__ void attn_check_kernel(const float* __restrict__ o, const float* __restrict__ m,
                                  const float* __restrict__ l, int dtype, uint32_t seed,
                                  uint32_t n, TileStats* __restrict__ stats) {
  const uint32_t tile = blockIdx.x / 16, part = blockIdx.x % 16;
  const uint32_t row = tile * gh::kAttnBlock + 4 * part + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  const gh::AttnExpected e = gh::attn_reference(seed, dtype, n, row, lane);
  const unsigned long long bad =
      __ballot(!(o[(size_t)row * gh::kAttnHeadDim + lane] == e.o));
  const unsigned long long bad_ml =
      __ballot((lane == 0 && !(m[row] == e.m)) || (lane == 1 && !(l[row] == e.l)));
  if ((bad | bad_ml) == 0 || lane != 0) return;
  atomicAdd(&stats[tile].mismatches, (unsigned long long)(__popcll(bad) + __popcll(bad_ml)));
  const uint32_t col = bad ? (uint32_t)(__ffsll(bad) - 1)
                           : gh::kAttnHeadDim + (uint32_t)(__ffsll(bad_ml) - 1);
  atomicMin(&stats[tile].first_bad, (unsigned long long)row * gh::kAttnOutCols + col);
}

}  // namespace

Result run_attn_exact(int dtype, int64_t m_in, int64_t n_in, uint32_t seed,
                      const AttnInject* inject, AttnDump* dump) {
  if (dtype != gh::BF16 && dtype != gh::F16)
    throw std::invalid_argument("the attention check runs bf16 and f16 only");
  int device = 0, cu_total = 0;
  HIP_CHECK(hipGetDevice(&device));
  HIP_CHECK(hipDeviceGetAttribute(&cu_total, hipDeviceAttributeMultiprocessorCount, device));
  if (m_in == 0) m_in = (int64_t)gh::kAttnBlock * kWorkgroupsPerCu * std::max(cu_total, 1);
  if (n_in == 0) n_in = kAttnDefaultN;
  if (m_in < 0 || n_in < 0 || m_in % gh::kAttnBlock || n_in % gh::kAttnBlock)
    throw std::invalid_argument("m and n must be positive multiples of 64");
  if (n_in > gh::kAttnMaxN)
    throw std::invalid_argument("n must be at most 4096: beyond it the sums are not exact in fp32");
  if (m_in > gh::kAttnMaxM) throw std::invalid_argument("m must be at most 65536");
  const uint32_t m = (uint32_t)m_in, n = (uint32_t)n_in, tiles = m / gh::kAttnBlock;
  if (inject) {
    if (inject->which < ATTN_Q || inject->which > ATTN_V)
      throw std::invalid_argument("injected matrix must be q, k or v");
    if (inject->row >= (inject->which == ATTN_Q ? m : n) || inject->col >= gh::kAttnHeadDim)
      throw std::invalid_argument("injected element is outside the matrix");
    if (inject->mask == 0 || inject->mask > 0xFFFFu)
      throw std::invalid_argument("xor mask must be a non-zero 16-bit value");
  }

  DeviceScope scope;
  const size_t q_bytes = (size_t)m * gh::kAttnHeadDim * 2, kv_bytes = (size_t)n * gh::kAttnHeadDim * 2;
  const size_t o_bytes = (size_t)m * gh::kAttnHeadDim * sizeof(float), ml_bytes = m * sizeof(float);
  uint16_t* d_q = (uint16_t*)scope.alloc(q_bytes);
  uint16_t* d_k = (uint16_t*)scope.alloc(kv_bytes);
  uint16_t* d_v = (uint16_t*)scope.alloc(kv_bytes);
  float* d_o = (float*)scope.alloc(o_bytes);
  float* d_m = (float*)scope.alloc(ml_bytes);
  float* d_l = (float*)scope.alloc(ml_bytes);
  uint32_t* d_where = (uint32_t*)scope.alloc((size_t)tiles * sizeof(uint32_t));
  TileStats* d_stats = (TileStats*)scope.alloc((size_t)tiles * sizeof(TileStats));
  std::vector<TileStats> stats(tiles, TileStats{0, kNoBadWord});
  HIP_CHECK(hipMemcpy(d_stats, stats.data(), tiles * sizeof(TileStats), hipMemcpyHostToDevice));
  // an element or a key the kernel did not write fails the compare / names no CU
  HIP_CHECK(hipMemset(d_o, 0xFF, o_bytes));
  HIP_CHECK(hipMemset(d_m, 0xFF, ml_bytes));
  HIP_CHECK(hipMemset(d_l, 0xFF, ml_bytes));
  HIP_CHECK(hipMemset(d_where, 0xFF, (size_t)tiles * sizeof(uint32_t)));

  const uint64_t fill_items = (uint64_t)std::max(m, n) * gh::kAttnHeadDim / 2;
  hipLaunchKernelGGL(attn_fill_kernel,
                     dim3((unsigned)std::min<uint64_t>((fill_items + 255) / 256, 4096)), dim3(256),
                     0, 0, (uint32_t*)d_q, (uint32_t*)d_k, (uint32_t*)d_v, dtype, seed, m, n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (inject) {
    uint16_t* const base[3] = {d_q, d_k, d_v};
    const size_t element = (size_t)inject->row * gh::kAttnHeadDim + inject->col;
    // host read-xor-write of the dword that holds the element
    uint32_t* addr = (uint32_t*)base[inject->which] + element / 2;
    uint32_t word = 0;
    HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
    word ^= inject->mask << (16 * (element & 1u));
    HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
  }

  const AttnArgs args{d_q, d_k, d_v, d_o, d_m, d_l, d_where, n};
  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  if (dtype == gh::BF16)
    hipLaunchKernelGGL((attn_exact_kernel<gh::BF16>), dim3(tiles), dim3(kAttnThreads), 0, 0, args);
  else
    hipLaunchKernelGGL((attn_exact_kernel<gh::F16>), dim3(tiles), dim3(kAttnThreads), 0, 0, args);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, 0));
  hipLaunchKernelGGL(attn_check_kernel, dim3(tiles * 16), dim3(256), 0, 0, d_o, d_m, d_l, dtype,
                     seed, n, d_stats);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));

  std::vector<uint32_t> where(tiles);
  HIP_CHECK(hipMemcpy(stats.data(), d_stats, tiles * sizeof(TileStats), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(where.data(), d_where, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));

  Result res;
  res.dtype = dtype;
  res.m = m, res.n = n, res.k = gh::kAttnHeadDim;
  res.workgroups = (int)tiles;
  res.cu_total = cu_total;
  res.elapsed_ms = ms;
  std::vector<uint32_t> keys(where);
  std::sort(keys.begin(), keys.end());
  res.cu_seen = (int)(std::unique(keys.begin(), keys.end()) - keys.begin());
  unsigned long long first = kNoBadWord;
  for (uint32_t t = 0; t < tiles; ++t) {
    if (stats[t].mismatches == 0) continue;
    res.mismatches += stats[t].mismatches;
    first = std::min(first, stats[t].first_bad);
    res.faulty.push_back({t, 0, where[t], stats[t]});
  }
  if (first < (unsigned long long)m * gh::kAttnOutCols) {
    res.first_bad = (int64_t)first;
    const uint32_t row = (uint32_t)(first / gh::kAttnOutCols), col = (uint32_t)(first % gh::kAttnOutCols);
    const gh::AttnExpected e =
        gh::attn_reference(seed, dtype, n, row, col < gh::kAttnHeadDim ? col : 0);
    const float* src = col < gh::kAttnHeadDim ? d_o + (size_t)row * gh::kAttnHeadDim + col
                                              : (col == gh::kAttnHeadDim ? d_m : d_l) + row;
    HIP_CHECK(hipMemcpy(&res.got, src, 4, hipMemcpyDeviceToHost));
    res.expected = col < gh::kAttnHeadDim ? e.o : col == gh::kAttnHeadDim ? e.m : e.l;
  }
  if (dump) {
    dump->q = device_bytes(d_q, q_bytes);
    dump->k = device_bytes(d_k, kv_bytes);
    dump->v = device_bytes(d_v, kv_bytes);
    dump->o = device_bytes(d_o, o_bytes);
    dump->m = device_bytes(d_m, ml_bytes);
    dump->l = device_bytes(d_l, ml_bytes);
  }
  return res;
}

// Test hook, and how the lane maps in the comment at the top were learned: one
// wave, vdst = lane and vsrc = 64 + lane, so a value says where it came from.
__global__ __launch_bounds__(64) void permlane_dump_kernel(uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  const auto r16 = __builtin_amdgcn_permlane16_swap(lane, 64u + lane, false, false);
  const auto r32 = __builtin_amdgcn_permlane32_swap(lane, 64u + lane, false, false);
  out[lane] = r16[0];
  out[64 + lane] = r16[1];
  out[128 + lane] = r32[0];
  out[192 + lane] = r32[1];
}

std::vector<std::vector<int>> run_debug_permlane_dump() {
  DeviceScope scope;
  uint32_t* d_out = (uint32_t*)scope.alloc(256 * sizeof(uint32_t));
  HIP_CHECK(hipMemset(d_out, 0xFF, 256 * sizeof(uint32_t)));
  hipLaunchKernelGGL(permlane_dump_kernel, dim3(1), dim3(64), 0, 0, d_out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  uint32_t host[256];
  HIP_CHECK(hipMemcpy(host, d_out, sizeof(host), hipMemcpyDeviceToHost));
  std::vector<std::vector<int>> out(4, std::vector<int>(64));
  for (int part = 0; part < 4; ++part)
    for (int l = 0; l < 64; ++l) out[part][l] = (int)host[64 * part + l];
  return out;
}

// Test hook: v_exp_f32 of -t for t = 0..126 and of -inf (t = 127), two a lane
__global__ __launch_bounds__(64) void exp2_dump_kernel(float* __restrict__ out) {
  for (uint32_t t = threadIdx.x; t < 128; t += 64)
    out[t] = __builtin_amdgcn_exp2f(t < 127 ? -(float)t : -std::numeric_limits<float>::infinity());
}

std::vector<float> run_debug_exp2_dump() {
  DeviceScope scope;
  float* d_out = (float*)scope.alloc(128 * sizeof(float));
  HIP_CHECK(hipMemset(d_out, 0xFF, 128 * sizeof(float)));
  hipLaunchKernelGGL(exp2_dump_kernel, dim3(1), dim3(64), 0, 0, d_out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<float> out(128);
  HIP_CHECK(hipMemcpy(out.data(), d_out, 128 * sizeof(float), hipMemcpyDeviceToHost));
  return out;
}

}  // namespace ghgemm
