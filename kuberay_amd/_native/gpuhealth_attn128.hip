// gpuhealth_attn128 — the causal attention check of the MI355X (gfx950)
// burn-in: exact unnormalised multi-head attention forward at head dimension
// 128 with a causal mask, online softmax, base 2, for bf16 and f16 on matrices
// in device memory. Bound to Python by gpuhealth.hip through
// gpuhealth_gemm.hpp; generators, the exactness premise with the mask, the
// reference, the work split and every LDS address function are in
// gpuhealth_ref.hpp. Built with the switches of gpuhealth_attn.hip (build.py):
// packed fp32 arithmetic is disabled for the device code.
//
// Burn-in, part 8. What the attention check of part 7 (gpuhealth_attn.hip,
// one head, head dimension 64, no mask) does not execute and a causal LLM
// attention does: LDS rows of 256 bytes that span all 64 banks, -inf as an
// operand of v_max_f32 and v_exp_f32, wave-uniform branches around MFMAs and
// LDS reads, 32 accumulator registers of O~ live across them, and a
// two-dimensional grid with per-head offsets.
//
//   s_ij = Q[hL + i]·K[hL + j],  j visible to i: !causal || j <= i
//   m[i] = max_j s_ij,  l[i] = Σ_j 2^(s_ij - m_i),  O~[i][d] = Σ_j 2^(s_ij - m_i) · V[hL + j][d]
//
// over the visible keys j of the query's own head. Q, K and V are [H·L, 128]
// row-major 16-bit; O~ ([H·L, 128]), m and l ([H·L]) are fp32. Scale 1, base
// 2. The final division O~ / l stays out: v_rcp_f32 is not exact, and the
// check compares with ==. causal = false is a debug setting that tells a
// fault of the mask from one of the wider rows.
//
// Work split: the grid is (L / 128, H). With nb = L / 64 query blocks a head,
// an even number, workgroup (pair, h) of four waves takes query blocks pair
// and nb - 1 - pair of head h, one after the other. Under the mask query block
// qb needs key blocks 0 .. qb, so every workgroup walks (pair + 1) + (nb -
// pair) = nb + 1 key blocks: equal work, no CU idles behind the long rows. A
// wave owns 16 queries of the query block and computes Sᵀ = K·Qᵀ, as part 7
// does, so that a lane's scores all belong to one query and P needs no LDS
// round trip on its way into the second product.
//
// Masking, three levels:
//   * key blocks beyond the diagonal (kb > qb) are neither loaded nor computed;
//   * in the diagonal block (kb == qb) wave w's queries are 16 w .. 16 w + 15
//     of the block and key tile kt is keys 16 kt .. + 15: a tile with kt > w is
//     masked for all of the wave's queries, its four MFMAs are skipped and its
//     scores are -inf (wave is in an SGPR, the branch is wave-uniform); a
//     32-key chunk c of P with 2 c > w is all zero and the chunk's 16 LDS
//     reads and 8 MFMAs of the second product are skipped the same way;
//   * the straddling tile kt == w is computed and gets -inf per element where
//     key 4 g + r > query i, before the maximum.
// m_run starts at -inf. Key 0 of the head is visible to every query, and a
// row's first step is always key block 0, so the first block maximum is finite:
// the first alpha is exp2(-inf - finite) = 0 on zeros, a masked p is
// exp2(-inf - finite) = 0, and -inf - -inf never occurs. From the second step
// on m_run is finite. v_exp_f32(-inf) = +0 is measured by debug_exp2_dump.
//
// Staging: a stage is 64 keys, 16 KiB of K and 16 KiB of V in rows of 256
// bytes; two stages make 64 KiB of LDS, so kWorkgroupsPerCu = 2 workgroups fit
// into a CU's 160 KiB. global_load_lds_dwordx4 lays a wave's 1 KiB down
// contiguously, lane l at + 16 l, and the lane fetches the chunk that
// gh::attn128_k_source / attn128_v_source say belongs into its slot (the
// swizzle is chosen on the global side); wave w issues loads 4 w .. 4 w + 3 of
// K and of V. A step issues the loads of the next step, computes its own, then
// s_waitcnt vmcnt(0) and one __syncthreads(). The double buffer runs on across
// the two query blocks: the steps of a workgroup are numbered through, stage =
// step & 1, and the last step of the first query block issues key block 0 of
// the second. Each wave loads its Q fragments once per query block, from
// device memory into registers: lane (i = l & 15, g = l >> 4) holds
// Q[query i][32 ds + 8 g .. + 7] for ds = 0..3.
//
// Scores: mfma_f32_16x16x32 with K rows as the A operand (ds_read_b128 at
// gh::attn128_k_read) and Q as the B operand, four d-steps for each of the four
// key tiles. Lane l then holds Sᵀ[key 16 kt + 4 g + r][query i], r = 0..3.
//
// Softmax: as part 7. The block maximum in-lane, then across the four lane
// groups with v_permlane16_swap and v_permlane32_swap at vdst = vsrc (lane
// maps measured by debug_permlane_dump), m_new = max(m_run, block max), alpha
// = exp2(m_run - m_new), p = exp2(s - m_new) with v_exp_f32, l kept per lane
// and summed across the groups in the epilogue.
//
// Second product: O~ᵀ += Vᵀ·Pᵀ, eight d-tiles (32 accumulator registers) times
// two chunks a step. p converted to bf16 / f16 in registers is the B operand
// as it stands (k-slot t of lane group g is key gh::attn_v_key(c, g, t)); Vᵀ is
// the A operand, two ds_read_b64_tr_b16 per fragment at gh::attn128_v_read.
//
// Epilogue, per query block: lane l holds O~ᵀ[d = 16 dt + 4 g + r][query i] and
// stores O~, lane group 0 stores m and l, plain vector stores. Lane 0 of wave 0
// stores the workgroup's location key at the end. No workgroup waits on
// another.
//
// The fill uses dword stores only. The check recomputes every element of O~, m
// and l from the generators in integer arithmetic (gh::attn128_reference), one
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

constexpr int kAttn128Threads = 256;
constexpr uint32_t kAttn128StageBytes = 2 * gh::kAttn128OperandBytes;  // K then V: 32 KiB
constexpr uint32_t kAttn128LdsBytes = 2 * kAttn128StageBytes;          // 64 KiB
constexpr uint32_t kDTiles = gh::kAttn128HeadDim / 16;                 // 8 d-tiles of O~ᵀ
constexpr uint32_t kDSteps = gh::kAttn128HeadDim / 32;                 // 4 d-steps of a score

struct Attn128Args {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  float* o;
  float* m;
  float* l;
  uint32_t* where;  // one location key per workgroup
  uint32_t L;
  uint32_t causal;
};

template <int DT> struct Attn128Frag { typedef frag_bf16_t type; typedef __bf16 elem; };
template <> struct Attn128Frag<gh::F16> { typedef frag_f16_t type; typedef _Float16 elem; };

template <int DT>
__device__ inline frag_cd_t attn128_mfma(typename Attn128Frag<DT>::type a,
                                         typename Attn128Frag<DT>::type b, frag_cd_t c) {
  if constexpr (DT == gh::BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// this wave's eight 1 KiB loads of the key block that starts at flat row first_row
__device__ inline void attn128_issue_stage(const Attn128Args& a, uint32_t first_row,
                                           GH_LDS unsigned char* stage, uint32_t wave,
                                           uint32_t lane) {
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t q = 4 * wave + t;
    const uint16_t* src_k =
        a.k + gh::attn128_global_offset(first_row, gh::attn128_k_source(64 * q + lane));
    const uint16_t* src_v =
        a.v + gh::attn128_global_offset(first_row, gh::attn128_v_source(64 * q + lane));
    __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src_k,
                                     (GH_LDS void*)(stage + 1024 * q), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src_v,
                                     (GH_LDS void*)(stage + gh::kAttn128OperandBytes + 1024 * q),
                                     16, 0, 0);
  }
}

// Both swaps with vdst = vsrc = x, as in gpuhealth_attn.hip: after the pair of
// them every lane has combined the x of lanes i, i + 16, i + 32 and i + 48.
__device__ inline float attn128_max_over_groups(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
  u = __builtin_bit_cast(uint32_t, x);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
}
__device__ inline float attn128_sum_over_groups(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
  u = __builtin_bit_cast(uint32_t, x);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
}

template <int DT>
__global__ __launch_bounds__(kAttn128Threads) void attn128_kernel(Attn128Args a) {
  static_assert(DT == gh::BF16 || DT == gh::F16, "the 16-bit paths only");
  typedef typename Attn128Frag<DT>::type frag_t;
  typedef typename Attn128Frag<DT>::elem elem_t;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kAttn128LdsBytes];
  GH_LDS unsigned char* lds = (GH_LDS unsigned char*)lds_raw;
  constexpr float kNegInf = -std::numeric_limits<float>::infinity();

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = lane & 15u, grp = lane >> 4;
  const uint32_t nb = a.L / gh::kAttn128Block, pair = blockIdx.x;
  const uint32_t head_row = blockIdx.y * a.L;  // the head's first flat row
  const bool causal = a.causal != 0;
  const uint32_t total = gh::attn128_key_blocks(nb, gh::attn128_query_block(nb, pair, 0), causal) +
                         gh::attn128_key_blocks(nb, gh::attn128_query_block(nb, pair, 1), causal);

  uint32_t step = 0;  // numbered through both query blocks: stage = step & 1
  attn128_issue_stage(a, head_row, lds, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (uint32_t phase = 0; phase < 2; ++phase) {
    const uint32_t qb = gh::attn128_query_block(nb, pair, phase);
    const uint32_t blocks = gh::attn128_key_blocks(nb, qb, causal);
    const uint32_t query = head_row + qb * gh::kAttn128Block + 16 * wave + i;  // this lane's

    frag_t qf[kDSteps];
#pragma unroll
    for (uint32_t ds = 0; ds < kDSteps; ++ds)
      qf[ds] = __builtin_bit_cast(
          frag_t,
          *(const frag_u32x4_t*)(a.q + (size_t)query * gh::kAttn128HeadDim + 32 * ds + 8 * grp));

    frag_cd_t acc[kDTiles];  // O~ᵀ, d-tile dt: [d = 16 dt + 4 grp + r][query]
#pragma unroll
    for (uint32_t dt = 0; dt < kDTiles; ++dt) acc[dt] = frag_cd_t{0.f, 0.f, 0.f, 0.f};
    float m_run = kNegInf, l_run = 0.f;

    for (uint32_t kb = 0; kb < blocks; ++kb, ++step) {
      GH_LDS unsigned char* k_lds = lds + (step & 1u) * kAttn128StageBytes;
      GH_LDS unsigned char* v_lds = k_lds + gh::kAttn128OperandBytes;
      if (step + 1 < total)  // the next key block, or key block 0 of the second query block
        attn128_issue_stage(a, head_row + (kb + 1 < blocks ? kb + 1 : 0) * gh::kAttn128Block,
                            lds + ((step + 1) & 1u) * kAttn128StageBytes, wave, lane);
      const bool diagonal = causal && kb == qb;

      // Sᵀ = K·Qᵀ: s[kt][r] = Sᵀ[key 16 kt + 4 grp + r][query]
      frag_cd_t s[4];
#pragma unroll
      for (uint32_t kt = 0; kt < 4; ++kt) {
        if (diagonal && kt > wave) {  // every key of the tile lies above the wave's queries
          s[kt] = frag_cd_t{kNegInf, kNegInf, kNegInf, kNegInf};
          continue;
        }
        s[kt] = frag_cd_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t ds = 0; ds < kDSteps; ++ds) {
          const frag_t kf = __builtin_bit_cast(
              frag_t,
              *(const GH_LDS frag_u32x4_t*)(k_lds + gh::attn128_k_read(16 * kt + i, ds, grp)));
          s[kt] = attn128_mfma<DT>(kf, qf[ds], s[kt]);
        }
        if (diagonal && kt == wave) {  // the tile that straddles the diagonal
#pragma unroll
          for (uint32_t r = 0; r < 4; ++r)
            if (4 * grp + r > i) s[kt][r] = kNegInf;
        }
      }

      float block_max = s[0][0];
#pragma unroll
      for (uint32_t kt = 0; kt < 4; ++kt)
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) block_max = fmaxf(block_max, s[kt][r]);
      block_max = attn128_max_over_groups(block_max);
      const float m_new = fmaxf(m_run, block_max);  // finite: key 0 is visible to every query
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;

      float p_sum = 0.f;
#pragma unroll
      for (uint32_t kt = 0; kt < 4; ++kt)
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
          s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - m_new);  // p from here on; 0 where masked
          p_sum += s[kt][r];
        }
      l_run = l_run * alpha + p_sum;
#pragma unroll
      for (uint32_t dt = 0; dt < kDTiles; ++dt)
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) acc[dt][r] *= alpha;

      // O~ᵀ += Vᵀ·Pᵀ: the lane's p of key tiles 2 c and 2 c + 1 are the B operand
#pragma unroll
      for (uint32_t c = 0; c < 2; ++c) {
        if (diagonal && 2 * c > wave) continue;  // both tiles masked: p is all zero
        frag_t pf;
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) pf[t] = (elem_t)s[2 * c + t / 4][t % 4];
#pragma unroll
        for (uint32_t dt = 0; dt < kDTiles; ++dt) {
          frag_i16x4_t half[2];
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h)
            half[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (GH_LDS frag_i16x4_t*)(v_lds + gh::attn128_v_read(c, h, dt, grp, i)));
          const frag_t vf = __builtin_bit_cast(
              frag_t, __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7));
          acc[dt] = attn128_mfma<DT>(vf, pf, acc[dt]);
        }
      }
      // the next step's stage has landed (this wave's part, then everybody's)
      // and this step's is no longer read: it is the target of the next issue
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }

    const float l_row = attn128_sum_over_groups(l_run);
#pragma unroll
    for (uint32_t dt = 0; dt < kDTiles; ++dt)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r)
        a.o[(size_t)query * gh::kAttn128HeadDim + 16 * dt + 4 * grp + r] = acc[dt][r];
    if (grp == 0) {
      a.m[query] = m_run;
      a.l[query] = l_row;
    }
  }
  if (threadIdx.x == 0)
    a.where[blockIdx.y * gridDim.x + pair] =
        gh::location_key(gh::decode_location(read_xcc_id_reg(), read_hw_id_reg()));
}

// Q, K and V two 16-bit elements per store (rows are 128 elements)
__global__ void attn128_fill_kernel(uint32_t* __restrict__ q, uint32_t* __restrict__ k,
                                    uint32_t* __restrict__ v, int dtype, uint32_t seed,
                                    uint32_t rows) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t hq = gh::gemm_matrix_hash(seed, dtype, gh::GEN_Q);
  const uint32_t hk = gh::gemm_matrix_hash(seed, dtype, gh::GEN_KEY);
  const uint32_t hv = gh::gemm_matrix_hash(seed, dtype, gh::GEN_V);
  constexpr uint32_t per_row = gh::kAttn128HeadDim / 2;
  for (uint64_t p = first; p < (uint64_t)rows * per_row; p += stride) {
    const uint32_t row = (uint32_t)(p / per_row), col = 2 * (uint32_t)(p % per_row);
    q[p] = (uint32_t)gh::gemm_encode(dtype, gh::attn_q_of(hq, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::attn_q_of(hq, row, col + 1)) << 16;
    k[p] = (uint32_t)gh::gemm_encode(dtype, gh::attn128_k_of(hk, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::attn128_k_of(hk, row, col + 1)) << 16;
    v[p] = (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hv, row, col)) |
           (uint32_t)gh::gemm_encode(dtype, gh::gemm_int_of(hv, row, col + 1)) << 16;
  }
}

// One thread per element of O~ recomputes it, and with it m and l of its row,
// from the generators in integer arithmetic, off the matrix pipe. A block is
// two flat rows, a row two waves of 64 columns: the thread of column d compares
// O~[row][d], those of columns 0 and 1 also m[row] and l[row]. The statistics
// are kept per workgroup of the attention kernel (gh::attn128_workgroup_of).
// One atomic pair per wave that saw a mismatch, none on a clean result.
__global__ void attn128_check_kernel(const float* __restrict__ o, const float* __restrict__ m,
                                     const float* __restrict__ l, int dtype, uint32_t seed,
                                     uint32_t L, uint32_t causal, TileStats* __restrict__ stats) {
  const uint32_t row = 2 * blockIdx.x + (threadIdx.x >> 7);
  const uint32_t d = threadIdx.x & 127u, lane = threadIdx.x & 63u;
  const gh::AttnExpected e = gh::attn128_reference(seed, dtype, L, causal != 0, row, d);
  const unsigned long long bad =
      __ballot(!(o[(size_t)row * gh::kAttn128HeadDim + d] == e.o));
  const unsigned long long bad_ml =
      __ballot((d == 0 && !(m[row] == e.m)) || (d == 1 && !(l[row] == e.l)));
  if ((bad | bad_ml) == 0 || lane != 0) return;
  TileStats* mine = stats + gh::attn128_workgroup_of(L, row);
  atomicAdd(&mine->mismatches, (unsigned long long)(__popcll(bad) + __popcll(bad_ml)));
  const uint32_t col = bad ? d + (uint32_t)(__ffsll(bad) - 1)
                           : gh::kAttn128HeadDim + (uint32_t)(__ffsll(bad_ml) - 1);
  atomicMin(&mine->first_bad, (unsigned long long)row * gh::kAttn128OutCols + col);
}

}  // namespace

Result run_attn128_exact(int dtype, int64_t heads_in, int64_t l_in, bool causal, uint32_t seed,
                         const AttnInject* inject, AttnDump* dump) {
  if (dtype != gh::BF16 && dtype != gh::F16)
    throw std::invalid_argument("the causal attention check runs bf16 and f16 only");
  int device = 0, cu_total = 0;
  HIP_CHECK(hipGetDevice(&device));
  HIP_CHECK(hipDeviceGetAttribute(&cu_total, hipDeviceAttributeMultiprocessorCount, device));
  if (l_in == 0) l_in = kAttn128DefaultL;
  if (l_in < 0 || l_in % (2 * gh::kAttn128Block))
    throw std::invalid_argument("seq must be a positive multiple of 128");
  if (l_in > gh::kAttn128MaxL)
    throw std::invalid_argument("seq must be at most 4096: beyond it the sums are not exact in fp32");
  const int64_t pairs = l_in / (2 * gh::kAttn128Block);  // workgroups of a head
  if (heads_in == 0)
    heads_in = ((int64_t)kWorkgroupsPerCu * std::max(cu_total, 1) + pairs - 1) / pairs;
  if (heads_in < 1) throw std::invalid_argument("heads must be at least 1");
  if (heads_in > gh::kAttn128MaxRows || heads_in * l_in > gh::kAttn128MaxRows)
    throw std::invalid_argument("heads * seq must be at most 131072");
  const uint32_t heads = (uint32_t)heads_in, L = (uint32_t)l_in, rows = heads * L;
  const uint32_t workgroups = heads * (uint32_t)pairs;
  if (inject) {
    if (inject->which < ATTN_Q || inject->which > ATTN_V)
      throw std::invalid_argument("injected matrix must be q, k or v");
    if (inject->row >= rows || inject->col >= gh::kAttn128HeadDim)
      throw std::invalid_argument("injected element is outside the matrix");
    if (inject->mask == 0 || inject->mask > 0xFFFFu)
      throw std::invalid_argument("xor mask must be a non-zero 16-bit value");
  }

  DeviceScope scope;
  const size_t qkv_bytes = (size_t)rows * gh::kAttn128HeadDim * 2;
  const size_t o_bytes = (size_t)rows * gh::kAttn128HeadDim * sizeof(float);
  const size_t ml_bytes = (size_t)rows * sizeof(float);
  uint16_t* d_q = (uint16_t*)scope.alloc(qkv_bytes);
  uint16_t* d_k = (uint16_t*)scope.alloc(qkv_bytes);
  uint16_t* d_v = (uint16_t*)scope.alloc(qkv_bytes);
  float* d_o = (float*)scope.alloc(o_bytes);
  float* d_m = (float*)scope.alloc(ml_bytes);
  float* d_l = (float*)scope.alloc(ml_bytes);
  uint32_t* d_where = (uint32_t*)scope.alloc((size_t)workgroups * sizeof(uint32_t));
  TileStats* d_stats = (TileStats*)scope.alloc((size_t)workgroups * sizeof(TileStats));
  std::vector<TileStats> stats(workgroups, TileStats{0, kNoBadWord});
  HIP_CHECK(hipMemcpy(d_stats, stats.data(), workgroups * sizeof(TileStats), hipMemcpyHostToDevice));
  // an element or a key the kernel did not write fails the compare / names no CU
  HIP_CHECK(hipMemset(d_o, 0xFF, o_bytes));
  HIP_CHECK(hipMemset(d_m, 0xFF, ml_bytes));
  HIP_CHECK(hipMemset(d_l, 0xFF, ml_bytes));
  HIP_CHECK(hipMemset(d_where, 0xFF, (size_t)workgroups * sizeof(uint32_t)));

  const uint64_t fill_items = (uint64_t)rows * gh::kAttn128HeadDim / 2;
  hipLaunchKernelGGL(attn128_fill_kernel,
                     dim3((unsigned)std::min<uint64_t>((fill_items + 255) / 256, 4096)), dim3(256),
                     0, 0, (uint32_t*)d_q, (uint32_t*)d_k, (uint32_t*)d_v, dtype, seed, rows);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (inject) {
    uint16_t* const base[3] = {d_q, d_k, d_v};
    const size_t element = (size_t)inject->row * gh::kAttn128HeadDim + inject->col;
    // host read-xor-write of the dword that holds the element
    uint32_t* addr = (uint32_t*)base[inject->which] + element / 2;
    uint32_t word = 0;
    HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
    word ^= inject->mask << (16 * (element & 1u));
    HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
  }

  const Attn128Args args{d_q, d_k, d_v, d_o, d_m, d_l, d_where, L, causal ? 1u : 0u};
  const dim3 grid((unsigned)pairs, heads);
  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  if (dtype == gh::BF16)
    hipLaunchKernelGGL((attn128_kernel<gh::BF16>), grid, dim3(kAttn128Threads), 0, 0, args);
  else
    hipLaunchKernelGGL((attn128_kernel<gh::F16>), grid, dim3(kAttn128Threads), 0, 0, args);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, 0));
  hipLaunchKernelGGL(attn128_check_kernel, dim3(rows / 2), dim3(256), 0, 0, d_o, d_m, d_l, dtype,
                     seed, L, causal ? 1u : 0u, d_stats);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));

  std::vector<uint32_t> where(workgroups);
  HIP_CHECK(hipMemcpy(stats.data(), d_stats, workgroups * sizeof(TileStats), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(where.data(), d_where, workgroups * sizeof(uint32_t), hipMemcpyDeviceToHost));

  Result res;
  res.dtype = dtype;
  res.m = heads, res.n = L, res.k = gh::kAttn128HeadDim;
  res.workgroups = (int)workgroups;
  res.cu_total = cu_total;
  res.elapsed_ms = ms;
  std::vector<uint32_t> keys(where);
  std::sort(keys.begin(), keys.end());
  res.cu_seen = (int)(std::unique(keys.begin(), keys.end()) - keys.begin());
  unsigned long long first = kNoBadWord;
  for (uint32_t t = 0; t < workgroups; ++t) {
    if (stats[t].mismatches == 0) continue;
    res.mismatches += stats[t].mismatches;
    first = std::min(first, stats[t].first_bad);
    res.faulty.push_back({t, 0, where[t], stats[t]});
  }
  if (first < (unsigned long long)rows * gh::kAttn128OutCols) {
    res.first_bad = (int64_t)first;
    const uint32_t row = (uint32_t)(first / gh::kAttn128OutCols);
    const uint32_t col = (uint32_t)(first % gh::kAttn128OutCols);
    const gh::AttnExpected e = gh::attn128_reference(seed, dtype, L, causal, row,
                                                     col < gh::kAttn128HeadDim ? col : 0);
    const float* src = col < gh::kAttn128HeadDim
                           ? d_o + (size_t)row * gh::kAttn128HeadDim + col
                           : (col == gh::kAttn128HeadDim ? d_m : d_l) + row;
    HIP_CHECK(hipMemcpy(&res.got, src, 4, hipMemcpyDeviceToHost));
    res.expected = col < gh::kAttn128HeadDim ? e.o : col == gh::kAttn128HeadDim ? e.m : e.l;
  }
  if (dump) {
    dump->q = device_bytes(d_q, qkv_bytes);
    dump->k = device_bytes(d_k, qkv_bytes);
    dump->v = device_bytes(d_v, qkv_bytes);
    dump->o = device_bytes(d_o, o_bytes);
    dump->m = device_bytes(d_m, ml_bytes);
    dump->l = device_bytes(d_l, ml_bytes);
  }
  return res;
}

}  // namespace ghgemm
