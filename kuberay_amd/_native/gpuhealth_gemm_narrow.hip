// gpuhealth_gemm_narrow — the narrow GEMM check of the MI355X (gfx950)
// burn-in: exact D = A·B + C for fp8 (OCP e4m3) and MXFP4 (e2m1 with one E8M0
// scale per 32 of K) on matrices in device memory. Bound to Python by
// gpuhealth.hip through gpuhealth_gemm.hpp; layouts, generators, the exactness
// premise and every LDS address function are in gpuhealth_ref.hpp. Built with
// the switches of gpuhealth_gemm.hip (build.py), for the reason given there.
//
// Burn-in, part 6. The work is tiled as in part 5 (gpuhealth_gemm.hip): a
// workgroup of four waves owns a 64 x 64 tile of D, a wave a 32 x 32 quadrant
// as 2 x 2 MFMA tiles whose accumulators start as C. Two LDS stages of 16 KiB,
// 8 KiB of A and 8 KiB of B each, behind s_waitcnt vmcnt(0) and one barrier; no
// workgroup waits on another. A stage is 128 bytes of every A row: 128 of K
// for fp8, 256 of K for mxfp4.
//
// Staging is one function over bytes for both types: global_load_lds_dwordx4
// takes 16 bytes from each lane's own global address and lays the wave's 1 KiB
// down contiguously, lane l at + 16 l, so slot 64 q + l of load q is filled
// with the chunk that gh::narrow_a_source / narrow_b_source say belongs there:
// the LDS layout and its swizzle are chosen on the global side. Wave w issues
// loads 2 w and 2 w + 1 of A and of B per stage.
//
// Operand reads (lane l, i = l & 15, g = l >> 4; the MFMA maps of part 2):
//   fp8, mfma_f32_16x16x32_fp8_fp8, four k-steps per stage; byte j of the
//   64-bit operand is k = 8 g + j.
//     A fragment: one ds_read_b64 of row i (gh::narrow_a_read).
//     B fragment: one ds_read_b64_tr_b8 (gh::narrow_b_read).
//   mxfp4, mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 4 and opsel 0,
//   two k-steps per stage; nibble j of VGPRs 0..3 is k = 32 g + j, VGPRs 4..7
//   are zero.
//     A fragment: one ds_read_b128 of row i.
//     B fragment: two ds_read_b64_tr_b4, 16 of k each.
//     Scales do not go through LDS: at MFMA step T of the whole K loop lane
//     (i, g) loads the bytes SA[row][4 T + g] and SB[4 T + g][col] from device
//     memory into a register with plain loads, the way kernels with
//     pre-shuffled scales feed the instruction. Scale staging through LDS is
//     not done.
// Lane maps of the two transposed reads, measured with debug_lds_tr_dump(bits=8)
// and (bits=4) before the GEMM ran at all and pinned by
// tests/test_gpu_gemm_narrow.py; both stay within a group of 16 lanes
// (b = l & ~15, i = l & 15), every lane hands in the address of 8 bytes:
//   tr_b8: out[l] byte e   = byte i % 8 of in[b + 2 e + i / 8],  e = 0..7
//   tr_b4: out[l] nibble e = nibble i   of in[b + e],            e = 0..15
// So the 8 x 16 byte block (16 x 16 nibble block) the 16 lanes point at row by
// row comes back transposed, column i to lane i: a row-major B gives k along
// the register, as the MFMA wants. gh::narrow_b_read derives the addresses from
// these maps (gh::narrow_tr8_source / narrow_tr4_source are their formulas), and
// tests/native/gemm_narrow_ref_check.cpp composes placement, read address and
// map on the host: every address in bounds and every register position the
// element the MFMA map wants.
//
// Epilogue and location key as in part 5. The fill uses dword stores only; the
// check recomputes every element of D from the generators in integer
// arithmetic, one thread per element, and compares with ==.

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

typedef __attribute__((ext_vector_type(4))) float frag_cd_t;
typedef __attribute__((ext_vector_type(2))) int frag_i32x2_t;
typedef __attribute__((ext_vector_type(4))) int frag_i32x4_t;
typedef __attribute__((ext_vector_type(8))) int frag_i32x8_t;

constexpr int kNarrowThreads = 256;
constexpr uint32_t kNarrowStageBytes = 2 * gh::kNarrowOperandBytes;  // A then B
constexpr uint32_t kNarrowLdsBytes = 2 * kNarrowStageBytes;          // 32 KiB

struct NarrowArgs {
  const unsigned char* a;
  const unsigned char* b;
  const unsigned char* sa;  // mxfp4 only
  const unsigned char* sb;
  const float* c;
  float* d;
  uint32_t* where;  // one location key per workgroup
  uint32_t n, k, tiles_n;
};

// this wave's four 1 KiB loads of stage s (128 bytes of every A row from byte
// 128 s, narrow_stage_k rows of B from row narrow_stage_k s)
template <int DT>
__device__ inline void narrow_issue_stage(const NarrowArgs& g, uint32_t m0, uint32_t n0, uint32_t s,
                                          GH_LDS unsigned char* stage, uint32_t wave,
                                          uint32_t lane) {
  constexpr uint32_t per = gh::narrow_per_byte(DT);
  const size_t a_row_bytes = g.k / per, b_row_bytes = g.n / per;
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t q = 2 * wave + t;
    const gh::NarrowChunk ca = gh::narrow_a_source(64 * q + lane);
    const gh::NarrowChunk cb = gh::narrow_b_source(DT, 64 * q + lane);
    const unsigned char* src_a = g.a + (size_t)(m0 + ca.row) * a_row_bytes + 128 * (size_t)s + ca.byte;
    const unsigned char* src_b = g.b + ((size_t)s * gh::narrow_stage_k(DT) + cb.row) * b_row_bytes +
                                 n0 / per + cb.byte;
    __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src_a,
                                     (GH_LDS void*)(stage + 1024 * q), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const GH_GLOBAL void*)src_b,
                                     (GH_LDS void*)(stage + gh::kNarrowOperandBytes + 1024 * q),
                                     16, 0, 0);
  }
}

template <int DT>
__global__ __launch_bounds__(kNarrowThreads) void gemm_narrow_kernel(NarrowArgs g) {
  static_assert(DT == gh::FP8 || DT == gh::MXFP4, "the 8-bit and 4-bit paths only");
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kNarrowLdsBytes];
  GH_LDS unsigned char* lds = (GH_LDS unsigned char*)lds_raw;

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = lane & 15u, grp = lane >> 4;
  const uint32_t m0 = (blockIdx.x / g.tiles_n) * gh::kGemmTile;
  const uint32_t n0 = (blockIdx.x % g.tiles_n) * gh::kGemmTile;
  const uint32_t wrow = 32 * (wave >> 1), wcol = 32 * (wave & 1u);  // the wave's quadrant

  frag_cd_t acc[2][2];
#pragma unroll
  for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
    for (uint32_t tn = 0; tn < 2; ++tn)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r)
        acc[tm][tn][r] = g.c[(size_t)(m0 + wrow + 16 * tm + 4 * grp + r) * g.n + n0 + wcol +
                             16 * tn + i];

  const uint32_t stages = g.k / gh::narrow_stage_k(DT);
  narrow_issue_stage<DT>(g, m0, n0, 0, lds, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (uint32_t s = 0; s < stages; ++s) {
    GH_LDS unsigned char* a_lds = lds + (s & 1u) * kNarrowStageBytes;
    GH_LDS unsigned char* b_lds = a_lds + gh::kNarrowOperandBytes;
    if (s + 1 < stages)
      narrow_issue_stage<DT>(g, m0, n0, s + 1, lds + ((s + 1) & 1u) * kNarrowStageBytes, wave,
                             lane);
    if constexpr (DT == gh::FP8) {
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        long a[2], b[2];
#pragma unroll
        for (uint32_t tm = 0; tm < 2; ++tm)
          a[tm] = *(const GH_LDS long*)(a_lds + gh::narrow_a_read(DT, wrow + 16 * tm + i, t, grp));
#pragma unroll
        for (uint32_t tn = 0; tn < 2; ++tn)
          b[tn] = __builtin_bit_cast(
              long, __builtin_amdgcn_ds_read_tr8_b64_v2i32((GH_LDS frag_i32x2_t*)(
                        b_lds + gh::narrow_b_read(DT, wcol + 16 * tn, t, grp, 0, i))));
#pragma unroll
        for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
          for (uint32_t tn = 0; tn < 2; ++tn)
            acc[tm][tn] =
                __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t) {
        frag_i32x8_t a[2], b[2];
        int sa[2], sb[2];
        const uint32_t block = 4 * (2 * s + t) + grp;  // of 32 along K
#pragma unroll
        for (uint32_t tm = 0; tm < 2; ++tm) {
          const uint32_t row = wrow + 16 * tm + i;
          const frag_i32x4_t lo =
              *(const GH_LDS frag_i32x4_t*)(a_lds + gh::narrow_a_read(DT, row, t, grp));
          a[tm] = frag_i32x8_t{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
          sa[tm] = g.sa[(size_t)(m0 + row) * (g.k / 32) + block];
        }
#pragma unroll
        for (uint32_t tn = 0; tn < 2; ++tn) {
          const uint32_t col = wcol + 16 * tn;
          frag_i32x2_t half[2];
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h)
            half[h] = __builtin_amdgcn_ds_read_tr4_b64_v2i32(
                (GH_LDS frag_i32x2_t*)(b_lds + gh::narrow_b_read(DT, col, t, grp, h, i)));
          b[tn] = frag_i32x8_t{half[0][0], half[0][1], half[1][0], half[1][1], 0, 0, 0, 0};
          sb[tn] = g.sb[(size_t)block * g.n + n0 + col + i];
        }
#pragma unroll
        for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
          for (uint32_t tn = 0; tn < 2; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                a[tm], b[tn], acc[tm][tn], 4, 4, 0, sa[tm], 0, sb[tn]);
      }
    }
    // stage s + 1 has landed (this wave's part, then everybody's) and stage s
    // is no longer read: its buffer is the target of the next issue
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

#pragma unroll
  for (uint32_t tm = 0; tm < 2; ++tm)
#pragma unroll
    for (uint32_t tn = 0; tn < 2; ++tn)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r)
        g.d[(size_t)(m0 + wrow + 16 * tm + 4 * grp + r) * g.n + n0 + wcol + 16 * tn + i] =
            acc[tm][tn][r];
  if (threadIdx.x == 0)
    g.where[blockIdx.x] =
        gh::location_key(gh::decode_location(read_xcc_id_reg(), read_hw_id_reg()));
}

// the dword at byte offset 4 p of a rows x row_bytes operand matrix
__device__ inline uint32_t narrow_operand_dword(uint32_t hash, int dtype, uint64_t p,
                                                uint32_t row_bytes) {
  const uint32_t row = (uint32_t)(4 * p / row_bytes), byte = (uint32_t)(4 * p % row_bytes);
  uint32_t word = 0;
  for (uint32_t j = 0; j < 4; ++j)
    word |= (uint32_t)gh::narrow_operand_byte(hash, dtype, row,
                                              (byte + j) * gh::narrow_per_byte(dtype)) << (8 * j);
  return word;
}
__device__ inline uint32_t narrow_scale_dword(uint32_t hash, uint64_t p, uint32_t row_bytes) {
  const uint32_t row = (uint32_t)(4 * p / row_bytes), col = (uint32_t)(4 * p % row_bytes);
  uint32_t word = 0;
  for (uint32_t j = 0; j < 4; ++j) word |= gh::gemm_scale_of(hash, row, col + j) << (8 * j);
  return word;
}

// Dword stores only: every row of A, B, SA and SB is a multiple of 4 bytes
// (K / 32 is a multiple of 8 for mxfp4). sa and sb are null for fp8.
__global__ void gemm_narrow_fill_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                        uint32_t* __restrict__ sa, uint32_t* __restrict__ sb,
                                        float* __restrict__ c, int dtype, uint32_t seed,
                                        uint32_t m, uint32_t n, uint32_t k) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t per = gh::narrow_per_byte(dtype);
  const uint32_t ha = gh::gemm_matrix_hash(seed, dtype, gh::GEN_A);
  const uint32_t hb = gh::gemm_matrix_hash(seed, dtype, gh::GEN_B);
  const uint32_t hc = gh::gemm_matrix_hash(seed, dtype, gh::GEN_C);
  for (uint64_t p = first; p < (uint64_t)m * (k / per) / 4; p += stride)
    a[p] = narrow_operand_dword(ha, dtype, p, k / per);
  for (uint64_t p = first; p < (uint64_t)k * (n / per) / 4; p += stride)
    b[p] = narrow_operand_dword(hb, dtype, p, n / per);
  for (uint64_t p = first; p < (uint64_t)m * n; p += stride)
    c[p] = (float)gh::gemm_int_of(hc, (uint32_t)(p / n), (uint32_t)(p % n));
  if (dtype != gh::MXFP4) return;
  const uint32_t hsa = gh::gemm_matrix_hash(seed, dtype, gh::GEN_SA);
  const uint32_t hsb = gh::gemm_matrix_hash(seed, dtype, gh::GEN_SB);
  for (uint64_t p = first; p < (uint64_t)m * (k / 32) / 4; p += stride)
    sa[p] = narrow_scale_dword(hsa, p, k / 32);
  for (uint64_t p = first; p < (uint64_t)(k / 32) * n / 4; p += stride)
    sb[p] = narrow_scale_dword(hsb, p, n);
}

// As gemm_check_kernel: one thread per element of D recomputes it from the
// generators in integer arithmetic, a wave is one row of a tile.
__global__ void gemm_narrow_check_kernel(const float* __restrict__ d, int dtype, uint32_t seed,
                                         uint32_t n, uint32_t k, uint32_t tiles_n,
                                         TileStats* __restrict__ stats) {
  const uint32_t tile = blockIdx.x / 16, part = blockIdx.x % 16;
  const uint32_t row = (tile / tiles_n) * gh::kGemmTile + 4 * part + (threadIdx.x >> 6);
  const uint32_t col0 = (tile % tiles_n) * gh::kGemmTile, lane = threadIdx.x & 63u;
  const float expected = gh::gemm_narrow_reference(seed, dtype, k, row, col0 + lane);
  const unsigned long long bad = __ballot(!(d[(size_t)row * n + col0 + lane] == expected));
  if (bad == 0 || lane != 0) return;
  atomicAdd(&stats[tile].mismatches, (unsigned long long)__popcll(bad));
  atomicMin(&stats[tile].first_bad,
            (unsigned long long)row * n + col0 + (unsigned long long)(__ffsll(bad) - 1));
}

}  // namespace

Result run_gemm_narrow_exact(int dtype, int64_t m_in, int64_t n_in, int64_t k_in, uint32_t seed,
                             const NarrowInject* inject, NarrowDump* dump) {
  if (dtype != gh::FP8 && dtype != gh::MXFP4)
    throw std::invalid_argument("the narrow GEMM check runs fp8 and mxfp4 only");
  const bool mx = dtype == gh::MXFP4;
  const int64_t stage_k = gh::narrow_stage_k(dtype), max_k = gh::narrow_max_k(dtype);
  int device = 0, cu_total = 0;
  HIP_CHECK(hipGetDevice(&device));
  HIP_CHECK(hipDeviceGetAttribute(&cu_total, hipDeviceAttributeMultiprocessorCount, device));
  uint32_t side = 1;
  while ((uint64_t)side * side < (uint64_t)kWorkgroupsPerCu * (uint64_t)std::max(cu_total, 1))
    ++side;
  if (m_in == 0) m_in = (int64_t)side * gh::kGemmTile;
  if (n_in == 0) n_in = (int64_t)side * gh::kGemmTile;
  if (k_in == 0) k_in = kDefaultK;
  if (m_in < 0 || n_in < 0 || m_in % gh::kGemmTile || n_in % gh::kGemmTile)
    throw std::invalid_argument("m and n must be positive multiples of 64");
  if (k_in < 0 || k_in % stage_k)
    throw std::invalid_argument("k must be a positive multiple of the stage depth: 128 for fp8, "
                                "256 for mxfp4");
  if (k_in > max_k)
    throw std::invalid_argument("k must be at most 65536 for fp8 and 4096 for mxfp4: beyond it "
                                "the sums are not exact in fp32");
  if (m_in > gh::kGemmMaxMN || n_in > gh::kGemmMaxMN)
    throw std::invalid_argument("m and n must be at most 65536");
  const uint32_t m = (uint32_t)m_in, n = (uint32_t)n_in, k = (uint32_t)k_in;
  const uint32_t tiles_n = n / gh::kGemmTile, tiles = (m / gh::kGemmTile) * tiles_n;
  const uint32_t per = gh::narrow_per_byte(dtype);
  // rows and columns, in elements, of what an inject may name
  const uint32_t rows_of[4] = {m, k, m, k / 32}, cols_of[4] = {k, n, k / 32, n};
  if (inject) {
    const bool scale = inject->which == NARROW_SA || inject->which == NARROW_SB;
    if (inject->which < NARROW_A || inject->which > NARROW_SB || (scale && !mx))
      throw std::invalid_argument("injected matrix must be a or b, or for mxfp4 sa or sb");
    if (inject->row >= rows_of[inject->which] || inject->col >= cols_of[inject->which])
      throw std::invalid_argument("injected element is outside the matrix");
    if (inject->mask == 0 || inject->mask > (mx && !scale ? 0xFu : 0xFFu))
      throw std::invalid_argument("xor mask must be a non-zero value of 8 bits, or of 4 bits for "
                                  "an e2m1 code");
  }

  DeviceScope scope;
  const size_t a_bytes = (size_t)m * k / per, b_bytes = (size_t)k * n / per;
  const size_t sa_bytes = mx ? (size_t)m * (k / 32) : 0, sb_bytes = mx ? (size_t)(k / 32) * n : 0;
  const size_t cd_bytes = (size_t)m * n * sizeof(float);
  unsigned char* d_a = (unsigned char*)scope.alloc(a_bytes);
  unsigned char* d_b = (unsigned char*)scope.alloc(b_bytes);
  unsigned char* d_sa = mx ? (unsigned char*)scope.alloc(sa_bytes) : nullptr;
  unsigned char* d_sb = mx ? (unsigned char*)scope.alloc(sb_bytes) : nullptr;
  float* d_c = (float*)scope.alloc(cd_bytes);
  float* d_d = (float*)scope.alloc(cd_bytes);
  uint32_t* d_where = (uint32_t*)scope.alloc((size_t)tiles * sizeof(uint32_t));
  TileStats* d_stats = (TileStats*)scope.alloc((size_t)tiles * sizeof(TileStats));
  std::vector<TileStats> stats(tiles, TileStats{0, kNoBadWord});
  HIP_CHECK(hipMemcpy(d_stats, stats.data(), tiles * sizeof(TileStats),
                      hipMemcpyHostToDevice));
  // an element or a key the GEMM did not write fails the compare / names no CU
  HIP_CHECK(hipMemset(d_d, 0xFF, cd_bytes));
  HIP_CHECK(hipMemset(d_where, 0xFF, (size_t)tiles * sizeof(uint32_t)));

  const uint64_t fill_items = std::max<uint64_t>((uint64_t)m * n, std::max(a_bytes, b_bytes) / 4);
  hipLaunchKernelGGL(gemm_narrow_fill_kernel,
                     dim3((unsigned)std::min<uint64_t>((fill_items + 255) / 256, 4096)), dim3(256),
                     0, 0, (uint32_t*)d_a, (uint32_t*)d_b, (uint32_t*)d_sa, (uint32_t*)d_sb, d_c,
                     dtype, seed, m, n, k);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (inject) {
    unsigned char* const base[4] = {d_a, d_b, d_sa, d_sb};
    const bool scale = inject->which >= NARROW_SA;
    // in elements; a dword holds 4 bytes or 8 e2m1 codes
    const size_t element = (size_t)inject->row * cols_of[inject->which] + inject->col;
    const uint32_t bits = mx && !scale ? 4 : 8, per_dword = 32 / bits;
    // host read-xor-write of the dword that holds the element
    uint32_t* addr = (uint32_t*)base[inject->which] + element / per_dword;
    uint32_t word = 0;
    HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
    word ^= inject->mask << (bits * (uint32_t)(element % per_dword));
    HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
  }

  const NarrowArgs args{d_a, d_b, d_sa, d_sb, d_c, d_d, d_where, n, k, tiles_n};
  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  if (mx)
    hipLaunchKernelGGL((gemm_narrow_kernel<gh::MXFP4>), dim3(tiles), dim3(kNarrowThreads), 0, 0,
                       args);
  else
    hipLaunchKernelGGL((gemm_narrow_kernel<gh::FP8>), dim3(tiles), dim3(kNarrowThreads), 0, 0,
                       args);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, 0));
  hipLaunchKernelGGL(gemm_narrow_check_kernel, dim3(tiles * 16), dim3(256), 0, 0, d_d, dtype, seed,
                     n, k, tiles_n, d_stats);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));

  std::vector<uint32_t> where(tiles);
  HIP_CHECK(hipMemcpy(stats.data(), d_stats, tiles * sizeof(TileStats),
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(where.data(), d_where, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));

  Result res;
  res.dtype = dtype;
  res.m = m, res.n = n, res.k = k;
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
    res.faulty.push_back({t / tiles_n, t % tiles_n, where[t], stats[t]});
  }
  if (first < (unsigned long long)m * n) {
    res.first_bad = (int64_t)first;
    HIP_CHECK(hipMemcpy(&res.got, d_d + first, 4, hipMemcpyDeviceToHost));
    res.expected = gh::gemm_narrow_reference(seed, dtype, k, (uint32_t)(first / n),
                                             (uint32_t)(first % n));
  }
  if (dump) {
    dump->a = device_bytes(d_a, a_bytes);
    dump->b = device_bytes(d_b, b_bytes);
    dump->c = device_bytes(d_c, cd_bytes);
    dump->d = device_bytes(d_d, cd_bytes);
    if (mx) {
      dump->sa = device_bytes(d_sa, sa_bytes);
      dump->sb = device_bytes(d_sb, sb_bytes);
    }
  }
  return res;
}

// Test hook, and how the two lane maps in the comment at the top were learned.
// One wave, lane l reads through the transposed read from byte 8 l of 512
// bytes. A byte or a nibble cannot hold its own index (9 and 10 bits), so the
// kernel runs once per slice of the index, each element of the LDS holding
// bits `shift` and up of its index, and the host puts the slices together.
template <int BITS>
__global__ __launch_bounds__(64) void lds_tr_narrow_dump_kernel(uint32_t* __restrict__ out,
                                                                uint32_t shift) {
  __shared__ __attribute__((aligned(16))) uint32_t words[128];
  const uint32_t lane = threadIdx.x;
  constexpr uint32_t per_dword = 32 / BITS, mask = (1u << BITS) - 1u;
  for (uint32_t w = lane; w < 128; w += 64) {
    uint32_t word = 0;
    for (uint32_t j = 0; j < per_dword; ++j)
      word |= (((per_dword * w + j) >> shift) & mask) << (BITS * j);
    words[w] = word;
  }
  __syncthreads();
  GH_LDS frag_i32x2_t* src = (GH_LDS frag_i32x2_t*)((GH_LDS unsigned char*)words + 8 * lane);
  frag_i32x2_t v;
  if constexpr (BITS == 8)
    v = __builtin_amdgcn_ds_read_tr8_b64_v2i32(src);
  else
    v = __builtin_amdgcn_ds_read_tr4_b64_v2i32(src);
  out[2 * lane] = (uint32_t)v[0];
  out[2 * lane + 1] = (uint32_t)v[1];
}

std::vector<std::vector<int>> run_debug_lds_tr_dump_narrow(int bits) {
  if (bits != 8 && bits != 4) throw std::invalid_argument("bits must be 16, 8 or 4");
  DeviceScope scope;
  uint32_t* d_out = (uint32_t*)scope.alloc(128 * sizeof(uint32_t));
  const int per_lane = 64 / bits, index_bits = bits == 8 ? 9 : 10;
  std::vector<std::vector<int>> out(64, std::vector<int>(per_lane, 0));
  for (int shift = 0; shift < index_bits; shift += bits) {
    HIP_CHECK(hipMemset(d_out, 0xFF, 128 * sizeof(uint32_t)));
    if (bits == 8)
      hipLaunchKernelGGL(lds_tr_narrow_dump_kernel<8>, dim3(1), dim3(64), 0, 0, d_out,
                         (uint32_t)shift);
    else
      hipLaunchKernelGGL(lds_tr_narrow_dump_kernel<4>, dim3(1), dim3(64), 0, 0, d_out,
                         (uint32_t)shift);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    uint32_t host[128];
    HIP_CHECK(hipMemcpy(host, d_out, sizeof(host), hipMemcpyDeviceToHost));
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < per_lane; ++e) {
        const int bit = bits * e;  // of the lane's 64-bit result
        out[l][e] |= (int)((host[2 * l + bit / 32] >> (bit % 32)) & ((1u << bits) - 1u)) << shift;
      }
  }
  return out;
}

}  // namespace ghgemm
