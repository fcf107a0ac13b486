// gpuhealth — on-device MI355X (gfx950) health probe kernels + pybind11 host.
//
// Used by the operator's GPU worker readiness/liveness gate
// (kuberay_amd/gpu/health.py, wired into pod readiness probes by
// kuberay_amd/common/pod.py). The reference operator (kuberay) has no
// GPU-level probing at all; on MI355X nodes a pod can be "Ready" while its
// GPU is wedged (queue hang, HBM fallout, xGMI link down).
//
// Quick gate (readiness/liveness, <50 ms) — proves the device executes and
// streams; it does not look at the data and cannot see silent corruption:
//
//   * mfma_smoke   — one wave per workgroup issues v_mfma_f32_16x16x32_bf16
//                    with all-ones inputs; every D element must equal K=32.
//                    Proves the matrix pipeline executes and returns. All-ones
//                    data is blind to lane routing and to low operand bits.
//                    The output buffer is preset to 0xFF bytes (NaN) before
//                    the launch, so an element the kernel did not write fails
//                    the exact host compare whatever the allocator handed
//                    back. Test hooks: mfma_smoke(corruptions=,
//                    launch_workgroups=) and debug_mfma_smoke_dump (the raw
//                    buffer of the same code path).
//   * hbm_stream   — float4 streaming copy sized ≫ L3 (256 MiB) across
//                    ≫256 workgroups; host computes GB/s and compares
//                    against a floor (healthy MI355X streams ≈6 TB/s; a
//                    sick HBM stack or thermally-parked clock shows up as a
//                    collapse by an order of magnitude). The copied data is
//                    never compared: bandwidth only.
//
// Burn-in level (opt-in startup probe, seconds) — verifies data:
//
//   * hbm_pattern  — fills up to a fraction of the free HBM (all chunks live
//                    at once) with an index-hashed pattern, re-derives and
//                    compares it, then repeats with the pattern inverted.
//                    Reports mismatching words, flipped bits, the OR of the
//                    differences (a stuck line is one bit) and the first bad
//                    offset. Moving inversion is what catches a stuck-at bit
//                    whichever value the pattern wanted there: shown with
//                    hbm_pattern_check(stuck=), which forces bits of a word
//                    after every fill; a single stuck bit is reported in
//                    exactly one phase of every pass
//                    (tests/test_gpu_input_faults.py).
//   * mfma_exact   — asymmetric hashed operands whose products are exact in
//                    fp32, through bf16, f16, OCP fp8 and block-scaled MXFP4
//                    MFMA, with a C input; D is checked element by element
//                    against integer dot products computed off the matrix
//                    pipeline. A lane-routing fault shows (the data is shown
//                    to expose each of them in tests/test_gpu_probe_kernels.py),
//                    and so does a fault on an operand bit that the data
//                    toggles: bf16 bits 15..5, f16 bits 15..8, e4m3 bits 7..1,
//                    every e2m1 and E8M0 scale bit. The operands are integers
//                    in [-8, 8], so the low mantissa bits of bf16 (4..0), f16
//                    (7..0) and fp8 (0) are 0 in every operand: a stuck-at-0
//                    fault there is outside what this data can show.
//                    Shown on the device with operand-side seeded faults
//                    (debug_mfma_dump / mfma_verify(inject_operand=), an xor
//                    into one operand register of one lane before the MFMA;
//                    tests/test_gpu_input_faults.py): which element of A, B,
//                    C and of the scales each register of each lane is, that
//                    the check flags a fault that came in through an operand
//                    (the low mantissa bits and an infinity or NaN included),
//                    and that the MX instruction takes the scale from byte 0
//                    of its register alone and FP4 data from VGPRs 0..3 of
//                    the eight-VGPR operand alone. Not shown: subnormal
//                    operands; and the test flips the low mantissa bits, but
//                    the production data still never sets them, so a
//                    stuck-at-0 there stays invisible to the probe.
//   * cu_sweep     — workgroups of four waves that each take the whole LDS of
//                    a CU (the device's maximum per block, so one workgroup
//                    owns its CU), read where they run (XCC_ID and HW_ID
//                    registers: XCC, SE, SH, CU, and the SIMD of each wave),
//                    march the pattern over all of that LDS (16-byte fill;
//                    verified with 16-byte reads and again with dword reads
//                    on a rotated lane map; plain and inverted) and run the
//                    four exact MFMA tiles on each wave's SIMD. Results go to
//                    a table with one slot per CU. Rounds are launched until
//                    as many CUs were visited as the device has, or a limit.
//                    Proves, for every CU it reports as covered: each LDS
//                    word held both values of each bit, and each of the four
//                    matrix pipes gave exact products; a fault is named by
//                    XCC/SE/SH/CU (and SIMD, data type). Cannot show: a CU
//                    the dispatcher never gave us (reported as incomplete
//                    coverage, fatal only on request), LDS faults that need
//                    another access pattern (ds_read_b64, transposed reads,
//                    neighbouring-cell coupling), and which CU is missing —
//                    only covered places are known. No workgroup waits on
//                    another. Test hooks: cu_sweep(inject_lds=, inject_mfma=,
//                    inject_lds_stuck=) and debug_cu_lds_dump (the fill's LDS,
//                    copied out). inject_lds_stuck forces bits of one LDS word
//                    after every fill of one visit: a stuck bit is reported by
//                    both verifies in exactly one phase of every pass, which
//                    shows the march's own inversion and that every pass runs.
//   * mfma_load    — opt-in (seconds, on request only): the checks above give
//                    right answers once, within a millisecond, at the idle
//                    clock. This one keeps all four matrix pipes of every CU
//                    busy for seconds and stays exactly checkable: a wave
//                    holds A, B and C of an exact tile and issues
//                    acc = mfma(A, B, acc), acc = mfma(-A, B, acc), ...
//                    (alternating-sign premise, gpuhealth_ref.hpp), so acc is
//                    C + A·B after an odd count and C after an even one, and
//                    every partial sum is exact in fp32. Workgroups of four
//                    waves, one per SIMD, that take the whole LDS of a CU; a
//                    wave keeps four independent chains going, compares them
//                    every check_every MFMAs (odd) with expectations computed
//                    off the matrix pipe and starts again from C; it stamps
//                    s_memtime and s_memrealtime around the loop. Launches of
//                    about 50 ms, sized by a first short one, go back to back
//                    (two in flight) until the time asked for is over; no
//                    workgroup waits on another and no kernel on a clock.
//                    Proves: for the time it ran, every matrix pipe of every
//                    covered CU gave exact sums under sustained load (a fault
//                    is named by XCC/SE/SH/CU, SIMD and data type), and the
//                    device sustained floor_tflops. Reports the clock the
//                    waves saw (Δmemtime ÷ Δmemrealtime × 100 MHz) and the
//                    cycles per MFMA, so a low rate can be told apart: a
//                    parked clock shows in the one, a stalled pipe in the
//                    other; the slowest CU is reported, never gating. Cannot
//                    show: an error that enters the accumulator below one
//                    unit of the data (1, or 1/16 for MXFP4) can be rounded
//                    away before the next check, check_every bounds that
//                    window; the operands' low mantissa bits are still never
//                    set; CUs the dispatcher never handed over are not
//                    covered (cu_covered says how many were). No HBM or LDS
//                    traffic is mixed in. Test hooks: mfma_load(inject_acc=),
//                    an xor into one accumulator register of lane 0 after a
//                    named MFMA of a named chunk (its own instantiation), and
//                    debug_mfma_load_dump (the accumulators of one workgroup
//                    after exactly n MFMAs, through the production loop; with
//                    alternate=False its instantiation alone keeps +A where
//                    -A belongs, so the same loop leaves C + n·A·B and every
//                    count of issued MFMAs gives another answer).
//
// What must agree between host and device (pattern, generators, encoders,
// reference) is in gpuhealth_ref.hpp.
//
// Build: hipcc --offload-arch=gfx950 (see kuberay_amd/_native/build.py).
// Wavefront width is 64 on CDNA4 — all wave math below hard-codes 64.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "gpuhealth_ref.hpp"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e) + " at " #expr);          \
    }                                                                          \
  } while (0)

// ---------------------------------------------------------------------------
// host helpers shared by every probe
// ---------------------------------------------------------------------------
static int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

// Every binding that takes a device ordinal goes through here: an ordinal that
// does not name a visible device is a ValueError like every other bad
// argument, not whatever hipSetDevice makes of it.
static void use_device(int device) {
  const int count = device_count();
  if (device < 0 || device >= count)
    throw py::value_error("device " + std::to_string(device) + " is outside [0, " +
                          std::to_string(count) + "), the devices visible to HIP");
  HIP_CHECK(hipSetDevice(device));
}

// Frees every device allocation and event it was handed, on every path out.
struct DeviceScope {
  std::vector<void*> ptrs;
  std::vector<hipEvent_t> events;
  ~DeviceScope() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (void* p : ptrs) (void)hipFree(p);
  }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes));
    ptrs.push_back(p);
    return p;
  }
  hipEvent_t event() {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    events.push_back(e);
    return e;
  }
};

// (index, xor mask) pairs a test hands in: the host xors the mask into that
// 32-bit word between a fill / MFMA pass and its check. Signed so that a
// negative value is reported as a ValueError and not as a conversion error.
typedef std::vector<std::pair<int64_t, int64_t>> corruptions_t;

// Sorted by index; rejects indices outside [0, limit), masks that are zero or
// wider than 32 bits, and an index named twice.
static corruptions_t checked_corruptions(corruptions_t c, uint64_t limit,
                                         const char* what) {
  std::sort(c.begin(), c.end());
  for (size_t n = 0; n < c.size(); ++n) {
    if (c[n].first < 0 || (uint64_t)c[n].first >= limit)
      throw py::value_error(std::string(what) + " is outside the checked range");
    if (c[n].second <= 0 || c[n].second > 0xFFFFFFFFll)
      throw py::value_error("xor mask must be a non-zero 32-bit value");
    if (n > 0 && c[n].first == c[n - 1].first)
      throw py::value_error(std::string(what) + " is named twice");
  }
  return c;
}

static uint32_t checked_mask(int64_t mask) {
  if (mask <= 0 || mask > 0xFFFFFFFFll)
    throw py::value_error("xor mask must be a non-zero 32-bit value");
  return (uint32_t)mask;
}

static uint32_t checked_index(int64_t v, uint64_t limit, const char* what) {
  if (v < 0 || (uint64_t)v >= limit)
    throw py::value_error(std::string(what) + " is outside the checked range");
  return (uint32_t)v;
}

// host read-xor-write of one 32-bit word of device memory
static void xor_device_word(void* addr, uint32_t mask) {
  uint32_t word = 0;
  HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
  word ^= mask;
  HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
}

// (index, mask, value) triples a test hands in: a stuck-at fault. After every
// fill the masked bits of that 32-bit word are forced to value (0 or 1),
// whatever the fill wrote there.
struct StuckWord {
  uint64_t word;
  uint32_t mask, value;
};
typedef std::vector<std::tuple<int64_t, int64_t, int64_t>> stuck_t;

// Sorted by index; the same rules as checked_corruptions, and value is 0 or 1.
static std::vector<StuckWord> checked_stuck(stuck_t s, uint64_t limit, const char* what) {
  std::sort(s.begin(), s.end());
  std::vector<StuckWord> out;
  for (size_t n = 0; n < s.size(); ++n) {
    const auto& [word, mask, value] = s[n];
    if (word < 0 || (uint64_t)word >= limit)
      throw py::value_error(std::string(what) + " is outside the checked range");
    if (value != 0 && value != 1) throw py::value_error("stuck value must be 0 or 1");
    if (n > 0 && word == std::get<0>(s[n - 1]))
      throw py::value_error(std::string(what) + " is named twice");
    out.push_back({(uint64_t)word, checked_mask(mask), (uint32_t)value});
  }
  return out;
}

GH_HD inline uint32_t forced_word(uint32_t word, uint32_t mask, uint32_t value) {
  return value ? (word | mask) : (word & ~mask);
}

// host read-force-write of one 32-bit word of device memory, the path of
// xor_device_word
static void force_device_word(void* addr, uint32_t mask, uint32_t value) {
  uint32_t word = 0;
  HIP_CHECK(hipMemcpy(&word, addr, 4, hipMemcpyDeviceToHost));
  word = forced_word(word, mask, value);
  HIP_CHECK(hipMemcpy(addr, &word, 4, hipMemcpyHostToDevice));
}

// ---------------------------------------------------------------------------
// MFMA smoke: D = A(1s) * B(1s) + 0  ->  every element == K == 32
// ---------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
// Only gfx950 is supported — refuse silently-wrong builds for other arches.
#error "gpuhealth targets gfx950 (MI355X) only"
#endif

typedef __attribute__((ext_vector_type(8))) __bf16 frag_ab_t;  // 8 bf16 = 4 VGPRs
typedef __attribute__((ext_vector_type(4))) float frag_cd_t;   // 4 fp32 acc

__global__ void mfma_smoke_kernel(float* __restrict__ out) {
  frag_ab_t a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = (__bf16)1.0f;
    b[i] = (__bf16)1.0f;
  }
  frag_cd_t acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  const int lane = threadIdx.x & 63;
  const int wg = blockIdx.x;
  // 4 accumulator elements per lane; layout-independent check (all == 32)
  for (int r = 0; r < 4; ++r) {
    out[(size_t)wg * 256 + lane * 4 + r] = acc[r];
  }
}

// The buffer is preset to 0xFF bytes (NaN): hipMalloc hands a freed block of
// the same size back, still holding the 32.0f of the previous good run, so
// without the preset a launch that wrote only part of the buffer would pass.
// corruptions: the host xors each mask into that element between the kernel
// and the check. launch_workgroups (test hook): -1 launches every tile, a
// value in [0, workgroups] only that many while the check still covers
// workgroups; 0 skips the launch. raw, when given, receives the checked buffer.
static bool run_mfma_smoke(int workgroups, corruptions_t corruptions = {},
                           int launch_workgroups = -1, std::string* raw = nullptr) {
  if (workgroups < 1 || workgroups > (1 << 20))
    throw py::value_error("workgroups must be in [1, 2^20]");
  if (launch_workgroups < -1 || launch_workgroups > workgroups)
    throw py::value_error("launch_workgroups must be -1 or in [0, workgroups]");
  const size_t n = (size_t)workgroups * 256;
  corruptions = checked_corruptions(std::move(corruptions), n, "corrupted element");

  DeviceScope scope;
  float* d_out = (float*)scope.alloc(n * sizeof(float));
  HIP_CHECK(hipMemset(d_out, 0xFF, n * sizeof(float)));
  const int launched = launch_workgroups < 0 ? workgroups : launch_workgroups;
  if (launched > 0) {
    hipLaunchKernelGGL(mfma_smoke_kernel, dim3(launched), dim3(64), 0, 0, d_out);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipDeviceSynchronize());
  for (const auto& [element, mask] : corruptions)
    xor_device_word(d_out + element, (uint32_t)mask);
  std::vector<float> host(n);
  HIP_CHECK(hipMemcpy(host.data(), d_out, n * sizeof(float), hipMemcpyDeviceToHost));
  if (raw) raw->assign((const char*)host.data(), n * sizeof(float));
  for (size_t i = 0; i < n; ++i) {
    if (host[i] != 32.0f) return false;  // exact, and true for a NaN
  }
  return true;
}

// ---------------------------------------------------------------------------
// HBM streaming copy (float4, grid-stride) — measures achievable bandwidth
// ---------------------------------------------------------------------------
__global__ void hbm_stream_kernel(const float4* __restrict__ src,
                                  float4* __restrict__ dst, size_t n_vec) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n_vec; i += stride) {
    dst[i] = src[i];
  }
}

// The one launch configuration of the stream kernel: ≫256 workgroups to fill
// 8 XCDs (guide §1); 256 threads/block.
static void launch_hbm_stream(const float4* d_src, float4* d_dst, size_t n_vec) {
  const int blocks = 4096;
  const int threads = 256;
  hipLaunchKernelGGL(hbm_stream_kernel, dim3(blocks), dim3(threads), 0, 0,
                     d_src, d_dst, n_vec);
}

static double run_hbm_stream(size_t bytes, int iters) {
  const size_t n_vec = bytes / sizeof(float4);
  DeviceScope scope;  // up to 4 GiB per buffer: freed on a throwing HIP_CHECK too
  float4* d_src = (float4*)scope.alloc(n_vec * sizeof(float4));
  float4* d_dst = (float4*)scope.alloc(n_vec * sizeof(float4));
  HIP_CHECK(hipMemset(d_src, 1, n_vec * sizeof(float4)));

  // warmup
  launch_hbm_stream(d_src, d_dst, n_vec);
  HIP_CHECK(hipDeviceSynchronize());

  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  for (int it = 0; it < iters; ++it) launch_hbm_stream(d_src, d_dst, n_vec);
  HIP_CHECK(hipEventRecord(t1, 0));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  // read + write traffic
  const double total_bytes = 2.0 * (double)n_vec * sizeof(float4) * iters;
  return total_bytes / (ms * 1e-3) / 1e9;  // GB/s
}

// ---------------------------------------------------------------------------
// Burn-in, part 1: HBM pattern sweep (fill, then re-derive and compare)
// ---------------------------------------------------------------------------
struct PatternStats {
  unsigned long long mismatched_words;
  unsigned long long flipped_bits;
  unsigned long long first_bad_word;  // global word index, ~0 when clean
  unsigned int bad_bit_mask;          // OR of every XOR difference
};

static constexpr unsigned long long kNoBadWord = ~0ull;

// n_vec 16-byte vectors; vector i holds words base_word + 4i .. + 4i+3
__global__ void hbm_pattern_fill(uint4* __restrict__ buf, uint64_t n_vec,
                                 uint64_t base_word, uint32_t seed,
                                 uint32_t invert_mask) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n_vec; i += stride) {
    const uint64_t w = base_word + 4 * i;
    uint4 v;
    v.x = gh::pattern_word(seed, w) ^ invert_mask;
    v.y = gh::pattern_word(seed, w + 1) ^ invert_mask;
    v.z = gh::pattern_word(seed, w + 2) ^ invert_mask;
    v.w = gh::pattern_word(seed, w + 3) ^ invert_mask;
    buf[i] = v;
  }
}

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline unsigned int wave_or_u32(unsigned int v) {
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
}

__global__ void hbm_pattern_verify(const uint4* __restrict__ buf, uint64_t n_vec,
                                   uint64_t base_word, uint32_t seed,
                                   uint32_t invert_mask,
                                   PatternStats* __restrict__ stats) {
  unsigned long long bad = 0, bits = 0, first = kNoBadWord;
  unsigned int mask = 0;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n_vec; i += stride) {
    const uint64_t w = base_word + 4 * i;
    const uint4 v = buf[i];
    const uint32_t got[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t x = got[j] ^ gh::pattern_word(seed, w + j) ^ invert_mask;
      if (x != 0) {
        ++bad;
        bits += __popc(x);
        mask |= x;
        if (w + j < first) first = w + j;
      }
    }
  }
  // per-lane partials -> wave reduction -> one atomic per wave, and only for a
  // wave that saw a mismatch: a clean sweep issues no atomics at all
  if (__ballot(bad != 0) == 0) return;
  bad = wave_sum_u64(bad);
  bits = wave_sum_u64(bits);
  first = wave_min_u64(first);
  mask = wave_or_u32(mask);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&stats->mismatched_words, bad);
    atomicAdd(&stats->flipped_bits, bits);
    atomicMin(&stats->first_bad_word, first);
    atomicOr(&stats->bad_bit_mask, mask);
  }
}

static int pattern_blocks(uint64_t n_vec) {
  // ≫256 workgroups to fill 8 XCDs, as the stream kernel; fewer for tiny runs
  const uint64_t want = (n_vec + 255) / 256;
  return (int)(want < 4096 ? (want ? want : 1) : 4096);
}

// The one launch configuration of the two sweep kernels; the sweep and every
// test hook go through these.
static void launch_pattern_fill(uint4* buf, uint64_t n_vec, uint64_t base_word,
                                uint32_t seed, uint32_t invert_mask) {
  hipLaunchKernelGGL(hbm_pattern_fill, dim3(pattern_blocks(n_vec)), dim3(256),
                     0, 0, buf, n_vec, base_word, seed, invert_mask);
}
static void launch_pattern_verify(const uint4* buf, uint64_t n_vec, uint64_t base_word,
                                  uint32_t seed, uint32_t invert_mask,
                                  PatternStats* d_stats) {
  hipLaunchKernelGGL(hbm_pattern_verify, dim3(pattern_blocks(n_vec)), dim3(256),
                     0, 0, buf, n_vec, base_word, seed, invert_mask, d_stats);
}

struct PatternResult {
  uint64_t bytes_checked = 0;
  int chunks = 0;
  PatternStats stats{0, 0, kNoBadWord, 0};  // first_bad_word relative to the sweep
  double gb_s = 0.0;
};

// target_bytes > 0: sweep exactly that much; else fraction x free memory.
// pattern_base is added to the word index that feeds the pattern, in the fill
// and in the verify; everything reported stays relative to the sweep.
// corruptions: (word, mask) relative to the sweep, applied between the fill and
// the verify of pass corrupt_pass, phase corrupt_phase.
// stuck: (word, mask, value) relative to the sweep, forced after every fill of
// every pass and both phases, after the corruptions where both name a word (a
// stuck bit stays stuck).
static PatternResult run_hbm_pattern(uint64_t target_bytes, double fraction,
                                     uint32_t seed, int passes,
                                     uint64_t max_chunk_bytes,
                                     uint64_t pattern_base = 0,
                                     corruptions_t corruptions = {},
                                     int corrupt_pass = 0, int corrupt_phase = 0,
                                     stuck_t stuck_in = {}) {
  if (target_bytes == 0) {
    if (!(fraction > 0.0) || fraction > 1.0)
      throw py::value_error("fraction must be in (0, 1] when no size is given");
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    target_bytes = (uint64_t)((double)free_b * fraction);
    target_bytes &= ~(uint64_t)15;
    if (target_bytes == 0) throw std::runtime_error("no free device memory to sweep");
  }
  if (target_bytes % 16 != 0) throw py::value_error("size must be a multiple of 16 bytes");
  if (max_chunk_bytes == 0 || max_chunk_bytes % 16 != 0)
    throw py::value_error("chunk size must be a positive multiple of 16 bytes");
  if (passes < 1) throw py::value_error("passes must be >= 1");
  if (pattern_base > ~(uint64_t)0 - target_bytes / 4)
    throw py::value_error("base_word plus the swept words must fit 64 bits");
  corruptions = checked_corruptions(std::move(corruptions), target_bytes / 4, "corrupted word");
  if (corrupt_pass < 0 || corrupt_pass >= passes || corrupt_phase < 0 || corrupt_phase > 1)
    throw py::value_error("corrupt_at must name a pass in [0, passes) and phase 0 or 1");
  const std::vector<StuckWord> stuck =
      checked_stuck(std::move(stuck_in), target_bytes / 4, "stuck word");

  struct Chunk { uint4* ptr; uint64_t bytes; uint64_t base_word; };
  DeviceScope scope;
  std::vector<Chunk> chunks;
  uint64_t covered = 0;
  // all chunks stay live together: free + re-allocate would hand back the
  // same pages and test them twice
  while (covered < target_bytes) {
    const uint64_t want = std::min(max_chunk_bytes, target_bytes - covered);
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();  // out of memory ends the allocation phase
      break;
    }
    scope.ptrs.push_back(p);
    chunks.push_back({(uint4*)p, want, covered / 4});
    covered += want;
  }
  if (chunks.empty()) throw std::runtime_error("could not allocate any device memory to sweep");
  if (!corruptions.empty() && (uint64_t)corruptions.back().first >= covered / 4)
    throw py::value_error("corrupted word is outside the memory that could be allocated");
  if (!stuck.empty() && stuck.back().word >= covered / 4)
    throw py::value_error("stuck word is outside the memory that could be allocated");
  // the address of sweep word w; callers walk sorted lists, so ci only grows
  auto word_addr = [&chunks](uint64_t w, size_t& ci) {
    while (w >= chunks[ci].base_word + chunks[ci].bytes / 4) ++ci;
    return (uint32_t*)chunks[ci].ptr + (w - chunks[ci].base_word);
  };

  PatternStats* d_stats = (PatternStats*)scope.alloc(sizeof(PatternStats));
  PatternResult res;
  HIP_CHECK(hipMemcpy(d_stats, &res.stats, sizeof(PatternStats), hipMemcpyHostToDevice));

  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  for (int pass = 0; pass < passes; ++pass) {
    // moving inversion: every bit is driven to 0 and to 1 and read back
    for (int phase = 0; phase < 2; ++phase) {
      const uint32_t inv = phase ? 0xFFFFFFFFu : 0u;
      for (const Chunk& c : chunks)
        launch_pattern_fill(c.ptr, c.bytes / 16, pattern_base + c.base_word, seed, inv);
      HIP_CHECK(hipGetLastError());
      if (pass == corrupt_pass && phase == corrupt_phase) {
        // both lists are sorted, so one walk finds every word's chunk
        size_t ci = 0;
        for (const auto& [word, mask] : corruptions)
          xor_device_word(word_addr((uint64_t)word, ci), (uint32_t)mask);
      }
      size_t ci = 0;
      for (const StuckWord& s : stuck) force_device_word(word_addr(s.word, ci), s.mask, s.value);
      for (const Chunk& c : chunks)
        launch_pattern_verify(c.ptr, c.bytes / 16, pattern_base + c.base_word, seed, inv,
                              d_stats);
      HIP_CHECK(hipGetLastError());
    }
  }
  HIP_CHECK(hipEventRecord(t1, 0));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipMemcpy(&res.stats, d_stats, sizeof(PatternStats), hipMemcpyDeviceToHost));
  // the kernels see pattern indices; pattern_base + words fits 64 bits (above),
  // so the smallest pattern index is the smallest sweep word
  if (res.stats.first_bad_word != kNoBadWord) res.stats.first_bad_word -= pattern_base;
  res.bytes_checked = covered;
  res.chunks = (int)chunks.size();
  // per pass: two fills (write) and two verifies (read) of every byte
  res.gb_s = ms > 0.f ? 4.0 * (double)covered * passes / (ms * 1e-3) / 1e9 : 0.0;
  return res;
}

// -- test hooks: what the kernels above leave in memory -----------------------
static constexpr uint64_t kDebugMaxBytes = 256ull << 20;

// One buffer, one production fill, read back raw. The buffer is preset so that
// a vector the fill skips reads back as 0x5A bytes and not as stale memory.
static std::string run_debug_pattern_fill(uint64_t bytes, uint32_t seed, bool invert,
                                          uint64_t base_word) {
  if (bytes == 0 || bytes % 16 != 0 || bytes > kDebugMaxBytes)
    throw py::value_error("bytes must be a positive multiple of 16, at most 256 MiB");
  if (base_word > ~(uint64_t)0 - bytes / 4)
    throw py::value_error("base_word plus the filled words must fit 64 bits");
  DeviceScope scope;
  uint4* d_buf = (uint4*)scope.alloc(bytes);
  HIP_CHECK(hipMemset(d_buf, 0x5A, bytes));
  launch_pattern_fill(d_buf, bytes / 16, base_word, seed, invert ? 0xFFFFFFFFu : 0u);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  std::string host(bytes, '\0');
  HIP_CHECK(hipMemcpy(&host[0], d_buf, bytes, hipMemcpyDeviceToHost));
  return host;
}

struct StreamCopyResult {
  PatternResult pattern;
  bool guard_intact = false;
};

// src holds the pattern, dst a sentinel; one production launch of the stream
// kernel; then the production verify reads dst. Both buffers are one vector
// longer than the copy: src's extra vector is zero, dst's is the guard, so a
// copy that runs one vector long overwrites the guard and still stays inside
// both allocations.
static StreamCopyResult run_debug_stream_copy(uint64_t bytes, uint32_t seed) {
  const uint64_t n_vec = bytes / 16;
  if (n_vec == 0 || bytes > kDebugMaxBytes)
    throw py::value_error("bytes must be at least 16 and at most 256 MiB");
  constexpr int kSentinel = 0xA5;
  DeviceScope scope;
  uint4* d_src = (uint4*)scope.alloc((n_vec + 1) * 16);
  uint4* d_dst = (uint4*)scope.alloc((n_vec + 1) * 16);
  PatternStats* d_stats = (PatternStats*)scope.alloc(sizeof(PatternStats));
  StreamCopyResult res;
  HIP_CHECK(hipMemcpy(d_stats, &res.pattern.stats, sizeof(PatternStats), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(d_src, 0, (n_vec + 1) * 16));
  HIP_CHECK(hipMemset(d_dst, kSentinel, (n_vec + 1) * 16));
  launch_pattern_fill(d_src, n_vec, 0, seed, 0u);
  launch_hbm_stream((const float4*)d_src, (float4*)d_dst, n_vec);
  launch_pattern_verify(d_dst, n_vec, 0, seed, 0u, d_stats);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(&res.pattern.stats, d_stats, sizeof(PatternStats), hipMemcpyDeviceToHost));
  unsigned char guard[16];
  HIP_CHECK(hipMemcpy(guard, d_dst + n_vec, sizeof(guard), hipMemcpyDeviceToHost));
  res.guard_intact = std::all_of(guard, guard + sizeof(guard),
                                 [](unsigned char b) { return b == kSentinel; });
  res.pattern.bytes_checked = 16 * n_vec;
  res.pattern.chunks = 1;
  return res;
}

// ---------------------------------------------------------------------------
// Burn-in, part 2: exact, layout-sensitive MFMA verification
//
// Operand lane maps (lane l, i = l & 15, g = l >> 4):
//   bf16 / f16 16x16x32 : fragment element j (0..7)  = A[i][8g + j], B[8g + j][i]
//   fp8 16x16x32        : byte j (0..7) of the 64-bit operand, same k = 8g + j
//   f8f6f4 16x16x128 FP4: nibble j (0..31) of the first 4 operand VGPRs is
//                         k = 32g + j, the even element in the low nibble; the
//                         lane's scale byte is the E8M0 of (row/col i, block g)
//   C/D (all paths)     : register r = D[4g + r][i]
// The maps are proven on the device by tests/test_gpu_burn_in.py and
// tests/test_gpu_probe_kernels.py: with asymmetric hashed data D equals
// A·B + C exactly only if all are right, up to a mistake that A and B share
// (j reversed in both, two k-groups swapped in both). Those are excluded by
// tests/test_gpu_input_faults.py: a fault seeded into one register of one lane
// changes D as this map says and not otherwise.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) _Float16 frag_f16_t;
typedef __attribute__((ext_vector_type(8))) int frag_i32x8_t;
typedef __attribute__((ext_vector_type(4))) uint32_t frag_u32x4_t;

// Test hook: an xor into one 32-bit register of one operand of one lane of one
// workgroup, applied after the operands are packed and before the MFMA reads
// them. reg counts the operand's dwords in that lane: 0..3 for bf16 / f16 A
// and B (elements 2 reg and 2 reg + 1, the even one in the low half), 0..1 for
// fp8 (bytes 4 reg .. 4 reg + 3), 0..7 for the eight-VGPR FP4 operand, 0..3
// for C, 0 for a scale. Only the INJECT instantiations read it; the kernels of
// burn_in() and of the CU sweep are the plain ones.
enum Operand : uint32_t { OP_A = 0, OP_B = 1, OP_C = 2, OP_SA = 3, OP_SB = 4 };
struct OperandInject {
  uint32_t wg = 0, lane = 0, operand = 0, reg = 0, mask = 0;
};

// dwords of the A or B operand one lane holds
static int operand_dwords(int dtype) {
  return dtype == gh::MXFP4 ? 8 : (dtype == gh::FP8 ? 2 : 4);
}

// a ^= mask on dword reg of an N-dword operand register; no dynamic indexing
template <int N, typename V>
__device__ inline void xor_dword(V& v, uint32_t reg, uint32_t mask) {
  for (uint32_t r = 0; r < (uint32_t)N; ++r) v[r] ^= (r == reg ? mask : 0u);
}

// The packed A and B of one exact tile as one lane holds them (MXFP4: with the
// two scale registers), kept apart from the MFMA so that a caller can hold on
// to them, negate A and issue again (mfma_load_kernel).
template <int DT> struct ExactOperands {
  frag_ab_t a, b;
};
template <> struct ExactOperands<gh::F16> {
  frag_f16_t a, b;
};
template <> struct ExactOperands<gh::FP8> {
  uint64_t a, b;
};
template <> struct ExactOperands<gh::MXFP4> {
  frag_i32x8_t a, b;
  int sa, sb;
};

// inj_mask is zero in every lane but the injected one
template <int DT, bool INJECT = false>
__device__ inline ExactOperands<DT> pack_exact_operands(uint32_t seed, uint32_t wg, int lane,
                                                        uint32_t inj_operand = 0,
                                                        uint32_t inj_reg = 0,
                                                        uint32_t inj_mask = 0) {
  const uint32_t i = lane & 15, g = lane >> 4;
  const uint32_t mask_a = inj_operand == OP_A ? inj_mask : 0u;
  const uint32_t mask_b = inj_operand == OP_B ? inj_mask : 0u;
  ExactOperands<DT> op;
  if constexpr (DT == gh::BF16) {
    frag_ab_t a, b;
    for (uint32_t j = 0; j < 8; ++j) {
      a[j] = __builtin_bit_cast(__bf16, gh::f32_to_bf16(
          (float)gh::gen_int(seed, wg, DT, gh::GEN_A, i, 8 * g + j)));
      b[j] = __builtin_bit_cast(__bf16, gh::f32_to_bf16(
          (float)gh::gen_int(seed, wg, DT, gh::GEN_B, i, 8 * g + j)));
    }
    if constexpr (INJECT) {
      frag_u32x4_t ua = __builtin_bit_cast(frag_u32x4_t, a);
      frag_u32x4_t ub = __builtin_bit_cast(frag_u32x4_t, b);
      xor_dword<4>(ua, inj_reg, mask_a);
      xor_dword<4>(ub, inj_reg, mask_b);
      a = __builtin_bit_cast(frag_ab_t, ua);
      b = __builtin_bit_cast(frag_ab_t, ub);
    }
    op.a = a;
    op.b = b;
  } else if constexpr (DT == gh::F16) {
    frag_f16_t a, b;
    for (uint32_t j = 0; j < 8; ++j) {
      a[j] = __builtin_bit_cast(_Float16, gh::f32_to_f16(
          (float)gh::gen_int(seed, wg, DT, gh::GEN_A, i, 8 * g + j)));
      b[j] = __builtin_bit_cast(_Float16, gh::f32_to_f16(
          (float)gh::gen_int(seed, wg, DT, gh::GEN_B, i, 8 * g + j)));
    }
    if constexpr (INJECT) {
      frag_u32x4_t ua = __builtin_bit_cast(frag_u32x4_t, a);
      frag_u32x4_t ub = __builtin_bit_cast(frag_u32x4_t, b);
      xor_dword<4>(ua, inj_reg, mask_a);
      xor_dword<4>(ub, inj_reg, mask_b);
      a = __builtin_bit_cast(frag_f16_t, ua);
      b = __builtin_bit_cast(frag_f16_t, ub);
    }
    op.a = a;
    op.b = b;
  } else if constexpr (DT == gh::FP8) {
    uint64_t a = 0, b = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      a |= (uint64_t)gh::f32_to_e4m3(
               (float)gh::gen_int(seed, wg, DT, gh::GEN_A, i, 8 * g + j)) << (8 * j);
      b |= (uint64_t)gh::f32_to_e4m3(
               (float)gh::gen_int(seed, wg, DT, gh::GEN_B, i, 8 * g + j)) << (8 * j);
    }
    if constexpr (INJECT) {
      a ^= (uint64_t)mask_a << (32 * (inj_reg & 1u));
      b ^= (uint64_t)mask_b << (32 * (inj_reg & 1u));
    }
    op.a = a;
    op.b = b;
  } else {
    frag_i32x8_t a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t v = 0; v < 4; ++v) {
      uint32_t wa = 0, wb = 0;
      for (uint32_t n = 0; n < 8; ++n) {
        const uint32_t k = 32 * g + 8 * v + n;
        wa |= gh::gen_fp4(seed, wg, gh::GEN_A, i, k) << (4 * n);
        wb |= gh::gen_fp4(seed, wg, gh::GEN_B, i, k) << (4 * n);
      }
      a[v] = (int)wa;
      b[v] = (int)wb;
    }
    int sa = (int)gh::gen_scale(seed, wg, gh::GEN_SA, i, g);
    int sb = (int)gh::gen_scale(seed, wg, gh::GEN_SB, i, g);
    if constexpr (INJECT) {
      xor_dword<8>(a, inj_reg, mask_a);
      xor_dword<8>(b, inj_reg, mask_b);
      sa ^= (int)(inj_operand == OP_SA ? inj_mask : 0u);
      sb ^= (int)(inj_operand == OP_SB ? inj_mask : 0u);
    }
    op.a = a;
    op.b = b;
    op.sa = sa;
    op.sb = sb;
  }
  return op;
}

// acc = A·B + acc on the matrix pipe of this wave's SIMD
template <int DT>
__device__ inline frag_cd_t issue_exact_mfma(const ExactOperands<DT>& op, frag_cd_t acc) {
  if constexpr (DT == gh::BF16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(op.a, op.b, acc, 0, 0, 0);
  } else if constexpr (DT == gh::F16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(op.a, op.b, acc, 0, 0, 0);
  } else if constexpr (DT == gh::FP8) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)op.a, (long)op.b, acc, 0, 0, 0);
  } else {
    // cbsz=4 / blgp=4: FP4 A and B, which the instruction takes from VGPRs 0..3
    // of each eight-VGPR operand; opsel 0: the scale is byte 0 of its register
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(op.a, op.b, acc, 4, 4, 0, op.sa, 0,
                                                            op.sb);
  }
}

// the same operands with every element of A negated (gh::negate_mask); of the
// eight-VGPR FP4 operand only VGPRs 0..3 hold data
template <int DT>
__device__ inline ExactOperands<DT> negated_a(ExactOperands<DT> op) {
  const uint32_t m = gh::negate_mask(DT);
  if constexpr (DT == gh::BF16 || DT == gh::F16) {
    frag_u32x4_t ua = __builtin_bit_cast(frag_u32x4_t, op.a);
    for (int r = 0; r < 4; ++r) ua[r] ^= m;
    op.a = __builtin_bit_cast(decltype(op.a), ua);
  } else if constexpr (DT == gh::FP8) {
    op.a ^= (uint64_t)m << 32 | m;
  } else {
    for (int r = 0; r < 4; ++r) op.a[r] ^= (int)m;
  }
  return op;
}

template <int DT, bool INJECT = false>
__device__ inline frag_cd_t mfma_exact_tile(uint32_t seed, uint32_t wg, int lane,
                                            frag_cd_t acc, uint32_t inj_operand = 0,
                                            uint32_t inj_reg = 0, uint32_t inj_mask = 0) {
  return issue_exact_mfma<DT>(
      pack_exact_operands<DT, INJECT>(seed, wg, lane, inj_operand, inj_reg, inj_mask), acc);
}

// one wave per workgroup; D tiles are row-major, tile wg at out + 256 * wg
template <int DT, bool INJECT>
__device__ inline void mfma_exact_body(float* __restrict__ out, uint32_t seed,
                                       uint32_t wg_base, const OperandInject& inj) {
  const int lane = threadIdx.x & 63;
  const uint32_t wg = wg_base + blockIdx.x;
  const uint32_t col = lane & 15, row0 = 4 * (lane >> 4);
  frag_cd_t acc;
  for (uint32_t r = 0; r < 4; ++r) acc[r] = (float)gh::gen_c(seed, wg, DT, row0 + r, col);
  if constexpr (INJECT) {
    const uint32_t mask = (wg == inj.wg && (uint32_t)lane == inj.lane) ? inj.mask : 0u;
    for (uint32_t r = 0; r < 4; ++r)
      if (inj.operand == OP_C && r == inj.reg)
        acc[r] = gh::bits_f32(gh::f32_bits(acc[r]) ^ mask);
    acc = mfma_exact_tile<DT, true>(seed, wg, lane, acc, inj.operand, inj.reg, mask);
  } else {
    acc = mfma_exact_tile<DT>(seed, wg, lane, acc);
  }
  float* tile = out + (size_t)blockIdx.x * 256;
  for (uint32_t r = 0; r < 4; ++r) tile[(row0 + r) * 16 + col] = acc[r];
}

template <int DT>
__global__ void mfma_exact_kernel(float* __restrict__ out, uint32_t seed,
                                  uint32_t wg_base) {
  mfma_exact_body<DT, false>(out, seed, wg_base, OperandInject{});
}

// the test hook's own instantiation: same packing, same MFMA, one xor between
template <int DT>
__global__ void mfma_exact_inject_kernel(float* __restrict__ out, uint32_t seed,
                                         uint32_t wg_base, OperandInject inj) {
  mfma_exact_body<DT, true>(out, seed, wg_base, inj);
}

struct MfmaStats {
  unsigned long long mismatches;
  unsigned long long first_bad;  // flat element index, ~0 when clean
};

// Checks D without the matrix pipeline: integer dot products over the same
// generators, four outputs per lane.
__global__ void mfma_check_kernel(const float* __restrict__ d, int dtype,
                                  uint32_t seed, uint32_t wg_base,
                                  MfmaStats* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const uint32_t wg = wg_base + blockIdx.x;
  const uint32_t col = lane & 15, row0 = 4 * (lane >> 4);
  unsigned long long bad = 0, first = kNoBadWord;
  for (uint32_t r = 0; r < 4; ++r) {
    const size_t idx = (size_t)blockIdx.x * 256 + (row0 + r) * 16 + col;
    const float expected = gh::reference_element(dtype, seed, wg, row0 + r, col);
    if (!(d[idx] == expected)) {
      ++bad;
      if (idx < first) first = idx;
    }
  }
  if (__ballot(bad != 0) == 0) return;
  bad = wave_sum_u64(bad);
  first = wave_min_u64(first);
  if (lane == 0) {
    atomicAdd(&stats->mismatches, bad);
    atomicMin(&stats->first_bad, first);
  }
}

template <int DT>
static void launch_mfma_exact_inject(float* d_out, const dim3& grid, uint32_t seed,
                                     uint32_t wg_base, const OperandInject& inj) {
  hipLaunchKernelGGL(mfma_exact_inject_kernel<DT>, grid, dim3(64), 0, 0, d_out, seed,
                     wg_base, inj);
}

// inject == nullptr launches the production kernels
static void launch_mfma_exact(int dtype, float* d_out, int workgroups,
                              uint32_t seed, uint32_t wg_base,
                              const OperandInject* inject = nullptr) {
  const dim3 grid(workgroups), block(64);
  if (inject) {
    switch (dtype) {
      case gh::BF16: launch_mfma_exact_inject<gh::BF16>(d_out, grid, seed, wg_base, *inject); break;
      case gh::F16: launch_mfma_exact_inject<gh::F16>(d_out, grid, seed, wg_base, *inject); break;
      case gh::FP8: launch_mfma_exact_inject<gh::FP8>(d_out, grid, seed, wg_base, *inject); break;
      default: launch_mfma_exact_inject<gh::MXFP4>(d_out, grid, seed, wg_base, *inject); break;
    }
    HIP_CHECK(hipGetLastError());
    return;
  }
  switch (dtype) {
    case gh::BF16:
      hipLaunchKernelGGL(mfma_exact_kernel<gh::BF16>, grid, block, 0, 0, d_out, seed, wg_base);
      break;
    case gh::F16:
      hipLaunchKernelGGL(mfma_exact_kernel<gh::F16>, grid, block, 0, 0, d_out, seed, wg_base);
      break;
    case gh::FP8:
      hipLaunchKernelGGL(mfma_exact_kernel<gh::FP8>, grid, block, 0, 0, d_out, seed, wg_base);
      break;
    default:
      hipLaunchKernelGGL(mfma_exact_kernel<gh::MXFP4>, grid, block, 0, 0, d_out, seed, wg_base);
      break;
  }
  HIP_CHECK(hipGetLastError());
}

struct MfmaResult {
  int tiles = 0;
  uint64_t mismatches = 0;
  int64_t first_bad = -1;  // flat element index
  float got = 0.f, expected = 0.f;
};

// what of an operand injection depends on the data type and on the launch
static void check_operand_inject(const OperandInject& inj, int dtype, int workgroups) {
  if (inj.wg >= (uint32_t)workgroups)
    throw py::value_error("injected workgroup is outside the launch");
  if ((inj.operand == OP_SA || inj.operand == OP_SB) && dtype != gh::MXFP4)
    throw py::value_error("only mxfp4 has the scale operands sa and sb");
  const uint32_t regs = inj.operand == OP_C ? 4u
                        : (inj.operand == OP_A || inj.operand == OP_B)
                            ? (uint32_t)operand_dwords(dtype) : 1u;
  if (inj.reg >= regs)
    throw py::value_error("injected register is outside the operand's " +
                          std::to_string(regs) + " dwords");
}

// corruptions: the host xors each mask into that element of D
// ((workgroup * 16 + row) * 16 + col) between the MFMA pass and the check.
// inject: an operand-side fault, applied by the kernel before the MFMA.
static MfmaResult run_mfma_verify(int dtype, int workgroups, uint32_t seed,
                                  corruptions_t corruptions = {},
                                  const OperandInject* inject = nullptr) {
  if (workgroups < 1 || workgroups > (1 << 20))
    throw py::value_error("workgroups must be in [1, 2^20]");
  const size_t n = (size_t)workgroups * 256;
  corruptions = checked_corruptions(std::move(corruptions), n, "corrupted element");
  if (inject) check_operand_inject(*inject, dtype, workgroups);

  DeviceScope scope;
  float* d_out = (float*)scope.alloc(n * sizeof(float));
  MfmaStats* d_stats = (MfmaStats*)scope.alloc(sizeof(MfmaStats));
  MfmaStats st{0, kNoBadWord};
  HIP_CHECK(hipMemcpy(d_stats, &st, sizeof(st), hipMemcpyHostToDevice));

  launch_mfma_exact(dtype, d_out, workgroups, seed, 0, inject);
  for (const auto& [element, mask] : corruptions)
    xor_device_word(d_out + element, (uint32_t)mask);
  hipLaunchKernelGGL(mfma_check_kernel, dim3(workgroups), dim3(64), 0, 0,
                     d_out, dtype, seed, 0u, d_stats);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(&st, d_stats, sizeof(st), hipMemcpyDeviceToHost));

  MfmaResult res;
  res.tiles = workgroups;
  res.mismatches = st.mismatches;
  if (st.mismatches != 0 && st.first_bad < n) {
    res.first_bad = (int64_t)st.first_bad;
    HIP_CHECK(hipMemcpy(&res.got, d_out + st.first_bad, 4, hipMemcpyDeviceToHost));
    res.expected = gh::reference_element(dtype, seed, (uint32_t)(st.first_bad / 256),
                                         (uint32_t)(st.first_bad / 16 % 16),
                                         (uint32_t)(st.first_bad % 16));
  }
  return res;
}

// test hook: the raw fp32 D buffer of the production MFMA pass
static std::string run_debug_mfma_dump(int dtype, int workgroups, uint32_t seed,
                                       const OperandInject* inject = nullptr) {
  if (workgroups < 1 || workgroups > 4096)
    throw py::value_error("workgroups must be in [1, 4096]");
  if (inject) check_operand_inject(*inject, dtype, workgroups);
  const size_t bytes = (size_t)workgroups * 256 * sizeof(float);
  DeviceScope scope;
  float* d_out = (float*)scope.alloc(bytes);
  HIP_CHECK(hipMemset(d_out, 0xFF, bytes));  // an unwritten element reads as NaN
  launch_mfma_exact(dtype, d_out, workgroups, seed, 0, inject);
  HIP_CHECK(hipDeviceSynchronize());
  std::string host(bytes, '\0');
  HIP_CHECK(hipMemcpy(&host[0], d_out, bytes, hipMemcpyDeviceToHost));
  return host;
}

// ---------------------------------------------------------------------------
// Burn-in, part 3: CU sweep — LDS march and exact MFMA per SIMD, with the
// place each workgroup ran on
//
// A workgroup of four waves takes lds_bytes of dynamic LDS; at the device's
// maximum it owns its CU. It never waits on another workgroup: coverage comes
// from launching more of them (run_cu_sweep), never from holding CUs.
// ---------------------------------------------------------------------------
constexpr int kSweepThreads = 256;
constexpr int kSweepWaves = kSweepThreads / 64;
// dword verify: lane-to-address map rotated against the fill's, by a
// non-multiple of 64 words so that each bank is read from another lane
constexpr uint32_t kLdsVerifyRotation = 17;

struct LdsStats {
  unsigned long long bad_words;
  unsigned long long flipped_bits;
  unsigned long long first_bad_word;  // LDS word index, ~0 when clean
  unsigned int bad_bit_mask;          // OR of every XOR difference
  unsigned int reserved;
};

struct CuSlot {
  unsigned int visits;
  unsigned int simd_seen;  // bit s: a wave of some visit ran on SIMD s
  LdsStats lds;
  unsigned int mfma_bad[gh::kNumSimds][gh::kNumDtypes];
};

// what one workgroup saw, at records[visit]; lds is per wave (plain stores,
// the host adds them up)
struct CuRecord {
  unsigned int written;  // 1 once wave 0 has been here
  unsigned int key;
  unsigned int xcc_id_reg, hw_id_reg;  // raw, as wave 0 read them
  unsigned int simd[kSweepWaves];
  LdsStats lds[kSweepWaves];
};

// test hook, applied by the kernel itself to the one visit it names
struct CuInject {
  uint32_t lds_on = 0, lds_visit = 0, lds_word = 0, lds_mask = 0, lds_phase = 0;
  uint32_t mfma_on = 0, mfma_visit = 0, mfma_wave = 0, mfma_dtype = 0,
           mfma_element = 0, mfma_mask = 0;
  // stuck-at: forced after every fill of that visit, in all passes and phases
  uint32_t stuck_on = 0, stuck_visit = 0, stuck_word = 0, stuck_mask = 0, stuck_value = 0;
};

__device__ inline uint32_t read_xcc_id_reg() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v;
}
__device__ inline uint32_t read_hw_id_reg() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}

__device__ inline uint4 lds_pattern_vec(uint32_t seed, uint32_t visit, uint32_t vec,
                                        uint32_t invert_mask) {
  uint4 v;
  v.x = gh::pattern_word(seed, gh::lds_pattern_index(visit, 4 * vec)) ^ invert_mask;
  v.y = gh::pattern_word(seed, gh::lds_pattern_index(visit, 4 * vec + 1)) ^ invert_mask;
  v.z = gh::pattern_word(seed, gh::lds_pattern_index(visit, 4 * vec + 2)) ^ invert_mask;
  v.w = gh::pattern_word(seed, gh::lds_pattern_index(visit, 4 * vec + 3)) ^ invert_mask;
  return v;
}

// the one fill of the march: 16-byte vectors, thread t takes t, t + 256, ...
__device__ inline void lds_fill(uint4* lds, uint32_t n_vec, uint32_t seed,
                                uint32_t visit, uint32_t invert_mask) {
  for (uint32_t v = threadIdx.x; v < n_vec; v += kSweepThreads)
    lds[v] = lds_pattern_vec(seed, visit, v, invert_mask);
}

struct LaneStats {
  unsigned long long bad = 0, bits = 0, first = kNoBadWord;
  unsigned int mask = 0;
  __device__ inline void see(uint32_t diff, uint32_t word) {
    if (diff != 0) {
      ++bad;
      bits += __popc(diff);
      mask |= diff;
      if (word < first) first = word;
    }
  }
};

// one exact tile on this wave's matrix pipe; returns this lane's bad D registers
template <int DT>
__device__ inline unsigned int sweep_mfma_bad(uint32_t seed, uint32_t wg, int lane,
                                              bool inject, uint32_t inj_element,
                                              uint32_t inj_mask) {
  const uint32_t col = lane & 15, row0 = 4 * (lane >> 4);
  frag_cd_t acc;
  for (uint32_t r = 0; r < 4; ++r) acc[r] = (float)gh::gen_c(seed, wg, DT, row0 + r, col);
  acc = mfma_exact_tile<DT>(seed, wg, lane, acc);
  unsigned int bad = 0;
  for (uint32_t r = 0; r < 4; ++r) {
    float got = acc[r];
    if (inject && inj_element == (row0 + r) * 16 + col)
      got = gh::bits_f32(gh::f32_bits(got) ^ inj_mask);
    if (!(got == gh::reference_element(DT, seed, wg, row0 + r, col))) ++bad;
  }
  return bad;
}

__global__ __launch_bounds__(kSweepThreads) void cu_sweep_kernel(
    CuSlot* __restrict__ slots, CuRecord* __restrict__ records, uint32_t visit_base,
    uint32_t seed, int passes, uint32_t lds_bytes, CuInject inj) {
  extern __shared__ uint4 lds_vec[];
  const uint32_t* lds_words = (const uint32_t*)lds_vec;
  const uint32_t visit = visit_base + blockIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t n_vec = lds_bytes / 16, n_words = lds_bytes / 4;

  // 1. locate: every wave reads its own registers
  const uint32_t xcc_reg = read_xcc_id_reg(), hw_reg = read_hw_id_reg();
  const gh::CuLocation loc = gh::decode_location(xcc_reg, hw_reg);
  const uint32_t key = gh::location_key(loc);
  CuSlot* slot = slots + key;
  CuRecord* rec = records + visit;

  // 2. LDS march
  LaneStats st;
  const uint32_t rot = kLdsVerifyRotation % n_words;
  for (int pass = 0; pass < passes; ++pass) {
    for (uint32_t phase = 0; phase < 2; ++phase) {
      const uint32_t inv = phase ? 0xFFFFFFFFu : 0u;
      __syncthreads();  // the previous phase's reads are done
      lds_fill(lds_vec, n_vec, seed, visit, inv);
      __syncthreads();
      if (inj.lds_on && visit == inj.lds_visit && phase == inj.lds_phase && pass == 0) {
        if (threadIdx.x == 0) ((uint32_t*)lds_vec)[inj.lds_word] ^= inj.lds_mask;
        __syncthreads();
      }
      if (inj.stuck_on && visit == inj.stuck_visit) {
        if (threadIdx.x == 0) {
          uint32_t* word = (uint32_t*)lds_vec + inj.stuck_word;
          *word = forced_word(*word, inj.stuck_mask, inj.stuck_value);
        }
        __syncthreads();
      }
      // 16-byte reads, the fill's own lane map
      for (uint32_t v = threadIdx.x; v < n_vec; v += kSweepThreads) {
        const uint4 got = lds_vec[v];
        const uint4 want = lds_pattern_vec(seed, visit, v, inv);
        st.see(got.x ^ want.x, 4 * v);
        st.see(got.y ^ want.y, 4 * v + 1);
        st.see(got.z ^ want.z, 4 * v + 2);
        st.see(got.w ^ want.w, 4 * v + 3);
      }
      // dword reads, rotated lane map
      for (uint32_t i = threadIdx.x; i < n_words; i += kSweepThreads) {
        uint32_t w = i + rot;
        if (w >= n_words) w -= n_words;
        const uint32_t want =
            gh::pattern_word(seed, gh::lds_pattern_index(visit, w)) ^ inv;
        st.see(lds_words[w] ^ want, w);
      }
    }
  }

  // 3. exact MFMA on the SIMD this wave sits on
  const uint32_t wg = visit * kSweepWaves + wave;
  const bool inj_here = inj.mfma_on && visit == inj.mfma_visit && wave == inj.mfma_wave;
  unsigned int mfma_bad[gh::kNumDtypes];
  mfma_bad[gh::BF16] = sweep_mfma_bad<gh::BF16>(
      seed, wg, lane, inj_here && inj.mfma_dtype == gh::BF16, inj.mfma_element, inj.mfma_mask);
  mfma_bad[gh::F16] = sweep_mfma_bad<gh::F16>(
      seed, wg, lane, inj_here && inj.mfma_dtype == gh::F16, inj.mfma_element, inj.mfma_mask);
  mfma_bad[gh::FP8] = sweep_mfma_bad<gh::FP8>(
      seed, wg, lane, inj_here && inj.mfma_dtype == gh::FP8, inj.mfma_element, inj.mfma_mask);
  mfma_bad[gh::MXFP4] = sweep_mfma_bad<gh::MXFP4>(
      seed, wg, lane, inj_here && inj.mfma_dtype == gh::MXFP4, inj.mfma_element, inj.mfma_mask);

  // 4. publish: wave reductions, then lane 0 alone; fault fields only when set
  const bool lds_faulty = __ballot(st.bad != 0) != 0;
  LdsStats ws{0, 0, kNoBadWord, 0, 0};
  if (lds_faulty) {
    ws.bad_words = wave_sum_u64(st.bad);
    ws.flipped_bits = wave_sum_u64(st.bits);
    ws.first_bad_word = wave_min_u64(st.first);
    ws.bad_bit_mask = wave_or_u32(st.mask);
  }
  for (int dt = 0; dt < gh::kNumDtypes; ++dt) {
    if (__ballot(mfma_bad[dt] != 0) == 0) continue;
    const unsigned int bad = (unsigned int)wave_sum_u64(mfma_bad[dt]);
    if (lane == 0) atomicAdd(&slot->mfma_bad[loc.simd][dt], bad);
  }
  if (lane != 0) return;
  atomicOr(&slot->simd_seen, 1u << loc.simd);
  if (lds_faulty) {
    atomicAdd(&slot->lds.bad_words, ws.bad_words);
    atomicAdd(&slot->lds.flipped_bits, ws.flipped_bits);
    atomicMin(&slot->lds.first_bad_word, ws.first_bad_word);
    atomicOr(&slot->lds.bad_bit_mask, ws.bad_bit_mask);
  }
  rec->simd[wave] = loc.simd;
  rec->lds[wave] = ws;
  if (wave == 0) {
    atomicAdd(&slot->visits, 1u);
    rec->key = key;
    rec->xcc_id_reg = xcc_reg;
    rec->hw_id_reg = hw_reg;
    rec->written = 1;
  }
}

// test hook: the production fill, then the whole LDS copied out. The LDS is
// preset first, so a word the fill skips reads back as 0x5A bytes.
__global__ __launch_bounds__(kSweepThreads) void cu_lds_dump_kernel(
    uint32_t* __restrict__ out, uint32_t lds_bytes, uint32_t seed, uint32_t visit,
    uint32_t invert_mask) {
  extern __shared__ uint4 lds_vec[];
  uint32_t* lds_words = (uint32_t*)lds_vec;
  const uint32_t n_words = lds_bytes / 4;
  for (uint32_t i = threadIdx.x; i < n_words; i += kSweepThreads) lds_words[i] = 0x5A5A5A5Au;
  __syncthreads();
  lds_fill(lds_vec, lds_bytes / 16, seed, visit, invert_mask);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_words; i += kSweepThreads) out[i] = lds_words[i];
}

static int current_device_attribute(hipDeviceAttribute_t attr) {
  int device = 0, value = 0;
  HIP_CHECK(hipGetDevice(&device));
  HIP_CHECK(hipDeviceGetAttribute(&value, attr, device));
  return value;
}

// 0 stands for the device's maximum, at which one workgroup owns a CU
static uint32_t checked_lds_bytes(uint64_t lds_bytes) {
  const uint64_t max_bytes =
      (uint64_t)current_device_attribute(hipDeviceAttributeMaxSharedMemoryPerBlock) & ~15ull;
  if (lds_bytes == 0) lds_bytes = max_bytes;
  if (lds_bytes < 16 || lds_bytes % 16 != 0 || lds_bytes > max_bytes)
    throw py::value_error("lds_bytes must be a positive multiple of 16, at most " +
                          std::to_string(max_bytes) + " on this device");
  return (uint32_t)lds_bytes;
}

template <typename Kernel>
static void allow_dynamic_lds(Kernel kernel, uint32_t lds_bytes) {
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
}

constexpr int kSweepMaxPasses = 64;
constexpr int kSweepMaxRounds = 64;
constexpr int kSweepMaxBlocksPerRound = 1 << 14;
constexpr uint64_t kSweepMaxVisits = 1ull << 18;

struct CuSweepResult {
  int cu_total = 0;
  int rounds = 0;
  uint32_t lds_bytes = 0;
  int blocks_per_round = 0;
  double elapsed_ms = 0.0;
  std::vector<CuSlot> slots;
  bool have_record = false;  // the injected visit was launched
  CuRecord record{};
};

static int covered_slots(const std::vector<CuSlot>& slots) {
  int n = 0;
  for (const CuSlot& s : slots) n += s.visits != 0;
  return n;
}

// Rounds of blocks_per_round workgroups (0: 4 x CUs) until as many slots have
// been visited as the device has CUs, or max_rounds. inject names visits of
// the whole run: visit = round * blocks_per_round + block.
static CuSweepResult run_cu_sweep(uint32_t seed, int passes, uint64_t lds_bytes,
                                  int blocks_per_round, int max_rounds,
                                  const CuInject& inject) {
  CuSweepResult res;
  res.cu_total = current_device_attribute(hipDeviceAttributeMultiprocessorCount);
  res.lds_bytes = checked_lds_bytes(lds_bytes);
  if (passes < 1 || passes > kSweepMaxPasses)
    throw py::value_error("passes must be in [1, " + std::to_string(kSweepMaxPasses) + "]");
  if (max_rounds < 1 || max_rounds > kSweepMaxRounds)
    throw py::value_error("max_rounds must be in [1, " + std::to_string(kSweepMaxRounds) + "]");
  if (blocks_per_round == 0) blocks_per_round = 4 * res.cu_total;
  if (blocks_per_round < 1 || blocks_per_round > kSweepMaxBlocksPerRound)
    throw py::value_error("blocks_per_round must be 0 or in [1, " +
                          std::to_string(kSweepMaxBlocksPerRound) + "]");
  const uint64_t visits = (uint64_t)blocks_per_round * max_rounds;
  if (visits > kSweepMaxVisits)
    throw py::value_error("blocks_per_round x max_rounds must be at most " +
                          std::to_string(kSweepMaxVisits));
  if (inject.lds_on) {
    if (inject.lds_visit >= visits)
      throw py::value_error("injected visit is outside [0, blocks_per_round x max_rounds)");
    if (inject.lds_word >= res.lds_bytes / 4)
      throw py::value_error("injected LDS word is outside the checked range");
  }
  if (inject.stuck_on) {
    if (inject.stuck_visit >= visits)
      throw py::value_error("injected visit is outside [0, blocks_per_round x max_rounds)");
    if (inject.stuck_word >= res.lds_bytes / 4)
      throw py::value_error("stuck LDS word is outside the checked range");
  }
  if (inject.mfma_on && inject.mfma_visit >= visits)
    throw py::value_error("injected visit is outside [0, blocks_per_round x max_rounds)");
  res.blocks_per_round = blocks_per_round;

  DeviceScope scope;
  CuSlot clean{};
  clean.lds.first_bad_word = kNoBadWord;
  res.slots.assign(gh::kCuSlots, clean);
  const size_t slot_bytes = gh::kCuSlots * sizeof(CuSlot);
  CuSlot* d_slots = (CuSlot*)scope.alloc(slot_bytes);
  CuRecord* d_records = (CuRecord*)scope.alloc(visits * sizeof(CuRecord));
  HIP_CHECK(hipMemcpy(d_slots, res.slots.data(), slot_bytes, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(d_records, 0, visits * sizeof(CuRecord)));
  allow_dynamic_lds(cu_sweep_kernel, res.lds_bytes);

  hipEvent_t t0 = scope.event(), t1 = scope.event();
  HIP_CHECK(hipEventRecord(t0, 0));
  while (res.rounds < max_rounds) {
    hipLaunchKernelGGL(cu_sweep_kernel, dim3(blocks_per_round), dim3(kSweepThreads),
                       res.lds_bytes, 0, d_slots, d_records,
                       (uint32_t)(res.rounds * blocks_per_round), seed, passes,
                       res.lds_bytes, inject);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(res.slots.data(), d_slots, slot_bytes, hipMemcpyDeviceToHost));
    ++res.rounds;
    if (covered_slots(res.slots) >= res.cu_total) break;
  }
  HIP_CHECK(hipEventRecord(t1, 0));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  res.elapsed_ms = ms;

  if (inject.lds_on || inject.stuck_on || inject.mfma_on) {
    const uint32_t visit = inject.lds_on ? inject.lds_visit
                           : inject.stuck_on ? inject.stuck_visit : inject.mfma_visit;
    if (visit < (uint64_t)res.rounds * blocks_per_round) {
      HIP_CHECK(hipMemcpy(&res.record, d_records + visit, sizeof(CuRecord),
                          hipMemcpyDeviceToHost));
      res.have_record = res.record.written != 0;
    }
  }
  return res;
}

static std::string run_debug_cu_lds_dump(uint64_t lds_bytes, uint32_t seed, bool invert,
                                         uint32_t visit) {
  const uint32_t bytes = checked_lds_bytes(lds_bytes);
  DeviceScope scope;
  uint32_t* d_out = (uint32_t*)scope.alloc(bytes);
  HIP_CHECK(hipMemset(d_out, 0xA5, bytes));
  allow_dynamic_lds(cu_lds_dump_kernel, bytes);
  hipLaunchKernelGGL(cu_lds_dump_kernel, dim3(1), dim3(kSweepThreads), bytes, 0, d_out,
                     bytes, seed, visit, invert ? 0xFFFFFFFFu : 0u);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  std::string host(bytes, '\0');
  HIP_CHECK(hipMemcpy(&host[0], d_out, bytes, hipMemcpyDeviceToHost));
  return host;
}

// ---------------------------------------------------------------------------
// Burn-in, part 4: MFMA load — all four matrix pipes of every CU kept busy for
// seconds on exact tiles, checked every check_every MFMAs, timed by the waves
//
// The chain and why it stays exact are in gpuhealth_ref.hpp (alternating-sign
// premise). A workgroup is four waves, one per SIMD, and takes the whole LDS of
// its CU as the sweep does; a wave keeps kLoadTiles independent chains going.
// No workgroup waits on another and no kernel waits on a clock: a launch is
// bounded by n_mfmas x chunks alone.
// ---------------------------------------------------------------------------
constexpr int kLoadWaves = (int)gh::kLoadWaves;
constexpr int kLoadTiles = (int)gh::kLoadTiles;
constexpr int kLoadThreads = 64 * kLoadWaves;
// +A / -A pairs per trip of the inner loop: 64 MFMAs. With one wave per SIMD
// nothing hides the loop's branch, some 19 cycles a trip; at one pair (8
// MFMAs, 128 cycles) per trip that is 15 %, at eight pairs under 2 %.
constexpr uint32_t kLoadUnroll = 8;

struct LoadSlot {
  unsigned int visits;
  unsigned int simd_seen;  // bit s: a wave of some visit ran on SIMD s
  unsigned int bad[gh::kNumSimds];  // D elements that failed a check, by SIMD
  // sums over the waves that ran here: s_memtime and s_memrealtime around the
  // loop, and the MFMAs issued inside it
  unsigned long long cycles, ticks, mfmas;
};

// where the workgroup of the injected visit ran (INJECT instantiation only)
struct LoadRecord {
  unsigned int written, key;
  unsigned int simd[kLoadWaves];
};

// Test hook: an xor into one accumulator register of lane 0, applied after
// MFMA number `after` (0-based, of that tile) of chunk `chunk`.
struct LoadInject {
  uint32_t visit = 0, wave = 0, tile = 0, chunk = 0, after = 0, reg = 0, mask = 0;
};

// mask is zero everywhere but in the lane, chunk and MFMA the hook names
__device__ inline void xor_accumulator(frag_cd_t (&acc)[kLoadTiles], uint32_t tile,
                                       uint32_t reg, uint32_t mask) {
#pragma unroll
  for (uint32_t t = 0; t < (uint32_t)kLoadTiles; ++t)
    for (uint32_t r = 0; r < 4; ++r)
      if (t == tile && r == reg) acc[t][r] = gh::bits_f32(gh::f32_bits(acc[t][r]) ^ mask);
}

// n_mfmas per tile and chunk: the production host passes an odd number, so a
// chunk ends on C + A·B; the dump hook passes any. dump (DUMP only) receives
// the accumulators as the last chunk left them, tile (wave, t) row-major at
// dump + 256 * (kLoadTiles * wave + t). dump_same_sign (read by DUMP only; it
// lies in what was padding behind inj, so no other argument moves) puts A where
// -A belongs: the same loop then leaves C + n_mfmas·A·B, which tells every
// count from every other where the alternating chain tells odd from even.
template <int DT, bool INJECT = false, bool DUMP = false>
__global__ __launch_bounds__(kLoadThreads) void mfma_load_kernel(
    LoadSlot* __restrict__ slots, uint32_t visit_base, uint32_t seed, uint32_t n_mfmas,
    uint32_t chunks, LoadInject inj, uint32_t dump_same_sign,
    LoadRecord* __restrict__ record, float* __restrict__ dump) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t visit = visit_base + blockIdx.x;
  const uint32_t col = lane & 15, row0 = 4 * (lane >> 4);

  const uint32_t xcc_reg = read_xcc_id_reg(), hw_reg = read_hw_id_reg();
  const gh::CuLocation loc = gh::decode_location(xcc_reg, hw_reg);
  const uint32_t key = gh::location_key(loc);
  LoadSlot* slot = slots + key;

  // operands and both expectations, once per operand set; the expectation is
  // integer arithmetic over the generators, off the matrix pipe
  ExactOperands<DT> pos[kLoadTiles], neg[kLoadTiles];
  frag_cd_t c0[kLoadTiles], want[kLoadTiles], acc[kLoadTiles];
#pragma unroll
  for (int t = 0; t < kLoadTiles; ++t) {
    const uint32_t wg = gh::load_tile_index(visit, wave, (uint32_t)t);
    pos[t] = pack_exact_operands<DT>(seed, wg, lane);
    neg[t] = negated_a<DT>(pos[t]);
    if constexpr (DUMP) {
      if (dump_same_sign) neg[t] = pos[t];
    }
    for (uint32_t r = 0; r < 4; ++r) {
      c0[t][r] = gh::expected_after(DT, seed, wg, row0 + r, col, 0);
      want[t][r] = gh::expected_after(DT, seed, wg, row0 + r, col, n_mfmas);
    }
  }

  const uint32_t pairs = (n_mfmas - 1) / 2;
  const bool tail = ((n_mfmas - 1) & 1u) != 0;
  [[maybe_unused]] const bool inj_here =
      INJECT && visit == inj.visit && wave == inj.wave && lane == 0;
  unsigned int bad = 0;

  const uint64_t cycles0 = __builtin_amdgcn_s_memtime();
  const uint64_t ticks0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_sched_barrier(0);
  for (uint32_t chunk = 0; chunk < chunks; ++chunk) {
    [[maybe_unused]] const bool inj_chunk = inj_here && chunk == inj.chunk;
    // acc = C again; opaque, so that no MFMA of a chunk is loop-invariant
#pragma unroll
    for (int t = 0; t < kLoadTiles; ++t) {
      acc[t] = c0[t];
      asm volatile("" : "+v"(acc[t]));
    }
#pragma unroll
    for (int t = 0; t < kLoadTiles; ++t) acc[t] = issue_exact_mfma<DT>(pos[t], acc[t]);
    if constexpr (INJECT)
      xor_accumulator(acc, inj.tile, inj.reg, inj_chunk && inj.after == 0 ? inj.mask : 0u);
    auto pair = [&](uint32_t p) {
#pragma unroll
      for (int t = 0; t < kLoadTiles; ++t) acc[t] = issue_exact_mfma<DT>(neg[t], acc[t]);
      if constexpr (INJECT)
        xor_accumulator(acc, inj.tile, inj.reg,
                        inj_chunk && inj.after == 2 * p + 1 ? inj.mask : 0u);
#pragma unroll
      for (int t = 0; t < kLoadTiles; ++t) acc[t] = issue_exact_mfma<DT>(pos[t], acc[t]);
      if constexpr (INJECT)
        xor_accumulator(acc, inj.tile, inj.reg,
                        inj_chunk && inj.after == 2 * p + 2 ? inj.mask : 0u);
    };
    // one wave per SIMD: nothing hides the loop branch, so it is paid once per
    // kLoadUnroll pairs (64 MFMAs) and not once per pair. Unrolled by hand: the
    // compiler does not unroll a loop of MFMAs with a run-time trip count.
    uint32_t p = 0;
    for (; p + kLoadUnroll <= pairs; p += kLoadUnroll) {
#pragma unroll
      for (uint32_t u = 0; u < kLoadUnroll; ++u) pair(p + u);
    }
    for (; p < pairs; ++p) pair(p);
    if (tail) {
#pragma unroll
      for (int t = 0; t < kLoadTiles; ++t) acc[t] = issue_exact_mfma<DT>(neg[t], acc[t]);
      if constexpr (INJECT)
        xor_accumulator(acc, inj.tile, inj.reg,
                        inj_chunk && inj.after == n_mfmas - 1 ? inj.mask : 0u);
    }
    // the compare of one tile runs under the last MFMAs of the others
#pragma unroll
    for (int t = 0; t < kLoadTiles; ++t)
      for (uint32_t r = 0; r < 4; ++r) bad += !(acc[t][r] == want[t][r]);
  }
  __builtin_amdgcn_sched_barrier(0);
  const uint64_t cycles1 = __builtin_amdgcn_s_memtime();
  const uint64_t ticks1 = __builtin_amdgcn_s_memrealtime();

  if constexpr (DUMP) {
#pragma unroll
    for (int t = 0; t < kLoadTiles; ++t) {
      float* tile = dump + 256 * (kLoadTiles * wave + t);
      for (uint32_t r = 0; r < 4; ++r) tile[(row0 + r) * 16 + col] = acc[t][r];
    }
  }

  // publish: wave reductions, then lane 0 alone
  if (__ballot(bad != 0) != 0) {
    const unsigned int wave_bad = (unsigned int)wave_sum_u64(bad);
    if (lane == 0) atomicAdd(&slot->bad[loc.simd], wave_bad);
  }
  if (lane != 0) return;
  atomicOr(&slot->simd_seen, 1u << loc.simd);
  atomicAdd(&slot->cycles, (unsigned long long)(cycles1 - cycles0));
  atomicAdd(&slot->ticks, (unsigned long long)(ticks1 - ticks0));
  atomicAdd(&slot->mfmas, (unsigned long long)kLoadTiles * n_mfmas * chunks);
  if (wave == 0) atomicAdd(&slot->visits, 1u);
  if constexpr (INJECT) {
    if (visit == inj.visit) {
      record->simd[wave] = loc.simd;
      if (wave == 0) {
        record->key = key;
        record->written = 1;
      }
    }
  }
}

// The smallest of 127, 143, ... 255 (steps of 16) whose TFLOP/s is within 3 %
// of the rate at 4095 for every data type; fp8 decides (2346 against 2413; 223
// gives 2339), bf16 alone would take 175, f16 159, MXFP4 127. And a launch
// length at which the once-per-launch operand build costs 0.3 % (MXFP4 2.7 %)
// (docs/benchmarks.md, "MFMA load").
constexpr int kLoadDefaultCheckEvery = 239;
constexpr double kLoadDefaultLaunchMs = 50.0;
constexpr int kLoadMaxCheckEvery = 4095;
constexpr int kLoadMaxBlocks = 1 << 14;
constexpr double kLoadMaxSeconds = 60.0;
// MFMAs per tile of one launch: about half a second of one wave
constexpr uint64_t kLoadMaxLaunchMfmas = 1ull << 24;
// MFMAs per tile of the calibration launch: about a millisecond
constexpr uint32_t kLoadCalibrationMfmas = 1u << 15;

struct LoadArgs {
  LoadSlot* slots;
  uint32_t visit_base, seed, n_mfmas, chunks;
  LoadInject inj;
  LoadRecord* record;
  float* dump;
  uint32_t dump_same_sign = 0;  // the dump hook's alternate=False
};

template <int DT, bool INJECT, bool DUMP>
static void launch_load_as(int blocks, uint32_t lds_bytes, const LoadArgs& a) {
  auto kernel = mfma_load_kernel<DT, INJECT, DUMP>;
  allow_dynamic_lds(kernel, lds_bytes);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kLoadThreads), lds_bytes, 0, a.slots,
                     a.visit_base, a.seed, a.n_mfmas, a.chunks, a.inj, a.dump_same_sign,
                     a.record, a.dump);
}

template <int DT>
static void launch_load_dt(int blocks, uint32_t lds_bytes, const LoadArgs& a) {
  if (a.dump) launch_load_as<DT, false, true>(blocks, lds_bytes, a);
  else if (a.record) launch_load_as<DT, true, false>(blocks, lds_bytes, a);
  else launch_load_as<DT, false, false>(blocks, lds_bytes, a);
}

// a.dump selects the dump instantiation, a.record the INJECT one, neither the
// production kernel
static void launch_mfma_load(int dtype, int blocks, uint32_t lds_bytes, const LoadArgs& a) {
  switch (dtype) {
    case gh::BF16: launch_load_dt<gh::BF16>(blocks, lds_bytes, a); break;
    case gh::F16: launch_load_dt<gh::F16>(blocks, lds_bytes, a); break;
    case gh::FP8: launch_load_dt<gh::FP8>(blocks, lds_bytes, a); break;
    default: launch_load_dt<gh::MXFP4>(blocks, lds_bytes, a); break;
  }
  HIP_CHECK(hipGetLastError());
}

struct LoadResult {
  int dtype = 0;
  int cu_total = 0;
  int launches = 0;
  int blocks = 0;
  uint32_t check_every = 0, chunks = 0;
  double elapsed_ms = 0.0;
  double floor_tflops = 0.0;
  std::vector<LoadSlot> slots;
  bool injected = false, have_record = false;
  LoadRecord record{};
};

// seconds == 0: exactly one launch of blocks workgroups (0: 4 x CUs) with
// chunks chunks of check_every MFMAs per tile. seconds > 0: chunks == 0 lets a
// short first launch size chunks so that a launch lasts about launch_ms; then
// launches go back to back, at most two in flight, until the event-timed
// elapsed time reaches seconds. The slot table is read once at the end.
static LoadResult run_mfma_load(int dtype, double seconds, int check_every, int64_t chunks_in,
                                int blocks, double launch_ms, uint32_t seed,
                                double floor_tflops, const LoadInject* inject) {
  if (!(seconds >= 0.0) || seconds > kLoadMaxSeconds)
    throw py::value_error("seconds must be in [0, 60]");
  if (check_every < 1 || check_every > kLoadMaxCheckEvery || check_every % 2 == 0)
    throw py::value_error("check_every must be odd and in [1, 4095]");
  const uint64_t max_chunks = kLoadMaxLaunchMfmas / (uint64_t)check_every;
  if (chunks_in < 0 || (uint64_t)chunks_in > max_chunks)
    throw py::value_error("chunks must be in [0, 2^24 / check_every]");
  if (seconds == 0.0 && chunks_in == 0)
    throw py::value_error("chunks must be at least 1 when seconds is 0");
  if (!(launch_ms >= 1.0) || launch_ms > 1000.0)
    throw py::value_error("launch_ms must be in [1, 1000]");
  if (!(floor_tflops >= 0.0)) throw py::value_error("floor_tflops must not be negative");
  if (inject && seconds != 0.0)
    throw py::value_error("inject_acc needs seconds == 0, the one launch it names");

  LoadResult res;
  res.dtype = dtype;
  res.floor_tflops = floor_tflops;
  res.check_every = (uint32_t)check_every;
  res.cu_total = current_device_attribute(hipDeviceAttributeMultiprocessorCount);
  if (blocks == 0) blocks = 4 * res.cu_total;
  if (blocks < 1 || blocks > kLoadMaxBlocks)
    throw py::value_error("blocks must be 0 or in [1, 2^14]");
  res.blocks = blocks;
  if (inject) {
    if (inject->visit >= (uint32_t)blocks)
      throw py::value_error("injected visit is outside the launch");
    if (inject->chunk >= (uint64_t)chunks_in)
      throw py::value_error("injected chunk is outside [0, chunks)");
    if (inject->after >= (uint32_t)check_every)
      throw py::value_error("injected MFMA is outside [0, check_every)");
    res.injected = true;
  }
  const uint32_t lds_bytes = checked_lds_bytes(0);

  DeviceScope scope;
  res.slots.assign(gh::kCuSlots, LoadSlot{});
  const size_t slot_bytes = gh::kCuSlots * sizeof(LoadSlot);
  LoadSlot* d_slots = (LoadSlot*)scope.alloc(slot_bytes);
  HIP_CHECK(hipMemset(d_slots, 0, slot_bytes));
  LoadRecord* d_record = nullptr;
  if (inject) {
    d_record = (LoadRecord*)scope.alloc(sizeof(LoadRecord));
    HIP_CHECK(hipMemset(d_record, 0, sizeof(LoadRecord)));
  }

  LoadArgs args{d_slots, 0, seed, (uint32_t)check_every, (uint32_t)chunks_in,
                inject ? *inject : LoadInject{}, d_record, nullptr};
  auto launch = [&]() {
    args.visit_base = (uint32_t)((uint64_t)res.launches * blocks);
    launch_mfma_load(dtype, blocks, lds_bytes, args);
    ++res.launches;
  };
  auto ms_between = [](hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return (double)ms;
  };

  const double want_ms = seconds * 1e3;
  hipEvent_t t0 = scope.event(), done[2] = {scope.event(), scope.event()};
  HIP_CHECK(hipEventRecord(t0, 0));
  if (seconds == 0.0) {
    launch();
    HIP_CHECK(hipEventRecord(done[0], 0));
    HIP_CHECK(hipEventSynchronize(done[0]));
    res.elapsed_ms = ms_between(t0, done[0]);
  } else {
    if (chunks_in == 0) {
      // the calibration launch is the run's first: what it checks and issues
      // counts like any other launch's
      args.chunks = std::max(1u, kLoadCalibrationMfmas / (uint32_t)check_every);
      launch();
      HIP_CHECK(hipEventRecord(done[0], 0));
      HIP_CHECK(hipEventSynchronize(done[0]));
      const double cal_ms = std::max(ms_between(t0, done[0]), 1e-3);
      const double scaled = (double)args.chunks * launch_ms / cal_ms;
      args.chunks = (uint32_t)std::min((double)max_chunks, std::max(1.0, scaled));
    }
    // launch n's end is done[n & 1]; elapsed and last are known up to launch n
    int first = res.launches;
    launch();
    HIP_CHECK(hipEventRecord(done[first & 1], 0));
    double prev_end = first ? ms_between(t0, done[0]) : 0.0, last = launch_ms;
    for (int n = first;; ++n) {
      // launch n is in flight. Another goes behind it unless launch n is
      // expected to reach the time asked for.
      const bool more = prev_end + last < want_ms;
      if (more) {
        launch();
        HIP_CHECK(hipEventRecord(done[(n + 1) & 1], 0));
      }
      HIP_CHECK(hipEventSynchronize(done[n & 1]));
      const double end = ms_between(t0, done[n & 1]);
      last = end - prev_end;
      prev_end = end;
      if (more) continue;
      if (end >= want_ms) break;
      launch();  // the estimate fell short: one more, alone
      HIP_CHECK(hipEventRecord(done[(n + 1) & 1], 0));
    }
    res.elapsed_ms = prev_end;
  }
  res.chunks = args.chunks;
  HIP_CHECK(hipMemcpy(res.slots.data(), d_slots, slot_bytes, hipMemcpyDeviceToHost));
  if (inject) {
    HIP_CHECK(hipMemcpy(&res.record, d_record, sizeof(LoadRecord), hipMemcpyDeviceToHost));
    res.have_record = res.record.written != 0;
  }
  return res;
}

// test hook: the accumulators of one workgroup's kLoadWaves x kLoadTiles tiles
// after exactly n_mfmas MFMAs each, through the production packing and loop;
// alternate == false issues +A every time (C + n_mfmas·A·B)
static std::string run_debug_mfma_load_dump(int dtype, int64_t n_mfmas, uint32_t seed,
                                            uint32_t visit, bool alternate) {
  if (n_mfmas < 1 || n_mfmas > kLoadMaxCheckEvery)
    throw py::value_error("mfmas must be in [1, 4095]");
  const size_t bytes = (size_t)kLoadWaves * kLoadTiles * 256 * sizeof(float);
  DeviceScope scope;
  float* d_out = (float*)scope.alloc(bytes);
  LoadSlot* d_slots = (LoadSlot*)scope.alloc(gh::kCuSlots * sizeof(LoadSlot));
  HIP_CHECK(hipMemset(d_out, 0xFF, bytes));  // an unwritten element reads as NaN
  HIP_CHECK(hipMemset(d_slots, 0, gh::kCuSlots * sizeof(LoadSlot)));
  launch_mfma_load(dtype, 1, checked_lds_bytes(0),
                   LoadArgs{d_slots, visit, seed, (uint32_t)n_mfmas, 1, LoadInject{}, nullptr,
                            d_out, alternate ? 0u : 1u});
  HIP_CHECK(hipDeviceSynchronize());
  std::string host(bytes, '\0');
  HIP_CHECK(hipMemcpy(&host[0], d_out, bytes, hipMemcpyDeviceToHost));
  return host;
}

// ---------------------------------------------------------------------------
// host API
// ---------------------------------------------------------------------------
static py::dict device_info(int device) {
  use_device(device);
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  py::dict d;
  d["name"] = std::string(prop.name);
  d["gcn_arch"] = std::string(prop.gcnArchName);
  d["total_mem_gb"] = (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0);
  d["multi_processor_count"] = prop.multiProcessorCount;
  d["warp_size"] = prop.warpSize;
  d["clock_mhz"] = prop.clockRate / 1000;
  return d;
}

static bool mfma_smoke(int device, int workgroups, corruptions_t corruptions,
                       int launch_workgroups) {
  use_device(device);
  return run_mfma_smoke(workgroups, std::move(corruptions), launch_workgroups);
}

// test hook: the raw fp32 buffer the smoke check reads, through the same code
static py::bytes debug_mfma_smoke_dump(int device, int workgroups, int launch_workgroups) {
  if (workgroups < 1 || workgroups > 4096)
    throw py::value_error("workgroups must be in [1, 4096]");
  use_device(device);
  std::string raw;
  (void)run_mfma_smoke(workgroups, {}, launch_workgroups, &raw);
  return py::bytes(raw);
}

static double hbm_bandwidth_gb_s(int device, double gib, int iters) {
  use_device(device);
  size_t bytes = (size_t)(gib * 1024.0 * 1024.0 * 1024.0);
  if (bytes < (64u << 20)) bytes = (64u << 20);
  return run_hbm_stream(bytes, iters);
}

static py::dict health_check(int device, double hbm_floor_gb_s, bool quick) {
  py::dict result;
  use_device(device);
  bool mfma_ok = run_mfma_smoke(quick ? 256 : 2048);
  // quick: 0.5 GiB per buffer (still > L2, probes real HBM); full: 4 GiB
  // (> 256 MiB L3 several times over per pass).
  double bw = run_hbm_stream(quick ? (512ull << 20) : (4ull << 30), quick ? 3 : 10);
  result["mfma_ok"] = mfma_ok;
  result["hbm_gb_s"] = bw;
  result["hbm_ok"] = bw >= hbm_floor_gb_s;
  result["healthy"] = mfma_ok && bw >= hbm_floor_gb_s;
  return result;
}

// -- burn-in bindings --------------------------------------------------------
static int parse_dtype(const std::string& s) {
  if (s == "bf16") return gh::BF16;
  if (s == "f16") return gh::F16;
  if (s == "fp8") return gh::FP8;
  if (s == "mxfp4") return gh::MXFP4;
  throw py::value_error("dtype must be one of bf16, f16, fp8, mxfp4 (got '" + s + "')");
}

static py::dict pattern_dict(const PatternResult& r) {
  py::dict d;
  d["bytes_checked"] = r.bytes_checked;
  d["chunks"] = r.chunks;
  d["mismatched_words"] = r.stats.mismatched_words;
  d["flipped_bits"] = r.stats.flipped_bits;
  d["bad_bit_mask"] = r.stats.bad_bit_mask;
  d["first_bad_offset"] = r.stats.first_bad_word == kNoBadWord
                              ? (int64_t)-1 : (int64_t)(4 * r.stats.first_bad_word);
  d["gb_s"] = r.gb_s;
  return d;
}

// corrupt_word >= 0 with corrupt_bit is shorthand for
// corruptions = [(corrupt_word, 1 << corrupt_bit)]
static py::dict hbm_pattern_check(int device, double mib, double fraction,
                                  uint32_t seed, int64_t corrupt_word,
                                  int corrupt_bit, uint64_t bytes,
                                  uint64_t max_chunk_mib, int passes,
                                  uint64_t base_word, corruptions_t corruptions,
                                  std::pair<int, int> corrupt_at, stuck_t stuck) {
  if (bytes == 0 && fraction == 0.0) {
    if (!(mib > 0.0)) throw py::value_error("mib must be positive");
    bytes = (uint64_t)(mib * 1048576.0) & ~(uint64_t)15;
  }
  if (max_chunk_mib == 0 || max_chunk_mib > 16384)
    throw py::value_error("max_chunk_mib must be in [1, 16384]");
  if (corrupt_bit < 0 || corrupt_bit > 31) throw py::value_error("corrupt_bit must be in [0, 31]");
  if (corrupt_word < -1) throw py::value_error("corrupt_word is outside the swept range");
  if (corrupt_word >= 0) corruptions.emplace_back(corrupt_word, (int64_t)1 << corrupt_bit);
  use_device(device);
  return pattern_dict(run_hbm_pattern(bytes, fraction, seed, passes, max_chunk_mib << 20,
                                      base_word, std::move(corruptions),
                                      corrupt_at.first, corrupt_at.second, std::move(stuck)));
}

static py::bytes debug_pattern_fill(int device, uint64_t bytes, uint32_t seed,
                                    bool invert, uint64_t base_word) {
  use_device(device);
  return py::bytes(run_debug_pattern_fill(bytes, seed, invert, base_word));
}

static py::dict debug_stream_copy_check(int device, uint64_t bytes, uint32_t seed) {
  use_device(device);
  const StreamCopyResult r = run_debug_stream_copy(bytes, seed);
  py::dict d = pattern_dict(r.pattern);
  d["guard_intact"] = r.guard_intact;
  return d;
}

static py::dict mfma_dict(const MfmaResult& r) {
  py::dict d;
  d["tiles"] = r.tiles;
  d["mismatches"] = r.mismatches;
  if (r.first_bad < 0) {
    d["first_bad"] = py::none();
  } else {
    d["first_bad"] = py::make_tuple(r.first_bad / 256, r.first_bad / 16 % 16,
                                    r.first_bad % 16, r.got, r.expected);
  }
  return d;
}

// corrupt_element >= 0 is shorthand for corruptions = [(corrupt_element,
// 1 << 20)], one mantissa bit
// (workgroup, lane, operand, reg, mask); what depends on the data type and the
// launch is checked by check_operand_inject
typedef std::optional<std::tuple<int64_t, int64_t, std::string, int64_t, int64_t>>
    inject_operand_t;

static std::optional<OperandInject> checked_operand_inject(const inject_operand_t& in) {
  if (!in) return std::nullopt;
  const auto& [wg, lane, operand, reg, mask] = *in;
  static const char* const kNames[] = {"a", "b", "c", "sa", "sb"};
  OperandInject inj;
  inj.operand = 5;
  for (uint32_t n = 0; n < 5; ++n)
    if (operand == kNames[n]) inj.operand = n;
  if (inj.operand == 5)
    throw py::value_error("operand must be one of a, b, c, sa, sb (got '" + operand + "')");
  inj.wg = checked_index(wg, 1ull << 20, "injected workgroup");
  inj.lane = checked_index(lane, 64, "injected lane");
  inj.reg = checked_index(reg, 8, "injected register");
  inj.mask = checked_mask(mask);
  return inj;
}

static py::dict mfma_verify(int device, const std::string& dtype, int workgroups,
                            uint32_t seed, int64_t corrupt_element,
                            corruptions_t corruptions, inject_operand_t inject_operand) {
  const int dt = parse_dtype(dtype);
  if (corrupt_element < -1) throw py::value_error("corrupt_element is outside the output buffer");
  if (corrupt_element >= 0) corruptions.emplace_back(corrupt_element, (int64_t)1 << 20);
  const std::optional<OperandInject> inj = checked_operand_inject(inject_operand);
  use_device(device);
  return mfma_dict(run_mfma_verify(dt, workgroups, seed, std::move(corruptions),
                                   inj ? &*inj : nullptr));
}

static py::bytes debug_mfma_dump(int device, const std::string& dtype, int workgroups,
                                 uint32_t seed, inject_operand_t inject_operand) {
  const int dt = parse_dtype(dtype);
  const std::optional<OperandInject> inj = checked_operand_inject(inject_operand);
  use_device(device);
  return py::bytes(run_debug_mfma_dump(dt, workgroups, seed, inj ? &*inj : nullptr));
}

typedef std::vector<std::vector<float>> matrix_t;

static py::tuple mfma_verify_tile(int device, const std::string& dtype,
                                  uint32_t seed, uint32_t workgroup) {
  const int dt = parse_dtype(dtype);
  const uint32_t K = (uint32_t)gh::k_of(dt);
  matrix_t A(16, std::vector<float>(K)), B(K, std::vector<float>(16)),
      C(16, std::vector<float>(16)), D(16, std::vector<float>(16));
  for (uint32_t i = 0; i < 16; ++i) {
    for (uint32_t k = 0; k < K; ++k) {
      A[i][k] = gh::logical_a(dt, seed, workgroup, i, k);
      B[k][i] = gh::logical_b(dt, seed, workgroup, k, i);
    }
    for (uint32_t c = 0; c < 16; ++c) C[i][c] = (float)gh::gen_c(seed, workgroup, dt, i, c);
  }
  use_device(device);
  DeviceScope scope;
  float* d_out = (float*)scope.alloc(256 * sizeof(float));
  launch_mfma_exact(dt, d_out, 1, seed, workgroup);
  HIP_CHECK(hipDeviceSynchronize());
  float host[256];
  HIP_CHECK(hipMemcpy(host, d_out, sizeof(host), hipMemcpyDeviceToHost));
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) D[r][c] = host[r * 16 + c];
  return py::make_tuple(A, B, C, D);
}

static matrix_t reference_tile_py(const std::string& dtype, uint32_t seed,
                                  uint32_t workgroup) {
  float ref[16][16];
  gh::reference_tile(parse_dtype(dtype), seed, workgroup, ref);
  matrix_t D(16, std::vector<float>(16));
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) D[r][c] = ref[r][c];
  return D;
}

static const char* const kDtypeNames[gh::kNumDtypes] = {"bf16", "f16", "fp8", "mxfp4"};

// -- CU sweep bindings -------------------------------------------------------
typedef std::optional<std::tuple<int64_t, int64_t, int64_t, int64_t>> inject_lds_t;
typedef std::optional<std::tuple<int64_t, int64_t, std::string, int64_t, int64_t>> inject_mfma_t;

// everything that does not depend on the device; run_cu_sweep checks the rest
static CuInject checked_inject(const inject_lds_t& lds, const inject_mfma_t& mfma,
                               const inject_lds_t& stuck) {
  CuInject inj;
  if (lds && stuck)
    throw py::value_error("inject_lds and inject_lds_stuck cannot be combined");
  if (stuck) {
    const auto& [visit, word, mask, value] = *stuck;
    inj.stuck_on = 1;
    inj.stuck_visit = checked_index(visit, kSweepMaxVisits, "injected visit");
    inj.stuck_word = checked_index(word, 1ull << 30, "stuck LDS word");
    inj.stuck_mask = checked_mask(mask);
    if (value != 0 && value != 1) throw py::value_error("stuck value must be 0 or 1");
    inj.stuck_value = (uint32_t)value;
  }
  if (lds) {
    const auto& [visit, word, mask, phase] = *lds;
    inj.lds_on = 1;
    inj.lds_visit = checked_index(visit, kSweepMaxVisits, "injected visit");
    inj.lds_word = checked_index(word, 1ull << 30, "injected LDS word");
    inj.lds_mask = checked_mask(mask);
    inj.lds_phase = checked_index(phase, 2, "injected phase");
  }
  if (mfma) {
    const auto& [visit, wave, dtype, element, mask] = *mfma;
    inj.mfma_on = 1;
    inj.mfma_visit = checked_index(visit, kSweepMaxVisits, "injected visit");
    inj.mfma_wave = checked_index(wave, kSweepWaves, "injected wave");
    inj.mfma_dtype = (uint32_t)parse_dtype(dtype);
    inj.mfma_element = checked_index(element, 256, "injected D element");
    inj.mfma_mask = checked_mask(mask);
  }
  if (lds && mfma && inj.lds_visit != inj.mfma_visit)
    throw py::value_error("inject_lds and inject_mfma must name the same visit");
  if (stuck && mfma && inj.stuck_visit != inj.mfma_visit)
    throw py::value_error("inject_lds_stuck and inject_mfma must name the same visit");
  return inj;
}

static py::dict location_dict(uint32_t key) {
  const gh::CuLocation loc = gh::location_of_key(key);
  py::dict d;
  d["xcc"] = loc.xcc;
  d["se"] = loc.se;
  d["sh"] = loc.sh;
  d["cu"] = loc.cu;
  return d;
}

static py::dict lds_stats_dict(const LdsStats& s) {
  py::dict d;
  d["bad_words"] = s.bad_words;
  d["flipped_bits"] = s.flipped_bits;
  d["bad_bit_mask"] = s.bad_bit_mask;
  d["first_bad_word"] = s.first_bad_word == kNoBadWord ? (int64_t)-1
                                                       : (int64_t)s.first_bad_word;
  return d;
}

static bool slot_faulty(const CuSlot& s) {
  if (s.lds.bad_words != 0) return true;
  for (uint32_t simd = 0; simd < gh::kNumSimds; ++simd)
    for (int dt = 0; dt < gh::kNumDtypes; ++dt)
      if (s.mfma_bad[simd][dt] != 0) return true;
  return false;
}

static py::dict cu_sweep_dict(const CuSweepResult& r, bool injected) {
  constexpr unsigned int kAllSimds = (1u << gh::kNumSimds) - 1u;
  py::dict d, xcc_covered;
  py::list faulty, locations;
  int covered = 0;
  bool simd_complete = true;
  for (uint32_t key = 0; key < gh::kCuSlots; ++key) {
    const CuSlot& s = r.slots[key];
    if (s.visits == 0) continue;
    ++covered;
    simd_complete = simd_complete && s.simd_seen == kAllSimds;
    py::dict where = location_dict(key);
    py::object xcc = where["xcc"];
    xcc_covered[xcc] = (xcc_covered.contains(xcc) ? xcc_covered[xcc].cast<int>() : 0) + 1;
    if (slot_faulty(s)) {
      py::dict f = location_dict(key);
      f["lds"] = lds_stats_dict(s.lds);
      py::list mfma;
      for (uint32_t simd = 0; simd < gh::kNumSimds; ++simd)
        for (int dt = 0; dt < gh::kNumDtypes; ++dt)
          if (s.mfma_bad[simd][dt] != 0) mfma.append(py::make_tuple(simd, kDtypeNames[dt]));
      f["mfma"] = mfma;
      faulty.append(f);
    }
    where["visits"] = s.visits;
    where["simd_seen"] = s.simd_seen;
    locations.append(where);
  }
  d["cu_total"] = r.cu_total;
  d["cu_covered"] = covered;
  d["rounds"] = r.rounds;
  d["lds_bytes"] = r.lds_bytes;
  d["blocks_per_round"] = r.blocks_per_round;
  d["elapsed_ms"] = r.elapsed_ms;
  d["xcc_covered"] = xcc_covered;
  d["simd_complete"] = simd_complete;
  d["faulty"] = faulty;
  d["locations"] = locations;
  if (injected) {
    if (!r.have_record) {
      d["record"] = py::none();
    } else {
      py::dict rec = location_dict(r.record.key);
      LdsStats sum{0, 0, kNoBadWord, 0, 0};
      py::list simd;
      for (int w = 0; w < kSweepWaves; ++w) {
        simd.append(r.record.simd[w]);
        sum.bad_words += r.record.lds[w].bad_words;
        sum.flipped_bits += r.record.lds[w].flipped_bits;
        sum.first_bad_word = std::min(sum.first_bad_word, r.record.lds[w].first_bad_word);
        sum.bad_bit_mask |= r.record.lds[w].bad_bit_mask;
      }
      rec["simd"] = simd;
      rec["lds"] = lds_stats_dict(sum);
      rec["xcc_id_reg"] = r.record.xcc_id_reg;
      rec["hw_id_reg"] = r.record.hw_id_reg;
      d["record"] = rec;
    }
  }
  return d;
}

static py::dict cu_sweep(int device, uint32_t seed, int passes, uint64_t lds_bytes,
                         int blocks_per_round, int max_rounds, inject_lds_t inject_lds,
                         inject_mfma_t inject_mfma, inject_lds_t inject_lds_stuck) {
  const CuInject inj = checked_inject(inject_lds, inject_mfma, inject_lds_stuck);
  use_device(device);
  return cu_sweep_dict(run_cu_sweep(seed, passes, lds_bytes, blocks_per_round, max_rounds, inj),
                       inj.lds_on || inj.stuck_on || inj.mfma_on);
}

static py::dict decode_location_py(uint32_t xcc_id_reg, uint32_t hw_id_reg) {
  const gh::CuLocation loc = gh::decode_location(xcc_id_reg, hw_id_reg);
  py::dict d = location_dict(gh::location_key(loc));
  d["simd"] = loc.simd;
  d["key"] = gh::location_key(loc);
  return d;
}

static py::bytes debug_cu_lds_dump(int device, uint64_t lds_bytes, uint32_t seed, bool invert,
                                   int64_t visit) {
  const uint32_t v = checked_index(visit, 1ull << 32, "visit");
  use_device(device);
  return py::bytes(run_debug_cu_lds_dump(lds_bytes, seed, invert, v));
}

// -- MFMA load bindings ------------------------------------------------------
// (visit, wave, tile, chunk, after_mfma, register, mask); what depends on the
// launch is checked by run_mfma_load
typedef std::optional<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>>
    inject_acc_t;

static std::optional<LoadInject> checked_load_inject(const inject_acc_t& in) {
  if (!in) return std::nullopt;
  const auto& [visit, wave, tile, chunk, after, reg, mask] = *in;
  LoadInject inj;
  inj.visit = checked_index(visit, kLoadMaxBlocks, "injected visit");
  inj.wave = checked_index(wave, kLoadWaves, "injected wave");
  inj.tile = checked_index(tile, kLoadTiles, "injected tile");
  inj.chunk = checked_index(chunk, kLoadMaxLaunchMfmas, "injected chunk");
  inj.after = checked_index(after, kLoadMaxCheckEvery, "injected MFMA");
  inj.reg = checked_index(reg, 4, "injected register");
  inj.mask = checked_mask(mask);
  return inj;
}

static double median_of(std::vector<double> v) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

// clock_mhz and cycles_per_mfma are medians over the covered CUs of each CU's
// sums over its waves (the table keeps sums, not one entry per wave)
static py::dict mfma_load_dict(const LoadResult& r) {
  py::dict d;
  py::list faulty, locations;
  std::vector<double> clocks, cycles_per;
  unsigned long long mfmas = 0, bad_total = 0;
  int covered = 0;
  double slowest = 0.0;
  py::object slowest_cu = py::none();
  for (uint32_t key = 0; key < gh::kCuSlots; ++key) {
    const LoadSlot& s = r.slots[key];
    if (s.visits == 0 && s.simd_seen == 0) continue;
    ++covered;
    mfmas += s.mfmas;
    if (s.ticks != 0) clocks.push_back((double)s.cycles / (double)s.ticks * 100.0);
    if (s.mfmas != 0) {
      const double per = (double)s.cycles / (double)s.mfmas;
      cycles_per.push_back(per);
      if (per > slowest) {
        slowest = per;
        slowest_cu = location_dict(key);
      }
    }
    for (uint32_t simd = 0; simd < gh::kNumSimds; ++simd) {
      if (s.bad[simd] == 0) continue;
      bad_total += s.bad[simd];
      py::dict f = location_dict(key);
      f["simd"] = simd;
      f["dtype"] = kDtypeNames[r.dtype];
      f["bad_elements"] = s.bad[simd];
      faulty.append(f);
    }
    py::dict where = location_dict(key);
    where["visits"] = s.visits;
    where["simd_seen"] = s.simd_seen;
    locations.append(where);
  }
  const double flop = (double)mfmas * (double)gh::flop_per_mfma(r.dtype);
  const double tflops = r.elapsed_ms > 0.0 ? flop / (r.elapsed_ms * 1e-3) / 1e12 : 0.0;
  if (!slowest_cu.is_none()) slowest_cu["cycles_per_mfma"] = slowest;
  d["dtype"] = kDtypeNames[r.dtype];
  d["mfmas"] = mfmas;
  d["flop"] = mfmas * gh::flop_per_mfma(r.dtype);
  d["elapsed_ms"] = r.elapsed_ms;
  d["tflops"] = tflops;
  d["clock_mhz"] = median_of(clocks);
  d["cycles_per_mfma"] = median_of(cycles_per);
  d["launches"] = r.launches;
  d["blocks"] = r.blocks;
  d["check_every"] = r.check_every;
  d["chunks"] = r.chunks;
  d["tiles_per_wave"] = kLoadTiles;
  d["cu_total"] = r.cu_total;
  d["cu_covered"] = covered;
  d["faulty"] = faulty;
  d["locations"] = locations;
  d["slowest_cu"] = slowest_cu;
  d["floor_tflops"] = r.floor_tflops;
  d["ok"] = bad_total == 0 && tflops >= r.floor_tflops;
  if (r.injected) {
    if (!r.have_record) {
      d["record"] = py::none();
    } else {
      py::dict rec = location_dict(r.record.key);
      py::list simd;
      for (int w = 0; w < kLoadWaves; ++w) simd.append(r.record.simd[w]);
      rec["simd"] = simd;
      d["record"] = rec;
    }
  }
  return d;
}

static py::dict mfma_load(int device, const std::string& dtype, double seconds, int check_every,
                          int64_t chunks, int blocks, double launch_ms, uint32_t seed,
                          double floor_tflops, inject_acc_t inject_acc) {
  const int dt = parse_dtype(dtype);
  const std::optional<LoadInject> inj = checked_load_inject(inject_acc);
  use_device(device);
  return mfma_load_dict(run_mfma_load(dt, seconds, check_every, chunks, blocks, launch_ms, seed,
                                      floor_tflops, inj ? &*inj : nullptr));
}

static py::bytes debug_mfma_load_dump(int device, const std::string& dtype, int64_t mfmas,
                                      uint32_t seed, int64_t visit, bool alternate) {
  const int dt = parse_dtype(dtype);
  const uint32_t v = checked_index(visit, 1ull << 32, "visit");
  use_device(device);
  return py::bytes(run_debug_mfma_load_dump(dt, mfmas, seed, v, alternate));
}

static py::dict burn_in(int device, double hbm_fraction, double hbm_floor_gb_s,
                        bool require_cu_coverage) {
  py::dict result = health_check(device, hbm_floor_gb_s, false);
  bool healthy = result["healthy"].cast<bool>();
  py::dict exact, first_bad;
  for (int dt = 0; dt < gh::kNumDtypes; ++dt) {
    const MfmaResult r = run_mfma_verify(dt, 1024, gh::kDefaultSeed);
    exact[kDtypeNames[dt]] = r.mismatches == 0;
    first_bad[kDtypeNames[dt]] = mfma_dict(r)["first_bad"];
    healthy = healthy && r.mismatches == 0;
  }
  const PatternResult p = run_hbm_pattern(0, hbm_fraction, gh::kDefaultSeed, 1,
                                          16384ull << 20);
  const bool pattern_ok = p.stats.mismatched_words == 0;
  result["mfma_exact"] = exact;
  result["mfma_first_bad"] = first_bad;
  result["hbm_pattern_ok"] = pattern_ok;
  result["hbm_pattern"] = pattern_dict(p);
  // every CU's LDS and every SIMD's matrix pipe, with the place of a fault.
  // Incomplete coverage is reported and fatal only on request: a CU mask or a
  // co-tenant can legitimately keep CUs away from this process.
  const py::dict sweep = cu_sweep_dict(run_cu_sweep(gh::kDefaultSeed, 1, 0, 0, 8, CuInject{}), false);
  const bool cu_ok = py::len(sweep["faulty"]) == 0;
  const bool cu_complete = sweep["cu_covered"].cast<int>() >= sweep["cu_total"].cast<int>();
  result["cu_sweep"] = sweep;
  result["cu_ok"] = cu_ok;
  result["cu_coverage_complete"] = cu_complete;
  result["healthy"] = healthy && pattern_ok && cu_ok && (cu_complete || !require_cu_coverage);
  return result;
}

PYBIND11_MODULE(gpuhealth, m) {
  m.doc() = "MI355X (gfx950) on-device health probes: MFMA smoke + HBM stream, "
            "and the burn-in level (HBM pattern sweep + exact MFMA checks)";
  m.attr("DEFAULT_SEED") = gh::kDefaultSeed;
  m.def("pattern_word", &gh::pattern_word, py::arg("seed"), py::arg("word_index"));
  m.def("reference_tile", &reference_tile_py, py::arg("dtype"), py::arg("seed"),
        py::arg("workgroup"));
  m.def("hbm_pattern_check", &hbm_pattern_check, py::arg("device") = 0,
        py::arg("mib") = 256.0, py::arg("fraction") = 0.0,
        py::arg("seed") = gh::kDefaultSeed, py::arg("corrupt_word") = -1,
        py::arg("corrupt_bit") = 0, py::arg("bytes") = 0,
        py::arg("max_chunk_mib") = 16384, py::arg("passes") = 1,
        py::arg("base_word") = 0, py::arg("corruptions") = corruptions_t{},
        py::arg("corrupt_at") = std::pair<int, int>(0, 0), py::arg("stuck") = stuck_t{});
  m.def("mfma_verify", &mfma_verify, py::arg("device") = 0, py::arg("dtype") = "bf16",
        py::arg("workgroups") = 1024, py::arg("seed") = gh::kDefaultSeed,
        py::arg("corrupt_element") = -1, py::arg("corruptions") = corruptions_t{},
        py::arg("inject_operand") = py::none());
  // test hooks: the production kernels through the production launch code,
  // with what they wrote handed back
  m.def("debug_pattern_fill", &debug_pattern_fill, py::arg("device") = 0,
        py::arg("bytes") = 4096, py::arg("seed") = gh::kDefaultSeed,
        py::arg("invert") = false, py::arg("base_word") = 0);
  m.def("debug_stream_copy_check", &debug_stream_copy_check, py::arg("device") = 0,
        py::arg("bytes") = 4096, py::arg("seed") = gh::kDefaultSeed);
  m.def("debug_mfma_dump", &debug_mfma_dump, py::arg("device") = 0,
        py::arg("dtype") = "bf16", py::arg("workgroups") = 64,
        py::arg("seed") = gh::kDefaultSeed, py::arg("inject_operand") = py::none());
  m.def("mfma_verify_tile", &mfma_verify_tile, py::arg("device") = 0,
        py::arg("dtype") = "bf16", py::arg("seed") = gh::kDefaultSeed,
        py::arg("workgroup") = 0);
  m.def("burn_in", &burn_in, py::arg("device") = 0, py::arg("hbm_fraction") = 0.9,
        py::arg("hbm_floor_gb_s") = 1000.0, py::arg("require_cu_coverage") = false);
  m.def("cu_sweep", &cu_sweep, py::arg("device") = 0, py::arg("seed") = gh::kDefaultSeed,
        py::arg("passes") = 1, py::arg("lds_bytes") = 0, py::arg("blocks_per_round") = 0,
        py::arg("max_rounds") = 8, py::arg("inject_lds") = py::none(),
        py::arg("inject_mfma") = py::none(), py::arg("inject_lds_stuck") = py::none());
  m.attr("MFMA_LOAD_TILES") = kLoadTiles;
  m.attr("MFMA_LOAD_CHECK_EVERY") = kLoadDefaultCheckEvery;
  m.attr("MFMA_LOAD_CALIBRATION_MFMAS") = kLoadCalibrationMfmas;
  m.def("mfma_load", &mfma_load, py::arg("device") = 0, py::arg("dtype") = "bf16",
        py::arg("seconds") = 2.0, py::arg("check_every") = kLoadDefaultCheckEvery,
        py::arg("chunks") = 0, py::arg("blocks") = 0,
        py::arg("launch_ms") = kLoadDefaultLaunchMs, py::arg("seed") = gh::kDefaultSeed,
        py::arg("floor_tflops") = 0.0, py::arg("inject_acc") = py::none());
  m.def("debug_mfma_load_dump", &debug_mfma_load_dump, py::arg("device") = 0,
        py::arg("dtype") = "bf16", py::arg("mfmas") = 1, py::arg("seed") = gh::kDefaultSeed,
        py::arg("visit") = 0, py::kw_only(), py::arg("alternate") = true);
  m.def("flop_per_mfma", [](const std::string& dtype) {
    return gh::flop_per_mfma(parse_dtype(dtype)); }, py::arg("dtype"));
  m.def("decode_location", &decode_location_py, py::arg("xcc_id_reg"), py::arg("hw_id_reg"));
  m.def("debug_cu_lds_dump", &debug_cu_lds_dump, py::arg("device") = 0,
        py::arg("lds_bytes") = 0, py::arg("seed") = gh::kDefaultSeed,
        py::arg("invert") = false, py::arg("visit") = 0);
  m.def("device_count", &device_count);
  m.def("device_info", &device_info, py::arg("device") = 0);
  m.def("mfma_smoke", &mfma_smoke, py::arg("device") = 0,
        py::arg("workgroups") = 2048, py::arg("corruptions") = corruptions_t{},
        py::arg("launch_workgroups") = -1);
  m.def("debug_mfma_smoke_dump", &debug_mfma_smoke_dump, py::arg("device") = 0,
        py::arg("workgroups") = 64, py::arg("launch_workgroups") = -1);
  m.def("hbm_bandwidth_gb_s", &hbm_bandwidth_gb_s, py::arg("device") = 0,
        py::arg("gib") = 1.0, py::arg("iters") = 10);
  m.def("health_check", &health_check, py::arg("device") = 0,
        py::arg("hbm_floor_gb_s") = 1000.0, py::arg("quick") = false);
}
