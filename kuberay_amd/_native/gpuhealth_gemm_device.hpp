// gpuhealth_gemm_device — what the translation units of the burn-in's GEMM and
// attention checks (gpuhealth_gemm.hip, gpuhealth_gemm_narrow.hip,
// gpuhealth_attn.hip, gpuhealth_attn128.hip, gpuhealth_attn_decode.hip,
// gpuhealth_moe.hip) share on the HIP side:
// the error check, the scope that frees device memory, the hardware-register
// reads of the location key and the result bookkeeping. Not for gpuhealth.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpuhealth_gemm.hpp"

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e) + " at " #expr);          \
    }                                                                          \
  } while (0)

#define GH_LDS __attribute__((address_space(3)))
#define GH_GLOBAL __attribute__((address_space(1)))

namespace ghgemm {
namespace {

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

constexpr unsigned long long kNoBadWord = ~0ull;

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

[[maybe_unused]] static std::string device_bytes(const void* ptr, size_t bytes) {
  std::string host(bytes, '\0');
  HIP_CHECK(hipMemcpy(&host[0], ptr, bytes, hipMemcpyDeviceToHost));
  return host;
}

}  // namespace
}  // namespace ghgemm
