// mtgv - MI355X-native recognition hot path. Shared host/device helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <stdexcept>

#include "status.h"  // Error, Status, MTGV_CHECK, guarded, ceil_div

namespace mtgv {

#define HIP_OK(expr)                                                       \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess)                                                  \
      throw ::mtgv::Error(::mtgv::ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(_e) + " at " __FILE__ ":" + std::to_string(__LINE__)); \
  } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));

// XCD-aware block order.  The hardware deals blocks to the eight XCDs round robin (block b runs on XCD b % 8); this maps
// b to a work index such that the blocks of one XCD walk a contiguous run of the nwg work items, so what neighbouring
// items share (halo rows, an A row-panel) is fetched into one L2 and not into all eight.  T: the caller's index type.
template <typename T>
__device__ __forceinline__ T xcd_block_order(T b, T nwg) {
  const T q = nwg >> 3, r = nwg & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// ---- exact unsigned division by a runtime constant (n * d < 2^40) ----
struct FastDiv {
  uint64_t mul;  // ceil(2^40 / d)
  uint32_t d;
};
static inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d ? d : 1;
  f.mul = ((1ull << 40) + f.d - 1) / f.d;
  return f;
}
__host__ __device__ static inline uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return (uint32_t)(((uint64_t)n * f.mul) >> 40);
}

// Per-device lazily created state (zero pages, function attributes, scratch words) is kept in small tables indexed by
// the HIP device ordinal: a handle is bound to the device current at its creation and several may coexist in a process.
constexpr int MTGV_MAX_DEVICES = 64;
static inline int current_device() {
  int d = 0;
  HIP_OK(hipGetDevice(&d));
  MTGV_CHECK(d >= 0 && d < MTGV_MAX_DEVICES, ERR_RUNTIME, "device ordinal %d outside [0, %d)", d, MTGV_MAX_DEVICES);
  return d;
}

// Opt the kernel `Kern` in to `need_bytes` of dynamic LDS per block: beyond the default 64 KiB a kernel has to ask, once per
// device (hipFuncSetAttribute is per device), for a limit of `limit_bytes` >= every size it will be launched with.
template <auto Kern>
static inline void lds_opt_in(size_t need_bytes, int limit_bytes) {
  if (need_bytes <= 64 * 1024) return;
  static bool done[MTGV_MAX_DEVICES] = {};
  bool& d = done[current_device()];
  if (d) return;
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, limit_bytes));
  d = true;
}

// atoi of the environment variable `name`, `if_unset` when it is not set (on/off and small integer switches)
static inline int env_int(const char* name, int if_unset) {
  const char* const e = getenv(name);
  return e != nullptr ? atoi(e) : if_unset;
}

// device buffer of floats owned by its holder
struct DevBuf {
  float* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void alloc(size_t floats);
  void ensure(size_t floats) {
    if (floats > n) alloc(floats);
  }
  void release();
};

enum Act : int { ACT_NONE = 0, ACT_GELU = 1, ACT_MISH = 2, ACT_SILU = 3, ACT_SIGMOID = 4 };

}  // namespace mtgv
