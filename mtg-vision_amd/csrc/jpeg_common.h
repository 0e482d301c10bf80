// Device pieces shared by the JPEG decoder (jpeg.hip) and encoder (jpeg_enc.hip): the zig-zag order and the scans that
// the ragged / prefix-sum launches of both are built from.  (The host side's zig-zag table is in jpeg_tables.h.)
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {

// zig-zag index -> natural (row-major) index
__constant__ uint8_t k_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ inline int find_base(const int64_t* base, int n, int64_t x) {  // largest i < n with base[i] <= x
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ inline int wave_incl(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// inclusive scan over a 256-thread workgroup; `total` gets the sum.  s: 4 ints of LDS.
__device__ inline int block_incl(int v, int* s, int& total) {
  const int wv = threadIdx.x >> 6;
  v = wave_incl(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) s[wv] = v;
  __syncthreads();
  int before = 0;
  for (int i = 0; i < wv; ++i) before += s[i];
  total = s[0] + s[1] + s[2] + s[3];
  return v + before;
}

}  // namespace
