// Registry of packed constant B operands (operand_registry.h) and the kernels that pack them.
#include "operand_registry.h"

#include <map>
#include <mutex>

#include "gemm_kernel.h"
#include "sp8.h"

namespace mtgv {

// ---- packing ----
// One wave per row: row maximum -> power-of-two scale (maximum lands in [2^13, 2^14)) -> split.  wscale = 2^-e.
__global__ __launch_bounds__(256) void sp8_pack_rows_kernel(const float* __restrict__ in, sp_h8* __restrict__ out,
                                                           float* __restrict__ wscale, long rows, int K) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* x = in + row * K;
  float mx = 0.f;
  for (int k = lane; k < K; k += 64) mx = fmaxf(mx, fabsf(x[k]));
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
  int e = 0;
  if (mx > 0.f && mx < INFINITY) {
    int ex;
    (void)frexpf(mx, &ex);  // mx = f * 2^ex, f in [0.5, 1)
    e = 14 - ex;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
  }
  const float sc = ldexpf(1.0f, e);
  if (lane == 0) wscale[row] = ldexpf(1.0f, -e);
  sp_h8* o = out + row * (K / 4);  // two 16-byte pieces per chunk of 8
  for (int c = lane; c < K / 8; c += 64) {
    const sp_f4 a = *reinterpret_cast<const sp_f4*>(x + c * 8) * sc, b = *reinterpret_cast<const sp_f4*>(x + c * 8 + 4) * sc;
    sp_h8 hi, lo;
    sp8_split8(a, b, hi, lo);
    o[2 * c] = hi;
    o[2 * c + 1] = lo;
  }
}

__global__ __launch_bounds__(256) void split_pack_kernel(const float* __restrict__ in, float* __restrict__ out, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f16x4 hi, lo;
  split_f16(reinterpret_cast<const f32x4*>(in)[i], hi, lo);
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = hi[j], o[4 + j] = lo[j];
  reinterpret_cast<f16x8*>(out)[i] = o;
}

// rows of row_k floats, stored scaled by 1 / wscale[row] (the power of two the SP8 copy of the same buffer uses)
__global__ __launch_bounds__(256) void split_pack_rows_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             const float* __restrict__ wscale, long n4, int rk4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float sc = 1.0f / wscale[i / rk4];  // exact: wscale is a power of two
  f16x4 hi, lo;
  split_f16(reinterpret_cast<const f32x4*>(in)[i] * sc, hi, lo);
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = hi[j], o[4 + j] = lo[j];
  reinterpret_cast<f16x8*>(out)[i] = o;
}

// ---- registry ----
namespace {
struct Operand {
  size_t n = 0;             // floats of the master
  int row_k = 0;            // > 0: rows of row_k floats with an SP8 copy; the split copy is then stored scaled per row
  char* sp8 = nullptr;      // SP8 rows
  float* wscale = nullptr;  // [n / row_k]
  float* split = nullptr;
  void release() {  // (hipFree(nullptr) is a no-op)
    (void)hipFree(sp8), (void)hipFree(wscale), (void)hipFree(split);
    sp8 = nullptr, wscale = nullptr, split = nullptr;
  }
};
std::map<const float*, Operand> g_ops;
std::mutex g_ops_mu;
}  // namespace

void operand_register(const float* W, size_t n_floats, int row_k, bool split) {
  if (W == nullptr || ((uintptr_t)W % 16) != 0) return;
  const int rk = (row_k > 0 && row_k % 8 == 0 && n_floats != 0 && n_floats % (size_t)row_k == 0) ? row_k : 0;
  if (split ? (n_floats < 64 || n_floats % 4 != 0) : rk == 0) return;
  std::lock_guard<std::mutex> lk(g_ops_mu);
  Operand& e = g_ops[W];
  if (e.n == n_floats && e.row_k == rk && (e.split != nullptr || !split)) return;  // same shape: the copies stay
  e.release();
  e.n = n_floats;
  e.row_k = rk;
  // a failed allocation must not leave an entry that lookups would report as a valid copy
  if ((rk > 0 && (hipMalloc((void**)&e.sp8, n_floats * sizeof(float)) != hipSuccess ||
                  hipMalloc((void**)&e.wscale, (n_floats / rk) * sizeof(float)) != hipSuccess)) ||
      (split && hipMalloc((void**)&e.split, n_floats * sizeof(float)) != hipSuccess)) {
    e.release();
    g_ops.erase(W);
    MTGV_CHECK(false, ERR_RUNTIME, "operand_register: out of device memory for %zu floats", n_floats);
  }
}

void operand_refresh(const float* W, size_t offset_floats, size_t n_floats, hipStream_t s) {
  Operand e;
  {
    std::lock_guard<std::mutex> lk(g_ops_mu);
    auto it = g_ops.find(W);
    if (it == g_ops.end()) return;
    e = it->second;
  }
  if (e.split != nullptr)
    MTGV_CHECK(offset_floats % 4 == 0 && n_floats % 4 == 0 && offset_floats + n_floats <= e.n, ERR_INVALID,
               "operand refresh outside the registered buffer");
  if (n_floats == 0) return;
  const float* const in = W + offset_floats;
  if (e.row_k > 0) {
    MTGV_CHECK(offset_floats % e.row_k == 0 && n_floats % e.row_k == 0 && offset_floats + n_floats <= e.n, ERR_INVALID,
               "operand refresh must cover whole rows inside the registered buffer");
    const long row0 = (long)(offset_floats / e.row_k), rows = (long)(n_floats / e.row_k);
    hipLaunchKernelGGL(sp8_pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, in,
                       reinterpret_cast<sp_h8*>(e.sp8 + offset_floats * sizeof(float)), e.wscale + row0, rows, e.row_k);
    HIP_OK(hipGetLastError());
  }
  if (e.split == nullptr) return;
  const long n4 = (long)(n_floats / 4);
  const dim3 grid((unsigned)((n4 + 255) / 256));
  if (e.row_k > 0)
    hipLaunchKernelGGL(split_pack_rows_kernel, grid, dim3(256), 0, s, in, e.split + offset_floats, e.wscale + offset_floats / e.row_k, n4,
                       e.row_k / 4);
  else
    hipLaunchKernelGGL(split_pack_kernel, grid, dim3(256), 0, s, in, e.split + offset_floats, n4);
  HIP_OK(hipGetLastError());
}

void operand_unregister(const float* W) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  auto it = g_ops.find(W);
  if (it == g_ops.end()) return;
  it->second.release();
  g_ops.erase(it);
}

bool operand_registered(const float* W) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  return g_ops.find(W) != g_ops.end();
}

bool operand_sp8(const float* W, int K, const char** sp8, const float** wscale) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  auto it = g_ops.upper_bound(W);  // first base > W
  if (it == g_ops.begin()) return false;
  --it;
  const Operand& e = it->second;
  const size_t off = (size_t)(W - it->first);
  if (e.sp8 == nullptr || off >= e.n || e.row_k != K || off % (size_t)K != 0) return false;
  if (sp8) *sp8 = e.sp8 + off * sizeof(float);
  if (wscale) *wscale = e.wscale + off / K;
  return true;
}

const float* operand_split(const float* W, int K, const float** wscale) {
  *wscale = nullptr;
  std::lock_guard<std::mutex> lk(g_ops_mu);
  auto it = g_ops.find(W);
  if (it == g_ops.end() || it->second.split == nullptr) return nullptr;
  if (it->second.row_k == 0) return it->second.split;
  if (it->second.row_k != K) return nullptr;
  *wscale = it->second.wscale;
  return it->second.split;
}

}  // namespace mtgv
