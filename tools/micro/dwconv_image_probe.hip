// Whole-image dwconv7_ln (dwconv7_ln_image_kernel: one image per block in LDS, one channel per thread, taps in registers,
// padded taps skipped at compile time) against the row-group kernel and the single-row kernel: time and bit-equality,
// SP8 and f32 output, inputs with exact and negative zeros included.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I mtg-vision_amd/csrc -Wno-inline-asm -Xclang -target-feature -Xclang -packed-fp32-ops \
//       tools/micro/dwconv_image_probe.hip -o tools/micro/build/dwconv_image_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "dwconv7_ln_kernel.h"
namespace mtgv { void set_last_error(const std::string&) {} }
using namespace mtgv;

template <typename F>
static float time_us(F f) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0), hipEventCreate(&e1);
  for (int it = 0; it < 3; ++it) f();
  hipEventRecord(e0);
  for (int it = 0; it < 20; ++it) f();
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  return ms / 20 * 1e3f;
}

template <int C, int H, int W, int SPLIT>
static int shape(int N, bool zeros) {
  const size_t n = (size_t)N * H * W * C;
  float *in, *out, *ref, *w49, *b, *lw, *lb;
  hipMalloc(&in, n * 4), hipMalloc(&out, n * 4), hipMalloc(&ref, n * 4), hipMalloc(&w49, 49 * C * 4), hipMalloc(&b, C * 4), hipMalloc(&lw, C * 4),
      hipMalloc(&lb, C * 4);
  std::vector<float> h(n > (size_t)49 * C ? n : (size_t)49 * C);
  srand(1);
  for (size_t i = 0; i < n; ++i) {
    h[i] = (rand() % 2001 - 1000) * 1e-3f;
    if (zeros && rand() % 3 == 0) h[i] = rand() % 2 ? 0.f : -0.f;
  }
  hipMemcpy(in, h.data(), n * 4, hipMemcpyHostToDevice);
  for (float* p : {w49, b, lw, lb}) {
    const size_t m = p == w49 ? 49 * C : C;
    for (size_t i = 0; i < m; ++i) h[i] = (rand() % 2001 - 1000) * 1e-3f;
    hipMemcpy(p, h.data(), m * 4, hipMemcpyHostToDevice);
  }
  std::vector<float> hr(n), ho(n);
  int fails = 0;
  for (int fmt = 1; fmt >= 0; --fmt) {
    setenv("MTGV_DW_IMAGE", "0", 1);
    setenv("MTGV_DW_ROWS", "0", 1);
    auto single = [&] { dwconv7_ln_dispatch(in, w49, b, lw, lb, ref, N, H, W, C, 1e-6f, nullptr, fmt); };
    const float t_single = time_us(single);
    hipDeviceSynchronize();
    hipMemcpy(hr.data(), ref, n * 4, hipMemcpyDeviceToHost);
    setenv("MTGV_DW_ROWS", "1", 1);
    auto rows = [&] { dwconv7_ln_dispatch(in, w49, b, lw, lb, out, N, H, W, C, 1e-6f, nullptr, fmt); };
    printf("%dx%dx%dx%d %s%s  single row: %.1f us   row groups: %.1f us\n", N, H, W, C, fmt ? "SP8" : "f32", zeros ? " zeros" : "", t_single, time_us(rows));
    hipMemset(out, 0xff, n * 4);
    auto image = [&] {
      if (fmt) dwconv7_ln_image_launch<C, H, W, SPLIT, true>(in, w49, b, lw, lb, out, N, 1e-6f, nullptr);
      else dwconv7_ln_image_launch<C, H, W, SPLIT, false>(in, w49, b, lw, lb, out, N, 1e-6f, nullptr);
    };
    const float us = time_us(image);
    hipError_t e = hipDeviceSynchronize();
    hipMemcpy(ho.data(), out, n * 4, hipMemcpyDeviceToHost);
    size_t bad = 0, first = 0;
    for (size_t i = 0; i < n; ++i)
      if (memcmp(&ho[i], &hr[i], 4)) { if (!bad) first = i; ++bad; }
    printf("   whole image SPLIT=%d     %.1f us  %s", SPLIT, us, bad ? "DIFFERS" : "bit-identical to the single-row kernel");
    if (bad) printf(" (%zu of %zu words, first at %zu: %g vs %g)", bad, n, first, ho[first], hr[first]);
    if (e != hipSuccess) printf(" [%s]", hipGetErrorString(e));
    printf("\n");
    fails += bad != 0 || e != hipSuccess;
    if (e != hipSuccess) exit(2);  // nothing more on a device that has reported an error
  }
  hipFree(in), hipFree(out), hipFree(ref), hipFree(w49), hipFree(b), hipFree(lw), hipFree(lb);
  return fails;
}

int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 256;
  int fails = 0;
  fails += shape<384, 12, 8, 2>(N, false);
  fails += shape<768, 6, 4, 1>(N, false);
  fails += shape<384, 12, 8, 2>(N, true);
  fails += shape<768, 6, 4, 1>(3, true);
  fails += shape<384, 12, 8, 2>(130, false);
  return fails != 0;
}
