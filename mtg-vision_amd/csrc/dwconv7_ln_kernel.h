// Depthwise 7x7 + LayerNorm kernel bodies and the dispatcher that picks one (instantiated in rowops.hip).
#pragma once
#include "common.h"
#include "dwconv7_ln_image_kernel.h"
#include "dwconv7_ln_stream_kernel.h"
#include "sp8.h"

namespace mtgv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// Depthwise 7x7 + LayerNorm over C in one pass (Block.dwconv + Block.norm, convnextv2.py:214-216): the conv
// result never goes to HBM un-normalised.  A block owns S whole strips (all C channels of TW pixels), so the
// per-pixel mean / variance over channels are block-local: partial sums go through LDS in a fixed order
// (two-pass variance like ln_rows_kernel, deterministic).
// ---------------------------------------------------------------------------
template <int TW, bool SP8>
__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const float* __restrict__ in, const float* __restrict__ w49,
                                                        const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                        const float* __restrict__ ln_b, float* __restrict__ out, int H, int W,
                                                        int C, int nstrips, long total_strips, int S, float eps) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int c4n = C >> 2;
  float* part = sm;                      // [S][c4n][TW]: a pixel's partial sums sit TW floats apart, so the lanes that reduce
                                         // pixels 0..TW-1 read consecutive words (no bank conflicts) in the same c4 order
  float* stat = sm + S * TW * c4n;       // [S][TW][2] mean, rstd
  long blk;
  {
    const long nwg = gridDim.x, b = blockIdx.x;
    const long q = nwg >> 3, r = nwg & 7, x = b & 7;
    blk = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
  }
  const int tid = threadIdx.x;
  const int sl = tid / c4n, c4 = tid % c4n;  // strip slot in block, channel quad
  const long strip = blk * S + sl;
  const bool live = sl < S && strip < total_strips;
  const int c = c4 * 4;
  int ws = 0, h = 0;
  long n = 0;
  if (live) {
    ws = (int)(strip % nstrips);
    const long t = strip / nstrips;
    h = (int)(t % H);
    n = t / H;
  }
  const int w0 = ws * TW;
  f32x4 acc[TW];
  if (live) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
    for (int j = 0; j < TW; ++j) acc[j] = bv;
#ifndef DW_DBG
#define DW_DBG 0  // tools/micro/dwconv_probe.hip: 1 centre row only, 2 loads without the FMAs, 3 no LayerNorm
#endif
#pragma unroll 1
    for (int kh = 0; kh < 7; ++kh) {
      const int ih = h + kh - 3;
      if (ih < 0 || ih >= H) continue;
      if (DW_DBG == 1 && kh != 3) continue;
      const float* rowp = in + ((n * H + ih) * W) * C + c;
      f32x4 r[TW + 6];
#pragma unroll
      for (int j = 0; j < TW + 6; ++j) {
        const int iw = w0 + j - 3;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iw >= 0 && iw < W) v = *reinterpret_cast<const f32x4*>(rowp + (long)iw * C);
        r[j] = v;
      }
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w49 + (kh * 7 + kw) * C + c);
#pragma unroll
        for (int j = 0; j < TW; ++j) {
          if (DW_DBG == 2) acc[j] += (kw == 0 ? r[j] + r[j + 6] : wv);  // keeps every load alive, 1/7 of the arithmetic
          else acc[j] += r[j + kw] * wv;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < TW; ++j) part[(sl * c4n + c4) * TW + j] = (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
  }
  __syncthreads();
  if (live && c4 < TW) {  // thread c4 of a strip reduces pixel j = c4
    const float* pp = part + sl * c4n * TW + c4;
    float sum = 0.f;
    for (int i = 0; i < c4n; ++i) sum += pp[i * TW];
    stat[(sl * TW + c4) * 2] = sum / (float)C;
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int j = 0; j < TW; ++j) {
      const f32x4 d = acc[j] - stat[(sl * TW + j) * 2];
      part[(sl * c4n + c4) * TW + j] = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  __syncthreads();
  if (live && c4 < TW) {
    const float* pp = part + sl * c4n * TW + c4;
    float sq = 0.f;
    for (int i = 0; i < c4n; ++i) sq += pp[i * TW];
    stat[(sl * TW + c4) * 2 + 1] = 1.0f / sqrtf(sq / (float)C + eps);
  }
  __syncthreads();
  if (live) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(ln_w + c);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(ln_b + c);
    float* op = out + ((n * H + h) * W + w0) * C + c;
#pragma unroll
    for (int j = 0; j < TW; ++j)
      if (w0 + j < W) {
        const float mean = stat[(sl * TW + j) * 2], rstd = stat[(sl * TW + j) * 2 + 1];
        const f32x4 o = (acc[j] - mean) * rstd * wv + bv;
        if (SP8)  // quads c4, c4^1 of a strip are adjacent lanes with the same predicates (C % 8 == 0)
          *reinterpret_cast<sp_h8*>(reinterpret_cast<char*>(op + (long)j * C - c) + (c4 >> 1) * 32 + (c4 & 1) * 16) =
              sp8_piece_from_quad(o, c4);
        else
          *reinterpret_cast<f32x4*>(op + (long)j * C) = o;
      }
  }
}


// Row-group form of the same kernel: a thread keeps TH output rows of its TW-pixel strip in registers and walks the TH + 6
// input rows once, so an input row is fetched (TH + 6) / TH times instead of 7 (tools/micro/dwconv_probe.hip: the six
// extra row fetches, not the FMAs, are 45 % of the single-row kernel's time at stage 0).  Every output still accumulates
// bias, then kh ascending, kw ascending: bit-identical to dwconv7_ln_kernel.
template <int TW, int TH, bool SP8, bool WL = false>
__global__ __launch_bounds__(256) void dwconv7_ln_rows_kernel(const float* __restrict__ in, const float* __restrict__ w49,
                                                             const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                             const float* __restrict__ ln_b, float* __restrict__ out, int H, int W,
                                                             int C, int nstrips, int nhg, long total_strips, int S, float eps) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int P = TH * TW;             // pixels a thread owns
  const int c4n = C >> 2;
  float* part = sm;                      // [S][c4n][P]
  float* stat = sm + S * P * c4n;        // [S][P][2] mean, rstd
  const float* wl = w49;                 // WL: the 49 x C tap table staged in LDS (a third of the kernel's L1 traffic otherwise)
  const int tid = threadIdx.x;
  if (WL) {
    float* wdst = stat + ((S * P * 2 + 3) & ~3);
    for (int i = tid; i < 49 * c4n; i += blockDim.x) reinterpret_cast<f32x4*>(wdst)[i] = reinterpret_cast<const f32x4*>(w49)[i];
    wl = wdst;
    __syncthreads();
  }
  const int sl = tid / c4n, c4 = tid % c4n;
  const int c = c4 * 4;
  long blk;
  {
    const long nwg = gridDim.x, b = blockIdx.x;
    const long q = nwg >> 3, r = nwg & 7, x = b & 7;
    blk = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
  }
  const long strip = blk * S + sl;
  const bool live = sl < S && strip < total_strips;
  int ws = 0, h0 = 0;
  long n = 0;
  if (live) {
    ws = (int)(strip % nstrips);
    const long t = strip / nstrips;
    h0 = (int)(t % nhg) * TH;
    n = t / nhg;
  }
  const int w0 = ws * TW;
  f32x4 acc[TH][TW];
  if (live) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
      for (int j = 0; j < TW; ++j) acc[t][j] = bv;
#pragma unroll 1
    for (int ir = 0; ir < TH + 6; ++ir) {
      const int ih = h0 + ir - 3;
      if (ih < 0 || ih >= H) continue;
      const float* rowp = in + ((n * H + ih) * W) * C + c;
      f32x4 r[TW + 6];
#pragma unroll
      for (int j = 0; j < TW + 6; ++j) {
        const int iw = w0 + j - 3;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iw >= 0 && iw < W) v = *reinterpret_cast<const f32x4*>(rowp + (long)iw * C);
        r[j] = v;
      }
#pragma unroll
      for (int t = 0; t < TH; ++t) {
        const int kh = ir - t;  // output row h0 + t sees this input row as its tap row kh
        if (kh < 0 || kh > 6) continue;
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + (kh * 7 + kw) * C + c);
#pragma unroll
          for (int j = 0; j < TW; ++j) acc[t][j] += r[j + kw] * wv;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
      for (int j = 0; j < TW; ++j)
        part[(sl * c4n + c4) * P + t * TW + j] = (acc[t][j][0] + acc[t][j][1]) + (acc[t][j][2] + acc[t][j][3]);
  }
  __syncthreads();
  if (live)
    for (int p = c4; p < P; p += c4n) {  // thread c4 of a strip reduces pixels c4, c4 + c4n, ...
      const float* pp = part + sl * c4n * P + p;
      float sum = 0.f;
      for (int i = 0; i < c4n; ++i) sum += pp[i * P];
      stat[(sl * P + p) * 2] = sum / (float)C;
    }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
      for (int j = 0; j < TW; ++j) {
        const f32x4 d = acc[t][j] - stat[(sl * P + t * TW + j) * 2];
        part[(sl * c4n + c4) * P + t * TW + j] = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      }
  }
  __syncthreads();
  if (live)
    for (int p = c4; p < P; p += c4n) {
      const float* pp = part + sl * c4n * P + p;
      float sq = 0.f;
      for (int i = 0; i < c4n; ++i) sq += pp[i * P];
      stat[(sl * P + p) * 2 + 1] = 1.0f / sqrtf(sq / (float)C + eps);
    }
  __syncthreads();
  if (live) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(ln_w + c);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(ln_b + c);
#pragma unroll
    for (int t = 0; t < TH; ++t) {
      if (h0 + t >= H) continue;
      float* op = out + ((n * H + h0 + t) * W + w0) * C + c;
#pragma unroll
      for (int j = 0; j < TW; ++j)
        if (w0 + j < W) {
          const float mean = stat[(sl * P + t * TW + j) * 2], rstd = stat[(sl * P + t * TW + j) * 2 + 1];
          const f32x4 o = (acc[t][j] - mean) * rstd * wv + bv;
          if (SP8)
            *reinterpret_cast<sp_h8*>(reinterpret_cast<char*>(op + (long)j * C - c) + (c4 >> 1) * 32 + (c4 & 1) * 16) =
                sp8_piece_from_quad(o, c4);
          else
            *reinterpret_cast<f32x4*>(op + (long)j * C) = o;
        }
    }
  }
}

template <int TW, int TH, bool SP8, bool WL = false>
static void dwconv7_ln_rows_launch(const float* in, const float* w49, const float* bias, const float* ln_w, const float* ln_b,
                                   float* out, int N, int H, int W, int C, float eps, hipStream_t s) {
  const int nstrips = ceil_div(W, TW), nhg = ceil_div(H, TH);
  const int c4n = C / 4;
  const int S = 256 / c4n;
  const long total_strips = (long)N * nhg * nstrips;
  const unsigned grid = (unsigned)((total_strips + S - 1) / S);
  const size_t lds = (size_t)(S * TH * TW * (c4n + 2) + 4 + (WL ? 49 * C : 0)) * sizeof(float);
  lds_opt_in<dwconv7_ln_rows_kernel<TW, TH, SP8, WL>>(lds, 160 * 1024);  // (not reached by the library's own launches: C <= 96)
  // S * c4n threads rounded up to a wave: at C = 384 / 640 / 768 a fourth wave would hold no strip and only sit at the barriers
  const unsigned threads = (unsigned)((S * c4n + 63) / 64 * 64);
  hipLaunchKernelGGL((dwconv7_ln_rows_kernel<TW, TH, SP8, WL>), dim3(grid), dim3(threads), lds, s, in, w49, bias, ln_w, ln_b, out, H, W, C,
                     nstrips, nhg, total_strips, S, eps);
  HIP_OK(hipGetLastError());
}

template <bool SP8>
static void dwconv7_ln_launch_fmt(const float* in, const float* w49, const float* bias, const float* ln_w, const float* ln_b,
                                  float* out, int N, int H, int W, int C, float eps, hipStream_t s) {
  // Row-group forms (tools/micro/dwconv_rows_probe.hip, profiles/r03_dwconv_rows_probe.txt; all bit-identical to the
  // single-row kernel): 4-pixel strips x 3 rows with the tap table in LDS while table + partial sums fit the default
  // 64 KB window (C <= 192: 121.5 vs 144-155 us at 256 x 48 x 32 x 96, 60.9 vs 66.7 at 24 x 16 x 192), else 3 rows of the
  // widest strip (34.7 vs 38.6 us at 12 x 8 x 384, 20.3 vs 24.7 at 6 x 4 x 768).  MTGV_DW_ROWS=0: single-row kernel.
  const bool rows_on = env_int("MTGV_DW_ROWS", 1) != 0;  // read per call: tests compare the forms inside one process
  // Row-streaming form (dwconv7_ln_stream_kernel.h: LDS-DMA row ring, one channel per thread, taps in registers;
  // bit-identical): one block per image, so it needs a batch that fills the CUs; measured against the row-group form
  // (tools/micro/dwconv_stream_probe.hip, profiles/r04_dwconv_stream_probe.txt) it wins where rows are long in pixels -
  // 48 x 32 x 96: 121 vs 129 us, 24 x 16 x 192: 61 vs 66 - and ties or loses at 12 x 8 x 384 / 6 x 4 x 768.
  // Whole-image form (dwconv7_ln_image_kernel.h: one image per block in LDS, one channel per thread with its taps in
  // registers, padded taps skipped at compile time, LayerNorm and output on channel quads; bit-identical) for the deep
  // stages of the tiny encoder, where an image fits a CU's LDS and C or 2 C threads fill every SIMD alike; one block per
  // image, so like the streaming form it needs a batch that fills the CUs (tools/micro/dwconv_image_probe.hip,
  // profiles/dwconv_image_probe.txt: 12 x 8 x 384 25.3 vs 37.5 us per launch in the encoder, 6 x 4 x 768 16.5 vs 23.4).
  // MTGV_DW_IMAGE=0: never, =1: at any batch size (tests).
  const int image_mode = env_int("MTGV_DW_IMAGE", -1);  // read per call, like MTGV_DW_ROWS
  if (rows_on && image_mode != 0 && (N >= 128 || image_mode == 1)) {
    if (C == 384 && H == 12 && W == 8) return dwconv7_ln_image_launch<384, 12, 8, 2, SP8>(in, w49, bias, ln_w, ln_b, out, N, eps, s);
    if (C == 768 && H == 6 && W == 4) return dwconv7_ln_image_launch<768, 6, 4, 1, SP8>(in, w49, bias, ln_w, ln_b, out, N, eps, s);
  }
  if (rows_on && N >= 128) {
    if (C == 96 && W == 32) return dwconv7_ln_stream_launch<96, 8, 4, 3, SP8>(in, w49, bias, ln_w, ln_b, out, N, H, 1, eps, s);
    if (C == 192 && W == 16) return dwconv7_ln_stream_launch<192, 4, 4, 3, SP8>(in, w49, bias, ln_w, ln_b, out, N, H, 1, eps, s);
  }
  if (rows_on && W >= 4) {
    const int c4n_ = C / 4, S_ = 256 / c4n_;
    const bool table = (size_t)(S_ * 12 * (c4n_ + 2) + 4 + 49 * C) * sizeof(float) <= 65536;
    if (table) dwconv7_ln_rows_launch<4, 3, SP8, true>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    else if (W >= 8) dwconv7_ln_rows_launch<8, 3, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    else dwconv7_ln_rows_launch<4, 3, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    return;
  }
  const int tw = W >= 8 ? 8 : (W >= 4 ? 4 : 2);
  const int nstrips = ceil_div(W, tw);
  const int c4n = C / 4;
  const int S = 256 / c4n;
  const long total_strips = (long)N * H * nstrips;
  const unsigned grid = (unsigned)((total_strips + S - 1) / S);
  const size_t lds = (size_t)(S * tw * c4n + S * tw * 2) * sizeof(float);
  auto kern = tw == 8 ? dwconv7_ln_kernel<8, SP8> : (tw == 4 ? dwconv7_ln_kernel<4, SP8> : dwconv7_ln_kernel<2, SP8>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, in, w49, bias, ln_w, ln_b, out, H, W, C, nstrips, total_strips, S, eps);
  HIP_OK(hipGetLastError());
}

// picks the kernel form for the shape and launches it; out_fmt 0: f32 rows, 1: SP8 rows
static void dwconv7_ln_dispatch(const float* in, const float* w49, const float* bias, const float* ln_w, const float* ln_b,
                                float* out, int N, int H, int W, int C, float eps, hipStream_t s, int out_fmt) {
  out_fmt == 1 ? dwconv7_ln_launch_fmt<true>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s)
               : dwconv7_ln_launch_fmt<false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
}

}  // namespace mtgv
