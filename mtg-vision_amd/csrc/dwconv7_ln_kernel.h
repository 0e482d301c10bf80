// Depthwise 7x7 + LayerNorm kernel bodies and the dispatcher that picks one (instantiated in rowops.hip).
#pragma once
#include "common.h"
#include "dwconv7_ln_image_kernel.h"
#include "dwconv7_ln_stream_kernel.h"
#include "sp8.h"

namespace mtgv {

// ---------------------------------------------------------------------------
// Depthwise 7x7 + LayerNorm over C in one pass (Block.dwconv + Block.norm, convnextv2.py:214-216): the conv
// result never goes to HBM un-normalised.  A block owns S whole strips (all C channels of TH rows of TW pixels), so the
// per-pixel mean / variance over channels are block-local: partial sums go through LDS in a fixed order
// (two-pass variance like ln_rows_kernel, deterministic).
// A thread keeps TH output rows of its strip in registers and walks the TH + 6 input rows once, so an input row is fetched
// (TH + 6) / TH times instead of 7 (the six extra row fetches, not the FMAs, are 45 % of the time at TH = 1, stage 0).
// TH = 1, WL = false is the single-row form (MTGV_DW_ROWS=0, and widths below 4); the result does not depend on TW, TH, WL.
// ---------------------------------------------------------------------------
template <int TW, int TH, bool SP8, bool WL = false>
__global__ __launch_bounds__(256) void dwconv7_ln_rows_kernel(const float* __restrict__ in, const float* __restrict__ w49,
                                                             const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                             const float* __restrict__ ln_b, float* __restrict__ out, int H, int W,
                                                             int C, int nstrips, int nhg, long total_strips, int S, float eps) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int P = TH * TW;             // pixels a thread owns
  const int c4n = C >> 2;
  float* part = sm;                      // [S][c4n][P]: a pixel's partial sums sit P floats apart, so the lanes that reduce
                                         // pixels 0..P-1 read consecutive words (no bank conflicts) in the same c4 order
  float* stat = sm + S * P * c4n;        // [S][P][2] mean, rstd
  const float* wl = w49;                 // WL: the 49 x C tap table staged in LDS (a third of the kernel's L1 traffic otherwise)
  const int tid = threadIdx.x;
  if (WL) {
    float* wdst = stat + ((S * P * 2 + 3) & ~3);
    for (int i = tid; i < 49 * c4n; i += blockDim.x) reinterpret_cast<sp_f4*>(wdst)[i] = reinterpret_cast<const sp_f4*>(w49)[i];
    wl = wdst;
    __syncthreads();
  }
  const int sl = tid / c4n, c4 = tid % c4n;  // strip slot in block, channel quad
  const int c = c4 * 4;
  const long strip = xcd_block_order<long>(blockIdx.x, gridDim.x) * S + sl;
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
  sp_f4 acc[TH][TW];
  if (live) {
    const sp_f4 bv = *reinterpret_cast<const sp_f4*>(bias + c);
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
      for (int j = 0; j < TW; ++j) acc[t][j] = bv;
#pragma unroll 1
    for (int ir = 0; ir < TH + 6; ++ir) {
      const int ih = h0 + ir - 3;
      if (ih < 0 || ih >= H) continue;
      const float* rowp = in + ((n * H + ih) * W) * C + c;
      sp_f4 r[TW + 6];
#pragma unroll
      for (int j = 0; j < TW + 6; ++j) {
        const int iw = w0 + j - 3;
        sp_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (iw >= 0 && iw < W) v = *reinterpret_cast<const sp_f4*>(rowp + (long)iw * C);
        r[j] = v;
      }
#pragma unroll
      for (int t = 0; t < TH; ++t) {
        const int kh = ir - t;  // output row h0 + t sees this input row as its tap row kh
        if (kh < 0 || kh > 6) continue;
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) {
          const sp_f4 wv = *reinterpret_cast<const sp_f4*>(wl + (kh * 7 + kw) * C + c);
#pragma unroll
          for (int j = 0; j < TW; ++j) acc[t][j] += r[j + kw] * wv;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
      for (int j = 0; j < TW; ++j) part[(sl * c4n + c4) * P + t * TW + j] = quad_sum(acc[t][j]);
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
      for (int j = 0; j < TW; ++j)
        part[(sl * c4n + c4) * P + t * TW + j] = quad_sumsq(acc[t][j] - stat[(sl * P + t * TW + j) * 2]);
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
    const sp_f4 wv = *reinterpret_cast<const sp_f4*>(ln_w + c);
    const sp_f4 bv = *reinterpret_cast<const sp_f4*>(ln_b + c);
#pragma unroll
    for (int t = 0; t < TH; ++t) {
      if (h0 + t >= H) continue;
      float* op = out + ((n * H + h0 + t) * W + w0) * C + c;
#pragma unroll
      for (int j = 0; j < TW; ++j)
        if (w0 + j < W) {
          const float mean = stat[(sl * P + t * TW + j) * 2], rstd = stat[(sl * P + t * TW + j) * 2 + 1];
          const sp_f4 o = (acc[t][j] - mean) * rstd * wv + bv;
          if (SP8)  // quads c4, c4^1 of a strip are adjacent lanes with the same predicates (C % 8 == 0)
            *reinterpret_cast<sp_h8*>(reinterpret_cast<char*>(op + (long)j * C - c) + (c4 >> 1) * 32 + (c4 & 1) * 16) =
                sp8_piece_from_quad(o, c4);
          else
            *reinterpret_cast<sp_f4*>(op + (long)j * C) = o;
        }
    }
  }
}

// LDS bytes of a row-group block at C channels: S strips' partial sums and statistics, and with WL the tap table
constexpr size_t dwconv7_ln_rows_lds_bytes(int TW, int TH, bool WL, int C) {
  const int c4n = C / 4, S = 256 / c4n;
  return (size_t)(S * TH * TW * (c4n + 2) + 4 + (WL ? 49 * C : 0)) * sizeof(float);
}

template <int TW, int TH, bool SP8, bool WL = false>
static void dwconv7_ln_rows_launch(const float* in, const float* w49, const float* bias, const float* ln_w, const float* ln_b,
                                   float* out, int N, int H, int W, int C, float eps, hipStream_t s) {
  const int nstrips = ceil_div(W, TW), nhg = ceil_div(H, TH);
  const int c4n = C / 4;
  const int S = 256 / c4n;
  const long total_strips = (long)N * nhg * nstrips;
  const unsigned grid = (unsigned)((total_strips + S - 1) / S);
  const size_t lds = dwconv7_ln_rows_lds_bytes(TW, TH, WL, C);
  lds_opt_in<dwconv7_ln_rows_kernel<TW, TH, SP8, WL>>(lds, 160 * 1024);  // (not reached by the library's own launches: C <= 96)
  // S * c4n threads rounded up to a wave: at C = 384 / 640 / 768 a fourth wave would hold no strip and only sit at the barriers
  const unsigned threads = (unsigned)((S * c4n + 63) / 64 * 64);
  hipLaunchKernelGGL((dwconv7_ln_rows_kernel<TW, TH, SP8, WL>), dim3(grid), dim3(threads), lds, s, in, w49, bias, ln_w, ln_b, out, H, W, C,
                     nstrips, nhg, total_strips, S, eps);
  HIP_OK(hipGetLastError());
}

// The kernel form of a launch: kind, and the TW / TH / WL of the instantiation (the streaming form's strip and row step; the
// whole-image form's full width and band height H / SPLIT; WL = 0 for both)
enum DwLnKind : int { DWLN_ROWS = 0, DWLN_STREAM = 1, DWLN_IMAGE = 2 };
struct DwLnPlan {
  int kind, tw, th, wl;
};

// The one selection rule: which form runs a shape dwconv7_ln_supported admits (host only; the launch below, the block and
// mtgv_op_dwconv7_ln_form all read it)
static inline DwLnPlan dwconv7_ln_plan(int N, int H, int W, int C) {
  // Row-group forms (tools/micro/dwconv_rows_probe.hip, profiles/r03_dwconv_rows_probe.txt; all bit-identical to the
  // single-row form): 4-pixel strips x 3 rows with the tap table in LDS while table + partial sums fit the default
  // 64 KB window (C <= 192: 121.5 vs 144-155 us at 256 x 48 x 32 x 96, 60.9 vs 66.7 at 24 x 16 x 192), else 3 rows of the
  // widest strip (34.7 vs 38.6 us at 12 x 8 x 384, 20.3 vs 24.7 at 6 x 4 x 768).  MTGV_DW_ROWS=0: single-row form (one
  // output row per thread, no tap table in LDS), and nothing but it.
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
    if (C == 384 && H == 12 && W == 8) return {DWLN_IMAGE, 8, 6, 0};  // <384, 12, 8, SPLIT 2>
    if (C == 768 && H == 6 && W == 4) return {DWLN_IMAGE, 4, 6, 0};   // <768, 6, 4, SPLIT 1>
  }
  if (rows_on && N >= 128) {
    if (C == 96 && W == 32) return {DWLN_STREAM, 4, 3, 0};   // <96, G 8, 4, 3>
    if (C == 192 && W == 16) return {DWLN_STREAM, 4, 3, 0};  // <192, G 4, 4, 3>
  }
  if (rows_on && W >= 4) {
    if (dwconv7_ln_rows_lds_bytes(4, 3, true, C) <= 65536) return {DWLN_ROWS, 4, 3, 1};
    return {DWLN_ROWS, W >= 8 ? 8 : 4, 3, 0};
  }
  // single-row form: the widest strip the width allows (dwconv7_ln_supported: C / 4 lanes of a strip cover its pixels)
  return {DWLN_ROWS, W >= 8 ? 8 : (W >= 4 ? 4 : 2), 1, 0};
}

// launches the instantiation the plan names
template <bool SP8>
static void dwconv7_ln_launch_fmt(const DwLnPlan& p, const float* in, const float* w49, const float* bias, const float* ln_w,
                                  const float* ln_b, float* out, int N, int H, int W, int C, float eps, hipStream_t s) {
  if (p.kind == DWLN_IMAGE) {
    if (C == 384) return dwconv7_ln_image_launch<384, 12, 8, 2, SP8>(in, w49, bias, ln_w, ln_b, out, N, eps, s);
    return dwconv7_ln_image_launch<768, 6, 4, 1, SP8>(in, w49, bias, ln_w, ln_b, out, N, eps, s);
  }
  if (p.kind == DWLN_STREAM) {
    if (C == 96) return dwconv7_ln_stream_launch<96, 8, 4, 3, SP8>(in, w49, bias, ln_w, ln_b, out, N, H, 1, eps, s);
    return dwconv7_ln_stream_launch<192, 4, 4, 3, SP8>(in, w49, bias, ln_w, ln_b, out, N, H, 1, eps, s);
  }
  switch (p.tw * 100 + p.th * 10 + p.wl) {
    case 431: return dwconv7_ln_rows_launch<4, 3, SP8, true>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    case 830: return dwconv7_ln_rows_launch<8, 3, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    case 430: return dwconv7_ln_rows_launch<4, 3, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    case 810: return dwconv7_ln_rows_launch<8, 1, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    case 410: return dwconv7_ln_rows_launch<4, 1, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
    case 210: return dwconv7_ln_rows_launch<2, 1, SP8, false>(in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
  }
  MTGV_CHECK(false, ERR_RUNTIME, "dwconv7_ln: no row-group kernel <%d, %d, %d>", p.tw, p.th, p.wl);
}

// launches the form p names; out_fmt 0: f32 rows, 1: SP8 rows
static void dwconv7_ln_dispatch_plan(const DwLnPlan& p, const float* in, const float* w49, const float* bias, const float* ln_w,
                                     const float* ln_b, float* out, int N, int H, int W, int C, float eps, hipStream_t s, int out_fmt) {
  out_fmt == 1 ? dwconv7_ln_launch_fmt<true>(p, in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s)
               : dwconv7_ln_launch_fmt<false>(p, in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s);
}

// picks the kernel form for the shape and launches it
static void dwconv7_ln_dispatch(const float* in, const float* w49, const float* bias, const float* ln_w, const float* ln_b,
                                float* out, int N, int H, int W, int C, float eps, hipStream_t s, int out_fmt) {
  dwconv7_ln_dispatch_plan(dwconv7_ln_plan(N, H, W, C), in, w49, bias, ln_w, ln_b, out, N, H, W, C, eps, s, out_fmt);
}

}  // namespace mtgv
