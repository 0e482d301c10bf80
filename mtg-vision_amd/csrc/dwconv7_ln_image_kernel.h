// Depthwise 7x7 + LayerNorm, whole-image form (Block.dwconv + Block.norm, convnextv2.py:198-200, 214-216) for the deep
// stages, where one image is small: 12 x 8 x 384 f32 = 144 KB, 6 x 4 x 768 = 72 KB - it fits one CU's LDS.
//
// A block owns ONE image.  The image enters LDS once, row-major exactly as in memory, by LDS-DMA (1 KB per wave
// instruction, no VGPR round trip): no ring, no halo re-read, no trip to global memory inside the FMA loop.
// Thread = ONE channel of a band of TH = H / SPLIT output rows at full width (lanes run over channels: LDS reads are
// consecutive words, conflict-free).  The 49 taps of the channel are 49 VGPRs, the TH x W outputs TH * W more; an input
// row is W ds_read_b32 per thread and feeds up to 7 W output taps.  Which input rows and columns a tap touches is known at
// compile time (H, W, the band), so taps outside the image are not multiplied at all: at 12 x 8 that is 33 % of the 49,
// at 6 x 4 59 %.  C * SPLIT = 768 threads = 12 waves: three live waves on every SIMD, none resident and idle.
//
// The rows arrive while the first ones are convolved: every wave issues its 1 KB piece of each row in row order, so
// "rows 0 .. r have landed" is s_waitcnt vmcnt(pieces of the rows after r) followed by a barrier.  The DMA is issued by
// inline assembly (sp_dma16_saddr): the compiler does not count it, so its own waits stay what they would be without
// it, and the taps are loaded - and pinned in their registers - BEFORE the bulk of the rows is issued (a compiler wait
// for a tap load issued after them would be vmcnt(0) and drain them all).
//
// LayerNorm and output run on channel QUADS again: once the taps are done the outputs change hands through the image's
// LDS ([pixel][channel]) and a thread takes four channels of PT / G pixels.  One channel per thread costs six to ten
// instructions per pixel for quad sums by DPP, squares and the SP8 split; per quad it is the quad kernels' own code.
//
// Arithmetic is the quad kernels' to the bit: bias, then taps kh ascending, kw ascending, one FMA each (only the
// products with a padded zero are gone); LayerNorm sums per pixel as (a0 + a1) + (a2 + a3) per channel quad, then the
// quads in ascending order by one lane; two-pass variance; sp8_piece_from_quad for the SP8 words.
#pragma once
#include <type_traits>

#include "common.h"
#include "sp8.h"

namespace mtgv {

template <int I, int N, typename F>
__device__ __forceinline__ void dwi_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    dwi_static_for<I + 1, N>(f);
  }
}

template <int C, int H, int W, int SPLIT, bool SP8>
__global__ __launch_bounds__(C* SPLIT) void dwconv7_ln_image_kernel(const float* __restrict__ in, const float* __restrict__ w49,
                                                                   const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                                   const float* __restrict__ ln_b, float* __restrict__ out, float eps) {
  constexpr int NT = C * SPLIT, NW = NT / 64, TH = H / SPLIT, ROWF = W * C, PT = H * W, C4N = C / 4;
  constexpr int DPW = ROWF * 4 / 1024 / NW;  // DMA instructions of a wave per row
  constexpr int PITCH = C4N + 4;             // floats between two pixels' quad partials: 16-byte rows, four banks apart
  constexpr int RB = 8;                      // 16-byte reads (four quad partials each) a reducing lane issues before it adds them
  constexpr int PPW = (PT + NW - 1) / NW;    // pixels a wave reduces
  constexpr int G = NT / C4N, PG = PT / G;   // LayerNorm and output: pixel groups of PG pixels, a thread = a channel quad of one
  // first input row of the last band: its k-th row is the latest row any band reads at its k-th step
  constexpr int LAST0 = (SPLIT - 1) * TH - 3 > 0 ? (SPLIT - 1) * TH - 3 : 0;
  constexpr int PRE = LAST0 + 1;             // rows issued before the taps are loaded
  static_assert(H % SPLIT == 0 && (SPLIT == 1 || (SPLIT == 2 && TH >= 3)), "bands must run the same number of row steps");
  static_assert(NT % 256 == 0 && NT <= 1024 && C % 64 == 0, "every SIMD carries the same number of waves; a wave is in one band");
  static_assert(ROWF * 4 % (1024 * NW) == 0 && H * DPW < 64, "whole DMA pieces per wave and row; counts fit s_waitcnt");
  static_assert(PT * PITCH + 2 * PT <= H * ROWF && PPW <= 64 && PT % 4 == 0 && C4N % (4 * RB) == 0, "LayerNorm scratch reuses the image's LDS");
  static_assert(NT % C4N == 0 && PT % G == 0 && C4N % 2 == 0, "whole pixel groups; SP8 lane pairs");
  extern __shared__ __attribute__((aligned(1024))) char dwi_smem[];
  float* const img = reinterpret_cast<float*>(dwi_smem);  // [H][W][C] while the taps run
  float* const part = img;                                // then [PT][PITCH] quad partials, a pixel's quads side by side
  float* const smean = img + PT * PITCH;                  // and [PT] mean, [PT] rstd
  float* const srstd = smean + PT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int band = __builtin_amdgcn_readfirstlane(tid / C);
  const int ch = tid - band * C;
  const int h0 = band * TH;
  const long n = blockIdx.x;
  const char* const src = reinterpret_cast<const char*>(in + n * H * ROWF);

  auto issue_rows = [&](int r0, int r1) {
    for (int r = r0; r < r1; ++r)
#pragma unroll
      for (int k = 0; k < DPW; ++k) {
        const int piece = k * NW + wave;  // 256 floats
        sp_dma16_saddr(src, (uint32_t)((r * ROWF + piece * 256 + lane * 4) * 4), reinterpret_cast<const char*>(img + r * ROWF + piece * 256));
      }
  };
  issue_rows(0, PRE);
  float wt[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) wt[t] = w49[t * C + ch];
  float bv = bias[ch];
  // in their registers now (the compiler waits here, for these and for the first rows, which are needed anyway)
#pragma unroll
  for (int t = 0; t < 49; ++t) asm volatile("" : "+v"(wt[t]));
  asm volatile("" : "+v"(bv));
  issue_rows(PRE, H);

  float acc[TH][W];
#pragma unroll
  for (int t = 0; t < TH; ++t)
#pragma unroll
    for (int j = 0; j < W; ++j) acc[t][j] = bv;

  auto conv_band = [&](auto BAND_T) {
    constexpr int B = decltype(BAND_T)::value;
    constexpr int H0 = B * TH, LO = H0 - 3 > 0 ? H0 - 3 : 0, HI = H0 + TH + 3 < H ? H0 + TH + 3 : H;
    dwi_static_for<0, HI - LO>([&](auto K_T) {
      constexpr int k = decltype(K_T)::value, ih = LO + k;
      // every band's k-th row has landed once rows 0 .. LAST0 + k have: each wave waits for its own pieces, the
      // barrier then says the same of every wave's
      constexpr int need = LAST0 + k < H - 1 ? LAST0 + k : H - 1;
      if constexpr (k == 0 || LAST0 + k <= H - 1) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((H - 1 - need) * DPW) : "memory");
        __syncthreads();
      }
      const float* const rowp = img + ih * ROWF + ch;
      float r[W];
#pragma unroll
      for (int j = 0; j < W; ++j) r[j] = rowp[j * C];
#pragma unroll
      for (int t = 0; t < TH; ++t) {
        const int kh = ih - (H0 + t) + 3;  // output row H0 + t sees this input row as its tap row kh
        if (kh < 0 || kh > 6) continue;
#pragma unroll
        for (int kw = 0; kw < 7; ++kw)
#pragma unroll
          for (int j = 0; j < W; ++j) {
            const int jj = j + kw - 3;
            if (jj < 0 || jj >= W) continue;  // a padded zero: adding 0 * w changes no bit
            acc[t][j] = __builtin_fmaf(r[jj], wt[kh * 7 + kw], acc[t][j]);
          }
      }
    });
  };
  if (SPLIT == 1 || band == 0) conv_band(std::integral_constant<int, 0>{});
  else conv_band(std::integral_constant<int, SPLIT - 1>{});

  // ---- LayerNorm over C per pixel ----
  // One channel per thread suits the taps, not what follows: quad sums, squares and the SP8 split cost a thread six to
  // ten instructions per pixel that way.  So the outputs change hands through LDS (the image's, free now): a thread takes
  // FOUR channels of PT / G pixels, as in the quad kernels, and the rest is their code.
  __syncthreads();  // the image has been read by every wave
#pragma unroll
  for (int t = 0; t < TH; ++t)
#pragma unroll
    for (int j = 0; j < W; ++j) img[((h0 + t) * W + j) * C + ch] = acc[t][j];
  __syncthreads();
  const int g = tid / C4N, q4 = tid - g * C4N;  // pixel group, channel quad
  sp_f4 v[PG];
#pragma unroll
  for (int i = 0; i < PG; ++i) v[i] = *reinterpret_cast<const sp_f4*>(img + (g * PG + i) * C + q4 * 4);
  __syncthreads();  // every output is in its new owner's registers: the same LDS now holds the partial sums
#pragma unroll
  for (int i = 0; i < PG; ++i) part[(g * PG + i) * PITCH + q4] = quad_sum(v[i]);
  __syncthreads();
  const int rp = wave * PPW + lane;  // lane < PPW of every wave reduces one pixel
  const bool reducer = lane < PPW && rp < PT;
  // a pixel's quad partials summed in ascending order, one add each - the quad kernels' chain; only the reads are
  // batched: four quads per ds_read_b128, RB of them in flight
  auto quad_chain = [&]() {
    const sp_f4* const pp = reinterpret_cast<const sp_f4*>(part + rp * PITCH);
    constexpr int NB = C4N / 4 / RB;
    float sum = 0.f;
#pragma unroll 1  // (unrolled, every read is hoisted to the top: 4 C4N registers)
    for (int b = 0; b < NB; ++b) {
      sp_f4 cur[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) cur[i] = pp[b * RB + i];
#pragma unroll
      for (int i = 0; i < RB; ++i) sum += cur[i][0], sum += cur[i][1], sum += cur[i][2], sum += cur[i][3];
    }
    return sum;
  };
  if (reducer) smean[rp] = quad_chain() / (float)C;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PG; ++i) part[(g * PG + i) * PITCH + q4] = quad_sumsq(v[i] - smean[g * PG + i]);
  __syncthreads();
  if (reducer) srstd[rp] = 1.0f / sqrtf(quad_chain() / (float)C + eps);
  __syncthreads();
  const sp_f4 lw = *reinterpret_cast<const sp_f4*>(ln_w + q4 * 4), lb = *reinterpret_cast<const sp_f4*>(ln_b + q4 * 4);
#pragma unroll
  for (int i = 0; i < PG; ++i) {
    const int p = g * PG + i;
    const float mean = smean[p], rstd = srstd[p];
    const sp_f4 o = (v[i] - mean) * rstd * lw + lb;
    float* const op = out + (n * PT + p) * C;
    if (SP8)  // quads q4, q4 ^ 1 are adjacent lanes (C4N is even)
      *reinterpret_cast<sp_h8*>(reinterpret_cast<char*>(op) + (q4 >> 1) * 32 + (q4 & 1) * 16) = sp8_piece_from_quad(o, q4);
    else
      *reinterpret_cast<sp_f4*>(op + q4 * 4) = o;
  }
}

// The shapes this form is built for: the image and the LayerNorm scratch in one CU's LDS, C * SPLIT threads a multiple
// of 256 (AE-nano's C = 320 / 640 make 10 waves: two SIMDs would carry three and two two - it stays on the row groups)
template <int C, int H, int W, int SPLIT, bool SP8>
static void dwconv7_ln_image_launch(const float* in, const float* w49, const float* bias, const float* ln_w, const float* ln_b, float* out,
                                    int N, float eps, hipStream_t s) {
  constexpr size_t lds = (size_t)H * W * C * sizeof(float);
  static_assert(lds <= 160 * 1024, "the image must fit one CU's LDS");
  constexpr auto kern = dwconv7_ln_image_kernel<C, H, W, SPLIT, SP8>;
  lds_opt_in<kern>(lds, 160 * 1024);
  hipLaunchKernelGGL(kern, dim3((unsigned)N), dim3(C * SPLIT), lds, s, in, w49, bias, ln_w, ln_b, out, eps);
  HIP_OK(hipGetLastError());
}

}  // namespace mtgv
