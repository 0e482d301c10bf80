// The detector's own device kernels (detector.hip launches them; the convolutions are gemm_launch's, gemm_f32.h):
//   decode_kernel, decode_obb_kernel, nhwc_to_nchw_kernel, mask_binarize_kernel, conv0_u8_kernel, conv0_u8_wide_kernel, maxpool5_sp8_kernel,
//   sppf_pools_sp8_kernel, mask_logits_kernel
#pragma once
#include "act.h"
#include "detector.h"
#include "head_decode.h"
#include "sp8.h"

#include <math.h>

namespace mtgv {

// decode: DFL expectation -> ltrb -> xywh * stride; class sigmoid; coefficient copy (the arithmetic is head_decode.h's,
// shared with the row form of nms_kernel)
// rows: [0,64) box logits (4 sides x 16 bins), [h.coef, +nm) coeffs, [h.cls, +nc) class logits (the detector's: detector.h)

__global__ __launch_bounds__(256) void decode_kernel(HeadRows h, float* __restrict__ pred, int n, int nc, int nm, int na) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * na) return;
  const int img = (int)(idx / na), a = (int)(idx % na);
  const HeadAnchor an = head_anchor(h, img, a);
  const float* row = an.row;
  float xywh[4];
  head_box(an, xywh);
  float* P = pred + (long)img * (4 + nc + nm) * na + a;
  P[0] = xywh[0];
  P[(long)na] = xywh[1];
  P[(long)2 * na] = xywh[2];
  P[(long)3 * na] = xywh[3];
  for (int c = 0; c < nc; ++c) P[(long)(4 + c) * na] = head_score(row[h.cls + c]);
  for (int c = 0; c < nm; c += 4) {
    if (c + 4 <= nm) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(row + h.coef + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) P[(long)(4 + nc + c + e) * na] = t[e];
    } else {
      for (int e = 0; c + e < nm; ++e) P[(long)(4 + nc + c + e) * na] = row[h.coef + c + e];
    }
  }
}

// OBB decode: head rows -> pred (n, 4 + nc + 1, na) = xywh in pixels, class sigmoids, angle (head_decode.h: head_rbox)
__global__ __launch_bounds__(256) void decode_obb_kernel(HeadRows h, float* __restrict__ pred, int n, int nc, int na) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * na) return;
  const int img = (int)(idx / na), a = (int)(idx % na);
  const HeadAnchor an = head_anchor(h, img, a);
  float r[5];
  head_rbox(an, an.row[h.coef], r);
  float* P = pred + (long)img * (5 + nc) * na + a;
  P[0] = r[0];
  P[(long)na] = r[1];
  P[(long)2 * na] = r[2];
  P[(long)3 * na] = r[3];
  for (int c = 0; c < nc; ++c) P[(long)(4 + c) * na] = head_score(an.row[h.cls + c]);
  P[(long)(4 + nc) * na] = r[4];
}

// NHWC -> NCHW (raw protos for parity tests)
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int C, long HW,
                                                          long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over N*C*HW (output order)
  if (idx >= total) return;
  const long p = idx % HW;
  const long t = idx / HW;
  const int c = (int)(t % C);
  const long n = t / C;
  out[idx] = in[(n * HW + p) * C + c];
}

// process_mask(..., upsample=True) tail: F.interpolate(bilinear, align_corners=False) x scale, then > 0.
// PX consecutive output pixels of a row per thread (one 16-byte store instead of sixteen 1-byte stores).
template <int PX>
__global__ __launch_bounds__(256) void mask_binarize_kernel(const float* __restrict__ logits, uint8_t* __restrict__ out, int mh,
                                                           int mw, int scale, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over n * (mh*scale) * (mw*scale / PX)
  if (idx >= total) return;
  const int ow = mw * scale, oh = mh * scale;
  const int owp = ow / PX;
  const int xg = (int)(idx % owp);
  const long t = idx / owp;
  const int y = (int)(t % oh);
  const long n = t / oh;
  const float inv = 1.0f / (float)scale;
  float sy = inv * ((float)y + 0.5f) - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  const int y0 = (int)sy;
  const int y1 = y0 + (y0 < mh - 1 ? 1 : 0);
  const float ly1 = sy - (float)y0;
  const float ly0 = 1.0f - ly1;
  const float* L = logits + n * mh * mw;
  uint8_t px[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int x = xg * PX + j;
    float sx = inv * ((float)x + 0.5f) - 0.5f;
    sx = sx < 0.f ? 0.f : sx;
    const int x0 = (int)sx;
    const int x1 = x0 + (x0 < mw - 1 ? 1 : 0);
    const float lx1 = sx - (float)x0;
    const float lx0 = 1.0f - lx1;
    const float v = ly0 * (lx0 * L[y0 * mw + x0] + lx1 * L[y0 * mw + x1]) + ly1 * (lx0 * L[y1 * mw + x0] + lx1 * L[y1 * mw + x1]);
    px[j] = v > 0.f ? 1 : 0;
  }
  uint8_t* const o = out + (n * oh + y) * (long)ow + (long)xg * PX;
  if (PX == 16) {
    *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(px);
  } else {
#pragma unroll
    for (int j = 0; j < PX; ++j) o[j] = px[j];
  }
}

// model.0 straight from the uint8 frame: Conv(3 -> 16, k3, s2, p1) + folded BN + SiLU, output SP8 or f32.
// K = 27 is too short for the matrix cores and the layer is bound by its 16-channel output; a thread computes four
// neighbouring output pixels x 16 channels with f32 FMAs, weights broadcast from LDS.  Fuses the u8 -> float
// conversion (img / 255, ultralytics preprocess) that used to be a separate pass over a 4-channel float copy.
template <bool SP8>
__global__ __launch_bounds__(256) void conv0_u8_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int H, int W, int flip,
                                                      long total) {
  __shared__ __attribute__((aligned(16))) float ws[16 * 9 * 4 + 16];  // [o][tap][4] (cin padded to 4) + bias
  for (int i = threadIdx.x; i < 16 * 9 * 4; i += 256) ws[i] = w[i];
  if (threadIdx.x < 16) ws[16 * 9 * 4 + threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int OS = H >> 1, OQ = W >> 3;  // output rows, groups of 4 output columns per row (W % 8 == 0)
  // Output staging: a thread's four pixels are 256 contiguous bytes and thread i + 1 continues where thread i ends, so
  // a store issued by every lane for its own piece would touch 64 different lines.  Each wave passes its pieces through
  // LDS (two pixels = 8 pieces of 16 B per thread at a time, rows padded to 144 B) and stores them back transposed:
  // eight lanes write one thread's 128 bytes, a store instruction writes eight whole lines.
  __shared__ __attribute__((aligned(16))) f32x4 stage[4][64][9];
  const long idx_raw = (long)blockIdx.x * 256 + threadIdx.x;  // over n * OS * OQ
  const long idx = idx_raw < total ? idx_raw : total - 1;     // (threads past the end compute a duplicate and store nothing)
  const int q = (int)(idx % OQ);
  const long t = idx / OQ;
  const int oh = (int)(t % OS);
  const long n = t / OS;
  const int ow0 = q * 4;
  float acc[4][16];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[p][o] = ws[16 * 9 * 4 + o];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * oh - 1 + kh;
    if (ih < 0 || ih >= H) continue;
    const uint8_t* const rowp = frames + ((n * H + ih) * (long)W) * 3;
    float x[9][3];  // input columns 2*ow0-1 .. 2*ow0+7
    // The nine pixels are bytes 24 q - 3 .. 24 q + 23 of the row: one dword for the pixel left of the strip (zero padding
    // at q == 0 - the only column that can fall outside, W = 8 OQ) and three aligned 8-byte loads for the other eight.
    uint32_t d[7];
    d[0] = q > 0 ? *reinterpret_cast<const uint32_t*>(rowp + 24 * q - 4) : 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint2 v = *reinterpret_cast<const uint2*>(rowp + 24 * q + 8 * k);
      d[1 + 2 * k] = v.x, d[2 + 2 * k] = v.y;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      float b[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int k = 1 + 3 * j + ch;  // byte index in d[]
        const float u = (float)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);  // v_cvt_f32_ubyteN
        // u / 255 correctly rounded without the division sequence: one Newton step on u * fl(1/255) gives the IEEE
        // quotient for every byte value (tests/test_oracle_detector_cpu.py checks all 256 against exact rational arithmetic)
        const float r255 = 1.0f / 255.0f;
        const float q0 = u * r255;
        b[ch] = __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, u), r255, q0);
      }
      x[j][0] = flip ? b[2] : b[0], x[j][1] = b[1], x[j][2] = flip ? b[0] : b[2];
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(&ws[(o * 9 + kh * 3 + kw) * 4]);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          float a = acc[p][o];
          a = __builtin_fmaf(x[2 * p + kw][0], wv[0], a);
          a = __builtin_fmaf(x[2 * p + kw][1], wv[1], a);
          a = __builtin_fmaf(x[2 * p + kw][2], wv[2], a);
          acc[p][o] = a;
        }
      }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long wave_idx0 = (long)blockIdx.x * 256 + wave * 64;  // output is contiguous in idx order: 64 floats per thread
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int p = half * 2 + pp;
      f32x4 v[4];
#pragma unroll
      for (int o = 0; o < 16; ++o) v[o >> 2][o & 3] = act_silu(acc[p][o]);
      if (SP8) {
        sp_h8 hi, lo;
        sp8_split8(v[0], v[1], hi, lo);
        stage[wave][lane][pp * 4 + 0] = __builtin_bit_cast(f32x4, hi), stage[wave][lane][pp * 4 + 1] = __builtin_bit_cast(f32x4, lo);
        sp8_split8(v[2], v[3], hi, lo);
        stage[wave][lane][pp * 4 + 2] = __builtin_bit_cast(f32x4, hi), stage[wave][lane][pp * 4 + 3] = __builtin_bit_cast(f32x4, lo);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) stage[wave][lane][pp * 4 + k] = v[k];
      }
    }
    // (one wave reads only what it wrote itself: LDS operations of a wave complete in order)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int T = i * 8 + (lane >> 3), k = lane & 7;
      const f32x4 piece = stage[wave][T][k];
      if (wave_idx0 + T < total) *reinterpret_cast<f32x4*>(out + (wave_idx0 + T) * 64 + half * 32 + k * 4) = piece;
    }
  }
}

// model.0 at the wider scales: Conv(3 -> COUT, k3, s2, p1) + folded BN + SiLU for COUT = 32 (s), 48 (YOLOv8 m), 64
// (YOLO11 m); COUT = 16 exists for the test that compares this kernel with conv0_u8_kernel bit for bit.  The same
// arithmetic per output - the exactly rounded u / 255, the flip swap, bias then FMAs in (kh, kw, c) order, SiLU - on TWO
// neighbouring output pixels x COUT channels per thread: 2 COUT accumulators (4 x 16 = 64 in conv0_u8_kernel; 64 / 96 /
// 128 here) stay in registers without scratch, and a thread's output is still one contiguous run of 2 COUT floats that
// starts where its neighbour's ends.  The five input pixels are bytes 12 q - 3 .. 12 q + 11 of the row: four aligned dwords
// (W % 8 == 0 keeps every row 8-byte aligned).  Stores go through the same per-wave LDS transpose in chunks of 128 bytes =
// four 8-channel groups (SP8: hi and lo piece of each): eight lanes write one thread's chunk, a store instruction writes
// eight whole lines.  With COUT = 48 a chunk straddles the two pixels; the groups are enumerated in memory order.
template <bool SP8, int COUT>
__global__ __launch_bounds__(256) void conv0_u8_wide_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out, int H, int W, int flip,
                                                           long total) {
  static_assert(COUT % 16 == 0 && COUT >= 16 && COUT <= 64, "whole 128-byte chunks per thread, accumulators in registers");
  constexpr int NW = COUT * 9 * 4;
  __shared__ __attribute__((aligned(16))) float ws[NW + COUT];  // [o][tap][4] (cin padded to 4) + bias
  for (int i = threadIdx.x; i < NW; i += 256) ws[i] = w[i];
  if (threadIdx.x < COUT) ws[NW + threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int OS = H >> 1, OQ = W >> 2;  // output rows, groups of 2 output columns per row
  __shared__ __attribute__((aligned(16))) f32x4 stage[4][64][9];  // (rows padded to 144 B)
  const long idx_raw = (long)blockIdx.x * 256 + threadIdx.x;  // over n * OS * OQ
  const long idx = idx_raw < total ? idx_raw : total - 1;     // (threads past the end compute a duplicate and store nothing)
  const int q = (int)(idx % OQ);
  const long t = idx / OQ;
  const int oh = (int)(t % OS);
  const long n = t / OS;
  float acc[2][COUT];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[p][o] = ws[NW + o];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * oh - 1 + kh;
    if (ih < 0 || ih >= H) continue;
    const uint8_t* const rowp = frames + ((n * H + ih) * (long)W) * 3;
    // input columns 4 q - 1 .. 4 q + 3: one dword for the pixel left of the pair (zero padding at q == 0 - the only column
    // that can fall outside, W = 4 OQ) and three for the other four
    uint32_t d[4];
    d[0] = q > 0 ? *reinterpret_cast<const uint32_t*>(rowp + 12 * q - 4) : 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[1 + k] = *reinterpret_cast<const uint32_t*>(rowp + 12 * q + 4 * k);
    float x[5][3];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float b[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int k = 1 + 3 * j + ch;  // byte index in d[]
        const float u = (float)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
        const float r255 = 1.0f / 255.0f;  // (conv0_u8_kernel: one Newton step gives the IEEE quotient u / 255)
        const float q0 = u * r255;
        b[ch] = __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, u), r255, q0);
      }
      x[j][0] = flip ? b[2] : b[0], x[j][1] = b[1], x[j][2] = flip ? b[0] : b[2];
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int o = 0; o < COUT; ++o) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(&ws[(o * 9 + kh * 3 + kw) * 4]);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          float a = acc[p][o];
          a = __builtin_fmaf(x[2 * p + kw][0], wv[0], a);
          a = __builtin_fmaf(x[2 * p + kw][1], wv[1], a);
          a = __builtin_fmaf(x[2 * p + kw][2], wv[2], a);
          acc[p][o] = a;
        }
      }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long wave_idx0 = (long)blockIdx.x * 256 + wave * 64;  // output is contiguous in idx order: 2 COUT floats per thread
  constexpr int G = COUT / 8;                                  // 8-channel groups per pixel
#pragma unroll
  for (int c = 0; c < COUT / 16; ++c) {  // 128-byte chunks of the thread's output
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int gi = c * 4 + g4, p = gi / G, o0 = (gi % G) * 8;
      f32x4 v0, v1;
#pragma unroll
      for (int e = 0; e < 4; ++e) v0[e] = act_silu(acc[p][o0 + e]), v1[e] = act_silu(acc[p][o0 + 4 + e]);
      if (SP8) {
        sp_h8 hi, lo;
        sp8_split8(v0, v1, hi, lo);
        stage[wave][lane][g4 * 2] = __builtin_bit_cast(f32x4, hi), stage[wave][lane][g4 * 2 + 1] = __builtin_bit_cast(f32x4, lo);
      } else {
        stage[wave][lane][g4 * 2] = v0, stage[wave][lane][g4 * 2 + 1] = v1;
      }
    }
    // (one wave reads only what it wrote itself: LDS operations of a wave complete in order)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int T = i * 8 + (lane >> 3), k = lane & 7;
      const f32x4 piece = stage[wave][T][k];
      if (wave_idx0 + T < total) *reinterpret_cast<f32x4*>(out + (wave_idx0 + T) * (2 * COUT) + c * 32 + k * 4) = piece;
    }
  }
}

// The 5x5 window (stride 1, pad 2) around pixel (h, w) of an H x W map of SP8 chunks, for both pool kernels below: per
// lane element the (hi, lo) pair with the greatest hi + lo, kept as it is (no re-rounding).  at(ih, iw) points to the
// chunk (hi piece, lo piece) of an in-frame pixel.  Rows, then columns, ascending; strict >: of equal sums the first wins.
// (Results come back by value: written through references, the two kernels compiled to half as much code again.)
struct Sp8Pair { sp_h8 hi, lo; };
template <class At>
__device__ __forceinline__ Sp8Pair sp8_max5x5(int h, int w, int H, int W, At at) {
  float best[8];
  sp_h8 bh, bl;
#pragma unroll
  for (int e = 0; e < 8; ++e) best[e] = -INFINITY, bh[e] = (_Float16)0.f, bl[e] = (_Float16)0.f;
  for (int dh = -2; dh <= 2; ++dh) {
    const int ih = h + dh;
    if (ih < 0 || ih >= H) continue;
    for (int dw = -2; dw <= 2; ++dw) {
      const int iw = w + dw;
      if (iw < 0 || iw >= W) continue;
      const sp_h8* const p = at(ih, iw);
      const sp_h8 vh = p[0], vl = p[1];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = (float)vh[e] + (float)vl[e];
        if (v > best[e]) best[e] = v, bh[e] = vh[e], bl[e] = vl[e];
      }
    }
  }
  return {bh, bl};
}

// 5x5 max pool (stride 1, pad 2) on SP8 channel slices: a thread owns one 8-channel chunk (sp8_max5x5)
__global__ __launch_bounds__(256) void maxpool5_sp8_kernel(const float* __restrict__ in, int ci_total, int ci_off,
                                                          float* __restrict__ out, int co_total, int co_off, int H, int W, int C,
                                                          long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over N*H*W*(C/8)
  if (idx >= total) return;
  const int c8n = C >> 3;
  const int c = (int)(idx % c8n) * 8;
  long t = idx / c8n;
  const int w = (int)(t % W);
  t /= W;
  const int h = (int)(t % H);
  const long n = t / H;
  const Sp8Pair best = sp8_max5x5(h, w, H, W, [&](int ih, int iw) {
    return reinterpret_cast<const sp_h8*>(in + ((n * H + ih) * W + iw) * ci_total + ci_off + c);
  });
  sp_h8* const o = reinterpret_cast<sp_h8*>(out + ((n * H + h) * W + w) * co_total + co_off + c);
  o[0] = best.hi, o[1] = best.lo;
}

// SPPF's three chained 5x5 max pools (y1 = m(x), y2 = m(y1), y3 = m(y2)) in ONE launch: a block owns one 8-channel chunk
// of one image, keeps the (hi, lo) pairs of all H x W pixels in LDS and runs the three rounds out of it - the three
// separate launches were 25 us each for 6.5 MB of data (latency-bound: 25 dependent loads per thread).  The same
// sp8_max5x5 per pixel: the pairs written are those of maxpool5_sp8_kernel, bit for bit.
__global__ __launch_bounds__(256) void sppf_pools_sp8_kernel(float* __restrict__ buf, int c_total, int ch, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) char sp_sm[];
  const int HW = H * W;
  sp_h8* const a = reinterpret_cast<sp_h8*>(sp_sm);  // [HW][2]: hi piece, lo piece
  sp_h8* const b = a + (size_t)HW * 2;
  const int c8n = ch >> 3;
  const long n = blockIdx.x / c8n;
  const int c = (int)(blockIdx.x % c8n) * 8;
  char* const img = reinterpret_cast<char*>(buf + n * (long)HW * c_total);
  for (int p = threadIdx.x; p < HW; p += 256) {
    const sp_h8* const src = reinterpret_cast<const sp_h8*>(img + ((long)p * c_total + c) * 4);
    a[2 * p] = src[0], a[2 * p + 1] = src[1];
  }
  __syncthreads();
  sp_h8 *in = a, *out = b;
  for (int round = 1; round <= 3; ++round) {
    for (int p = threadIdx.x; p < HW; p += 256) {
      const int h = p / W, w = p - h * W;
      const Sp8Pair best = sp8_max5x5(h, w, H, W, [&](int ih, int iw) { return in + 2 * (ih * W + iw); });
      out[2 * p] = best.hi, out[2 * p + 1] = best.lo;
      sp_h8* const dst = reinterpret_cast<sp_h8*>(img + ((long)p * c_total + round * ch + c) * 4);
      dst[0] = best.hi, dst[1] = best.lo;
    }
    __syncthreads();
    sp_h8* const t = in;
    in = out, out = t;
  }
}

// Mask logits of a few detections per frame (process_mask + crop_mask behind od_export.py:152): out[z][m][px] =
// <coef[z][m], protos[z][px]> inside box m, 0 outside - f32 FMA chain in k order.  One thread per prototype pixel reads
// its 32 channels once (128 contiguous bytes) and serves all the frame's kept rows; coefficients and scaled boxes sit in
// LDS.  Rows beyond n_det[z] are written as zeros (empty masks).
__global__ __launch_bounds__(256) void mask_logits_kernel(const float* __restrict__ coef, const float* __restrict__ protos,
                                                         const int* __restrict__ n_det, const float* __restrict__ boxes,
                                                         float* __restrict__ out, int npx, int pw, int mask_rows, int max_det,
                                                         float crop_scale) {
  __shared__ __attribute__((aligned(16))) float sc[16 * 32];
  __shared__ float sb[16 * 4];
  const int z = blockIdx.y;
  const int mc = n_det[z] < mask_rows ? n_det[z] : mask_rows;
  for (int i = threadIdx.x; i < mc * 32; i += 256) sc[i] = coef[(long)z * max_det * 32 + i];
  if (threadIdx.x < mc * 4) sb[threadIdx.x] = __fmul_rn(boxes[(long)z * max_det * 4 + threadIdx.x], crop_scale);
  __syncthreads();
  const int px = blockIdx.x * 256 + threadIdx.x;
  if (px >= npx) return;
  f32x4 p[8];
  const f32x4* src = reinterpret_cast<const f32x4*>(protos + ((long)z * npx + px) * 32);
#pragma unroll
  for (int q = 0; q < 8; ++q) p[q] = src[q];
  const int py = px / pw;
  const float fx = (float)(px - py * pw), fy = (float)py;
  for (int m = 0; m < mc; ++m) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 c = *reinterpret_cast<const f32x4*>(&sc[m * 32 + q * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(c[e], p[q][e], acc);
    }
    const bool inside = fx >= sb[m * 4] && fx < sb[m * 4 + 2] && fy >= sb[m * 4 + 1] && fy < sb[m * 4 + 3];
    out[((long)z * mask_rows + m) * npx + px] = inside ? acc : 0.f;
  }
  for (int m = mc; m < mask_rows; ++m) out[((long)z * mask_rows + m) * npx + px] = 0.f;
}

}  // namespace mtgv
