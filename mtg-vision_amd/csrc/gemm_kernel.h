// The implicit-GEMM kernel template and its tile dispatcher.  Included by exactly two translation units,
// one per operand precision, so that the two sets of instantiations compile in parallel:
//   gemm_f32.hip    PREC 0: f32 operands on v_mfma_f32_32x32x2_f32 (exact products, 157 TFLOP/s ceiling)
//   gemm_f16x3.hip  PREC 1: every f32 operand split on the fly into fp16 hi + lo, three
//                           v_mfma_f32_32x32x16_f16 per product (hi*hi + hi*lo + lo*hi, f32 accumulate)
//
// Tile: 256 threads = 4 waves stacked along M.  Block tile BM = 128 rows by
// BN = 32*TN columns; wave w owns rows [w*32, (w+1)*32) x all BN columns
// as TN accumulators of 32x32.  K is consumed in BK-wide steps staged
// through LDS, with the next step's global loads in flight while the current one feeds the MFMAs.
#pragma once
#include "gemm_f32.h"
#include "act.h"

#include <type_traits>

namespace mtgv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct GemmDev {
  GemmArgs a;
  FastDiv d_ohw, d_ow, d_cin, d_kwcin, d_hw, d_cw;
  int tiles_m, tiles_n;
  int remap;     // output rows are not simply m
  int nseg_max;  // APRO: images a 128-row tile can touch (sizes the LDS multiplier tile)
  int off32_ok;  // every operand of the launch spans less than 4 GiB: 32-bit byte offsets are enough
};

// The tiles the kernel is built for, BM = 128 rows x BN = 32*tn columns, K staged bk at a time.  This is the one list:
// gemm_dispatch instantiates one set of kernels per entry (launch_tile) and gemm_plan refuses any other tile.
struct GemmTile {
  int tn, bk;
};
constexpr GemmTile kGemmTiles[] = {{1, 16}, {2, 16}, {3, 16}, {4, 16}, {5, 16}, {1, 32}};
constexpr GemmTile kGemmTopkTile = {2, 16};  // the top-k epilogues' instance (EPI 1 / 3)
constexpr GemmTile kGemmLnTile = {3, 16};    // the LayerNorm epilogue's instance (EPI 2): the stem's 128 x 96 x 16
constexpr bool gemm_tile_built(int tn, int bk) {
  for (const GemmTile& t : kGemmTiles)
    if (t.tn == tn && t.bk == bk) return true;
  return false;
}
static_assert(gemm_tile_built(kGemmTopkTile.tn, kGemmTopkTile.bk) && gemm_tile_built(kGemmLnTile.tn, kGemmLnTile.bk),
              "the epilogue instances sit on built tiles");

// tile of one launch (chosen by gemm_launch, gemm_f32.hip)
struct GemmPlan {
  int tn, bk;  // BM = 128, BN = 32*tn
  int tiles_m, tiles_n;
  int bm() const { return 128; }
  int bn() const { return 32 * tn; }
};

// x = hi + lo + O(2^-22 |x|) while lo is a normal fp16 (|x| >= 2^-3); below that lo is subnormal and the error floor is
// 2^-25 ABSOLUTE (fp16 subnormals are kept by the matrix unit).  Registered weights therefore carry a power-of-two scale
// per row (wscale, undone on the f32 accumulator) that puts the row maximum at 2^13..2^14; activations are O(1) per row
// (LayerNorm outputs, activations, pixels), and a launch whose A may exceed the fp16 range passes a_mul (sp8.h).
// A truncated hi (mask off 13 mantissa bits, no conversion back to f32) is 1 % faster and as accurate on one GEMM,
// but its remainder always has the sign of x, so the dropped lo*lo term becomes a systematic bias that adds up over
// the detector's layers (proto error vs the oracle 1.0e-4 instead of 1.7e-5): rounding it is.
// |x| beyond the fp16 range (65504) becomes inf: visible, not silently wrong - such data belongs on PREC 0.
__device__ __forceinline__ void split_f16(const f32x4 x, f16x4& hi, f16x4& lo) {
  hi = __builtin_convertvector(x, f16x4);
  lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x4), f16x4);
}

// C layout of a 32x32 accumulator: register r of a lane holds column lane & 31 of row gemm_c_row(r) + 4 * (lane >> 5)
__device__ __forceinline__ constexpr int gemm_c_row(int r) { return (r & 3) + 8 * (r >> 2); }

// accumulator -> the value the activation sees.  PREC 1 undoes the weight row's scale and a_mul on the way (ws is a power
// of two times a_unmul: the fused form rounds like multiply-then-add)
template <int PREC>
__device__ __forceinline__ float gemm_scale_bias(float acc, float ws, float bv) {
#pragma clang fp contract(off)
  return PREC == 1 ? __builtin_fmaf(acc, ws, bv) : acc + bv;
}

// column n's entries of the launch's per-column vectors; ok = false for a column past N (nothing is read)
__device__ __forceinline__ float gemm_col_bias(const float* bias, int n, bool ok = true) { return (bias != nullptr && ok) ? bias[n] : 0.f; }
template <int PREC>
__device__ __forceinline__ float gemm_col_unscale(const float* wscale, float a_unmul, int n, bool ok = true) {
#pragma clang fp contract(off)
  return (PREC == 1 && wscale != nullptr && ok) ? wscale[n] * a_unmul : a_unmul;
}

// conv output row m -> (image, output y, output x); ohw = OH * OW.  The A gather and the output row remap both use it.
struct GemmPixel {
  uint32_t img, oh, ow;
};
__device__ __forceinline__ GemmPixel gemm_pixel(uint32_t m, FastDiv d_ohw, FastDiv d_ow, int ohw, int ow_) {
  const uint32_t img = fdiv(m, d_ohw);
  const uint32_t rem = m - img * (uint32_t)ohw;
  const uint32_t oh = fdiv(rem, d_ow);
  return {img, oh, rem - oh * (uint32_t)ow_};
}

}  // namespace mtgv

#include "gemm_epi.h"  // after the helpers above: the epilogue uses them

namespace mtgv {

// LDS bytes of one launch.  PREC 0: f32 rows padded by 16 B (conflict-free ds_read_b128) + the APRO multiplier
// tile.  PREC 1: two fp16 planes (hi, lo) per operand; 16-half rows are contiguous, 32-half rows padded by 16 B.
template <int TN, int BK, bool APRO, int PREC>
constexpr size_t gemm_lds_bytes(int nseg_max) {
  if (PREC == 1) return (size_t)2 * 2 * (128 + 32 * TN) * (BK == 16 ? 16 : BK + 8) * sizeof(_Float16);
  return (size_t)2 * (128 + 32 * TN) * (BK + 4) * sizeof(float) + (APRO ? (size_t)2 * nseg_max * BK * sizeof(float) : 0);
}

template <int TN, int BK, bool CONV, bool APRO, int EPI, int ACT, int PREC>
__global__ __launch_bounds__(256, (TN == 1 ? (BK == 16 ? 6 : 4) : TN == 2 ? (BK == 16 ? 5 : 4) : TN == 3 ? (BK == 16 ? 4 : 3) : TN == 4 ? (BK == 16 ? 3 : 2) : 2)) void gemm_f32_kernel(const GemmDev g) {
#pragma clang fp contract(off)  // loader scaling and epilogue arithmetic identical in every instantiation (act.h)
  constexpr int BM = 128, BN = 32 * TN, LS = BK + 4;
  constexpr int LSH = BK == 16 ? 16 : BK + 8;  // PREC 1: halves per staged row
  constexpr int KQ = BK / 4;      // float4 per staged row
  constexpr int RPP = 256 / KQ;   // rows staged per pass
  constexpr int AP = BM / RPP;
  constexpr int BP = (BN + RPP - 1) / RPP;
  static_assert(BM % RPP == 0, "A tile must be a whole number of passes");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                // PREC 0: [2][BM][LS]
  float* Bs = smem + 2 * BM * LS;  // PREC 0: [2][BN][LS]
  _Float16* const Ah = reinterpret_cast<_Float16*>(smem);  // PREC 1: [buf 2][plane 2][BM][LSH]
  _Float16* const Bh = Ah + 2 * 2 * BM * LSH;              // PREC 1: [buf 2][plane 2][BN][LSH]

  const GemmArgs& p = g.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int z = blockIdx.y;
  const float* const Ap = p.A + (long)z * p.strideA;
  const float* const Wp = p.W + (long)z * p.strideW;
  // PREC 1: B already split into fp16 hi/lo halves in memory (registered weights / bank): no conversion work for it
  const bool b_presplit = PREC == 1 && p.W_split != nullptr;
  const float* const Wld = b_presplit ? p.W_split : Wp;
  float* const Op = p.Out + (long)z * p.strideO;
  int M_eff = p.M;
  if (p.m_count != nullptr) {
    const int mc = p.m_count[z];
    M_eff = mc < p.M ? mc : p.M;
  }

  // XCD-aware tile order: blocks that share an XCD (equal blockIdx % 8) walk a
  // contiguous run of tiles, n fastest, so an A row-panel is fetched once per L2.
  const int L = xcd_block_order<int>(blockIdx.x, gridDim.x);
  const int tile_n = L % g.tiles_n, tile_m = L / g.tiles_n;
  const int bm0 = tile_m * BM, bn0 = tile_n * BN;
  if (bm0 >= M_eff) return;  // whole tile beyond this batch's rows (uniform per block)

  // ---- loader state: each thread stages fixed rows, one float4 column ----
  const int lrow = tid / KQ, lk = (tid % KQ) * 4;
  long a_row[AP];   // CONV: pixel index of image start; dense: element offset of row
  int a_ih0[AP], a_iw0[AP];
  bool a_ok[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int m = bm0 + lrow + i * RPP;
    a_ok[i] = m < M_eff;
    const uint32_t mm = a_ok[i] ? (uint32_t)m : 0u;
    if (CONV) {
      const GemmPixel px = gemm_pixel(mm, g.d_ohw, g.d_ow, p.OH * p.OW, p.OW);
      a_row[i] = (long)px.img * p.H * p.Wd;
      a_ih0[i] = (int)px.oh * p.stride - p.pad;
      a_iw0[i] = (int)px.ow * (p.stride_w > 0 ? p.stride_w : p.stride) - p.pad;
    } else {
      a_row[i] = (long)mm * p.c_total + p.c_off;
      a_ih0[i] = a_iw0[i] = 0;
    }
  }
  long b_row[BP];
  bool b_ok[BP];
#pragma unroll
  for (int i = 0; i < BP; ++i) {
    const int rr = lrow + i * RPP;
    const int n = bn0 + rr;
    b_ok[i] = (rr < BN) && (n < p.N);
    b_row[i] = (long)(b_ok[i] ? n : 0) * p.K;
  }

  f32x4 ra[AP], rb[BP];
  // APRO (GRN apply), PREC 0: the multipliers s[img][k] of the images this tile touches are staged per K step
  // into LDS (Ss[2][nseg][BK]) and applied to the A fragments as they are read - the A loads stay plain.
  // PREC 1 has to scale before the fp16 split: each staged float4 of A loads its own multipliers (L2-resident
  // table) and is multiplied on its way into LDS.
  constexpr int SPT = (APRO && PREC == 0) ? (BM * KQ + 255) / 256 : 1;  // multiplier float4s a thread may have to stage
  f32x4 rsl[SPT];
  f32x4 rsa[(APRO && PREC == 1) ? AP : 1];
  long a_srow[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    a_srow[i] = 0;
    if (APRO && PREC == 1) {
      const int m = bm0 + lrow + i * RPP;
      a_srow[i] = (long)fdiv((uint32_t)(m < M_eff ? m : M_eff - 1), g.d_hw) * p.K;
    }
  }
  float* Ss = Bs + 2 * BN * LS;
  const int img_first_t = APRO ? (int)fdiv((uint32_t)bm0, g.d_hw) : 0;
  int nseg_t = 1;
  if (APRO) {
    const int m_end_t = (bm0 + BM < M_eff) ? bm0 + BM : M_eff;
    nseg_t = (int)fdiv((uint32_t)(m_end_t - 1), g.d_hw) - img_first_t + 1;
  }
  // FAST (chosen per block, below): a dense tile that lies completely inside the problem with K a multiple of BK needs
  // no predicates and no zero fill, and every address is a block-uniform base (advanced by the scalar unit) plus a
  // 32-bit per-thread byte offset: 65 instead of 130 VALU instructions per K step of a 128x96 f16x3 tile (9 MFMAs).
  // Measured effect on the whole step: -1 % GEMM time - the loop is not bound by VALU issue alone.
  unsigned a_off[AP], b_off[BP], s_off[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    a_off[i] = (unsigned)((a_row[i] + lk) * (long)sizeof(float));
    s_off[i] = (unsigned)((a_srow[i] + lk) * (long)sizeof(float));
  }
#pragma unroll
  for (int i = 0; i < BP; ++i) b_off[i] = (unsigned)((b_row[i] + lk) * (long)sizeof(float));
  // APRO, PREC 0: this thread's float4s of the K step's multiplier tile (the fast path needs no k < K test)
  auto load_mults = [&](int kt, auto fast_c) {
    if constexpr (APRO && PREC == 0) {
#pragma unroll
      for (int u = 0; u < SPT; ++u) {
        const int e = tid + u * 256;  // (segment, float4 column) of the multiplier tile
        const int seg = e / KQ, kq = (e % KQ) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (seg < nseg_t && (decltype(fast_c)::value || kt * BK + kq < p.K))
          v = *reinterpret_cast<const f32x4*>(p.a_scale + (long)(img_first_t + seg) * p.K + kt * BK + kq);
        rsl[u] = v;
      }
    }
  };
  auto load_tile = [&](int kt, auto fast_c) {
    if constexpr (decltype(fast_c)::value) {
      const char* const Ak = reinterpret_cast<const char*>(Ap) + (size_t)kt * BK * sizeof(float);
      const char* const Wk = reinterpret_cast<const char*>(Wld) + (size_t)kt * BK * sizeof(float);
#pragma unroll
      for (int i = 0; i < AP; ++i) ra[i] = *reinterpret_cast<const f32x4*>(Ak + a_off[i]);
      if (APRO && PREC == 1) {
        const char* const Sk = reinterpret_cast<const char*>(p.a_scale) + (size_t)kt * BK * sizeof(float);
#pragma unroll
        for (int i = 0; i < AP; ++i) rsa[i] = *reinterpret_cast<const f32x4*>(Sk + s_off[i]);
      }
#pragma unroll
      for (int i = 0; i < BP; ++i) rb[i] = *reinterpret_cast<const f32x4*>(Wk + b_off[i]);  // rows past BN: row 0, never stored
      load_mults(kt, fast_c);
      return;
    }
    const int k = kt * BK + lk;
    const bool kok = k < p.K;
    int kh = 0, kw = 0, c = 0;
    if (CONV) {
      const uint32_t kk = kok ? (uint32_t)k : 0u;
      kh = (int)fdiv(kk, g.d_kwcin);
      const uint32_t r = kk - (uint32_t)kh * (uint32_t)(p.KW * p.Cin);
      kw = (int)fdiv(r, g.d_cin);
      c = (int)(r - (uint32_t)kw * (uint32_t)p.Cin);
    }
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (CONV) {
        const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
        if (a_ok[i] && kok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.Wd)
          v = *reinterpret_cast<const f32x4*>(Ap + (a_row[i] + (long)ih * p.Wd + iw) * p.c_total + p.c_off + c);
      } else {
        if (a_ok[i] && kok) v = *reinterpret_cast<const f32x4*>(Ap + a_row[i] + k);
      }
      ra[i] = v;
      if (APRO && PREC == 1) {
        f32x4 sv = {0.f, 0.f, 0.f, 0.f};
        if (a_ok[i] && kok) sv = *reinterpret_cast<const f32x4*>(p.a_scale + a_srow[i] + k);
        rsa[i] = sv;
      }
    }
#pragma unroll
    for (int i = 0; i < BP; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (b_ok[i] && kok) v = *reinterpret_cast<const f32x4*>(Wld + b_row[i] + k);
      rb[i] = v;
    }
    load_mults(kt, fast_c);
  };
  auto store_tile = [&](int buf) {
    if constexpr (PREC == 1) {
#pragma unroll
      for (int i = 0; i < AP; ++i) {
        f16x4 hi, lo;
        split_f16((APRO ? ra[i] * rsa[i] : ra[i]) * p.a_mul, hi, lo);
        const int o = (lrow + i * RPP) * LSH + lk;
        *reinterpret_cast<f16x4*>(&Ah[(buf * 2 + 0) * BM * LSH + o]) = hi;
        *reinterpret_cast<f16x4*>(&Ah[(buf * 2 + 1) * BM * LSH + o]) = lo;
      }
#pragma unroll
      for (int i = 0; i < BP; ++i)
        if (lrow + i * RPP < BN) {
          f16x4 hi, lo;
          if (b_presplit) {
            const f16x8 hl = __builtin_bit_cast(f16x8, rb[i]);
            hi = f16x4{hl[0], hl[1], hl[2], hl[3]}, lo = f16x4{hl[4], hl[5], hl[6], hl[7]};
          } else {
            split_f16(rb[i], hi, lo);
          }
          const int o = (lrow + i * RPP) * LSH + lk;
          *reinterpret_cast<f16x4*>(&Bh[(buf * 2 + 0) * BN * LSH + o]) = hi;
          *reinterpret_cast<f16x4*>(&Bh[(buf * 2 + 1) * BN * LSH + o]) = lo;
        }
      return;
    }
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const f32x4 v = ra[i];
      *reinterpret_cast<f32x4*>(&As[(buf * BM + lrow + i * RPP) * LS + lk]) = v;
    }
#pragma unroll
    for (int i = 0; i < BP; ++i)
      if (lrow + i * RPP < BN) *reinterpret_cast<f32x4*>(&Bs[(buf * BN + lrow + i * RPP) * LS + lk]) = rb[i];
    if (APRO) {
#pragma unroll
      for (int u = 0; u < SPT; ++u) {
        const int e = tid + u * 256;
        if (e / KQ < nseg_t) *reinterpret_cast<f32x4*>(&Ss[(buf * g.nseg_max + e / KQ) * BK + (e % KQ) * 4]) = rsl[u];
      }
    }
  };

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int wrow0 = bm0 + wave * 32;  // this wave's first row of the problem
  const int col = lane & 31, half = lane >> 5;
  const int arow = wave * 32 + col;
  const int kh4 = 4 * half;

  // a wave whose rows all lie beyond M (ragged last tile, tiny-M problems) skips its MFMAs
  const bool wave_active = wrow0 < M_eff;
  int seg_lane = 0;
  if (APRO) {
    const int m = bm0 + arow;
    seg_lane = (int)fdiv((uint32_t)(m < M_eff ? m : M_eff - 1), g.d_hw) - img_first_t;
  }
  const int nk = (p.K + BK - 1) / BK;
  auto k_loop = [&](auto fast_c) {
    load_tile(0, fast_c);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) load_tile(kt + 1, fast_c);
      const int cur = kt & 1;
      const float* Ab = As + cur * BM * LS;
      const float* Bb = Bs + cur * BN * LS;
      if constexpr (PREC == 1) {
        if (wave_active) {
          const _Float16* const Ahi = Ah + (cur * 2 + 0) * BM * LSH;
          const _Float16* const Alo = Ah + (cur * 2 + 1) * BM * LSH;
          const _Float16* const Bhi = Bh + (cur * 2 + 0) * BN * LSH;
          const _Float16* const Blo = Bh + (cur * 2 + 1) * BN * LSH;
#pragma unroll
          for (int ks = 0; ks < BK / 16; ++ks) {
            // lane half h holds k = ks*16 + 8h + j in element j of both operands' fragments
            const int ko = ks * 16 + 8 * half;
            const f16x8 ah = *reinterpret_cast<const f16x8*>(&Ahi[arow * LSH + ko]);
            const f16x8 al = *reinterpret_cast<const f16x8*>(&Alo[arow * LSH + ko]);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const f16x8 bh = *reinterpret_cast<const f16x8*>(&Bhi[(j * 32 + col) * LSH + ko]);
              const f16x8 bl = *reinterpret_cast<const f16x8*>(&Blo[(j * 32 + col) * LSH + ko]);
              // small cross terms first, the hi*hi product last
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[j], 0, 0, 0);
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[j], 0, 0, 0);
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[j], 0, 0, 0);
            }
          }
        }
      } else if (wave_active) {
#pragma unroll
      for (int kk = 0; kk < BK / 8; ++kk) {
        // lane half h holds k = kk*8 + 4h + j in element j; A and B use the same
        // k assignment, so MFMA j multiplies matching k pairs {j, 4+j}.
        f32x4 a = *reinterpret_cast<const f32x4*>(&Ab[arow * LS + kk * 8 + kh4]);
        if (APRO) a = a * *reinterpret_cast<const f32x4*>(&Ss[(cur * g.nseg_max + seg_lane) * BK + kk * 8 + kh4]);
        f32x4 b[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(&Bb[(j * 32 + col) * LS + kk * 8 + kh4]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[j][e], acc[j], 0, 0, 0);
      }
      }
      if (kt + 1 < nk) store_tile(cur ^ 1);
      __syncthreads();
    }
  };
  if constexpr (!CONV) {
    const bool fast_tile = bm0 + BM <= M_eff && bn0 + BN <= p.N && p.K % BK == 0 && g.off32_ok;
    if (fast_tile)
      k_loop(std::true_type{});
    else
      k_loop(std::false_type{});
  } else {
    k_loop(std::false_type{});
  }

  if constexpr (EPI == 1 || EPI == 3) {
    // ---- fused per-tile top-k (match path): the tile's scores never leave registers.
    // A row's BN scores sit in the 32 lanes of one wave half x TN registers; each
    // round picks the (score desc, id asc) maximum with a 5-step butterfly and
    // retires it.  Candidates go to cand[m][tile_n][kk]; a merge kernel finishes.
    // LAB (EPI 3, row labels, Bank::topk_labelled): a column whose tags fail the row's (all_of, any_of, none_of) masks
    // scores -inf like a column past N; with topk_distinct the winner's group travels with (score, id) through the
    // butterfly and the retire step retires every column of that group (group >= 0), so a tile reports its best eligible
    // rows of pairwise different groups.  A lane owns TN columns: their tags and groups are TN registers each, a row's
    // masks are read once, when the row is filtered.
    constexpr bool LAB = EPI == 3;
    unsigned long tg[LAB ? TN : 1];
    int gr[LAB ? TN : 1];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = bn0 + j * 32 + col;
      const bool nok = n < p.N;
      const float ws = gemm_col_unscale<PREC>(p.wscale, p.a_unmul, n, nok);
      if constexpr (LAB) {
        tg[j] = (p.row_masks != nullptr && nok) ? p.col_tags[n] : 0ul;
        gr[j] = (p.topk_distinct != 0 && nok) ? p.col_groups[n] : -1;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = nok ? acc[j][r] * ws : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wrow0 + gemm_c_row(r) + 4 * half;
      if constexpr (LAB) {
        // (straight-line on purpose: bitwise & and | on the three tests and a select, no short-circuit branches)
        const bool mok = p.row_masks != nullptr && m < M_eff;
        const unsigned long m_all = mok ? p.row_masks[3 * (long)m] : 0ul;
        const unsigned long m_any = mok ? p.row_masks[3 * (long)m + 1] : 0ul;
        const unsigned long m_none = mok ? p.row_masks[3 * (long)m + 2] : 0ul;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const bool el = ((tg[j] & m_all) == m_all) & ((m_any == 0ul) | ((tg[j] & m_any) != 0ul)) & ((tg[j] & m_none) == 0ul);
          acc[j][r] = el ? acc[j][r] : -INFINITY;
        }
      }
      for (int kk = 0; kk < p.topk; ++kk) {
        float bs = -INFINITY;
        int bi = 0x7fffffff, bg = -1;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const float v = acc[j][r];
          if (v > bs) {
            bs = v, bi = bn0 + j * 32 + col;
            if constexpr (LAB) bg = gr[j];
          }
        }
#pragma unroll
        for (int mask = 16; mask > 0; mask >>= 1) {
          const float os = __shfl_xor(bs, mask);
          const int oi = __shfl_xor(bi, mask);
          const int og = LAB ? __shfl_xor(bg, mask) : -1;
          if (os > bs || (os == bs && oi < bi)) bs = os, bi = oi, bg = og;
        }
        if (col == 0 && m < M_eff) {
          const long o = ((long)m * g.tiles_n + tile_n) * p.topk + kk;
          p.cand_s[o] = bs;
          p.cand_i[o] = (bs == -INFINITY) ? -1 : bi;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          bool out = bn0 + j * 32 + col == bi;
          if constexpr (LAB) out = out || (bg >= 0 && gr[j] == bg);
          if (out) acc[j][r] = -INFINITY;
        }
      }
    }
    return;
  }

  // ---- epilogue: bias, activation, residual, store (C layout: col = lane&31, row = gemm_c_row(r) + 4*(lane>>5)).
  // ACT >= 0 fixes the activation at compile time.  Every branch leaves the activated values in acc for the GRN sums. ----
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const bool interior = (bm0 + BM <= M_eff) && (bn0 + BN <= p.N) && !g.remap && p.crop_boxes == nullptr;
  if (interior) {
    // Whole tile inside the problem, rows map 1:1: no per-element predicates, and every address is
    // (wave-uniform base) + (32-bit lane offset), so stores/loads need no per-element address VALU.
    const long row0 = (long)bm0 + (long)wave_u * 32;
    float* const obase = Op + row0 * p.ldo + p.o_off + bn0;
    const unsigned loff = (unsigned)(4 * half) * (unsigned)p.ldo + (unsigned)col;
    float bv[TN], wsv[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      bv[j] = gemm_col_bias(p.bias, bn0 + j * 32 + col);
      wsv[j] = gemm_col_unscale<PREC>(p.wscale, p.a_unmul, bn0 + j * 32 + col);
    }
    if (p.res != nullptr) {
      const float* const rbase = p.res + row0 * p.ldr + bn0;
      const unsigned roff = (unsigned)(4 * half) * (unsigned)p.ldr + (unsigned)col;
      // the residual was written several kernels ago: every load is an HBM / Infinity-Cache round trip.
      // Issue them in two batches of 8 rows ahead of the math and the stores, so the latencies overlap
      // instead of being paid once per output row.
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        float rv[8][TN];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const long rr = gemm_c_row(hb * 8 + q);
#pragma unroll
          for (int j = 0; j < TN; ++j) rv[q][j] = (rbase + rr * p.ldr + j * 32)[roff];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int r = hb * 8 + q;
          const long rr = gemm_c_row(r);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float v = act_fixed<ACT>(gemm_scale_bias<PREC>(acc[j][r], wsv[j], bv[j]), p.act);
            (obase + rr * p.ldo + j * 32)[loff] = v + rv[q][j];
            acc[j][r] = v;
          }
        }
      }
    } else if constexpr (EPI == 2) {
      gemm_epi_ln<TN, PREC>(acc, bv, wsv, p.ln_w, p.ln_b, p.ln_eps, obase, p.ldo, loff, col);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long rr = gemm_c_row(r);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const float v = act_fixed<ACT>(gemm_scale_bias<PREC>(acc[j][r], wsv[j], bv[j]), p.act);
          (obase + rr * p.ldo + j * 32)[loff] = v;
          acc[j][r] = v;
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = bn0 + j * 32 + col;
      const bool nok = n < p.N;
      const float bv = gemm_col_bias(p.bias, n, nok);
      const float ws = gemm_col_unscale<PREC>(p.wscale, p.a_unmul, n, nok);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = wrow0 + gemm_c_row(r) + 4 * half;
        float v = 0.f;
        if (m < M_eff && nok) {
          v = act_fixed<ACT>(gemm_scale_bias<PREC>(acc[j][r], ws, bv), p.act);
          if (p.crop_boxes != nullptr) {
            const float* bx = p.crop_boxes + ((long)z * p.crop_rows + m) * 4;
            const uint32_t py = fdiv((uint32_t)n, g.d_cw);
            const float fx = (float)((uint32_t)n - py * (uint32_t)p.crop_w), fy = (float)py;
            const bool inside = fx >= __fmul_rn(bx[0], p.crop_scale) && fx < __fmul_rn(bx[2], p.crop_scale) &&
                                fy >= __fmul_rn(bx[1], p.crop_scale) && fy < __fmul_rn(bx[3], p.crop_scale);
            if (!inside) v = 0.f;
          }
          float o = v;
          if (p.res != nullptr) o += p.res[(long)m * p.ldr + n];
          long orow = m;
          if (g.remap) {
            const GemmPixel px = gemm_pixel((uint32_t)m, g.d_ohw, g.d_ow, p.OH * p.OW, p.OW);
            orow = ((long)px.img * p.OH2 + px.oh * p.os + p.oy) * p.OW2 + px.ow * p.os + p.ox;
          }
          Op[orow * p.ldo + p.o_off + n] = o;
        }
        acc[j][r] = v;
      }
    }
  }

  // GRN partial sums of squares over acc (red = smem: the K loop ended on a barrier, LDS is free)
  if (p.grn_part != nullptr) {
    float* red = smem;  // [4][BN]; the K loop ended on a barrier, LDS is free
    const int m_end = (bm0 + BM < M_eff) ? bm0 + BM : M_eff;
    const int img_first = (int)fdiv((uint32_t)bm0, g.d_hw);
    const int img_last = (int)fdiv((uint32_t)(m_end - 1), g.d_hw);
    const bool one_image = interior && img_first == img_last;  // every row of the tile in one image: no row tests
    for (int s = 0; s <= img_last - img_first; ++s) {
      const int lo = (img_first + s) * p.hw, hi = lo + p.hw;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float sum = 0.f;
        if (one_image) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sum += acc[j][r] * acc[j][r];
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = wrow0 + gemm_c_row(r) + 4 * half;
            const float v = acc[j][r];
            sum += (m >= lo && m < hi) ? v * v : 0.f;
          }
        }
        sum += __shfl_xor(sum, 32);
        if (half == 0) red[wave * BN + j * 32 + col] = sum;
      }
      __syncthreads();
      if (tid < BN) {
        const int n = bn0 + tid;
        if (n < p.N)
          p.grn_part[((long)tile_m * p.segmax + s) * p.N + n] =
              ((red[tid] + red[BN + tid]) + red[2 * BN + tid]) + red[3 * BN + tid];
      }
      __syncthreads();
    }
  }
}

template <int TN, int BK, bool CONV, bool APRO, int EPI, int ACT, int PREC>
static void launch_one(const GemmDev& g, int grid, hipStream_t s) {
  const size_t lds = gemm_lds_bytes<TN, BK, APRO, PREC>(g.nseg_max);
  lds_opt_in<gemm_f32_kernel<TN, BK, CONV, APRO, EPI, ACT, PREC>>(lds, 96 * 1024);
  hipLaunchKernelGGL((gemm_f32_kernel<TN, BK, CONV, APRO, EPI, ACT, PREC>), dim3(grid, g.a.batch), dim3(256), lds, s, g);
}

// activation fixed at compile time for the combinations the path uses; anything else takes the
// runtime-switch instance (ACT = -1)
template <int TN, int BK, int PREC>
static void launch_variant(const GemmDev& g, bool conv, bool apro, int grid, hipStream_t s) {
  const int act = g.a.act;
  if (apro) {
    launch_one<TN, BK, false, true, 0, ACT_NONE, PREC>(g, grid, s);
  } else if (conv) {
    if (act == ACT_SILU) launch_one<TN, BK, true, false, 0, ACT_SILU, PREC>(g, grid, s);
    else if (act == ACT_NONE) launch_one<TN, BK, true, false, 0, ACT_NONE, PREC>(g, grid, s);
    else launch_one<TN, BK, true, false, 0, -1, PREC>(g, grid, s);
  } else {
    if (act == ACT_NONE) launch_one<TN, BK, false, false, 0, ACT_NONE, PREC>(g, grid, s);
    else if (act == ACT_MISH) launch_one<TN, BK, false, false, 0, ACT_MISH, PREC>(g, grid, s);
    else if (act == ACT_GELU) launch_one<TN, BK, false, false, 0, ACT_GELU, PREC>(g, grid, s);
    else if (act == ACT_SILU) launch_one<TN, BK, false, false, 0, ACT_SILU, PREC>(g, grid, s);
    else launch_one<TN, BK, false, false, 0, -1, PREC>(g, grid, s);
  }
}

// one case per entry of kGemmTiles: the instances are the list
template <int PREC, size_t I = 0>
static bool launch_tile(const GemmDev& g, const GemmPlan& pl, bool conv, bool apro, int grid, hipStream_t s) {
  if constexpr (I < sizeof(kGemmTiles) / sizeof(kGemmTiles[0])) {
    constexpr GemmTile T = kGemmTiles[I];
    if (pl.tn == T.tn && pl.bk == T.bk) {
      launch_variant<T.tn, T.bk, PREC>(g, conv, apro, grid, s);
      return true;
    }
    return launch_tile<PREC, I + 1>(g, pl, conv, apro, grid, s);
  }
  return false;
}

// Picks the instantiation for a plan (a planned tile is a built one: gemm_plan).  top-k launches (match path: scores +
// per-tile top-k) use one tile shape, 128 queries x 64 bank rows, BK 16.
template <int PREC>
static void gemm_dispatch(const GemmDev& g, const GemmPlan& pl, bool conv, bool apro, int grid, hipStream_t s) {
  if (g.a.topk > 0) {
    constexpr GemmTile T = kGemmTopkTile;
    MTGV_CHECK(pl.tn == T.tn && pl.bk == T.bk, ERR_INVALID, "gemm: top-k planned on tile tn=%d bk=%d", pl.tn, pl.bk);
    if (topk_labelled(g.a)) launch_one<T.tn, T.bk, false, false, 3, ACT_NONE, PREC>(g, grid, s);  // row labels: filter / distinct
    else launch_one<T.tn, T.bk, false, false, 1, ACT_NONE, PREC>(g, grid, s);
    return;
  }
  if (g.a.ln_w != nullptr) {  // fused LayerNorm epilogue: the stem's tile only (gemm_ln_fusable)
    constexpr GemmTile T = kGemmLnTile;
    MTGV_CHECK(pl.tn == T.tn && pl.bk == T.bk && conv && !apro && g.a.act == ACT_NONE, ERR_INVALID,
               "gemm: no LayerNorm epilogue for this launch (tn=%d bk=%d)", pl.tn, pl.bk);
    launch_one<T.tn, T.bk, true, false, 2, ACT_NONE, PREC>(g, grid, s);
    return;
  }
  const bool found = launch_tile<PREC>(g, pl, conv, apro, grid, s);
  MTGV_CHECK(found, ERR_INVALID, "gemm: no kernel for tile tm=1 tn=%d bk=%d", pl.tn, pl.bk);
}

}  // namespace mtgv

