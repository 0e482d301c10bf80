// The tail of a C2f block as one launch: its last bottleneck (3x3 -> 3x3, optional shortcut) and the block's closing 1x1
// conv over the concat, on SP8 activations (sp8.h), with the bottleneck's two intermediates kept in LDS.
//
//   t     = SiLU(W1 (*) y_last + b1)             3x3 / stride 1 / pad 1, ch -> ch
//   y_new = [y_last +] SiLU(W2 (*) t + b2)       3x3 / stride 1 / pad 1, ch -> ch
//   out   = SiLU(W3 . [cat slices | y_new] + b3) 1x1, (2 + n) ch -> 2 ch
//
// y_last is the last ch-channel slice of `cat` in front of the bottleneck.  Neither t nor y_new goes to HBM: the
// launch reads the earlier slices of cat (y_last with a 2-pixel halo) and writes out.
//
// A block of four waves owns an 8 x 32 tile of output pixels of one frame (ch = 16; the ch = 32 form is described at
// c2f_tail32_kernel below):
//   P0  LDS-DMA, pieces as they lie in HBM: the 12 x 36 window of y_last (pixels outside the frame come from the zero
//       page), the three weight matrices, and the tile's pixels of the slices in front of y_last
//   P1  the 1x1's k16 steps over the slices that exist already (cat[0 : ch], then y_last out of the window) - k ascending,
//       so these come first; the accumulators stay in registers until y_new exists, and the early slices' LDS is free
//   P2  t on the 10 x 34 pixels the second conv reads, split to SP8 into LDS; pixels of t outside the frame are ZERO (the
//       second conv pads t with zeros - it does not see the conv of a zero-padded input)
//   P3  y_new on the tile, (+ y_last out of the window,) split to SP8 into LDS over t
//   P4  the 1x1's last step(s) over y_new, epilogue, SP8 rows staged through LDS and stored as whole lines
//
// Bit-identical to the three gemm_sp_kernel launches it replaces (gemm_sp_kernel.h): the same v_mfma_f32_32x32x16_f16
// with the 16 output channels of the 3x3 convs padded to 32 columns (SP_CFG_WIN16), K walked tap by tap over 16-channel
// slices (SP_A_WINDOW), the 1x1 in ascending k16 steps including the zero step that pads K = 48 to the dense kernel's
// 32-k stage, lo*hi + hi*lo + hi*hi per step, and the same scale * acc + bias -> SiLU -> (+ residual) -> split epilogue.
// The window holds real zeros where the original predicates a tap's fragment to zero: the same operand values.
//
// LDS rows are pixels of 64 bytes (one 16-channel SP8 slice), 16-byte slots swizzled by the pixel index like the
// 64-byte rows of a gemm_sp_kernel stage: slot' = slot ^ ((pixel >> 2) & 3).
#pragma once
#include "act.h"
#include "gemm_sp_kernel.h"
#include "sp8.h"

namespace mtgv {

// Geometry and LDS layout of the ch = 16 instance, shared by the kernel and its launcher.
struct C2fTail16 {
  static constexpr int CH = 16, RB = 64;            // channels per slice, bytes per pixel of a slice
  static constexpr int TH = 8, TW = 32;             // output tile: one 32-pixel MFMA row block per tile row
  static constexpr int WH = TH + 4, WW = TW + 4;    // window of y_last
  static constexpr int UH = TH + 2, UW = TW + 2;    // pixels of t
  static constexpr int WIN_PX = WH * WW, T_PX = UH * UW, T_BLK = (T_PX + 31) / 32;
  static constexpr int NW = 4;                      // waves; each owns TH / NW tile rows
  static constexpr int K3 = 3 * CH, N3 = 2 * CH;    // the 1x1: [cat0 | y_last | y_new] -> 2 ch
  static_assert(WIN_PX * RB % kSpPiece == 0 && TH % NW == 0 && TW == 32, "whole DMA pieces, whole row blocks");
  // [window][t, first the early slice then y_new over it][W1][W2, the store staging over both][W3]
  static constexpr int WIN = 0;
  static constexpr int T = WIN + WIN_PX * RB;
  static constexpr int W1 = T + T_BLK * 32 * RB;
  static constexpr int W2 = W1 + 9 * CH * RB;
  static constexpr int W3 = W2 + 9 * CH * RB;
  static constexpr int LDS = W3 + (K3 / 16) * N3 * RB;
  static_assert(TH * TW * RB <= T_BLK * 32 * RB && NW * 32 * N3 * 4 <= W3 - W1, "the early slice / y_new fit t; the staging fits W1 + W2");
  static_assert((size_t)LDS <= kSpTwoPerCu, "two blocks per CU");
};

struct C2fTailDev {
  const char* cat = nullptr;  // SP8 NHWC, rowb bytes per pixel
  long rowb = 0;
  int e_offb = 0, y_offb = 0;  // byte offsets inside a pixel of the first slice of cat and of y_last (slice n)
  int H = 0, W = 0, tiles_x = 0, tiles_per_img = 0;
  FastDiv d_tpi, d_tx;
  const char *W1 = nullptr, *W2 = nullptr, *W3 = nullptr;  // SP8 [ch][9 ch], [ch][9 ch], [2 ch][(2 + n) ch]
  const float *ws1 = nullptr, *b1 = nullptr, *ws2 = nullptr, *b2 = nullptr, *ws3 = nullptr, *b3 = nullptr;
  float* out = nullptr;
  long ldo = 0;
  int o_off = 0;
  int shortcut = 0;
  const char* zero = nullptr;  // >= 16 zero bytes
};

// Blocks go round the eight XCDs: each XCD gets a contiguous run of tiles, so the halo lines that rows of tiles share
// are read into one L2 (gemm_sp_kernel's tile order).
__device__ __forceinline__ int c2f_tile_of_block() { return xcd_block_order<int>(blockIdx.x, gridDim.x); }

// A lane's quad of activated outputs (columns 8 gq + 4 h + 0..3 of its pixel: the MFMA accumulator layout) split as the
// SP8_OUT epilogue splits it (sp8_split4), written as the lane's 8 bytes of the chunk's hi piece and of its lo piece.
__device__ __forceinline__ void c2f_put_quad(char* base, unsigned hi_at, unsigned lo_at, int h, const sp_f4 v) {
  sp_h4 hi, lo;
  sp8_split4(v, hi, lo);
  *reinterpret_cast<sp_h4*>(base + hi_at + h * 8) = hi;
  *reinterpret_cast<sp_h4*>(base + lo_at + h * 8) = lo;
}

__global__ __launch_bounds__(64 * C2fTail16::NW, 2) void c2f_tail_kernel(const C2fTailDev g) {
#pragma clang fp contract(off)
  using G = C2fTail16;
  constexpr int RB = G::RB;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  const int L = c2f_tile_of_block();
  const int img = (int)fdiv((uint32_t)L, g.d_tpi);
  const int trem = L - img * g.tiles_per_img;
  const int tyi = (int)fdiv((uint32_t)trem, g.d_tx);
  const int y0 = tyi * G::TH, x0 = (trem - tyi * g.tiles_x) * G::TW;
  const long px0 = (long)img * g.H * g.W;  // first pixel of the frame

  // byte offset of logical 16-byte slot `slot` of pixel (or weight row) p in a region of 64-byte rows
  auto at = [](int p, int slot) -> unsigned { return (unsigned)(p * RB + ((slot ^ ((p >> 2) & 3)) << 4)); };

  // ---- P0: everything the tile reads, by DMA; a piece is 16 rows x 64 bytes, lane -> (row lane / 4, slot lane % 4) ----
  {
    const int lp = lane >> 2, ls = lane & 3;
    auto dma = [&](const char* sp, int lds_off) {
      __builtin_amdgcn_global_load_lds((sp_gptr)sp, (sp_lptr)(smem + lds_off), 16, 0, 0);
    };
    for (int pc = wave; pc < G::WIN_PX / 16; pc += G::NW) {
      const int w = pc * 16 + lp;
      const int wy = w / G::WW, wx = w - wy * G::WW;
      const int fy = y0 - 2 + wy, fx = x0 - 2 + wx;
      const int slot = ls ^ ((w >> 2) & 3);
      const bool ok = (unsigned)fy < (unsigned)g.H && (unsigned)fx < (unsigned)g.W;
      dma(ok ? g.cat + (px0 + (long)fy * g.W + fx) * g.rowb + g.y_offb + slot * 16 : g.zero, G::WIN + pc * 1024);
    }
    for (int pc = wave; pc < G::TH * G::TW / 16; pc += G::NW) {  // the early slice, into t's place (free until P2)
      const int p = pc * 16 + lp;
      const int slot = ls ^ ((p >> 2) & 3);
      dma(g.cat + (px0 + (long)(y0 + (p >> 5)) * g.W + x0 + (p & 31)) * g.rowb + g.e_offb + slot * 16, G::T + pc * 1024);
    }
    const int wslot = ls ^ ((lp >> 2) & 3);  // weight rows: row & 15 == lp in every piece
    for (int pc = wave; pc < 9; pc += G::NW) {  // [tap][16 rows]
      dma(g.W1 + (long)lp * (9 * G::CH * 4) + pc * RB + wslot * 16, G::W1 + pc * 1024);
      dma(g.W2 + (long)lp * (9 * G::CH * 4) + pc * RB + wslot * 16, G::W2 + pc * 1024);
    }
    for (int pc = wave; pc < (G::K3 / 16) * (G::N3 / 16); pc += G::NW) {  // [k16 step][32 rows]
      const int step = pc / (G::N3 / 16), row = (pc % (G::N3 / 16)) * 16 + lp;
      dma(g.W3 + (long)row * (G::K3 * 4) + step * RB + wslot * 16, G::W3 + pc * 1024);
    }
  }
  // epilogue constants under the DMA: a lane owns columns 8 gq + 4 h + 0..3 of its pixel (the MFMA's accumulator layout)
  sp_f4 ws1[2], b1[2], ws2[2], b2[2], ws3[4], b3[4];
#pragma unroll
  for (int gq = 0; gq < 2; ++gq) {
    ws1[gq] = *reinterpret_cast<const sp_f4*>(g.ws1 + 8 * gq + 4 * h), b1[gq] = *reinterpret_cast<const sp_f4*>(g.b1 + 8 * gq + 4 * h);
    ws2[gq] = *reinterpret_cast<const sp_f4*>(g.ws2 + 8 * gq + 4 * h), b2[gq] = *reinterpret_cast<const sp_f4*>(g.b2 + 8 * gq + 4 * h);
  }
#pragma unroll
  for (int gq = 0; gq < 4; ++gq)
    ws3[gq] = *reinterpret_cast<const sp_f4*>(g.ws3 + 8 * gq + 4 * h), b3[gq] = *reinterpret_cast<const sp_f4*>(g.b3 + 8 * gq + 4 * h);

  constexpr int RW = G::TH / G::NW;  // tile rows (32-pixel row blocks) of a wave
  const int ty0 = wave * RW;
  const char* const win = smem + G::WIN;
  char* const tl = smem + G::T;

  // the hi (half 0) / lo (half 1) fragment of pixel p of a region (A operand) or of row p of a weight image (B operand).
  // Every k16 step below issues its three split products small cross terms first, like gemm_sp_kernel's main loop.
  auto frag = [&](const char* base, int p, int half) -> sp_h8 { return *reinterpret_cast<const sp_h8*>(base + at(p, h * 2 + half)); };

  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // ---- P1: the 1x1 over cat[0 : ch] (k 0..15) and y_last (k 16..31) ----
  spf16 acc3[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc3[i][q] = 0.f;
  {
    const char* const w3 = smem + G::W3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const sp_h8 bh = frag(w3 + s * (G::N3 * RB), r, 0), bl = frag(w3 + s * (G::N3 * RB), r, 1);
      sp_h8 ah[RW], al[RW];
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int p = s == 0 ? (ty0 + i) * G::TW + r : (ty0 + i + 2) * G::WW + r + 2;
        ah[i] = frag(s == 0 ? tl : win, p, 0), al[i] = frag(s == 0 ? tl : win, p, 1);
      }
#pragma unroll
      for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(bl, ah[i], acc3[i]);
#pragma unroll
      for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(bh, al[i], acc3[i]);
#pragma unroll
      for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(bh, ah[i], acc3[i]);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave has read the early slice: t may overwrite it

  auto put_quad = [&](char* base, unsigned hi_at, unsigned lo_at, const sp_f4 v) { c2f_put_quad(base, hi_at, lo_at, h, v); };

  // ---- P2: t = SiLU(W1 (*) y_last + b1) on the T_PX pixels around the tile; row block wave + NW i ----
  // (twin: P2 of c2f_tail32_kernel - same epilogue arithmetic, 64-byte pixels and two quads here; change both together)
  {
    constexpr int NB = (G::T_BLK + G::NW - 1) / G::NW;
    const char* const w1 = smem + G::W1;
    int q[NB], qy[NB], qx[NB], wb[NB];
    spf16 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      q[i] = (wave + G::NW * i) * 32 + r;  // (beyond T_PX: computed on the last pixel's window and dropped)
      const int qc = q[i] < G::T_PX ? q[i] : G::T_PX - 1;
      qy[i] = qc / G::UW, qx[i] = qc - qy[i] * G::UW;
      wb[i] = (qy[i] + 1) * G::WW + qx[i] + 1;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int shift = (tap / 3 - 1) * G::WW + (tap % 3 - 1);
      const sp_h8 bh = frag(w1 + tap * 1024, r & 15, 0), bl = frag(w1 + tap * 1024, r & 15, 1);
      sp_h8 ah[NB], al[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) ah[i] = frag(win, wb[i] + shift, 0), al[i] = frag(win, wb[i] + shift, 1);
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[i] = sp_mfma(bl, ah[i], acc[i]);
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[i] = sp_mfma(bh, al[i], acc[i]);
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[i] = sp_mfma(bh, ah[i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool inside = (unsigned)(y0 - 1 + qy[i]) < (unsigned)g.H && (unsigned)(x0 - 1 + qx[i]) < (unsigned)g.W;
      if (q[i] < G::T_PX) {
#pragma unroll
        for (int gq = 0; gq < 2; ++gq) {
          sp_f4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc[i][4 * gq + e], ws1[gq][e], b1[gq][e]));
          if (!inside) v = sp_f4{0.f, 0.f, 0.f, 0.f};
          put_quad(tl, at(q[i], 2 * gq), at(q[i], 2 * gq + 1), v);
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // t is complete

  // ---- P3: y_new = [y_last +] SiLU(W2 (*) t + b2) on the wave's tile rows ----
  {
    const char* const w2 = smem + G::W2;
    spf16 acc[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int shift = (tap / 3 - 1) * G::UW + (tap % 3 - 1);
      const sp_h8 bh = frag(w2 + tap * 1024, r & 15, 0), bl = frag(w2 + tap * 1024, r & 15, 1);
      sp_h8 ah[RW], al[RW];
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int tb = (ty0 + i + 1) * G::UW + r + 1;
        ah[i] = frag(tl, tb + shift, 0), al[i] = frag(tl, tb + shift, 1);
      }
#pragma unroll
      for (int i = 0; i < RW; ++i) acc[i] = sp_mfma(bl, ah[i], acc[i]);
#pragma unroll
      for (int i = 0; i < RW; ++i) acc[i] = sp_mfma(bh, al[i], acc[i]);
#pragma unroll
      for (int i = 0; i < RW; ++i) acc[i] = sp_mfma(bh, ah[i], acc[i]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave has read t: y_new goes over it, each wave's own pixels
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int p = (ty0 + i) * G::TW + r, wp = (ty0 + i + 2) * G::WW + r + 2;
#pragma unroll
      for (int gq = 0; gq < 2; ++gq) {
        sp_f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc[i][4 * gq + e], ws2[gq][e], b2[gq][e]));
        if (g.shortcut) {
          const sp_h4 rh = *reinterpret_cast<const sp_h4*>(win + at(wp, 2 * gq) + h * 8);
          const sp_h4 rl = *reinterpret_cast<const sp_h4*>(win + at(wp, 2 * gq + 1) + h * 8);
          v = v + (__builtin_convertvector(rh, sp_f4) + __builtin_convertvector(rl, sp_f4));
        }
        put_quad(tl, at(p, 2 * gq), at(p, 2 * gq + 1), v);
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (a wave reads back only the pixels it wrote)

  // ---- P4: the 1x1 over y_new (k 32..47), the zero step that fills the dense kernel's 32-k stage, epilogue ----
  {
    const char* const w3 = smem + G::W3 + 2 * (G::N3 * RB);
    const sp_h8 bh = frag(w3, r, 0), bl = frag(w3, r, 1);
    const sp_h8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    sp_h8 ah[RW], al[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) ah[i] = frag(tl, (ty0 + i) * G::TW + r, 0), al[i] = frag(tl, (ty0 + i) * G::TW + r, 1);
#pragma unroll
    for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(bl, ah[i], acc3[i]);
#pragma unroll
    for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(bh, al[i], acc3[i]);
#pragma unroll
    for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(bh, ah[i], acc3[i]);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(z8, z8, acc3[i]);
  }
  // (twin: the store sequence of c2f_tail32_kernel; change both together)
  // a row block's SP8 rows (32 pixels x 128 bytes, slots swizzled by the pixel) go through the wave's staging slab -
  // W1 / W2 are dead since the barrier above - and leave 8 lanes per 128-byte row: whole lines
  char* const stg = smem + G::W1 + wave * (32 * G::N3 * 4);
#pragma unroll
  for (int i = 0; i < RW; ++i) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      sp_f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc3[i][4 * gq + e], ws3[gq][e], b3[gq][e]));
      put_quad(stg, (unsigned)(r * 128 + (((2 * gq) ^ (r & 7)) << 4)), (unsigned)(r * 128 + (((2 * gq + 1) ^ (r & 7)) << 4)), v);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int sl = lane & 7, lrow = lane >> 3;
    float* const orow = g.out + (px0 + (long)(y0 + ty0 + i) * g.W + x0) * g.ldo + g.o_off + sl * 4;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + lrow;
      *reinterpret_cast<sp_f4*>(orow + (long)row * g.ldo) = *reinterpret_cast<const sp_f4*>(stg + row * 128 + ((sl ^ (row & 7)) << 4));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read back before the next row block is staged
  }
}

// ---- ch = 32: the 80 x 80 blocks (C2f-4: two bottlenecks, shortcut, K3 = 128; C2f-15: one, no shortcut, K3 = 96) ----
//
// Pixels are 128 bytes per 32-channel slice (slot' = slot ^ ((pixel >> 1) & 7), the swizzle of a 128-byte stage row), the
// tile is 8 x 16 output pixels - one 32-pixel row block (two tile rows) per wave - and the weights no longer fit beside
// the window and t: they stream through a ring of two 12 KB buffers in chunks, one s_barrier per chunk, in the order the
// phases consume them:
//   the 1x1's 32-k stages over the slices that exist (8 KB each: 64 rows x 128 B), W1 in three groups of three taps
//   (3 x 32 rows x 128 B), W2 likewise, the 1x1's last stage.
// The slices in front of y_last need no LDS: a lane's fragments of its own pixel (16 bytes each) go straight from HBM to
// the registers the MFMAs read.  The store staging is the wave's own 4 KB of y_new, once per 32 output columns.
struct C2fTail32 {
  static constexpr int CH = 32, RB = 128;
  static constexpr int TH = 8, TW = 16;
  static constexpr int WH = TH + 4, WW = TW + 4;
  static constexpr int UH = TH + 2, UW = TW + 2;
  static constexpr int WIN_PX = WH * WW, T_PX = UH * UW, T_BLK = (T_PX + 31) / 32;
  static constexpr int NW = 4;
  static constexpr int N3 = 2 * CH;
  static constexpr int CHUNK = 3 * CH * RB;  // three taps of a 3x3; a stage of the 1x1 (N3 x RB) is smaller
  static_assert(WIN_PX * RB % kSpPiece == 0 && TH * TW == NW * 32 && N3 * RB <= CHUNK, "whole DMA pieces, one row block per wave");
  static constexpr int WIN = 0;
  static constexpr int T = WIN + WIN_PX * RB;   // t, then y_new (and the store staging) over it
  static constexpr int RING = T + T_BLK * 32 * RB;
  static constexpr int LDS = RING + 2 * CHUNK;
  static_assert((size_t)LDS <= kSpTwoPerCu, "two blocks per CU");
};

// NB: bottlenecks of the block = slices of cat in front of y_last
template <int NB>
__global__ __launch_bounds__(64 * C2fTail32::NW, 2) void c2f_tail32_kernel(const C2fTailDev g) {
#pragma clang fp contract(off)
  using G = C2fTail32;
  constexpr int RB = G::RB, K3 = (2 + NB) * G::CH;
  constexpr int NC = NB + 8;  // weight chunks: NB + 1 stages of the 1x1, 3 + 3 tap groups, the 1x1's last stage
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  const int L = c2f_tile_of_block();
  const int img = (int)fdiv((uint32_t)L, g.d_tpi);
  const int trem = L - img * g.tiles_per_img;
  const int tyi = (int)fdiv((uint32_t)trem, g.d_tx);
  const int y0 = tyi * G::TH, x0 = (trem - tyi * g.tiles_x) * G::TW;
  const long px0 = (long)img * g.H * g.W;

  auto at = [](int p, int slot) -> unsigned { return (unsigned)(p * RB + ((slot ^ ((p >> 1) & 7)) << 4)); };
  // fragment of k16 step ks of pixel / weight row p: hi (half 0) or lo (half 1)
  auto frag = [&](const char* base, int p, int ks, int half) -> sp_h8 {
    return *reinterpret_cast<const sp_h8*>(base + at(p, ks * 4 + h * 2 + half));
  };

  const int lp = lane >> 3, ls = lane & 7;  // a DMA piece is 8 rows x 128 bytes
  auto dma = [&](const char* sp, int lds_off) {
    __builtin_amdgcn_global_load_lds((sp_gptr)sp, (sp_lptr)(smem + lds_off), 16, 0, 0);
  };
  // weight chunk c into ring buffer c & 1; every wave issues the same number of pieces
  auto load_chunk = [&](int c) {
    const int dst = G::RING + (c & 1) * G::CHUNK;
    if (c <= NB || c == NC - 1) {  // stage s of the 1x1: [64 rows][128 B]
      const int s = c <= NB ? c : NB + 1;
      for (int pc = wave; pc < G::N3 / 8; pc += G::NW) {
        const int row = pc * 8 + lp;
        dma(g.W3 + (long)row * (K3 * 4) + s * RB + ((ls ^ ((row >> 1) & 7)) << 4), dst + pc * 1024);
      }
    } else {  // taps 3 gi .. 3 gi + 2 of W1 / W2: [tap][32 rows][128 B]
      const int gi = c - (NB + 1);
      const char* const wsrc = gi < 3 ? g.W1 : g.W2;
      const int tap0 = (gi < 3 ? gi : gi - 3) * 3;
      for (int pc = wave; pc < 3 * G::CH / 8; pc += G::NW) {
        const int row = (pc & 3) * 8 + lp;
        dma(wsrc + (long)row * (9 * G::CH * 4) + (tap0 + (pc >> 2)) * RB + ((ls ^ ((row >> 1) & 7)) << 4), dst + pc * 1024);
      }
    }
  };
  // chunk c has landed for every wave and chunk c - 1 has been read by every wave: its buffer takes chunk c + 1
  auto advance = [&](int c) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (c + 1 < NC) load_chunk(c + 1);
  };

  // ---- P0: the window and the first weight chunk by DMA, the early slices' fragments into registers ----
  for (int pc = wave; pc < G::WIN_PX / 8; pc += G::NW) {
    const int w = pc * 8 + lp;
    const int wy = w / G::WW, wx = w - wy * G::WW;
    const int fy = y0 - 2 + wy, fx = x0 - 2 + wx;
    const bool ok = (unsigned)fy < (unsigned)g.H && (unsigned)fx < (unsigned)g.W;
    dma(ok ? g.cat + (px0 + (long)fy * g.W + fx) * g.rowb + g.y_offb + ((ls ^ ((w >> 1) & 7)) << 4) : g.zero, G::WIN + pc * 1024);
  }
  load_chunk(0);
  const int p = wave * 32 + r;  // the lane's output pixel of the tile
  const int ty = p >> 4, tx = p & 15;
  const long gpix = px0 + (long)(y0 + ty) * g.W + x0 + tx;
  sp_h8 ea[NB][2][2];
#pragma unroll
  for (int s = 0; s < NB; ++s)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int half = 0; half < 2; ++half)
        ea[s][ks][half] = *reinterpret_cast<const sp_h8*>(g.cat + gpix * g.rowb + g.e_offb + s * RB + (ks * 4 + h * 2 + half) * 16);
  // a layer's row scales and biases for the lane's columns (8 gq + 4 h + 0..3 of a 32-column block), fetched at the head
  // of the phase whose epilogue uses them: the MFMAs of the phase cover the latency, and no phase carries another's
  auto colvecs = [&](const float* ws, const float* b, sp_f4 (&wv)[4], sp_f4 (&bv)[4]) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
      wv[gq] = *reinterpret_cast<const sp_f4*>(ws + 8 * gq + 4 * h), bv[gq] = *reinterpret_cast<const sp_f4*>(b + 8 * gq + 4 * h);
  };
  const char* const win = smem + G::WIN;
  char* const tl = smem + G::T;
  auto ring = [&](int c) -> const char* { return smem + G::RING + (c & 1) * G::CHUNK; };

  auto put_quad = [&](char* base, unsigned hi_at, unsigned lo_at, const sp_f4 v) { c2f_put_quad(base, hi_at, lo_at, h, v); };

  // one 32-k stage of the 1x1 out of chunk c: both column blocks of the lane's pixel
  spf16 acc3[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc3[j][q] = 0.f;
  auto stage3 = [&](int c, const sp_h8 (&a)[2][2]) {
    const char* const wb = ring(c);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      sp_h8 bh[2], bl[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bh[j] = frag(wb, j * 32 + r, ks, 0), bl[j] = frag(wb, j * 32 + r, ks, 1);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc3[j] = sp_mfma(bl[j], a[ks][0], acc3[j]);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc3[j] = sp_mfma(bh[j], a[ks][1], acc3[j]);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc3[j] = sp_mfma(bh[j], a[ks][0], acc3[j]);
    }
  };

  // ---- P1: the 1x1 over the slices in front of y_last and over y_last (out of the window), k ascending ----
#pragma unroll
  for (int s = 0; s <= NB; ++s) {
    advance(s);
    if (s < NB) {
      stage3(s, ea[s]);
    } else {
      const int wp = (ty + 2) * G::WW + tx + 2;
      const sp_h8 a[2][2] = {{frag(win, wp, 0, 0), frag(win, wp, 0, 1)}, {frag(win, wp, 1, 0), frag(win, wp, 1, 1)}};
      stage3(s, a);
    }
  }

  // a 3x3 over NBLK row blocks of a wave: chunks c0 .. c0 + 2, fragments of pixel base[i] + tap shift out of `src`
  auto conv3 = [&](auto& acc, const int* base, const char* src, int pitch, int c0) {
    constexpr int NBLK = sizeof(acc) / sizeof(acc[0]);
#pragma unroll
    for (int gi = 0; gi < 3; ++gi) {
      advance(c0 + gi);
      const char* const wb = ring(c0 + gi);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int shift = (gi - 1) * pitch + (t - 1);  // tap 3 gi + t: (dy, dx) = (gi - 1, t - 1)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const sp_h8 bh = frag(wb + t * (G::CH * RB), r, ks, 0), bl = frag(wb + t * (G::CH * RB), r, ks, 1);
          sp_h8 ah[NBLK], al[NBLK];
#pragma unroll
          for (int i = 0; i < NBLK; ++i) ah[i] = frag(src, base[i] + shift, ks, 0), al[i] = frag(src, base[i] + shift, ks, 1);
#pragma unroll
          for (int i = 0; i < NBLK; ++i) acc[i] = sp_mfma(bl, ah[i], acc[i]);
#pragma unroll
          for (int i = 0; i < NBLK; ++i) acc[i] = sp_mfma(bh, al[i], acc[i]);
#pragma unroll
          for (int i = 0; i < NBLK; ++i) acc[i] = sp_mfma(bh, ah[i], acc[i]);
        }
      }
    }
  };

  // ---- P2: t on the T_PX pixels around the tile (row blocks wave, wave + NW), zero outside the frame ----
  // (twin: P2 of c2f_tail_kernel - same epilogue arithmetic, 128-byte pixels and four quads here; change both together)
  {
    constexpr int NBLK = (G::T_BLK + G::NW - 1) / G::NW;
    int q[NBLK], qy[NBLK], qx[NBLK], wb[NBLK];
    spf16 acc[NBLK];
    sp_f4 ws1[4], b1[4];
    colvecs(g.ws1, g.b1, ws1, b1);
#pragma unroll
    for (int i = 0; i < NBLK; ++i) {
      q[i] = (wave + G::NW * i) * 32 + r;  // (beyond T_PX: computed on the last pixel's window and dropped)
      const int qc = q[i] < G::T_PX ? q[i] : G::T_PX - 1;
      qy[i] = qc / G::UW, qx[i] = qc - qy[i] * G::UW;
      wb[i] = (qy[i] + 1) * G::WW + qx[i] + 1;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    }
    conv3(acc, wb, win, G::WW, NB + 1);
#pragma unroll
    for (int i = 0; i < NBLK; ++i) {
      const bool inside = (unsigned)(y0 - 1 + qy[i]) < (unsigned)g.H && (unsigned)(x0 - 1 + qx[i]) < (unsigned)g.W;
      if (q[i] < G::T_PX) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          sp_f4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc[i][4 * gq + e], ws1[gq][e], b1[gq][e]));
          if (!inside) v = sp_f4{0.f, 0.f, 0.f, 0.f};
          put_quad(tl, at(q[i], 2 * gq), at(q[i], 2 * gq + 1), v);
        }
      }
    }
  }

  // ---- P3: y_new on the wave's row block (the first barrier of conv3 says t is complete) ----
  {
    spf16 acc[1];
    sp_f4 ws2[4], b2[4];
    colvecs(g.ws2, g.b2, ws2, b2);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][e] = 0.f;
    const int tb[1] = {(ty + 1) * G::UW + tx + 1};
    conv3(acc, tb, tl, G::UW, NB + 4);
    advance(NC - 1);  // every wave has read t: y_new goes over it, each wave's own pixels; the 1x1's last stage has landed
    const int wp = (ty + 2) * G::WW + tx + 2;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      sp_f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc[0][4 * gq + e], ws2[gq][e], b2[gq][e]));
      if (g.shortcut) {
        const sp_h4 rh = *reinterpret_cast<const sp_h4*>(win + at(wp, 2 * gq) + h * 8);
        const sp_h4 rl = *reinterpret_cast<const sp_h4*>(win + at(wp, 2 * gq + 1) + h * 8);
        v = v + (__builtin_convertvector(rh, sp_f4) + __builtin_convertvector(rl, sp_f4));
      }
      put_quad(tl, at(p, 2 * gq), at(p, 2 * gq + 1), v);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (a wave reads back only the pixels it wrote)

  // ---- P4: the 1x1 over y_new, epilogue ----
  sp_f4 ws3[2][4], b3[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) colvecs(g.ws3 + 32 * j, g.b3 + 32 * j, ws3[j], b3[j]);
  {
    const sp_h8 a[2][2] = {{frag(tl, p, 0, 0), frag(tl, p, 0, 1)}, {frag(tl, p, 1, 0), frag(tl, p, 1, 1)}};
    stage3(NC - 1, a);
  }
  // (twin: the store sequence of c2f_tail_kernel; change both together)
  // 32 columns at a time through the wave's own 4 KB of y_new (read above), 8 lanes per 128-byte row segment
  char* const stg = tl + wave * (32 * RB);
  const int sl = lane & 7, lrow = lane >> 3;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      sp_f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc3[j][4 * gq + e], ws3[j][gq][e], b3[j][gq][e]));
      put_quad(stg, (unsigned)(r * 128 + (((2 * gq) ^ (r & 7)) << 4)), (unsigned)(r * 128 + (((2 * gq + 1) ^ (r & 7)) << 4)), v);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + lrow, po = wave * 32 + row;
      const long m = px0 + (long)(y0 + (po >> 4)) * g.W + x0 + (po & 15);
      *reinterpret_cast<sp_f4*>(g.out + m * g.ldo + g.o_off + j * 32 + sl * 4) =
          *reinterpret_cast<const sp_f4*>(stg + row * 128 + ((sl ^ (row & 7)) << 4));
    }
  }
}

}  // namespace mtgv
