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
// A block of four waves owns a TH x TW tile of output pixels of one frame, as row blocks of 32 pixels (the MFMA's rows):
//   P0  LDS-DMA, pieces as they lie in HBM: the (TH + 4) x (TW + 4) window of y_last (pixels outside the frame come from
//       the zero page) and the first weights
//   P1  the 1x1's k16 steps over the slices that exist already (cat[0 : n ch], then y_last out of the window) - k
//       ascending, so these come first; the accumulators stay in registers until y_new exists
//   P2  t on the (TH + 2) x (TW + 2) pixels the second conv reads, split to SP8 into LDS; pixels of t outside the frame
//       are ZERO (the second conv pads t with zeros - it does not see the conv of a zero-padded input)
//   P3  y_new on the tile, (+ y_last out of the window,) split to SP8 into LDS over t
//   P4  the 1x1's last step(s) over y_new, epilogue, SP8 rows staged through LDS and stored as whole lines
// The phases' arithmetic exists once, as the functions over the geometry below.  The two instances differ in where the
// operands wait:
//                   c2f_tail_kernel (ch = 16, 8 x 32 tile)                c2f_tail32_kernel<n> (ch = 32, 8 x 16 tile)
//   weights         all three matrices resident in LDS from P0 on         stream through a ring of two 12 KB buffers in the
//                                                                         order the phases consume them, one s_barrier a chunk
//   early slice(s)  cat[0 : ch] by DMA into t's place (free until P2)     a lane's fragments of its own pixel straight from HBM
//                                                                         to the registers the MFMAs read
//   row blocks      two tile rows per wave                                one (two tile rows of 16 pixels) per wave
//   store staging   a 4 KB slab per wave over W1 / W2 (dead after P3)     the wave's own 4 KB of y_new, once per 32 columns
//
// Bit-identical to the three gemm_sp_kernel launches it replaces (gemm_sp_kernel.h): the same v_mfma_f32_32x32x16_f16
// with the 16 output channels of the ch = 16 3x3 convs padded to 32 columns (SP_CFG_WIN16), K walked tap by tap over
// 16-channel slices (SP_A_WINDOW), the 1x1 in ascending k16 steps including the zero step that pads K = 48 to the dense
// kernel's 32-k stage, lo*hi + hi*lo + hi*hi per step, and the same scale * acc + bias -> SiLU -> (+ residual) -> split
// epilogue.  The window holds real zeros where the original predicates a tap's fragment to zero: the same operand values.
#pragma once
#include "act.h"
#include "gemm_sp_kernel.h"
#include "sp8.h"

namespace mtgv {

// Geometry of an instance and the part of its LDS map both share: [window][t, then y_new over it][the weights].  LDS rows
// are pixels (or weight rows) of RB bytes - one ch-channel SP8 slice - with their 16-byte slots swizzled by the row index
// like the rows of a gemm_sp_kernel stage: over the rows that share a 256-byte bank row.
template <int CH_, int TW_>
struct C2fTailGeom {
  static constexpr int CH = CH_, RB = 4 * CH;          // channels per slice, bytes per pixel of a slice
  static constexpr int TH = 8, TW = TW_;               // output tile
  static constexpr int WH = TH + 4, WW = TW + 4;       // window of y_last
  static constexpr int UH = TH + 2, UW = TW + 2;       // pixels of t
  static constexpr int WIN_PX = WH * WW, T_PX = UH * UW, T_BLK = (T_PX + 31) / 32;
  static constexpr int NW = 4;                         // waves
  static constexpr int RW = TH * TW / 32 / NW;         // row blocks of the tile per wave: wave * RW + i
  static constexpr int TB = (T_BLK + NW - 1) / NW;     // row blocks of t per wave: wave + NW i
  static constexpr int N3 = 2 * CH;                    // output channels of the 1x1
  static constexpr int NQ = CH / 8;                    // quads a lane holds of a 3x3 output pixel
  static constexpr int KS = RB / 64;                   // k16 steps per slice
  static constexpr int SPR = RB / 16, PR = kSpPiece / RB;  // slots per row; rows per 1 KB DMA piece: lane -> (row lane / SPR, slot lane % SPR)
  static constexpr int WIN = 0;
  static constexpr int T = WIN + WIN_PX * RB;
  static constexpr int T_END = T + T_BLK * 32 * RB;
  static_assert(WIN_PX * RB % kSpPiece == 0 && TH * TW == NW * RW * 32 && 32 % TW == 0, "whole DMA pieces, whole row blocks per wave");
  static_assert(TH * TW <= T_BLK * 32, "the early slice / y_new fit t");

  static __host__ __device__ constexpr int swz(int p, int slot) { return slot ^ ((p >> (RB == 64 ? 2 : 1)) & (SPR - 1)); }
  // byte offset of logical 16-byte slot `slot` of pixel (or weight row) p in a region of RB-byte rows
  static __host__ __device__ constexpr unsigned at(int p, int slot) { return (unsigned)(p * RB + (swz(p, slot) << 4)); }
  // the hi (half 0) / lo (half 1) fragment of k16 step ks of pixel p of a region (A operand) or of row p of a weight
  // image (B operand), for the lanes of half h
  static __device__ __forceinline__ sp_h8 frag(const char* base, int p, int ks, int h, int half) {
    return *reinterpret_cast<const sp_h8*>(base + at(p, ks * 4 + h * 2 + half));
  }
  // pixel p = y * TW + x of the tile: its y and x, and p as a pixel of t and of the window
  static __host__ __device__ constexpr int ty(int p) { return (int)((unsigned)p / TW); }
  static __host__ __device__ constexpr int tx(int p) { return (int)((unsigned)p % TW); }
  static __host__ __device__ constexpr int t_of(int p) { return (ty(p) + 1) * UW + tx(p) + 1; }
  static __host__ __device__ constexpr int win_of(int p) { return (ty(p) + 2) * WW + tx(p) + 2; }
};

// ch = 16: [window][t, first the early slice then y_new over it][W1][W2, the store staging over both][W3]
struct C2fTail16 : C2fTailGeom<16, 32> {
  static constexpr int K3 = 3 * CH;  // the 1x1: [cat0 | y_last | y_new] -> 2 ch
  static constexpr int W1 = T_END;
  static constexpr int W2 = W1 + 9 * CH * RB;
  static constexpr int W3 = W2 + 9 * CH * RB;
  static constexpr int LDS = W3 + (K3 / 16) * N3 * RB;
  static_assert(NW * 32 * N3 * 4 <= W3 - W1, "the staging fits W1 + W2");
  static_assert((size_t)LDS <= kSpTwoPerCu, "two blocks per CU");
};

// ch = 32, the 80 x 80 blocks (C2f-4: two bottlenecks, shortcut, K3 = 128; C2f-15: one, no shortcut, K3 = 96):
// [window][t, then y_new (and the store staging) over it][ring of two weight chunks]
struct C2fTail32 : C2fTailGeom<32, 16> {
  static constexpr int CHUNK = 3 * CH * RB;  // three taps of a 3x3; a stage of the 1x1 (N3 x RB) is smaller
  static constexpr int RING = T_END;
  static constexpr int LDS = RING + 2 * CHUNK;
  static_assert(N3 * RB <= CHUNK && RW == 1, "a stage of the 1x1 fits a chunk; one row block per wave");
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

struct C2fTile {
  int y0, x0;  // the tile's first pixel in its frame
  long px0;    // the frame's first pixel
};

// Blocks go round the eight XCDs: each XCD gets a contiguous run of tiles, so the halo lines that rows of tiles share
// are read into one L2 (gemm_sp_kernel's tile order).
template <class G>
__device__ __forceinline__ C2fTile c2f_tile(const C2fTailDev& g) {
  const int L = xcd_block_order<int>(blockIdx.x, gridDim.x);
  const int img = (int)fdiv((uint32_t)L, g.d_tpi);
  const int trem = L - img * g.tiles_per_img;
  const int tyi = (int)fdiv((uint32_t)trem, g.d_tx);
  return {tyi * G::TH, (trem - tyi * g.tiles_x) * G::TW, (long)img * g.H * g.W};
}

// one 1 KB piece: 16 bytes per lane to consecutive LDS
__device__ __forceinline__ void c2f_dma(const char* sp, char* lds) {
  __builtin_amdgcn_global_load_lds((sp_gptr)sp, (sp_lptr)lds, 16, 0, 0);
}

// P0: the window of y_last; pixels outside the frame come from the zero page
template <class G>
__device__ __forceinline__ void c2f_dma_window(const C2fTailDev& g, const C2fTile& t, char* smem, int wave, int lane) {
  const int lp = lane / G::SPR, ls = lane % G::SPR;
  for (int pc = wave; pc < G::WIN_PX / G::PR; pc += G::NW) {
    const int w = pc * G::PR + lp;
    const int wy = w / G::WW, wx = w - wy * G::WW;
    const int fy = t.y0 - 2 + wy, fx = t.x0 - 2 + wx;
    const bool ok = (unsigned)fy < (unsigned)g.H && (unsigned)fx < (unsigned)g.W;
    c2f_dma(ok ? g.cat + (t.px0 + (long)fy * g.W + fx) * g.rowb + g.y_offb + (G::swz(w, ls) << 4) : g.zero, smem + G::WIN + pc * 1024);
  }
}

// a layer's row scales and biases for the lane's columns: 8 gq + 4 h + 0..3 of its pixel, the MFMA's accumulator layout
template <int NQ>
__device__ __forceinline__ void c2f_colvecs(const float* ws, const float* b, int h, sp_f4 (&wv)[NQ], sp_f4 (&bv)[NQ]) {
#pragma unroll
  for (int gq = 0; gq < NQ; ++gq)
    wv[gq] = *reinterpret_cast<const sp_f4*>(ws + 8 * gq + 4 * h), bv[gq] = *reinterpret_cast<const sp_f4*>(b + 8 * gq + 4 * h);
}

template <int N>
__device__ __forceinline__ void c2f_zero(spf16 (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
}

// A k16 step over N row blocks: the three split products, small cross terms first, like gemm_sp_kernel's main loop.
template <int N>
__device__ __forceinline__ void c2f_step(spf16 (&acc)[N], const sp_h8 bh, const sp_h8 bl, const sp_h8 (&ah)[N], const sp_h8 (&al)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = sp_mfma(bl, ah[i], acc[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = sp_mfma(bh, al[i], acc[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = sp_mfma(bh, ah[i], acc[i]);
}

// A 3x3 over N row blocks of a wave: tap by tap, fragments of pixel base[i] + tap shift out of `src` (rows of `pitch`
// pixels) against the tap's [CH rows][RB] weight image wtap(tap); 16 rows are read twice to fill the MFMA's 32 columns.
template <class G, int N, class WTap>
__device__ __forceinline__ void c2f_conv3(spf16 (&acc)[N], const int (&base)[N], const char* src, int pitch, int r, int h, WTap wtap) {
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const char* const wb = wtap(tap);
    const int shift = (tap / 3 - 1) * pitch + (tap % 3 - 1);
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) {
      const sp_h8 bh = G::frag(wb, r & (G::CH - 1), ks, h, 0), bl = G::frag(wb, r & (G::CH - 1), ks, h, 1);
      sp_h8 ah[N], al[N];
#pragma unroll
      for (int i = 0; i < N; ++i) ah[i] = G::frag(src, base[i] + shift, ks, h, 0), al[i] = G::frag(src, base[i] + shift, ks, h, 1);
      c2f_step<N>(acc, bh, bl, ah, al);
    }
  }
}

// A lane's quad of activated outputs (columns 8 gq + 4 h + 0..3 of its pixel: the MFMA accumulator layout) split as the
// SP8_OUT epilogue splits it (sp8_split4), written as the lane's 8 bytes of the chunk's hi piece and of its lo piece.
__device__ __forceinline__ void c2f_put_quad(char* base, unsigned hi_at, unsigned lo_at, int h, const sp_f4 v) {
  sp_h4 hi, lo;
  sp8_split4(v, hi, lo);
  *reinterpret_cast<sp_h4*>(base + hi_at + h * 8) = hi;
  *reinterpret_cast<sp_h4*>(base + lo_at + h * 8) = lo;
}

// The epilogue of a 3x3 on one pixel: SiLU(scale * acc + bias), ZERO where `zero`, + pixel p of the tile out of the
// window where `shortcut`; split to SP8 into pixel `dst` of t's region.
template <class G>
__device__ __forceinline__ void c2f_epilogue(const spf16& acc, const sp_f4 (&ws)[G::NQ], const sp_f4 (&b)[G::NQ], char* smem, int dst, int h,
                                             bool zero, bool shortcut, int p) {
#pragma clang fp contract(off)
  const char* const win = smem + G::WIN;
#pragma unroll
  for (int gq = 0; gq < G::NQ; ++gq) {
    sp_f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc[4 * gq + e], ws[gq][e], b[gq][e]));
    if (zero) v = sp_f4{0.f, 0.f, 0.f, 0.f};
    if (shortcut) {
      const sp_h4 rh = *reinterpret_cast<const sp_h4*>(win + G::at(G::win_of(p), 2 * gq) + h * 8);
      const sp_h4 rl = *reinterpret_cast<const sp_h4*>(win + G::at(G::win_of(p), 2 * gq + 1) + h * 8);
      v = v + (__builtin_convertvector(rh, sp_f4) + __builtin_convertvector(rl, sp_f4));
    }
    c2f_put_quad(smem + G::T, G::at(dst, 2 * gq), G::at(dst, 2 * gq + 1), h, v);
  }
}

// P2: t = SiLU(W1 (*) y_last + b1) on the T_PX pixels around the tile, row blocks wave + NW i; zero outside the frame
template <class G, class WTap>
__device__ __forceinline__ void c2f_make_t(const C2fTailDev& g, const C2fTile& t, char* smem, int wave, int r, int h, const sp_f4 (&ws)[G::NQ],
                                           const sp_f4 (&b)[G::NQ], WTap wtap) {
  constexpr int N = G::TB;
  int q[N], qy[N], qx[N], wb[N];
  spf16 acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    q[i] = (wave + G::NW * i) * 32 + r;  // (beyond T_PX: computed on the last pixel's window and dropped)
    const int qc = q[i] < G::T_PX ? q[i] : G::T_PX - 1;
    qy[i] = qc / G::UW, qx[i] = qc - qy[i] * G::UW;
    wb[i] = (qy[i] + 1) * G::WW + qx[i] + 1;
  }
  c2f_zero(acc);
  c2f_conv3<G>(acc, wb, smem + G::WIN, G::WW, r, h, wtap);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool inside = (unsigned)(t.y0 - 1 + qy[i]) < (unsigned)g.H && (unsigned)(t.x0 - 1 + qx[i]) < (unsigned)g.W;
    if (q[i] < G::T_PX) c2f_epilogue<G>(acc[i], ws, b, smem, q[i], h, !inside, false, 0);
  }
}

// P3: y_new = [y_last +] SiLU(W2 (*) t + b2) on the wave's row blocks.  all_read_t() returns when every wave has read t:
// y_new goes over it, each wave's own pixels.
template <class G, class WTap, class Sync>
__device__ __forceinline__ void c2f_make_y(const C2fTailDev& g, char* smem, int wave, int r, int h, const sp_f4 (&ws)[G::NQ],
                                           const sp_f4 (&b)[G::NQ], WTap wtap, Sync all_read_t) {
  constexpr int N = G::RW;
  int tb[N];
  spf16 acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) tb[i] = G::t_of((wave * N + i) * 32 + r);
  c2f_zero(acc);
  c2f_conv3<G>(acc, tb, smem + G::T, G::UW, r, h, wtap);
  all_read_t();
#pragma unroll
  for (int i = 0; i < N; ++i) c2f_epilogue<G>(acc[i], ws, b, smem, (wave * N + i) * 32 + r, h, false, g.shortcut != 0, (wave * N + i) * 32 + r);
}

// P4's store: 32 output columns from col0 on of row block blk of the tile.  The SP8 rows (32 pixels x 128 bytes, slots
// swizzled by the pixel) go through the wave's staging slab and leave 8 lanes per 128-byte row: whole lines.
template <class G>
__device__ __forceinline__ void c2f_store32(const C2fTailDev& g, const C2fTile& t, int blk, int col0, const spf16& acc, const sp_f4 (&ws)[4],
                                            const sp_f4 (&b)[4], char* stg, int lane) {
#pragma clang fp contract(off)
  const int r = lane & 31, h = lane >> 5, sl = lane & 7, lrow = lane >> 3;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // what the slab held has been read
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    sp_f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_silu(__builtin_fmaf(acc[4 * gq + e], ws[gq][e], b[gq][e]));
    c2f_put_quad(stg, (unsigned)(r * 128 + (((2 * gq) ^ (r & 7)) << 4)), (unsigned)(r * 128 + (((2 * gq + 1) ^ (r & 7)) << 4)), h, v);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // the row block starts a tile row (32 % TW == 0): its first pixel, then row by row from there
  float* const o0 = g.out + (t.px0 + (long)(t.y0 + G::ty(blk * 32)) * g.W + t.x0) * g.ldo + g.o_off + col0 + sl * 4;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + lrow;
    *reinterpret_cast<sp_f4*>(o0 + (long)(G::ty(row) * g.W + G::tx(row)) * g.ldo) = *reinterpret_cast<const sp_f4*>(stg + row * 128 + ((sl ^ (row & 7)) << 4));
  }
}

__global__ __launch_bounds__(64 * C2fTail16::NW, 2) void c2f_tail_kernel(const C2fTailDev g) {
#pragma clang fp contract(off)
  using G = C2fTail16;
  constexpr int RB = G::RB, RW = G::RW;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const C2fTile t = c2f_tile<G>(g);

  // ---- P0: everything the tile reads, by DMA ----
  c2f_dma_window<G>(g, t, smem, wave, lane);
  {
    const int lp = lane / G::SPR, ls = lane % G::SPR;
    for (int pc = wave; pc < G::TH * G::TW / G::PR; pc += G::NW) {  // the early slice, into t's place (free until P2)
      const int p = pc * G::PR + lp;
      c2f_dma(g.cat + (t.px0 + (long)(t.y0 + G::ty(p)) * g.W + t.x0 + G::tx(p)) * g.rowb + g.e_offb + (G::swz(p, ls) << 4), smem + G::T + pc * 1024);
    }
    const int wslot = G::swz(lp, ls);  // weight rows: row & 15 == lp in every piece
    for (int pc = wave; pc < 9; pc += G::NW) {  // [tap][16 rows]
      c2f_dma(g.W1 + (long)lp * (9 * G::CH * 4) + pc * RB + wslot * 16, smem + G::W1 + pc * 1024);
      c2f_dma(g.W2 + (long)lp * (9 * G::CH * 4) + pc * RB + wslot * 16, smem + G::W2 + pc * 1024);
    }
    for (int pc = wave; pc < (G::K3 / 16) * (G::N3 / 16); pc += G::NW) {  // [k16 step][32 rows]
      const int step = pc / (G::N3 / 16), row = (pc % (G::N3 / 16)) * 16 + lp;
      c2f_dma(g.W3 + (long)row * (G::K3 * 4) + step * RB + wslot * 16, smem + G::W3 + pc * 1024);
    }
  }
  // epilogue constants under the DMA
  sp_f4 ws1[2], b1[2], ws2[2], b2[2], ws3[4], b3[4];
  c2f_colvecs(g.ws1, g.b1, h, ws1, b1);
  c2f_colvecs(g.ws2, g.b2, h, ws2, b2);
  c2f_colvecs(g.ws3, g.b3, h, ws3, b3);

  const char* const win = smem + G::WIN;
  const char* const tl = smem + G::T;
  const char* const w3 = smem + G::W3;  // [k16 step][N3 rows]

  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // ---- P1: the 1x1 over cat[0 : ch] (k 0..15) and y_last (k 16..31) ----
  spf16 acc3[RW];
  c2f_zero(acc3);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const sp_h8 bh = G::frag(w3 + s * (G::N3 * RB), r, 0, h, 0), bl = G::frag(w3 + s * (G::N3 * RB), r, 0, h, 1);
    sp_h8 ah[RW], al[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int p = (wave * RW + i) * 32 + r;
      ah[i] = G::frag(s == 0 ? tl : win, s == 0 ? p : G::win_of(p), 0, h, 0), al[i] = G::frag(s == 0 ? tl : win, s == 0 ? p : G::win_of(p), 0, h, 1);
    }
    c2f_step<RW>(acc3, bh, bl, ah, al);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave has read the early slice: t may overwrite it

  c2f_make_t<G>(g, t, smem, wave, r, h, ws1, b1, [&](int tap) { return smem + G::W1 + tap * 1024; });
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // t is complete

  c2f_make_y<G>(g, smem, wave, r, h, ws2, b2, [&](int tap) { return smem + G::W2 + tap * 1024; }, [] {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  });
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (a wave reads back only the pixels it wrote)

  // ---- P4: the 1x1 over y_new (k 32..47), the zero step that fills the dense kernel's 32-k stage, epilogue ----
  {
    const sp_h8 bh = G::frag(w3 + 2 * (G::N3 * RB), r, 0, h, 0), bl = G::frag(w3 + 2 * (G::N3 * RB), r, 0, h, 1);
    const sp_h8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    sp_h8 ah[RW], al[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) ah[i] = G::frag(tl, (wave * RW + i) * 32 + r, 0, h, 0), al[i] = G::frag(tl, (wave * RW + i) * 32 + r, 0, h, 1);
    c2f_step<RW>(acc3, bh, bl, ah, al);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < RW; ++i) acc3[i] = sp_mfma(z8, z8, acc3[i]);
  }
  // the wave's staging slab: W1 / W2 are dead since the barrier of P3
#pragma unroll
  for (int i = 0; i < RW; ++i) c2f_store32<G>(g, t, wave * RW + i, 0, acc3[i], ws3, b3, smem + G::W1 + wave * (32 * G::N3 * 4), lane);
}

// NB: bottlenecks of the block = slices of cat in front of y_last.  The weight chunks, in the order the phases consume
// them: the 1x1's 32-k stages over the slices that exist (8 KB each: 64 rows x 128 B), W1 in three groups of three taps
// (3 x 32 rows x 128 B), W2 likewise, the 1x1's last stage.
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
  const C2fTile t = c2f_tile<G>(g);

  const int lp = lane / G::SPR, ls = lane % G::SPR;
  // weight chunk c into ring buffer c & 1; every wave issues the same number of pieces
  auto load_chunk = [&](int c) {
    char* const dst = smem + G::RING + (c & 1) * G::CHUNK;
    if (c <= NB || c == NC - 1) {  // stage s of the 1x1: [64 rows][128 B]
      const int s = c <= NB ? c : NB + 1;
      for (int pc = wave; pc < G::N3 / G::PR; pc += G::NW) {
        const int row = pc * G::PR + lp;
        c2f_dma(g.W3 + (long)row * (K3 * 4) + s * RB + (G::swz(row, ls) << 4), dst + pc * 1024);
      }
    } else {  // taps 3 gi .. 3 gi + 2 of W1 / W2: [tap][32 rows][128 B]
      const int gi = c - (NB + 1);
      const char* const wsrc = gi < 3 ? g.W1 : g.W2;
      const int tap0 = (gi < 3 ? gi : gi - 3) * 3;
      for (int pc = wave; pc < 3 * G::CH / G::PR; pc += G::NW) {
        const int row = (pc & 3) * G::PR + lp;
        c2f_dma(wsrc + (long)row * (9 * G::CH * 4) + (tap0 + (pc >> 2)) * RB + (G::swz(row, ls) << 4), dst + pc * 1024);
      }
    }
  };
  // chunk c has landed for every wave and chunk c - 1 has been read by every wave: its buffer takes chunk c + 1
  auto advance = [&](int c) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (c + 1 < NC) load_chunk(c + 1);
  };
  auto ring = [&](int c) -> const char* { return smem + G::RING + (c & 1) * G::CHUNK; };
  // tap 0..8 of the 3x3 whose chunks are c0 .. c0 + 2
  auto ring_taps = [&](int c0) {
    return [&advance, &ring, c0](int tap) {
      if (tap % 3 == 0) advance(c0 + tap / 3);
      return ring(c0 + tap / 3) + (tap % 3) * (G::CH * RB);
    };
  };

  // ---- P0: the window and the first weight chunk by DMA, the early slices' fragments into registers ----
  c2f_dma_window<G>(g, t, smem, wave, lane);
  load_chunk(0);
  const int p = wave * 32 + r;  // the lane's output pixel of the tile
  const long gpix = t.px0 + (long)(t.y0 + G::ty(p)) * g.W + t.x0 + G::tx(p);
  sp_h8 ea[NB][2][2];
#pragma unroll
  for (int s = 0; s < NB; ++s)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int half = 0; half < 2; ++half)
        ea[s][ks][half] = *reinterpret_cast<const sp_h8*>(g.cat + gpix * g.rowb + g.e_offb + s * RB + (ks * 4 + h * 2 + half) * 16);
  const char* const win = smem + G::WIN;
  const char* const tl = smem + G::T;

  // one 32-k stage of the 1x1 out of chunk c: both column blocks of the lane's pixel
  spf16 acc3[2];
  c2f_zero(acc3);
  auto stage3 = [&](int c, const sp_h8 (&a)[2][2]) {
    const char* const wb = ring(c);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      sp_h8 bh[2], bl[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bh[j] = G::frag(wb, j * 32 + r, ks, h, 0), bl[j] = G::frag(wb, j * 32 + r, ks, h, 1);
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
      const int wp = G::win_of(p);
      const sp_h8 a[2][2] = {{G::frag(win, wp, 0, h, 0), G::frag(win, wp, 0, h, 1)}, {G::frag(win, wp, 1, h, 0), G::frag(win, wp, 1, h, 1)}};
      stage3(s, a);
    }
  }

  // ---- P2, P3: a layer's scales and biases are fetched at the head of the phase whose epilogue uses them: the MFMAs of
  // the phase cover the latency, and no phase carries another's.  The first barrier of P3's conv says t is complete. ----
  {
    sp_f4 ws1[4], b1[4];
    c2f_colvecs(g.ws1, g.b1, h, ws1, b1);
    c2f_make_t<G>(g, t, smem, wave, r, h, ws1, b1, ring_taps(NB + 1));
  }
  {
    sp_f4 ws2[4], b2[4];
    c2f_colvecs(g.ws2, g.b2, h, ws2, b2);
    c2f_make_y<G>(g, smem, wave, r, h, ws2, b2, ring_taps(NB + 4), [&] { advance(NC - 1); });  // (the 1x1's last stage has landed too)
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (a wave reads back only the pixels it wrote)

  // ---- P4: the 1x1 over y_new, epilogue; 32 columns at a time through the wave's own 4 KB of y_new (read here) ----
  sp_f4 ws3[2][4], b3[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) c2f_colvecs(g.ws3 + 32 * j, g.b3 + 32 * j, h, ws3[j], b3[j]);
  {
    const sp_h8 a[2][2] = {{G::frag(tl, p, 0, h, 0), G::frag(tl, p, 0, h, 1)}, {G::frag(tl, p, 1, h, 0), G::frag(tl, p, 1, h, 1)}};
    stage3(NC - 1, a);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) c2f_store32<G>(g, t, wave, 32 * j, acc3[j], ws3[j], b3[j], smem + G::T + wave * (32 * RB), lane);
}

}  // namespace mtgv
