// The LDS-DMA split GEMM's compile-time facts, each written once: the tile table, the names of the configurations the
// planner singles out, the A modes and epilogue shapes, and the LDS layout of a launch.  Shared by the kernel
// (gemm_sp_kernel.h), the per-tile instance ladders (gemm_sp_inst.h) and the planner / launcher (gemm_sp.hip), so a
// launch covers the rows the kernel computes and asks for the bytes the kernel lays out.
#pragma once
#include <stddef.h>

namespace mtgv {

// ---- tiles ----
// Block of wm x wn waves, wave tile (32 tm) rows x (32 tn) columns, K in stages of ks k16 steps.
struct SpTile {
  int wm, wn, tm, tn, ks;
  constexpr int bm() const { return 32 * tm * wm; }
  constexpr int bn() const { return 32 * tn * wn; }
  constexpr int rb() const { return 64 * ks; }      // bytes per staged row
  constexpr int kps() const { return 16 * ks; }     // k per stage
  constexpr int waves() const { return wm * wn; }
  constexpr int wave_rows() const { return 32 * tm; }  // rows of one wave: a GRN partial unit
  constexpr int wave_cols() const { return 32 * tn; }  // columns of one wave: a top-k candidate group
};

// One translation unit each (gemm_sp_c<id>.hip).  The planner's efficiencies sit beside this table in gemm_sp.hip.
constexpr SpTile kSpTile[] = {
    {2, 2, 2, 2, 2},  // 128 x 128
    {2, 2, 2, 3, 2},  // 128 x 192
    {4, 1, 1, 3, 2},  // 128 x  96
    {4, 1, 1, 2, 2},  // 128 x  64
    {4, 1, 1, 1, 2},  // 128 x  32
    {4, 2, 1, 3, 2},  // 128 x 192 on eight waves
    {4, 1, 1, 1, 1},  // 128 x  32 in 16-k stages
    {4, 1, 1, 5, 2},  // 128 x 160: the detector heads' stacked first 3x3 convs in one column tile (window conv only)
};
constexpr int kSpNumCfg = sizeof(kSpTile) / sizeof(kSpTile[0]);

// The configurations the planner names (everything else is found by the cost search):
enum SpCfgId : int {
  SP_CFG_TOPK = 1,    // the match path's tile: the only one with the fused top-k epilogue (and the fp16 first pass)
  SP_CFG_OS_NQ = 3,   // whole-ConvTranspose launches: one column group of 64 per tile
  SP_CFG_PW1_8W = 5,  // eight-wave twin of SP_CFG_TOPK's 128 x 192, swapped in for pwconv1-shaped launches
  SP_CFG_WIN16 = 6,   // window convs with 16-channel slices
  SP_CFG_N160 = 7,    // window convs with 160 output columns: no dead columns, one window fill (SiLU, SP8 out: its only instance)
};
static_assert(kSpTile[SP_CFG_PW1_8W].bm() == kSpTile[SP_CFG_TOPK].bm() && kSpTile[SP_CFG_PW1_8W].bn() == kSpTile[SP_CFG_TOPK].bn(),
              "the eight-wave twin covers the same block");
static_assert(kSpTile[SP_CFG_WIN16].ks == 1 && kSpTile[SP_CFG_OS_NQ].bn() == 64 && kSpTile[SP_CFG_N160].bn() == 160, "named configurations");

// Chained 1x1 (SP_EPI_CHAIN): one wave holds whole output rows, of at most 96 columns.  The instance ladder builds those
// kernels for exactly the tiles this admits, and the planner picks a chain tile through sp_chain_cfg, so it cannot name
// one without a kernel.
constexpr bool sp_tile_chains(const SpTile& t) { return t.wn == 1 && t.tm == 1 && t.ks == 2 && t.tn <= 3; }
// the chain tile whose one column tile is N wide, or -1
constexpr int sp_chain_cfg(int N) {
  for (int c = 0; c < kSpNumCfg; ++c)
    if (sp_tile_chains(kSpTile[c]) && kSpTile[c].bn() == N) return c;
  return -1;
}
constexpr int sp_chain_max_n() {
  int n = 0;
  for (int c = 0; c < kSpNumCfg; ++c)
    if (sp_tile_chains(kSpTile[c]) && kSpTile[c].bn() > n) n = kSpTile[c].bn();
  return n;
}

// ---- A modes and epilogue shapes (template arguments of gemm_sp_kernel; its header comment says what each one does) ----
enum SpAMode : int {
  SP_A_SP8 = 0,      // dense SP8 rows by DMA
  SP_A_REG = 1,      // f32 rows through registers
  SP_A_CONV = 2,     // SP8 NHWC gather
  SP_A_F32_MUL = 3,  // f32 rows by DMA with per-image multipliers
  SP_A_F32 = 4,      // f32 rows by DMA
  SP_A_WINDOW = 5,   // SP8 3x3 / stride-1 conv out of a staged input window
  SP_A_HI16 = 6,     // fp16 rows on both sides
};
enum SpEpi : int {
  SP_EPI_ARGS = -1,    // shape read from the arguments
  SP_EPI_F32 = 0,      // f32 out
  SP_EPI_SP8_OUT = 1,  // bits: SP8 out,
  SP_EPI_RES_F32 = 2,  //       + f32 residual (pwconv2),
  SP_EPI_RES_SP8 = 4,  //       + SP8 residual (detector, with SP8_OUT),
  SP_EPI_GRN = 8,      //       + GRN sums (pwconv1)
  SP_EPI_TOPK = 16,    // fused top-k
  SP_EPI_TOPK_LABELS = 17,  // fused top-k that honours row labels: tag filter and one row per group (own translation unit)
  SP_EPI_CHAIN = 32,   // chained 1x1
  SP_EPI_CHAIN_PHASE = 96,  // chained 1x1 + remapped Out2 rows + first-layer bias per row from a nine-class border table
};
constexpr bool sp_epi_chains(int epi) { return epi == SP_EPI_CHAIN || epi == SP_EPI_CHAIN_PHASE; }
constexpr int SP_ACT_ARGS = -1;  // ACT: activation read from the arguments

// ---- LDS of a launch ----
constexpr int kSpPiece = 1024;       // one DMA piece: 64 lanes x 16 bytes
constexpr int kSpSlab = 32 * 128;    // 32 rows x 32 f32 columns: one accumulator column block, or one 32-row SP8 stage
constexpr int kSpRing = 2;           // ring depth of every launch but the short window convs:
constexpr int kSpDeepRing = 4;       // sp_window_ring
constexpr long kSpRoundTiles = 512;  // tiles in flight at two blocks per CU

// A stage of the ring: [A rows][B rows][AMODE 3: 8 images x 32 k multipliers]; the window conv rings weights only.
constexpr int sp_stage_a(const SpTile& t, int amode) { return amode == SP_A_WINDOW ? 0 : t.bm() * t.rb(); }
constexpr int sp_stage_b(const SpTile& t) { return t.bn() * t.rb(); }
constexpr int sp_stage_mul(int amode) { return amode == SP_A_F32_MUL ? kSpPiece : 0; }
constexpr int sp_stage(const SpTile& t, int amode) { return sp_stage_a(t, amode) + sp_stage_b(t) + sp_stage_mul(amode); }
constexpr size_t sp_ring(const SpTile& t, int amode, int nst) { return (size_t)nst * sp_stage(t, amode); }

// The window conv's staged input window, in front of the ring: the tile's bm output pixels plus a row and a pixel on
// either side, in whole pieces, rb bytes per pixel.  (The kernel calls the integer form on g.Wd: handed its tile by
// reference instead, every window kernel gets another register allocation.)
constexpr int sp_window_px(int bm, int rb, int Wd) {
  const int rpp = kSpPiece / rb;
  return (bm + 2 * Wd + 2 + rpp - 1) / rpp * rpp;
}
constexpr size_t sp_window_bytes(const SpTile& t, int Wd) { return (size_t)sp_window_px(t.bm(), t.rb(), Wd) * t.rb(); }

// Epilogue staging: a wave stages a 32-row slab of all its columns over the ring.  Eight-wave blocks (two blocks of them
// per CU = four waves per SIMD) stage their slabs in two rounds, waves 0..3 first: the ring holds four slabs, not eight.
// (The window conv's launch is sized for all slabs instead, sp_launch_lds.)
constexpr int sp_staging_wave(const SpTile& t) { return 32 * 128 * t.tn; }
constexpr int sp_staging_rounds(const SpTile& t, int amode, int nst) {
  return (amode != SP_A_WINDOW && (size_t)t.waves() * sp_staging_wave(t) > sp_ring(t, amode, nst)) ? 2 : 1;
}

// Chained 1x1, after the main loop: [waves x one accumulator column block][waves x tn A2 stages][tn stages x N2 rows x
// 128 B of W2]
constexpr int sp_chain_a2(const SpTile& t) { return t.waves() * kSpSlab; }
constexpr int sp_chain_w2(const SpTile& t) { return t.waves() * kSpSlab * (1 + t.tn); }
constexpr size_t sp_chain_bytes(const SpTile& t, int N2) { return (size_t)sp_chain_w2(t) + (size_t)t.tn * N2 * 128; }

// Dynamic LDS a launch asks for.  The chain is sized for the widest second layer the chain predicate admits (N2 <= N).
constexpr size_t sp_launch_lds(const SpTile& t, int amode, int epi, int nst, int Wd) {
  size_t lds = sp_ring(t, amode, nst);
  if (amode == SP_A_WINDOW) {
    const size_t win = sp_window_bytes(t, Wd) + lds, stage = (size_t)t.waves() * sp_staging_wave(t);
    lds = win > stage ? win : stage;
  }
  if (sp_epi_chains(epi) && lds < sp_chain_bytes(t, sp_chain_max_n())) lds = sp_chain_bytes(t, sp_chain_max_n());
  return lds;
}

// Policy.  Two blocks per CU (160 KB of LDS) is what the tiles' efficiencies were measured at:
constexpr size_t kSpTwoPerCu = 80 * 1024;
// 3x3 / stride 1 / pad 1 convs whose channels come in whole stages: stage the tile's input window once per slice instead
// of gathering every tap from L2 (1.65 - 2.2x fewer LDS fill bytes), while two blocks still fit a CU
constexpr bool sp_window_fits(const SpTile& t, int Wd) {
  return sp_window_bytes(t, Wd) + sp_ring(t, SP_A_WINDOW, kSpRing) <= kSpTwoPerCu;
}
// window conv: a four-deep weight ring (three taps ahead) for launches of at most one round of tiles - there a tile's
// latency is the launch's duration (12800-row layers -15..-25 %); with several rounds the blocks per CU matter more
// (the deeper ring costs one: 204800 x 32 layers +12 %) and the two-deep ring stays
constexpr int sp_window_ring(const SpTile& t, int Wd, long tiles) {
  return (tiles <= kSpRoundTiles && sp_window_bytes(t, Wd) + sp_ring(t, SP_A_WINDOW, kSpDeepRing) <= kSpTwoPerCu) ? kSpDeepRing : kSpRing;
}
// whether any map is narrow enough for the deep ring on this tile (SP_CFG_N160's four-deep ring never fits twice per
// CU: no such instance is built)
constexpr bool sp_window_ring_deepens(const SpTile& t) { return sp_window_ring(t, 1, 1) == kSpDeepRing; }
// SP_CFG_N160 at the widest map it is named for (P3 of a 640 x 640 frame, Wd = 80): window + two-deep ring and the epilogue
// staging both leave room for a second block on the CU
static_assert(sp_window_fits(kSpTile[SP_CFG_N160], 80) && !sp_window_ring_deepens(kSpTile[SP_CFG_N160]) &&
                  sp_launch_lds(kSpTile[SP_CFG_N160], SP_A_WINDOW, SP_EPI_SP8_OUT, kSpRing, 80) <= kSpTwoPerCu,
              "the 128 x 160 tile runs two blocks per CU");

}  // namespace mtgv
