// Split GEMM epilogue: the chained 1x1 (SP_EPI_CHAIN) and its phase form (SP_EPI_CHAIN_PHASE).
// Included by gemm_sp_kernel.h, which defines SpDev, spf16 and the helpers used here (sp_sw, sp_slots,
// sp_pixel, sp_mfma3, sp_block_put / sp_block_get).
//
// A following 1x1 conv / Linear whose input is this launch's whole output row runs here: the activated values of the
// first layer are split into SP8 pieces and written to LDS as the wave's own A stages, W2 arrives by DMA while that
// happens, a second MFMA pass multiplies them and a second read-back stores Out2.  Same SP8 values, same product order as
// two launches.  PHASE: Out2's rows go through the output row remap and the first layer's bias is read per row from a
// table of nine border classes (SpDev::bias_tab).
//
// LDS after the main loop, sized by sp_chain_bytes (gemm_sp_cfg.h; sp_launch_lds asks for the widest N2 the chain admits):
//   [NW x 4 KB: one column block of each wave's accumulators]
//   [NW x TN x 4 KB: each wave's A2 stages, row-major 128-byte rows with the main loop's swizzle]   at sp_chain_a2
//   [TN stages x N2 rows x 128 B: W2]                                                              at sp_chain_w2
// Barriers: one, after the first layer's read-back, when W2 has landed for every wave; the caller has already passed the
// barrier that frees the ring.  Inactive waves (rows beyond M) take part in the DMA and the barrier and then leave.
#pragma once

namespace mtgv {

// WM waves of 32 rows x 32 TN columns (sp_tile_chains); mw0: first row of this wave, n0: first column of the tile
template <bool PHASE, int ACT, int WM, int TN>
__device__ __forceinline__ void sp_epi_chain(const SpDev& g, spf16 (&acc)[1][TN], char* smem, int mw0, int n0, int wave, int lane, bool wave_active) {
#pragma clang fp contract(off)
  constexpr SpTile T{WM, 1, 1, TN, 2};
  static_assert(sp_tile_chains(T), "chained 1x1: one wave holds whole rows");
  constexpr int NW = T.waves(), CB = kSpSlab;
  const int r = lane & 31, h = lane >> 5;
  const int slot = lane & 7, lrow = lane >> 3;
  char* const stg1 = smem + wave * CB;
  char* const a2 = smem + sp_chain_a2(T) + wave * (TN * CB);
  char* const w2 = smem + sp_chain_w2(T);
  const int n2g = g.N2 >> 3;  // 8-row DMA pieces per stage
  for (int p = wave; p < TN * n2g; p += NW) {
    const int s = p / n2g, rg = p - s * n2g;
    const int row = rg * 8 + (lane >> 3);
    const int slot_s = (lane & 7) ^ sp_sw<2>(row);
    const char* const sp = g.W2 + (long)row * ((long)g.N * 4) + s * 128 + slot_s * 16;
    __builtin_amdgcn_global_load_lds((sp_gptr)sp, (sp_lptr)(w2 + s * (g.N2 * 128) + rg * 1024), 16, 0, 0);
  }
  // PHASE: where each of this lane's four rows goes in Out2, and its border class
  long orow2[4];
  int bcls[4];
  if constexpr (PHASE) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      int m = mw0 + it * 8 + lrow;
      m = m < g.M ? m : g.M - 1;
      uint32_t img, oh, ow;
      sp_pixel(g, (uint32_t)m, img, oh, ow);
      const int y = (int)oh * g.os + g.oy, x = (int)ow * g.os + g.ox;
      orow2[it] = ((long)img * g.OH2 + y) * g.OW2 + x;
      bcls[it] = (y == 0 ? 0 : (y == g.OH2 - 1 ? 2 : 1)) * 3 + (x == 0 ? 0 : (x == g.OW2 - 1 ? 2 : 1));
    }
  }
  // first layer: scale, bias, activation, and the row's SP8 form into the wave's A2 stages
  if (wave_active) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + j * 32 + slot * 4;
      const sp_f4 w1 = *reinterpret_cast<const sp_f4*>(g.wscale + n);
      const sp_f4 b1 = g.bias != nullptr ? *reinterpret_cast<const sp_f4*>(g.bias + n) : sp_f4{0.f, 0.f, 0.f, 0.f};
      sp_block_put<128>(stg1, acc[0][j], 0, r, h);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + lrow;
        const sp_f4 raw = sp_block_get<128>(stg1, 0, it, lrow, slot);
        sp_f4 br = b1;  // PHASE: the row's own bias (the launch has no bias vector)
        if constexpr (PHASE) br = *reinterpret_cast<const sp_f4*>(g.bias_tab + bcls[it] * g.N + n);
        sp_f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_fixed<ACT>(__builtin_fmaf(raw[e], w1[e] * g.a_unmul, br[e]), g.act);
        // this lane's 16-byte piece of the row's SP8 form (even quads: the chunk's hi halves, odd quads: its lo halves)
        *reinterpret_cast<sp_f4*>(a2 + j * CB + row * 128 + ((slot ^ sp_sw<2>(row)) << 4)) = __builtin_bit_cast(sp_f4, sp8_piece_from_quad(v, slot));
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // W2 has landed for every wave (each waited for its own pieces)
  if (!wave_active) return;
  // second layer: A2 stage s is column block s of the first layer, k ascending
  const int tn2 = g.N2 >> 5;
  spf16 acc2[1][TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc2[0][j][q] = 0.f;
#pragma unroll
  for (int s = 0; s < TN; ++s) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const SpSlots so = sp_slots(ks, h, sp_sw<2>(r));
      const sp_h8 ah[1] = {*reinterpret_cast<const sp_h8*>(a2 + s * CB + r * 128 + so.hi)};
      const sp_h8 al[1] = {*reinterpret_cast<const sp_h8*>(a2 + s * CB + r * 128 + so.lo)};
      sp_h8 bh[TN], bl[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int rowb = j < tn2 ? j * 32 + r : r;  // (column blocks beyond N2 are computed on block 0's rows and dropped)
        bh[j] = *reinterpret_cast<const sp_h8*>(w2 + s * (g.N2 * 128) + rowb * 128 + so.hi);
        bl[j] = *reinterpret_cast<const sp_h8*>(w2 + s * (g.N2 * 128) + rowb * 128 + so.lo);
      }
      sp_mfma3<1, TN>(acc2, bh, bl, ah, al);
    }
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    if (j >= tn2) break;
    const int n = j * 32 + slot * 4;
    const sp_f4 w1 = *reinterpret_cast<const sp_f4*>(g.wscale2 + n);
    const sp_f4 b1 = g.bias2 != nullptr ? *reinterpret_cast<const sp_f4*>(g.bias2 + n) : sp_f4{0.f, 0.f, 0.f, 0.f};
    sp_block_put<128>(stg1, acc2[0][j], 0, r, h);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int m = mw0 + it * 8 + lrow;
      const sp_f4 raw = sp_block_get<128>(stg1, 0, it, lrow, slot);
      sp_f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = __builtin_fmaf(raw[e], w1[e], b1[e]);
        v[e] = g.act2 == ACT_SILU ? act_silu(t) : (g.act2 == ACT_NONE ? t : apply_act(t, g.act2));
      }
      sp_f4 piece = v;
      if (g.out_fmt2 == 1) piece = __builtin_bit_cast(sp_f4, sp8_piece_from_quad(v, slot));  // every lane takes part
      const long orow = PHASE ? orow2[it] : (long)m;
      if (m < g.M) *reinterpret_cast<sp_f4*>(g.Out2 + orow * g.ldo2 + g.o_off2 + n) = piece;
    }
  }
}

}  // namespace mtgv
