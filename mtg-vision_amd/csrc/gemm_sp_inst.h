// One tile configuration of the LDS-DMA split GEMM per translation unit (they compile in parallel): a file defines
// SP_CFG_ID and includes this header, which instantiates that row of kSpTile (gemm_sp_cfg.h).
#pragma once
#include "gemm_sp_kernel.h"

namespace mtgv {

namespace {
template <int ID, int AMODE, int ACT, int EPI, int NST = kSpRing>
void sp_launch_one(const SpDev& g, hipStream_t s) {
  constexpr SpTile T = kSpTile[ID];
  if constexpr (AMODE == SP_A_WINDOW && NST == kSpRing && sp_window_ring_deepens(T)) {
    if (sp_window_ring(T, g.Wd, (long)g.tiles_m * g.tiles_n) == kSpDeepRing) return sp_launch_one<ID, AMODE, ACT, EPI, kSpDeepRing>(g, s);
  }
  const size_t lds = sp_launch_lds(T, AMODE, EPI, NST, g.Wd);
  constexpr auto kern = gemm_sp_kernel<T.wm, T.wn, T.tm, T.tn, T.ks, NST, AMODE, ACT, EPI>;
  lds_opt_in<kern>(lds, (AMODE == SP_A_WINDOW || sp_epi_chains(EPI)) ? 160 * 1024 : (int)lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(64 * T.waves()), lds, s, g);
}

// launches the instance whose EPI equals `epi` if it is one of those listed, the generic one otherwise
template <int ID, int AMODE, int ACT>
void sp_pick(const SpDev& g, int epi, hipStream_t s) {
  MTGV_CHECK(!sp_epi_chains(epi), ERR_RUNTIME, "gemm_sp: no chained-1x1 instance for A mode %d in configuration %d", AMODE, ID);
  sp_launch_one<ID, AMODE, ACT, SP_EPI_ARGS>(g, s);
}
template <int ID, int AMODE, int ACT, int E0, int... ES>
void sp_pick(const SpDev& g, int epi, hipStream_t s) {
  if (epi == E0) sp_launch_one<ID, AMODE, ACT, E0>(g, s);
  else sp_pick<ID, AMODE, ACT, ES...>(g, epi, s);
}

// SP8 out, and SP8 out + SP8 residual (detector): the SiLU convs' specialised epilogues
constexpr int SP8_RES = SP_EPI_SP8_OUT | SP_EPI_RES_SP8;

// convs (SP_A_CONV / SP_A_WINDOW): SiLU with the detector's epilogues - and the chained 1x1 on the tiles that chain
// (sp_tile_chains) - get kernels of their own; the phase form of the chain (Proto's folded ConvTranspose + cv2: 2x2 taps,
// never a window conv) on the tap gather only
template <int ID, int AMODE>
void sp_pick_conv(const SpDev& g, int epi, hipStream_t s) {
  if (g.act != ACT_SILU) sp_pick<ID, AMODE, SP_ACT_ARGS>(g, epi, s);
  else if constexpr (sp_tile_chains(kSpTile[ID]) && AMODE == SP_A_CONV)
    sp_pick<ID, AMODE, ACT_SILU, SP_EPI_SP8_OUT, SP8_RES, SP_EPI_CHAIN, SP_EPI_CHAIN_PHASE>(g, epi, s);
  else if constexpr (sp_tile_chains(kSpTile[ID])) sp_pick<ID, AMODE, ACT_SILU, SP_EPI_SP8_OUT, SP8_RES, SP_EPI_CHAIN>(g, epi, s);
  else sp_pick<ID, AMODE, ACT_SILU, SP_EPI_SP8_OUT, SP8_RES>(g, epi, s);
}
}  // namespace

// The instances of configuration ID (gemm_sp.hip dispatches on the plan's cfg): per A mode, the activations and
// epilogue shapes the executors use get kernels of their own, everything else the generic one.
template <int ID>
void gemm_sp_launch_cfg(const SpDev& g, int amode, hipStream_t s);

#if SP_CFG_ID == 7
// SP_CFG_N160: one instance - the planner names this tile for that launch shape only (gemm_sp.hip)
static_assert(SP_CFG_ID == SP_CFG_N160, "the single-instance configuration");
template <>
void gemm_sp_launch_cfg<SP_CFG_N160>(const SpDev& g, int amode, hipStream_t s) {
  MTGV_CHECK(amode == SP_A_WINDOW && g.act == ACT_SILU && g.topk == 0 && sp_epi_of(g) == SP_EPI_SP8_OUT, ERR_RUNTIME,
             "gemm_sp: configuration %d runs SiLU window convs with SP8 output only (A mode %d, act %d)", (int)SP_CFG_N160, amode, g.act);
  sp_launch_one<SP_CFG_N160, SP_A_WINDOW, ACT_SILU, SP_EPI_SP8_OUT>(g, s);
}
#endif

template <int ID>
void gemm_sp_launch_cfg(const SpDev& g, int amode, hipStream_t s) {
  constexpr SpTile T = kSpTile[ID];
  if (g.topk > 0) {  // match path: f32 queries by DMA, fused top-k epilogue; only SP_CFG_TOPK carries it
    if constexpr (ID == SP_CFG_TOPK) {
      MTGV_CHECK((amode == SP_A_F32 || amode == SP_A_HI16) && g.act == ACT_NONE, ERR_INVALID, "gemm_sp: top-k needs aligned f32 queries");
      if (amode == SP_A_HI16) sp_launch_one<ID, SP_A_HI16, ACT_NONE, SP_EPI_TOPK>(g, s);  // fp16 rows on both sides: the approximate first pass
      else sp_launch_one<ID, SP_A_F32, ACT_NONE, SP_EPI_TOPK>(g, s);
      return;
    } else {
      MTGV_CHECK(false, ERR_INVALID, "gemm_sp: no top-k instance in this configuration");
    }
  }
  const int epi = sp_epi_of(g);
  if constexpr (T.ks != 2) {
    // the 16-k configuration exists for the conv paths only (window conv, and the tap gather it falls back to)
    MTGV_CHECK(amode == SP_A_WINDOW || amode == SP_A_CONV, ERR_RUNTIME, "gemm_sp: configuration %d runs convolutions only (A mode %d)", ID, amode);
    if (amode == SP_A_WINDOW) sp_pick_conv<ID, SP_A_WINDOW>(g, epi, s);
    else sp_pick_conv<ID, SP_A_CONV>(g, epi, s);
  } else if (amode == SP_A_SP8) {
    switch (g.act) {
      case ACT_NONE: sp_pick<ID, SP_A_SP8, ACT_NONE, SP_EPI_F32, SP_EPI_SP8_OUT>(g, epi, s); break;
      case ACT_MISH: sp_pick<ID, SP_A_SP8, ACT_MISH, SP_EPI_GRN>(g, epi, s); break;
      case ACT_GELU: sp_pick<ID, SP_A_SP8, ACT_GELU, SP_EPI_GRN>(g, epi, s); break;
      case ACT_SILU: sp_pick<ID, SP_A_SP8, ACT_SILU, SP_EPI_SP8_OUT, SP8_RES>(g, epi, s); break;
      default: sp_pick<ID, SP_A_SP8, SP_ACT_ARGS>(g, epi, s); break;
    }
  } else if (amode == SP_A_REG) {
    if (g.act == ACT_NONE) sp_pick<ID, SP_A_REG, ACT_NONE>(g, epi, s);
    else sp_pick<ID, SP_A_REG, SP_ACT_ARGS>(g, epi, s);
  } else if (amode == SP_A_F32_MUL) {
    if (g.act == ACT_NONE) sp_pick<ID, SP_A_F32_MUL, ACT_NONE, SP_EPI_RES_F32>(g, epi, s);
    else sp_pick<ID, SP_A_F32_MUL, SP_ACT_ARGS>(g, epi, s);
  } else if (amode == SP_A_F32) {
    if (g.act == ACT_NONE) sp_pick<ID, SP_A_F32, ACT_NONE, SP_EPI_F32, SP_EPI_RES_F32>(g, epi, s);
    else sp_pick<ID, SP_A_F32, SP_ACT_ARGS>(g, epi, s);
  } else if (amode == SP_A_WINDOW) {
    sp_pick_conv<ID, SP_A_WINDOW>(g, epi, s);
  } else if (g.act == ACT_NONE) {
    sp_pick<ID, SP_A_CONV, ACT_NONE, SP_EPI_F32, SP_EPI_SP8_OUT>(g, epi, s);
  } else {
    sp_pick_conv<ID, SP_A_CONV>(g, epi, s);
  }
}

#if SP_CFG_ID != 7
template void gemm_sp_launch_cfg<SP_CFG_ID>(const SpDev& g, int amode, hipStream_t s);
#endif

}  // namespace mtgv
