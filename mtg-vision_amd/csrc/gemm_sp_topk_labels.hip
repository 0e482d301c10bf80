// LDS-DMA split GEMM: the match path's labelled top-k (SP_EPI_TOPK_LABELS), its one instance - the SP_CFG_TOPK tile with
// f32 queries by DMA - in a translation unit of its own, beside the per-configuration ones (gemm_sp_c<id>.hip).
#include "gemm_sp.h"
#include "gemm_sp_kernel.h"

namespace mtgv {

void gemm_sp_topk_labels_launch(const SpDev& g, hipStream_t s) {
  constexpr SpTile T = kSpTile[SP_CFG_TOPK];
  MTGV_CHECK(g.topk > 0 && g.topk <= T.wave_cols() && g.act == ACT_NONE && g.cand_s != nullptr && g.cand_i != nullptr, ERR_INVALID,
             "gemm_sp: labelled top-k of %d per range of %d columns", g.topk, T.wave_cols());
  MTGV_CHECK((g.row_masks == nullptr || g.col_tags != nullptr) && (g.distinct == 0 || g.col_groups != nullptr), ERR_INVALID,
             "gemm_sp: labelled top-k without its label arrays");
  MTGV_CHECK(((uintptr_t)g.col_tags & 15) == 0 && ((uintptr_t)g.col_groups & 15) == 0, ERR_INVALID, "gemm_sp: label arrays must be 16-byte aligned");
  constexpr size_t lds = sp_launch_lds(T, SP_A_F32, SP_EPI_TOPK_LABELS, kSpRing, 1);
  constexpr auto kern = gemm_sp_kernel<T.wm, T.wn, T.tm, T.tn, T.ks, kSpRing, SP_A_F32, ACT_NONE, SP_EPI_TOPK_LABELS>;
  lds_opt_in<kern>(lds, (int)lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(64 * T.waves()), lds, s, g);
}

}  // namespace mtgv
