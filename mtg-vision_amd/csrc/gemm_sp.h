// Host side of the LDS-DMA split-precision GEMM (gemm_sp_kernel.h): tile selection and launch.  gemm_launch
// (gemm_f32.hip) routes every eligible f16x3 launch here; B operands come from the registry (operand_registry.h), the
// tile table, configuration names, A modes, epilogue shapes and LDS layout from gemm_sp_cfg.h.
#pragma once
#include "gemm_f32.h"

namespace mtgv {

struct SpPlan {
  int cfg = -1;          // index into kSpTile (gemm_sp_cfg.h); -1: not eligible
  int bm = 0, bn = 0;
  int unit_rows = 0;     // rows of one GRN partial unit (a wave's rows)
  int tiles_m = 0, tiles_n = 0;
};

// f16x3 operand mode: the LDS-DMA kernel runs, and executors keep activations in SP8
bool gemm_sp_active();
// Can (and should) this launch run on the SP kernel?  a.a_fmt says how A is stored.
SpPlan gemm_sp_plan(const GemmArgs& a);
// true when a dense [M][K] x [N][K]^T launch with these sizes would take SP8 activations (producer kernels ask before
// choosing their output format)
bool gemm_sp_takes_sp8(const float* W, int M, int N, int K, int lda, int c_off);
// only through gemm_launch, which has checked the arguments and filled in a.segmax for GRN launches
void gemm_sp_launch(const GemmArgs& a, const SpPlan& pl, hipStream_t s);
// The kernel gemm_sp_launch runs for (a, pl), from the code it launches with: tile configuration, A mode (SpAMode),
// epilogue shape (sp_epi_of) and ring depth (sp_window_ring for the window conv).  Test surface.
struct SpPath {
  int cfg, amode, epi, ring;
};
SpPath gemm_sp_path(const GemmArgs& a, const SpPlan& pl);
// can the launch described by `a` (W2 / bias2 / Out2 / N2 ... set) run with its second layer chained into the epilogue?
bool gemm_sp_chain_ok(const GemmArgs& a);
bool gemm_sp_topk_layout(const GemmArgs& a, int* slots, int* cols);  // gemm_topk_layout when the SP kernel takes the launch
double gemm_sp_fill_bytes(const GemmArgs& a, const SpPlan& pl);  // LDS fill bytes of the launch (profiling aid)
void gemm_sp_stamps_dump(const char* path);  // tuning aid, see gemm_sp.hip

// Approximate scores for the bank match's first pass: q_hi [b][K] and bank_hi [N][K] are fp16 rows (the hi halves of the
// exact operands, the bank's scaled per row by 1 / wscale), one fp16 MFMA per product; per (query, 96-column wave
// range) the kp best (score, column) pairs go to cand_s / cand_i like the exact top-k launch's.  128 x 192 tiles;
// b >= 128, N >= 192, K % 64 == 0.  *slots = candidate groups per query.
void gemm_sp_topk_hi16_launch(const void* q_hi, const void* bank_hi, const float* wscale, int b, int N, int K, int kp, float* cand_s,
                              int* cand_i, int* slots, hipStream_t s);
int gemm_sp_topk_hi16_slots(int N);
int gemm_sp_topk_hi16_range_cols();  // columns per candidate group: group w covers columns [w * cols, (w + 1) * cols)

// >= 256 zero bytes on the current device (K tails and padding taps of the DMA paths read them)
const char* sp_zero_page();

// f32 [rows][K] -> SP8 rows, unscaled (activations; test surface)
void sp8_pack_plain_launch(const float* in, void* out, long rows, int K, hipStream_t s);

}  // namespace mtgv
