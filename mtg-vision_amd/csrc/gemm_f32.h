// Implicit-GEMM convolution / linear layer on the gfx950 f32 matrix cores.
//
//   Out[orow(m)][o_off + n] = act( sum_k A(m,k) * W[n][k] + bias[n] ) (+ res[m][n])
//
// A(m,k) is gathered on the fly from an NHWC activation tensor (no im2col):
//   m -> (img, oh, ow), k -> (kh, kw, c), A = in[img][oh*s+kh-p][ow*s+kw-p][c_off+c].
// W is [N][K] row-major with K ordered (kh, kw, c) - the same order nn.Linear
// uses for 1x1 (convnextv2.py:202-207) and what conv weights are repacked to
// at load time.
#pragma once
#include "common.h"

namespace mtgv {

struct GemmArgs {
  const float* A = nullptr;     // NHWC activation base
  int a_fmt = 0;                // 0: f32; 1: SP8 (sp8.h) - only launches gemm_sp_plan accepts (gemm_sp_takes_sp8)
  const float* W = nullptr;     // [N][K]
  // f16x3 only, optional: W with every aligned group of 4 floats replaced by their 4 fp16 hi + 4 fp16 lo halves
  // (same byte layout, so the same offsets address it).  gemm_launch fills it in for registered weights (operand_registry.h).
  const float* W_split = nullptr;
  // per-column power-of-two scales of W_split (registered rows are stored scaled, operand_registry.h); filled in by gemm_launch
  const float* wscale = nullptr;
  // f16x3 only: A is multiplied by a_mul (a power of two) before it is split and the accumulator by a_unmul = 1/a_mul.
  // For launches whose activations may exceed the fp16 range (|a| > 65504); 1 everywhere on the recognition path.
  float a_mul = 1.0f, a_unmul = 1.0f;
  float* Out = nullptr;
  int out_fmt = 0;              // 0: f32; 1: SP8 (LDS-DMA kernel only)
  const float* bias = nullptr;  // [N] or null
  const float* res = nullptr;   // residual [M][ldr] or null
  int res_fmt = 0;              // format of the residual rows (0 f32, 1 SP8)
  int M = 0, N = 0, K = 0;

  // A gather geometry (1x1/linear: KH=KW=1, stride=1, pad=0, H*W = rows per image)
  int H = 1, Wd = 1;            // input spatial size
  int c_total = 0;              // input channel stride (floats per pixel)
  int c_off = 0;                // first input channel used
  int Cin = 0;                  // channels consumed per tap (K = KH*KW*Cin)
  int KH = 1, KW = 1, stride = 1, pad = 0;
  int stride_w = 0;             // 0 = same as stride (the 4x4 stem views rows of 12 floats as pixels: stride 4 x 1)
  int OH = 1, OW = 1;           // output grid that m enumerates

  // output mapping: orow = (img*OH2 + oh*os + oy)*OW2 + ow*os + ox
  int ldo = 0, o_off = 0;
  int os = 1, oy = 0, ox = 0, OH2 = 1, OW2 = 1;
  // os_nq > 0 (LDS-DMA kernel only): the N columns are os * os groups of os_nq channels and group q scatters to
  // (oy, ox) = (q / os, q % os), channel n % os_nq - a whole ConvTranspose2d(k = s = os) as ONE launch that reads its
  // input once (W rows ordered (kh, kw, cout); bias repeated per group).  os_nq % 8 == 0.
  int os_nq = 0;
  // Chained 1x1 (LDS-DMA kernel only, gemm_sp_chain_ok): a second layer W2 [N2][N] (+ bias2, act2) applied to this launch's
  // activated output rows inside the epilogue; only Out2 is stored (Out may be null).  N in {32, 64, 96}, N2 % 32 == 0, N2 <= N.
  const float* W2 = nullptr;
  const float* bias2 = nullptr;
  float* Out2 = nullptr;
  int N2 = 0, ldo2 = 0, o_off2 = 0, out_fmt2 = 0, act2 = ACT_NONE;
  int ldr = 0;
  int act = ACT_NONE;

  // GRN (convnextv2.py:171-174): per-(tile, image-segment, n) partial sums of out^2
  float* grn_part = nullptr;    // [units][segmax][N], sized by gemm_grn_layout
  int hw = 0;                   // rows per image for GRN / prologue segmentation
  // written by gemm_launch (GrnLayout::segmax / unit_rows of the launch) when grn_part is set; callers leave them alone
  int segmax = 0;
  int grn_unit_rows = 0;
  // GRN apply fused into the A load of pwconv2: a' = a * a_scale[img][k] + a_shift[k]
  const float* a_scale = nullptr;
  const float* a_shift = nullptr;

  // batched launch (grid.y = batch index z): operands advance by these element strides per z
  int batch = 1;
  long strideA = 0, strideW = 0, strideO = 0;
  const int* m_count = nullptr;       // [batch] valid rows of batch z (rows beyond are neither read nor written)
  // crop_mask of process_mask: rows are detections, columns mask pixels n = py*crop_w + px;
  // values outside the row's box (xyxy image pixels * crop_scale, x in [x1,x2), y in [y1,y2)) become 0
  const float* crop_boxes = nullptr;  // [batch][crop_rows][4]
  int crop_rows = 0;                  // boxes per batch (>= M)
  float crop_scale = 0.f;
  int crop_w = 1;

  // match path: instead of storing Out, keep the top-`topk` (score desc, id asc)
  // columns of every row per column tile: cand[m][tile_n][topk]
  float* cand_s = nullptr;
  int* cand_i = nullptr;
  int topk = 0;
  // LayerNorm over the N outputs of every row fused into the epilogue (the encoder's stem: conv k4 s4 + LN,
  // convnextv2.py:253-256).  Only where gemm_ln_fusable() says so: one tile covers the whole row, whole tiles only.
  const float* ln_w = nullptr;
  const float* ln_b = nullptr;
  float ln_eps = 0.f;

  // (LDS-DMA kernel only; appended: the convert-on-load kernel takes this struct as its argument and reads none of these)
  // Asymmetric padding of the tap gather: rows of zero padding above / columns left of the image, < 0 = same as pad.
  // The padding below and right follows from OH / OW: taps outside the image read zeros.
  int pad_h = -1, pad_w = -1;
  // Chained 1x1 in its phase form (gemm_sp_kernel.h, EPI 96): Out2's rows go through the output mapping above (os, oy,
  // ox, OH2, OW2) and the first layer's bias of a row is bias_tab[3 * r + c][N], r / c = 0 first, 1 inner, 2 last row /
  // column of the OH2 x OW2 grid (bias stays null).  One output phase of a ConvTranspose2d(k2, s2) folded into the 3x3
  // conv behind it (Detector::proto).
  const float* bias_tab = nullptr;
  // algorithmic FLOPs the launch profiler credits this launch with besides its own 2 M N K (+ the chained layer's): a
  // launch that stands for more arithmetic than it runs (folded layers)
  double xflops = 0.0;
  // Labelled top-k (topk > 0; appended, read only by the labelled epilogues: gemm_kernel.h EPI 3, gemm_sp_kernel.h
  // SP_EPI_TOPK_LABELS).  Column n is eligible for row m when col_tags[n] passes row_masks[m] = (all_of, any_of, none_of);
  // with topk_distinct a candidate group keeps only the best column of every col_groups value >= 0.  gemm_launch takes
  // the labelled kernels when row_masks is set or topk_distinct is; launches without them are the plain top-k.
  const uint64_t* col_tags = nullptr;    // [N]
  const int* col_groups = nullptr;       // [N]
  const uint64_t* row_masks = nullptr;   // [M][3] or null: no filter
  int topk_distinct = 0;
};
inline bool topk_labelled(const GemmArgs& a) { return a.topk > 0 && (a.row_masks != nullptr || a.topk_distinct != 0); }

// A is gathered through a window (anything but a dense 1x1 / linear)
inline int conv_pad_h(const GemmArgs& a) { return a.pad_h >= 0 ? a.pad_h : a.pad; }
inline int conv_pad_w(const GemmArgs& a) { return a.pad_w >= 0 ? a.pad_w : a.pad; }
inline bool is_conv(const GemmArgs& a) {
  return !(a.KH == 1 && a.KW == 1 && a.stride == 1 && a.stride_w <= 1 && a.pad == 0 && conv_pad_h(a) == 0 && conv_pad_w(a) == 0);
}
// output row m is scattered to another grid (orow != m)
inline bool is_remap(const GemmArgs& a) { return !(a.os == 1 && a.oy == 0 && a.ox == 0 && a.OH2 == a.OH && a.OW2 == a.OW); }

// The two ways a launch is described; a caller then sets only what is special about it (residual, GRN, chained layer ...).
// Dense layer: Out[M][ldo] = act(A[M][lda] . W[N][K]^T + bias)
GemmArgs linear_args(const float* A, int lda, const float* W, const float* bias, float* Out, int ldo, int M, int N, int K,
                     int act);
// Convolution over channels [co, co + c) of an NHWC tensor with ct floats per pixel, into channels [co, co + cout) of another
struct ConvIn {
  const float* p;
  int n, h, w, ct, co, c, fmt;  // images, spatial size, floats per pixel, first channel, channels, format (GemmArgs::a_fmt)
};
struct ConvOut {
  float* p;
  int h, w, ct, co, fmt;        // output grid, floats per pixel, first channel, format (GemmArgs::out_fmt)
};
// Sets every geometry field (M, K, OH2 / OW2 included); W is [cout][kh][kw][in.c].  The stem's stride_w, the scatter of
// a ConvTranspose (os, oy, ox, os_nq, OH2, OW2: out.h x out.w is then the grid that m enumerates) are the caller's.
GemmArgs conv_args(const ConvIn& in, const float* W, const float* bias, int cout, int kh, int kw, int stride, int pad,
                   const ConvOut& out, int act);

// Runs the launch `a` describes.  The kernel and its tile follow from the arguments alone: the LDS-DMA kernel
// (gemm_sp.h) when it takes the launch, else the convert-on-load kernel (gemm_kernel.h) with the tile of its cost model
// (MTGV_GEMM_TILE=tm,tn,bk forces one; top-k launches have a fixed tile).
void gemm_launch(const GemmArgs& a, hipStream_t s);
// can this launch (no activation, no residual, not routed to the LDS-DMA kernel) normalise its rows in the epilogue?
bool gemm_ln_fusable(const GemmArgs& a);
// candidate groups of a top-k launch (a.topk > 0): per row, `slots` groups of `cols` columns each
void gemm_topk_layout(const GemmArgs& a, int* slots, int* cols);

// Operand precision of every GEMM launch of the process (see gemm_f32.hip): GEMM_PREC_F32 = f32 MFMA,
// GEMM_PREC_F16X3 = fp16 hi+lo split, three fp16 MFMAs per product.  Initial value from MTGV_GEMM_PREC=f32|f16x3.
enum { GEMM_PREC_F32 = 0, GEMM_PREC_F16X3 = 1 };
int gemm_precision();
void gemm_set_precision(int prec);
// out[n] = bias[n] + W[n][:] . shift  (GRN beta folded into the next Linear's bias; a_shift is not applied by the GEMM)
void fold_shift_into_bias_launch(const float* W, const float* shift, const float* bias, float* out, int N, int K, hipStream_t s);

// launch profiler for the roofline measurement (off by default; adds two event records per launch)
void gemm_profile_enable(bool on);
bool gemm_profile_enabled();
void gemm_profile_read(double* ms, double* flops, long* launches);
void gemm_profile_dump(const char* path);
double gemm_profile_bytes();  // compulsory operand + result bytes of the launches recorded since enable
// For launches that do the work of a GEMM layer outside gemm_launch (mlp_fused.hip): record `a`'s shape (M, N, K, act,
// a_scale / grn_part / res as flags) with the given LDS fill and compulsory bytes, bracketed by events on s.  xflops: the
// algorithmic FLOPs of further layers the launch runs besides `a` (c2f_tail.hip: three layers in one launch).
void gemm_profile_begin(const GemmArgs& a, hipStream_t s, int sp, double fill, double bytes, double xflops = 0.0);
void gemm_profile_end(hipStream_t s);

// Layout of the GRN partial sums a launch with these arguments writes: [ceil(M / unit_rows)][segmax][N] floats.
// Depends on which kernel gemm_launch will pick, so grn_part must be set (to any non-null pointer) already.
struct GrnLayout {
  int unit_rows = 0, segmax = 0;
  size_t floats = 0;
};
GrnLayout gemm_grn_layout(const GemmArgs& a);
// upper bound of GrnLayout::floats over every kernel / tile that could be chosen
size_t gemm_grn_part_floats_max(int M, int N, int hw);

// sum the partials of one GEMM into the GRN apply table
//   scale[img][n] = gamma[n] * Gx / (mean_n Gx + 1e-6) + 1,  Gx = sqrt(sum x^2)
void grn_finalize_launch(const float* part, const GrnLayout& l, int n_img, int hw, int N, const float* gamma, float* scale,
                         hipStream_t s);

}  // namespace mtgv
