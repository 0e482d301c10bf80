// C ABI (include/mtgv.h): encoder, bank and single-op entry points.
// Detector / NMS / warp entry points live next to their kernels (detector.hip, nms.hip, warp.hip).
#include "mtgv.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>

#include "c2f_tail.h"
#include "encoder.h"
#include "match.h"
#include "rowops.h"
#include "gemm_sp.h"
#include "operand_registry.h"
#include "track.h"

namespace mtgv {
const char* last_error_cstr();
}

using namespace mtgv;

namespace {
// The single-op entry points take raw weight pointers.  To run them on the same kernels the handles use, a constant
// operand is registered (SP8 copy + row scales) for the duration of the call; the call then synchronises the stream.
// Temporary registrations are visible to every thread through the registry: the single-op entry points therefore run
// one at a time (a process-wide lock held from before the lookup until the temporary copy has been released), so no
// other call can pick up a copy that is about to be freed.
std::recursive_mutex g_op_mu;
struct ScopedWeights {
  const float* w = nullptr;
  hipStream_t s;
  std::unique_lock<std::recursive_mutex> lk;
  ScopedWeights(const float* W, int n, int k, hipStream_t stream) : s(stream), lk(g_op_mu) {
    if (W == nullptr || k % 8 != 0 || gemm_precision() != GEMM_PREC_F16X3 || ((uintptr_t)W % 16) != 0) return;
    if (operand_sp8(W, k, nullptr, nullptr)) return;  // the caller already owns a registration
    operand_register(W, (size_t)n * k, k, false);  // the SP kernel's copy only
    operand_refresh(W, 0, (size_t)n * k, s);
    w = W;
  }
  ~ScopedWeights() {
    if (w == nullptr) return;
    (void)hipStreamSynchronize(s);
    operand_unregister(w);
  }
};
thread_local GrnLayout t_last_grn;

// max |x| of a device tensor (test / composition surface: one small kernel + a host read)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ out) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));  // non-negative floats order like their bit patterns
}

// A power of two that brings an activation tensor into the fp16 range of the split GEMM (1 when it already is):
// the single-op entry points take arbitrary f32 data, the handles know their activations are LayerNorm outputs etc.
void range_guard(GemmArgs& g, const float* a_dev, long n, hipStream_t s) {
  if (gemm_precision() != GEMM_PREC_F16X3 || n <= 0) return;
  static unsigned* d_max_dev[MTGV_MAX_DEVICES] = {};  // one scratch word per device
  unsigned*& d_max = d_max_dev[current_device()];
  if (d_max == nullptr) HIP_OK(hipMalloc((void**)&d_max, sizeof(unsigned)));
  HIP_OK(hipMemsetAsync(d_max, 0, sizeof(unsigned), s));
  const unsigned grid = (unsigned)std::min<long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, s, a_dev, n, d_max);
  unsigned bits = 0;
  HIP_OK(hipMemcpyAsync(&bits, d_max, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  float mx;
  memcpy(&mx, &bits, sizeof(float));
  if (!(mx > 16384.0f) || !(mx < INFINITY)) return;
  int ex;
  (void)frexpf(mx, &ex);  // mx = f * 2^ex, f in [0.5, 1): scaled maximum lands in [2^13, 2^14)
  g.a_mul = ldexpf(1.0f, 14 - ex);
  g.a_unmul = ldexpf(1.0f, ex - 14);
}
}  // namespace

struct mtgv_encoder {
  Encoder impl;
  explicit mtgv_encoder(const mtgv_encoder_cfg& c) : impl(c) {}
};
struct mtgv_bank {
  Bank impl;
  mtgv_bank(int d, int64_t c) : impl(d, c) {}
};

struct mtgv_tracker {
  Tracker impl;
  mtgv_tracker(const mtgv_tracker_cfg& c, int32_t flags, int embed_budget = 0) : impl(c, flags, embed_budget) {}
};

extern "C" {

MTGV_API const char* mtgv_last_error(void) { return last_error_cstr(); }
// 101: mtgv_detector_cfg.task, the OBB calls; 102: in_h / in_w, mtgv_head_rows h / w, the rect letterbox calls;
// 103: mtgv_detector_cfg.scale, mtgv_op_stem_u8; 104: the mtgv_tracker_* calls;
// 105: bank row labels (mtgv_bank_set_labels / _get_labels / mtgv_bank_topk_ex);
// 106: progressive JPEG (mtgv_jpeg_info_ex / mtgv_jpeg_decoder_create_ex, MTGV_JPEG_PROGRESSIVE)
// 108: labels across the sharded exchange (mtgv_bank_topk_packed_ex / mtgv_topk_merge_gathered_ex)
// 109: mtgv_detector_cfg.arch = 12 (YOLO12), mtgv_op_area_attn
// 110: mtgv_tracker_create_ex, MTGV_TRACKER_WIDE (256 tracks per stream, 64 cards per frame)
// 111: mtgv_letterbox_ragged_u8, mtgv_warp_quads_src (crops from full-resolution source frames)
// 112: mtgv_op_c2f_tail (the fused C2f tail as a single op)
// 113: mtgv_op_dwconv7_ln, mtgv_op_dwconv7_ln_form (the fused depthwise 7x7 + LayerNorm as a single op, and its kernel form)
// 114: mtgv_op_psa_attn, mtgv_op_dwconv3 (YOLO11's C2PSA attention and the depthwise 3x3 as single ops)
// 115: the embed budget (mtgv_tracker_create_budget, mtgv_tracker_update_budget, mtgv_tracker_gather_u8_pad, mtgv_op_track_select)
// 116: mtgv_op_mask_logits (the detector's mask stage as a single op)
// 117: mtgv_letterbox_tiles_u8, mtgv_tiles_merge (tiled detection: the cut and the merge)
// 118: mtgv_bank_prepass_layout, mtgv_bank_prepass_candidates (test surface: the two-pass match's first pass on its own)
// 119: mtgv_tiles_merge_obb, mtgv_op_quad_inter (tiled detection for OBB detectors: the rotated merge and its pair function)
MTGV_API int mtgv_version(void) { return 119; }
MTGV_API int mtgv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- GEMM operand precision ----
MTGV_API int mtgv_set_gemm_precision(int32_t prec) {
  return guarded([&] { gemm_set_precision(prec); });
}
MTGV_API int mtgv_get_gemm_precision(int32_t* prec) {
  return guarded([&] {
    MTGV_CHECK(prec != nullptr, ERR_INVALID, "null output");
    *prec = gemm_precision();
  });
}

// ---- GEMM launch profiler ----
MTGV_API int mtgv_profile_gemm(int32_t enable) {
  return guarded([&] { gemm_profile_enable(enable != 0); });
}
MTGV_API int mtgv_profile_gemm_read(double* total_ms, double* total_flops, int64_t* launches) {
  return guarded([&] {
    long l = 0;
    gemm_profile_read(total_ms, total_flops, &l);
    if (launches) *launches = l;
  });
}

MTGV_API int mtgv_profile_gemm_bytes(double* total_bytes) {
  return guarded([&] {
    MTGV_CHECK(total_bytes != nullptr, ERR_INVALID, "null output");
    *total_bytes = gemm_profile_bytes();
  });
}

MTGV_API int mtgv_profile_gemm_dump(const char* csv_path) {
  return guarded([&] {
    MTGV_CHECK(csv_path != nullptr, ERR_INVALID, "null path");
    gemm_profile_dump(csv_path);
  });
}

// ---- encoder ----
MTGV_API int mtgv_encoder_create(const mtgv_encoder_cfg* cfg, mtgv_encoder** out) {
  return guarded([&] {
    MTGV_CHECK(cfg != nullptr && out != nullptr, ERR_INVALID, "null argument");
    *out = new mtgv_encoder(*cfg);
  });
}
MTGV_API void mtgv_encoder_destroy(mtgv_encoder* h) { delete h; }
MTGV_API int mtgv_encoder_set_param(mtgv_encoder* h, const char* key, const float* data_host, int64_t numel) {
  return guarded([&] {
    MTGV_CHECK(h && key && data_host, ERR_INVALID, "null argument");
    h->impl.set_param(key, data_host, numel);
  });
}
MTGV_API int mtgv_encoder_missing_params(const mtgv_encoder* h) { return h ? h->impl.missing() : -1; }
MTGV_API int mtgv_encoder_forward(mtgv_encoder* h, const void* x_dev, int32_t layout, int32_t n, float* z_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.forward(x_dev, layout, n, z_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_encoder_set_graph(mtgv_encoder* h, int32_t mode, int32_t max_n) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.set_graph_mode(mode, max_n);
  });
}
MTGV_API int mtgv_encoder_set_capture(mtgv_encoder* h, int32_t on) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.set_capture(on != 0);
  });
}
MTGV_API int mtgv_encoder_stage_output(mtgv_encoder* h, int32_t stage, int32_t n, float* out_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && out_dev != nullptr, ERR_INVALID, "null argument");
    h->impl.stage_output(stage, n, out_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_encoder_flops(const mtgv_encoder* h, double* gemm_flops, double* dw_flops) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.flops(gemm_flops, dw_flops);
  });
}

// ---- bank ----
MTGV_API int mtgv_bank_create(int32_t dim, int64_t capacity, mtgv_bank** out) {
  return guarded([&] {
    MTGV_CHECK(out != nullptr, ERR_INVALID, "null argument");
    *out = new mtgv_bank(dim, capacity);
  });
}
MTGV_API void mtgv_bank_destroy(mtgv_bank* h) { delete h; }
MTGV_API int64_t mtgv_bank_size(const mtgv_bank* h) { return h ? h->impl.size() : -1; }
MTGV_API int mtgv_bank_append(mtgv_bank* h, const float* vecs, int64_t n, int32_t is_device, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && (vecs != nullptr || n == 0), ERR_INVALID, "null argument");
    h->impl.append(vecs, n, is_device != 0, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_set_row(mtgv_bank* h, int64_t row, const float* vec_host, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && vec_host != nullptr, ERR_INVALID, "null argument");
    h->impl.set_row(row, vec_host, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_clear(mtgv_bank* h) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.clear();
  });
}
MTGV_API int mtgv_bank_get_rows(const mtgv_bank* h, int64_t row, int64_t n, float* out_host) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && (out_host != nullptr || n == 0), ERR_INVALID, "null argument");
    h->impl.get_rows(row, n, out_host);
  });
}
MTGV_API int mtgv_bank_topk(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, float score_threshold,
                            int64_t* ids_dev, float* scores_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    MTGV_CHECK(!(score_threshold != score_threshold), ERR_INVALID, "bank: score_threshold is NaN");
    h->impl.topk(q_dev, b, k, id_base, score_threshold, ids_dev, scores_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_set_labels(mtgv_bank* h, int64_t row0, int64_t n, const uint64_t* tags_host, const int32_t* groups_host, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.set_labels(row0, n, tags_host, groups_host, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_get_labels(const mtgv_bank* h, int64_t row0, int64_t n, uint64_t* tags_host, int32_t* groups_host) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.get_labels(row0, n, tags_host, groups_host);
  });
}
MTGV_API int mtgv_bank_topk_ex(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, float score_threshold,
                               const uint64_t* masks_dev, int32_t distinct, int64_t* ids_dev, float* scores_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    MTGV_CHECK(!(score_threshold != score_threshold), ERR_INVALID, "bank: score_threshold is NaN");
    if (masks_dev == nullptr && distinct == 0)  // nothing to honour: mtgv_bank_topk itself, two-pass pre-pass included
      h->impl.topk(q_dev, b, k, id_base, score_threshold, ids_dev, scores_dev, (hipStream_t)stream);
    else
      h->impl.topk_labelled(q_dev, b, k, id_base, score_threshold, masks_dev, distinct != 0, ids_dev, scores_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_topk_packed(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, int64_t* packed_dev,
                                   void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && packed_dev != nullptr, ERR_INVALID, "null argument");
    h->impl.topk(q_dev, b, k, id_base, -INFINITY, packed_dev, nullptr, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_topk_merge_gathered(const int64_t* gathered_dev, int32_t n_ranks, int32_t b_total, int32_t k, int32_t row0, int32_t b,
                                      float score_threshold, int64_t* ids_dev, float* scores_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(gathered_dev && ids_dev && scores_dev, ERR_INVALID, "null argument");
    MTGV_CHECK(!(score_threshold != score_threshold), ERR_INVALID, "topk_merge_gathered: score_threshold is NaN");
    topk_merge_gathered_launch(gathered_dev, n_ranks, b_total, k, row0, b, score_threshold, false, ids_dev, scores_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_topk_packed_ex(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, const uint64_t* masks_dev,
                                      int32_t distinct, int64_t* packed_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && packed_dev != nullptr, ERR_INVALID, "null argument");
    h->impl.topk_packed_labelled(q_dev, b, k, id_base, masks_dev, distinct != 0, packed_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_topk_merge_gathered_ex(const int64_t* gathered_dev, int32_t n_ranks, int32_t b_total, int32_t k, int32_t row0, int32_t b,
                                         float score_threshold, int32_t distinct, int64_t* ids_dev, float* scores_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(gathered_dev && ids_dev && scores_dev, ERR_INVALID, "null argument");
    MTGV_CHECK(!(score_threshold != score_threshold), ERR_INVALID, "topk_merge_gathered: score_threshold is NaN");
    // distinct == 0: groups play no part, mtgv_topk_merge_gathered itself
    topk_merge_gathered_launch(gathered_dev, n_ranks, b_total, k, row0, b, score_threshold, distinct != 0, ids_dev, scores_dev,
                               (hipStream_t)stream);
  });
}
MTGV_API int mtgv_bank_prepass_fallbacks(const mtgv_bank* h, int64_t* count) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && count != nullptr, ERR_INVALID, "null argument");
    *count = h->impl.prepass_fallbacks();
  });
}
MTGV_API int mtgv_bank_prepass_layout(const mtgv_bank* h, int32_t* slots, int32_t* range_cols, int32_t* per_range) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && slots != nullptr && range_cols != nullptr && per_range != nullptr, ERR_INVALID, "null argument");
    int sl = 0, rc = 0, kp = 0;
    h->impl.prepass_layout(&sl, &rc, &kp);
    *slots = sl, *range_cols = rc, *per_range = kp;
  });
}
MTGV_API int mtgv_bank_prepass_candidates(mtgv_bank* h, const float* q_dev, int32_t b, float* cand_scores_dev, int32_t* cand_cols_dev,
                                          int32_t* slots, int32_t* range_cols, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    int sl = 0, rc = 0;
    h->impl.prepass_candidates(q_dev, b, cand_scores_dev, cand_cols_dev, &sl, &rc, (hipStream_t)stream);
    if (slots != nullptr) *slots = sl;
    if (range_cols != nullptr) *range_cols = rc;
  });
}
MTGV_API int mtgv_topk_merge(float* cand_scores_dev, const int64_t* cand_ids_dev, int32_t b, int32_t ncand, int32_t k,
                             float score_threshold, int64_t* ids_dev, float* scores_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(cand_scores_dev && cand_ids_dev && ids_dev && scores_dev, ERR_INVALID, "null argument");
    MTGV_CHECK(!(score_threshold != score_threshold), ERR_INVALID, "topk_merge: score_threshold is NaN");
    topk_merge_launch_i64(cand_scores_dev, cand_ids_dev, b, ncand, k, score_threshold, ids_dev, scores_dev, (hipStream_t)stream);
  });
}

// ---- tracker ----
MTGV_API int mtgv_tracker_create(const mtgv_tracker_cfg* cfg, mtgv_tracker** out) { return mtgv_tracker_create_ex(cfg, 0, out); }
MTGV_API int mtgv_tracker_create_ex(const mtgv_tracker_cfg* cfg, int32_t flags, mtgv_tracker** out) {
  return guarded([&] {
    MTGV_CHECK(cfg != nullptr && out != nullptr, ERR_INVALID, "tracker: null argument");
    (void)tracker_resolve_cfg(*cfg, flags);  // the range check before any HIP call
    *out = new mtgv_tracker(*cfg, flags);
  });
}
MTGV_API int mtgv_tracker_create_budget(const mtgv_tracker_cfg* cfg, int32_t flags, int32_t embed_budget, mtgv_tracker** out) {
  return guarded([&] {
    MTGV_CHECK(cfg != nullptr && out != nullptr, ERR_INVALID, "tracker: null argument");
    (void)tracker_resolve_cfg(*cfg, flags);  // the range checks before any HIP call
    (void)tracker_check_budget(embed_budget);
    *out = new mtgv_tracker(*cfg, flags, embed_budget);
  });
}
MTGV_API void mtgv_tracker_destroy(mtgv_tracker* h) { delete h; }
MTGV_API int mtgv_tracker_reset(mtgv_tracker* h, int32_t stream_or_minus_1, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.reset(stream_or_minus_1, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_tracker_update(mtgv_tracker* h, const float* quads_dev, const int32_t* n_det_dev, const int32_t* state_dev, int32_t frames,
                                 const int32_t* stream_of_frame_host, const double* now_host, int32_t* track_id_dev, int32_t* due_idx_dev,
                                 int32_t* n_due_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.update(quads_dev, n_det_dev, state_dev, frames, stream_of_frame_host, now_host, track_id_dev, due_idx_dev, n_due_dev, nullptr,
                   (hipStream_t)stream);
  });
}
MTGV_API int mtgv_tracker_update_budget(mtgv_tracker* h, const float* quads_dev, const int32_t* n_det_dev, const int32_t* state_dev, int32_t frames,
                                        const int32_t* stream_of_frame_host, const double* now_host, int32_t* track_id_dev, int32_t* due_idx_dev,
                                        int32_t* n_due_dev, int32_t* n_deferred_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && n_deferred_dev != nullptr, ERR_INVALID, "null handle or n_deferred");
    h->impl.update(quads_dev, n_det_dev, state_dev, frames, stream_of_frame_host, now_host, track_id_dev, due_idx_dev, n_due_dev, n_deferred_dev,
                   (hipStream_t)stream);
  });
}
MTGV_API int mtgv_tracker_gather_u8(const uint8_t* src_dev, int64_t src_rows, int64_t row_bytes, const int32_t* due_idx_dev,
                                    const int32_t* n_due_dev, int32_t max_rows, uint8_t* dst_dev, void* stream) {
  return guarded([&] { tracker_gather_u8_launch(src_dev, src_rows, row_bytes, due_idx_dev, n_due_dev, max_rows, dst_dev, false, (hipStream_t)stream); });
}
MTGV_API int mtgv_tracker_gather_u8_pad(const uint8_t* src_dev, int64_t src_rows, int64_t row_bytes, const int32_t* due_idx_dev,
                                        const int32_t* n_due_dev, int32_t max_rows, uint8_t* dst_dev, void* stream) {
  return guarded([&] { tracker_gather_u8_launch(src_dev, src_rows, row_bytes, due_idx_dev, n_due_dev, max_rows, dst_dev, true, (hipStream_t)stream); });
}
MTGV_API int mtgv_op_track_select(const double* waited_dev, int32_t n, int32_t budget, int32_t* due_idx_dev, int32_t* rank_of_dev, int32_t* n_due_dev,
                                  int32_t* n_deferred_dev, void* stream) {
  return guarded([&] { tracker_select_launch(waited_dev, n, budget, due_idx_dev, rank_of_dev, n_due_dev, n_deferred_dev, (hipStream_t)stream); });
}
MTGV_API int mtgv_tracker_commit(mtgv_tracker* h, const float* z_dev, float* q_dev, int32_t rows, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.commit(z_dev, q_dev, rows, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_tracker_store(mtgv_tracker* h, const int64_t* ids_dev, const float* scores_dev, int32_t rows, int64_t* out_ids_dev,
                                float* out_scores_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.store(ids_dev, scores_dev, rows, out_ids_dev, out_scores_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_tracker_get_state(mtgv_tracker* h, int32_t stream_index, double* kal_host, int32_t* ints_host, double* last_update_host,
                                    float* avg_z_host, int64_t* match_ids_host, float* match_scores_host, int32_t* counters_host, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.get_state(stream_index, kal_host, ints_host, last_update_host, avg_z_host, match_ids_host, match_scores_host, counters_host,
                      (hipStream_t)stream);
  });
}

// ---- single ops ----
MTGV_API int mtgv_op_linear(const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev, float* out_dev,
                            int32_t m, int32_t n, int32_t k, int32_t act, void* stream) {
  return guarded([&] {
    MTGV_CHECK(a_dev && w_dev && out_dev, ERR_INVALID, "null argument");
    ScopedWeights reg(w_dev, n, k, (hipStream_t)stream);
    GemmArgs g = linear_args(a_dev, k, w_dev, bias_dev, out_dev, n, m, n, k, act);
    g.res = res_dev;
    g.ldr = n;
    range_guard(g, a_dev, (long)m * k, (hipStream_t)stream);
    gemm_launch(g, (hipStream_t)stream);
  });
}
MTGV_API int64_t mtgv_op_linear_ex_part_floats(int32_t m, int32_t n, int32_t k, int32_t act, int32_t hw) {
  if (m <= 0 || n <= 0 || k <= 0 || hw <= 0) return 0;
  (void)act;
  return (int64_t)gemm_grn_part_floats_max(m, n, hw);
}
MTGV_API int mtgv_op_last_grn_layout(int32_t* unit_rows, int32_t* segmax) {
  return guarded([&] {
    MTGV_CHECK(unit_rows && segmax, ERR_INVALID, "null output");
    *unit_rows = t_last_grn.unit_rows;
    *segmax = t_last_grn.segmax;
  });
}
MTGV_API int mtgv_op_linear_ex(const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev, float* out_dev,
                               int32_t m, int32_t n, int32_t k, int32_t act, int32_t hw, const float* a_scale_dev,
                               const float* a_shift_dev, float* grn_part_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(a_dev && w_dev && out_dev, ERR_INVALID, "null argument");
    ScopedWeights reg(w_dev, n, k, (hipStream_t)stream);
    GemmArgs g = linear_args(a_dev, k, w_dev, bias_dev, out_dev, n, m, n, k, act);
    g.res = res_dev;
    g.ldr = n;
    g.hw = hw;
    g.a_scale = a_scale_dev;
    static DevBuf fold_tmp;  // test surface only: shift folded into a temporary bias
    if (a_shift_dev != nullptr) {
      fold_tmp.ensure((size_t)n);
      fold_shift_into_bias_launch(w_dev, a_shift_dev, bias_dev, fold_tmp.p, n, k, (hipStream_t)stream);
      g.bias = fold_tmp.p;
    }
    if (grn_part_dev) {
      g.grn_part = grn_part_dev;  // before the layout: the kernel choice depends on it
      t_last_grn = gemm_grn_layout(g);
    }
    gemm_launch(g, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_conv2d(const float* x_dev, const float* w_dev, const float* bias_dev, float* out_dev, int32_t n, int32_t h,
                            int32_t w, int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                            int32_t act, void* stream) {
  return guarded([&] {
    MTGV_CHECK(x_dev && w_dev && out_dev, ERR_INVALID, "null argument");
    MTGV_CHECK(stride > 0 && kh > 0 && kw > 0 && pad >= 0, ERR_INVALID, "bad conv geometry");
    const int oh = (h + 2 * pad - kh) / stride + 1, ow = (w + 2 * pad - kw) / stride + 1;
    MTGV_CHECK(oh > 0 && ow > 0, ERR_INVALID, "empty conv output");
    gemm_launch(conv_args({x_dev, n, h, w, cin, 0, cin, 0}, w_dev, bias_dev, cout, kh, kw, stride, pad, {out_dev, oh, ow, cout, 0, 0}, act),
                (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_conv2d_ex(const mtgv_conv_ex* d, int32_t* path, void* stream) {
  return guarded([&] {
    MTGV_CHECK(d && d->x && d->wt && (d->out || d->w2), ERR_INVALID, "null argument");
    MTGV_CHECK(d->stride > 0 && d->kh > 0 && d->kw > 0 && d->pad >= 0 && d->n > 0 && d->cin > 0 && d->cout > 0, ERR_INVALID, "bad conv geometry");
    const int oh = (d->h + 2 * d->pad - d->kh) / d->stride + 1, ow = (d->w + 2 * d->pad - d->kw) / d->stride + 1;
    MTGV_CHECK(oh > 0 && ow > 0, ERR_INVALID, "empty conv output");
    hipStream_t s = (hipStream_t)stream;
    ScopedWeights reg(d->wt, d->cout, d->kh * d->kw * d->cin, s), reg2(d->w2, d->cout2, d->cout, s);
    GemmArgs g = conv_args({(const float*)d->x, d->n, d->h, d->w, d->x_ct, d->x_co, d->cin, d->x_fmt}, d->wt, d->bias, d->cout, d->kh, d->kw,
                           d->stride, d->pad, {(float*)d->out, oh, ow, d->out_ct, d->out_co, d->out_fmt}, d->act);
    if (d->res) g.res = (const float*)d->res + d->res_co, g.ldr = d->res_ct, g.res_fmt = d->res_fmt;
    if (d->os > 1) {  // Detector::proto
      MTGV_CHECK(d->oy >= 0 && d->oy < d->os && d->ox >= 0 && d->ox < d->os && d->os_nq >= 0, ERR_INVALID, "bad scatter");
      g.os = d->os, g.OH2 = oh * d->os, g.OW2 = ow * d->os;
      if (d->os_nq > 0) g.os_nq = d->os_nq;
      else g.oy = d->oy, g.ox = d->ox;
    }
    if (d->w2) {  // Detector::conv_pair
      MTGV_CHECK(d->out2 && d->cout2 > 0, ERR_INVALID, "null argument");
      g.Out = nullptr;  // only the second layer's output is stored
      g.W2 = d->w2, g.bias2 = d->bias2, g.Out2 = (float*)d->out2, g.N2 = d->cout2, g.ldo2 = d->out2_ct, g.o_off2 = d->out2_co;
      g.out_fmt2 = d->out2_fmt, g.act2 = d->act2;
      MTGV_CHECK(gemm_sp_chain_ok(g), ERR_INVALID, "conv2d_ex: this pair cannot run as a chained launch");
    }
    if (path) {
      path[0] = -1, path[1] = path[2] = path[3] = 0;
      const SpPlan sp = gemm_sp_plan(g);  // gemm_launch decides by the same call
      if (sp.cfg >= 0) {
        const SpPath p = gemm_sp_path(g, sp);
        path[0] = p.cfg, path[1] = p.amode, path[2] = p.epi, path[3] = p.ring;
      }
    }
    gemm_launch(g, s);
  });
}
MTGV_API int mtgv_op_c2f_tail(const mtgv_c2f_tail* d, void* stream) {
  return guarded([&] {
    MTGV_CHECK(d && d->cat && d->out && d->w1 && d->w2 && d->w3, ERR_INVALID, "c2f_tail: null argument");
    MTGV_CHECK(d->n > 0 && d->h > 0 && d->w > 0 && d->ch > 0 && d->nb > 0 && d->cout > 0, ERR_INVALID, "c2f_tail: bad geometry");
    hipStream_t s = (hipStream_t)stream;
    const int k3 = (2 + d->nb) * d->ch;
    ScopedWeights reg1(d->w1, d->ch, 9 * d->ch, s), reg2(d->w2, d->ch, 9 * d->ch, s), reg3(d->w3, d->cout, k3, s);
    C2fTailArgs a;
    a.cat = (const float*)d->cat, a.cat_ct = d->cat_ct, a.cat_co = d->cat_co, a.n_img = d->n, a.H = d->h, a.W = d->w;
    a.ch = d->ch, a.nb = d->nb, a.shortcut = d->shortcut != 0;
    a.w1 = d->w1, a.b1 = d->b1, a.w2 = d->w2, a.b2 = d->b2, a.w3 = d->w3, a.b3 = d->b3, a.cout = d->cout;
    a.out = (float*)d->out, a.out_ct = d->out_ct, a.out_co = d->out_co;
    // the fused launch or an error: the three launches it replaces are mtgv_op_conv2d_ex's to run
    MTGV_CHECK(c2f_tail_ok(a), ERR_INVALID,
               "c2f_tail: no fused kernel for ch=%d nb=%d cout=%d on %d x %d (cat %d/%d, out %d/%d, f16x3 mode, biases, alignment)", d->ch,
               d->nb, d->cout, d->h, d->w, d->cat_ct, d->cat_co, d->out_ct, d->out_co);
    c2f_tail_launch(a, s);
    HIP_OK(hipStreamSynchronize(s));
  });
}
MTGV_API int mtgv_op_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, float* out_dev, int64_t rows,
                               int32_t c, float eps, void* stream) {
  return guarded([&] {
    MTGV_CHECK(x_dev && w_dev && b_dev && out_dev, ERR_INVALID, "null argument");
    ln_rows_launch(x_dev, c, 0, out_dev, c, 0, w_dev, b_dev, rows, c, eps, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_dwconv7(const float* x_dev, const float* w49_dev, const float* bias_dev, float* out_dev, int32_t n,
                             int32_t h, int32_t w, int32_t c, void* stream) {
  return guarded([&] {
    MTGV_CHECK(x_dev && w49_dev && bias_dev && out_dev, ERR_INVALID, "null argument");
    dwconv7_launch(x_dev, w49_dev, bias_dev, out_dev, n, h, w, c, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_dwconv7_ln_form(int32_t n, int32_t h, int32_t w, int32_t c, int32_t form[4]) {
  return guarded([&] {
    MTGV_CHECK(form != nullptr, ERR_INVALID, "dwconv7_ln: null form");
    MTGV_CHECK(n > 0 && h > 0 && w > 0 && c > 0, ERR_INVALID, "dwconv7_ln: bad geometry");
    dwconv7_ln_form(n, h, w, c, form);
  });
}
MTGV_API int mtgv_op_dwconv7_ln(const float* x_dev, const float* w49_dev, const float* bias_dev, const float* ln_w_dev,
                                const float* ln_b_dev, float* out_dev, int32_t n, int32_t h, int32_t w, int32_t c, float eps,
                                int32_t out_fmt, int32_t form[4], void* stream) {
  return guarded([&] {
    MTGV_CHECK(x_dev && w49_dev && bias_dev && ln_w_dev && ln_b_dev && out_dev && form, ERR_INVALID, "dwconv7_ln: null argument");
    MTGV_CHECK(n > 0 && h > 0 && w > 0 && c > 0 && (out_fmt == 0 || out_fmt == 1), ERR_INVALID, "dwconv7_ln: bad geometry or format");
    // the fused launch or an error: the unfused pair is mtgv_op_dwconv7 and mtgv_op_layernorm's to run
    int32_t f[4];  // the plan the launch ran, from the launch itself
    dwconv7_ln_launch(x_dev, w49_dev, bias_dev, ln_w_dev, ln_b_dev, out_dev, n, h, w, c, eps, (hipStream_t)stream, out_fmt, f);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    memcpy(form, f, sizeof(f));  // (a refused call leaves it as it was)
  });
}
MTGV_API int64_t mtgv_op_block_workspace_floats(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  return (int64_t)block_ws_size(n, h, w, c).total();
}
MTGV_API int mtgv_op_block(const float* x_dev, float* out_dev, int32_t n, int32_t h, int32_t w, int32_t c, int32_t act,
                           const float* dw_w49, const float* dw_b, const float* ln_w, const float* ln_b, const float* w1,
                           const float* b1, const float* gamma, const float* beta, const float* w2, const float* b2,
                           float* ws_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(x_dev && out_dev && ws_dev && x_dev != out_dev, ERR_INVALID, "null or aliased tensor");
    MTGV_CHECK(c % 4 == 0, ERR_INVALID, "block: C=%d must be a multiple of 4", c);
    BlockW bw;
    bw.dw_w49 = (float*)dw_w49, bw.dw_b = (float*)dw_b, bw.ln_w = (float*)ln_w, bw.ln_b = (float*)ln_b;
    bw.w1 = (float*)w1, bw.b1 = (float*)b1, bw.gamma = (float*)gamma, bw.beta = (float*)beta;
    bw.w2 = (float*)w2, bw.b2 = (float*)b2;
    ScopedWeights reg1(w1, 4 * c, c, (hipStream_t)stream), reg2(w2, c, 4 * c, (hipStream_t)stream);
    const BlockWs ws = block_ws_carve(ws_dev, block_ws_size(n, h, w, c));
    run_block(x_dev, out_dev, n, h, w, c, act, bw, ws, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_l2norm(const float* x_dev, float* out_dev, int64_t rows, int32_t d, void* stream) {
  return guarded([&] {
    MTGV_CHECK(x_dev && out_dev, ERR_INVALID, "null argument");
    l2norm_rows_launch(x_dev, out_dev, rows, d, (hipStream_t)stream);
  });
}

}  // extern "C"
