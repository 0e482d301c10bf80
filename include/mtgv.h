/* mtgv.h - C ABI of libmtgv.so: the MI355X-native recognition hot path of mtg-vision
 * (detect -> crop -> embed -> cosine top-k over the card bank).
 *
 * Every entry point is what a binding for that path would call.  The reference
 * (nmichlo/mtg-vision, all paths relative to its root) is pure Python; the
 * interface each group replaces is cited.  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *   - return value: 0 = ok, 1 = invalid argument (reference: AssertionError),
 *     2 = unknown key/name (KeyError), 3 = runtime failure (RuntimeError).
 *     mtgv_last_error() returns the message of the calling thread's last failure.
 *   - pointers named *_dev are device (HIP) pointers owned by the caller
 *     (torch tensors on cuda:<i>); *_host are host pointers.  The library owns
 *     only weights / bank / workspace inside its opaque handles and allocates
 *     nothing on the hot path after the first call at a given batch size.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  A handle is
 *     bound to the HIP device current at creation and is not thread-safe; calls on
 *     one handle must be serialised by the caller (the reference is single-threaded
 *     per process: mtgvision/server.py:29-35, :280).
 *   - activations are float32; images are NHWC unless stated.
 */
#ifndef MTGV_H
#define MTGV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MTGV_API __attribute__((visibility("default")))
#else
#define MTGV_API
#endif

MTGV_API const char* mtgv_last_error(void);
/* 110: mtgv_tracker_create_ex / MTGV_TRACKER_WIDE (256 tracks per stream, 64 cards per frame)
 * 111: mtgv_letterbox_ragged_u8, mtgv_warp_quads_src (crops from full-resolution source frames)
 * 115: the embed budget of the tracker (mtgv_tracker_create_budget, mtgv_tracker_update_budget, mtgv_tracker_gather_u8_pad,
 *      mtgv_op_track_select)
 * 116: mtgv_op_mask_logits (the detector's mask stage as a single op)
 * 117: mtgv_letterbox_tiles_u8, mtgv_tiles_merge (detection on overlapping windows of large source frames)
 * 119: mtgv_tiles_merge_obb, mtgv_op_quad_inter (the same for OBB detectors: oriented quads merged across windows) */
MTGV_API int mtgv_version(void);
/* number of HIP devices visible; does not initialise a device context */
MTGV_API int mtgv_device_count(void);

/* Operand precision of every GEMM-shaped kernel launch of the process (convs, linears, mask and bank GEMMs).
 *   MTGV_PREC_F32   (0)  f32 operands on the f32-input matrix instruction (exact products).
 *   MTGV_PREC_F16X3 (1)  each f32 operand represented as fp16 hi + lo; three fp16 matrix instructions per
 *                        product, f32 accumulate.  Error vs fp64 at the f32 level, ~2x the GEMM rate.  Weights carry
 *                        a power-of-two scale per output row (undone in the accumulator), so their magnitude does
 *                        not matter; activations inside the handles are O(1) by construction; mtgv_op_linear, which
 *                        takes arbitrary f32 data, rescales inputs beyond 2^14 by a power of two (the other mtgv_op_*
 *                        entry points expect activations within the fp16 range, as the handles produce them).
 *                        Values that leave the fp16 range turn into inf - visible, never silently wrong.
 * The initial value comes from the environment (MTGV_GEMM_PREC=f32|f16x3, default f16x3).  Both
 * meet the path's 1e-4 contract against the reference (tests/test_gpu_precision.py).  Not thread-safe: set it
 * before the worker threads start.
 * Concurrency contract for F16X3 (measured on MI355X / ROCm 7.2): kernels that use packed-FP32
 * arithmetic (v_pk_mul_f32, v_pk_fma_f32) and run on ANOTHER STREAM of the same GPU while F16X3 launches are in
 * flight can get wrong lanes.  This library is built without those instructions (every translation unit).  Streams
 * the library itself uses besides the caller's: mtgv_detector_forward forks its prototype branch and two head branches
 * onto library-owned streams and joins them before it returns control of the caller's stream (library kernels only;
 * MTGV_DET_FORK=0 keeps the forward on one stream).  mtgv.Pipeline overlaps its stages (detect + crop / embed / match: three streams, the
 * latter two at high priority, the detector's fork-join off) only with MTGV_OVERLAP=on, and then runs nothing but library kernels on them - its output tensors are uninitialised allocations filled by the
 * kernels, the glue between the stages is mtgv_select_cards / mtgv_obb_cards - plus, with a sharded bank, RCCL's own all-gather kernels
 * (mtgv_bank_topk_packed / mtgv_topk_merge_gathered and their _ex forms keep every other step of the exchange inside the library).  A caller
 * that runs foreign kernels (PyTorch elementwise ops included) concurrently on a second stream must either serialise
 * them against the library's stream or select MTGV_PREC_F32. */
#define MTGV_PREC_F32 0
#define MTGV_PREC_F16X3 1
MTGV_API int mtgv_set_gemm_precision(int32_t prec);
MTGV_API int mtgv_get_gemm_precision(int32_t* prec);

/* Measurement aid: when enabled, every launch of the GEMM kernel is bracketed by HIP
 * events on its own stream.  _read waits for them and returns the summed kernel time (ms), the
 * summed algorithmic FLOPs (2*M*N*K of the unpadded problems) and the launch count since enable. */
MTGV_API int mtgv_profile_gemm(int32_t enable);
MTGV_API int mtgv_profile_gemm_read(double* total_ms, double* total_flops, int64_t* launches);
/* compulsory HBM bytes of the launches since enable: every operand element read once, every result written once */
MTGV_API int mtgv_profile_gemm_bytes(double* total_bytes);
/* write one CSV row per recorded launch (shape, tile, ms, TFLOP/s) */
MTGV_API int mtgv_profile_gemm_dump(const char* csv_path);

/* ------------------------------------------------------------------------- */
/* Encoder: ConvNeXt-V2 embedding forward.                                    */
/* Replaces CoreMlEncoder.predict (mtgvision/encoder_export.py:85-110),       */
/* ConvNeXtV2Encoder.forward (mtgvision/models/convnextv2ae.py:256-266),      */
/* ConvNeXtV2.forward (mtgvision/models/convnextv2.py:292-303) and            */
/* MtgVisionEncoder.encode (mtgvision/encoder_train.py:356-358).              */
/* ------------------------------------------------------------------------- */
typedef struct mtgv_encoder mtgv_encoder;

enum { MTGV_ENC_AE = 0, MTGV_ENC_PLAIN = 1 };
enum {
  MTGV_HEAD_CONV_LINEAR = 0, /* convnextv2ae.py:219-235 */
  MTGV_HEAD_CONV_MLP = 1,
  MTGV_HEAD_CONV_ACT_MLP = 2,
  MTGV_HEAD_POOL_LINEAR = 3, /* convnextv2ae.py:236-248 */
  MTGV_HEAD_POOL_MLP = 4,
  MTGV_HEAD_PLAIN = 5        /* GAP -> nn.LayerNorm -> Linear, convnextv2.py:280-303 */
};
enum { MTGV_IN_NCHW_F32 = 0, MTGV_IN_NHWC_F32 = 1, MTGV_IN_NHWC_U8 = 2 };

typedef struct {
  int32_t kind;       /* MTGV_ENC_* */
  int32_t image_h, image_w;
  int32_t in_chans;   /* 3 */
  int32_t z_size;
  int32_t depths[4];
  int32_t dims[4];
  int32_t head_type;  /* MTGV_HEAD_* */
  int32_t scale_io;   /* x*2-1 first (convnextv2ae.py:257-258) */
  int32_t max_batch;  /* workspace is sized for this many images */
} mtgv_encoder_cfg;

MTGV_API int mtgv_encoder_create(const mtgv_encoder_cfg* cfg, mtgv_encoder** out);
MTGV_API void mtgv_encoder_destroy(mtgv_encoder* h);
/* Upload one parameter by its reference state_dict key (layout as stored by
 * PyTorch: conv OIHW, linear [out,in]); numel must match.  Unknown key -> 2. */
MTGV_API int mtgv_encoder_set_param(mtgv_encoder* h, const char* key, const float* data_host, int64_t numel);
/* number of parameters still unset (0 = ready) */
MTGV_API int mtgv_encoder_missing_params(const mtgv_encoder* h);
/* x_dev: n images in `layout`; z_dev: (n, z_size) float32. */
MTGV_API int mtgv_encoder_forward(mtgv_encoder* h, const void* x_dev, int32_t layout, int32_t n, float* z_dev, void* stream);
/* mode 1: forwards of <= max_n images (default 16, 0 keeps it) replay a hipGraph captured per batch size;
 * mode 0 (default): every launch eager.  Measured: no latency gain on this path - its ~90 short kernels are
 * serialised by dependent-kernel boundaries, which a graph does not remove (profiles/README.md). */
MTGV_API int mtgv_encoder_set_graph(mtgv_encoder* h, int32_t mode, int32_t max_n);
/* keep a copy of every stage output of subsequent forwards (test/debug aid; off by default) */
MTGV_API int mtgv_encoder_set_capture(mtgv_encoder* h, int32_t on);
/* copy stage s (0..3) output of the last forward, NHWC (n, h, w, c), into out_dev; for tests */
MTGV_API int mtgv_encoder_stage_output(mtgv_encoder* h, int32_t stage, int32_t n, float* out_dev, void* stream);
/* algorithmic FLOPs (2*MAC) of one image's forward, split MFMA-eligible GEMM / depthwise */
MTGV_API int mtgv_encoder_flops(const mtgv_encoder* h, double* gemm_flops, double* dw_flops);

/* ------------------------------------------------------------------------- */
/* Bank: exact cosine top-k over all card vectors.                            */
/* Replaces VectorStoreQdrant.query_nearby / save_points / retrieve           */
/* (mtgvision/qdrant.py:17-111; collection "mtg", size 768, Distance.COSINE). */
/* ------------------------------------------------------------------------- */
typedef struct mtgv_bank mtgv_bank;

MTGV_API int mtgv_bank_create(int32_t dim, int64_t capacity, mtgv_bank** out);
MTGV_API void mtgv_bank_destroy(mtgv_bank* h);
MTGV_API int64_t mtgv_bank_size(const mtgv_bank* h);
/* append n vectors (device or host memory, is_device says which); stored L2-normalised */
MTGV_API int mtgv_bank_append(mtgv_bank* h, const float* vecs, int64_t n, int32_t is_device, void* stream);
/* overwrite row `row` (save_points on an existing id) */
MTGV_API int mtgv_bank_set_row(mtgv_bank* h, int64_t row, const float* vec_host, void* stream);
MTGV_API int mtgv_bank_clear(mtgv_bank* h);
/* copy stored (normalised) rows [row, row+n) to out_host */
MTGV_API int mtgv_bank_get_rows(const mtgv_bank* h, int64_t row, int64_t n, float* out_host);
/* q_dev: (b, dim) raw query vectors.  Writes ids (b,k) int64 (row index + id_base, -1 = none)
 * and scores (b,k) float32, sorted by score desc then id asc.  score_threshold is query_nearby's
 * (mtgvision/qdrant.py:83,93): hits scoring below it are dropped on the device (id -1 / score -inf, like a bank with
 * fewer than k rows); -INFINITY keeps everything, NaN is rejected. */
MTGV_API int mtgv_bank_topk(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, float score_threshold,
                            int64_t* ids_dev, float* scores_dev, void* stream);
/* Row labels (version 105): the payload filters and grouped queries of a vector store, kept on the device beside the rows.
 *   tags   uint64 bit set per row; what a bit means is the caller's business.  Default 0.
 *   group  int32 per row, >= 0, or -1 (the default): the row is its own group.
 * A bank whose labels were never set behaves as all-default and allocates nothing for them.  mtgv_bank_append gives new rows
 * the defaults, mtgv_bank_set_row keeps the row's labels (an upsert changes the vector, not the card), mtgv_bank_clear resets
 * them.  Labels are indexed by local row (id_base plays no part).  set: a null array leaves that label unchanged; rows
 * outside [0, size) and groups below -1 are refused.  get: a null array is not written. */
MTGV_API int mtgv_bank_set_labels(mtgv_bank* h, int64_t row0, int64_t n, const uint64_t* tags_host, const int32_t* groups_host, void* stream);
MTGV_API int mtgv_bank_get_labels(const mtgv_bank* h, int64_t row0, int64_t n, uint64_t* tags_host, int32_t* groups_host);
/* mtgv_bank_topk over labelled rows.  masks_dev: (b, 3) uint64 per query = (all_of, any_of, none_of), or NULL.  Row n is
 * eligible for query m when (tags[n] & all_of) == all_of, and any_of == 0 or (tags[n] & any_of) != 0, and
 * (tags[n] & none_of) == 0.  distinct != 0: among the eligible rows a group >= 0 is represented by its best row (score
 * desc, id asc) only - no two results share a non-negative group; rows of group -1 never suppress one another.  Order,
 * id_base and pads as mtgv_bank_topk; score_threshold is applied last (a representative below it becomes a pad, it is
 * not replaced by another row of its group).  Masks that admit no row are not an error: k pads.  The result is the
 * exact filtered / distinct top k.  With masks_dev == NULL and distinct == 0 the call IS mtgv_bank_topk (two-pass
 * pre-pass included); otherwise it always runs the one-pass exact kernel with the labelled epilogue, whatever b is.
 * Over a row-sharded bank the same answer comes from mtgv_bank_topk_packed_ex / mtgv_topk_merge_gathered_ex (below).
 * The first labelled call on a bank whose labels were never set allocates the label arrays and synchronises the device
 * once (so do mtgv_bank_set_labels and, on a labelled bank, mtgv_bank_clear): make it before capturing a stream. */
MTGV_API int mtgv_bank_topk_ex(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, float score_threshold,
                               const uint64_t* masks_dev, int32_t distinct, int64_t* ids_dev, float* scores_dev, void* stream);
/* Batches of >= 128 queries (dim % 64 == 0, k <= 4, F16X3 mode) are matched in two passes: approximate fp16 scores over a
 * hi-only copy of the bank, then an exact re-rank of the best candidates with a bound that proves no other row can enter
 * the top k; a query whose bound fails is scanned exactly, so the answer is always the exact top k.  count: how many
 * queries took that scan so far (banks with many near-duplicate rows); synchronises the device.  An all-zero query (every
 * score exactly 0, so no bound could hold) is answered directly with that scan's result - the k first rows at score 0 - and
 * is not counted (version 115; before, each took the scan of the whole bank and counted).  MTGV_MATCH_PREPASS=0 keeps to the
 * one-pass exact kernel. */
MTGV_API int mtgv_bank_prepass_fallbacks(const mtgv_bank* h, int64_t* count);
/* TEST SURFACE (version 118): the first pass of the two-pass match on its own - the queries' normalisation, their fp16
 * copy and the fp16 x fp16 launch that mtgv_bank_topk runs before the re-rank, same functions and arguments - with the
 * candidates in caller buffers.  cand_scores_dev / cand_cols_dev: [b][slots][per_range] float32 / int32 on the device;
 * range w covers the bank rows [w * range_cols, (w + 1) * range_cols) and reports its per_range best approximate scores
 * (score desc, row asc) with their rows; a range with fewer rows pads with (-inf, -1).  mtgv_bank_prepass_layout gives
 * slots, range_cols and per_range for the bank's current size (pure arithmetic, any bank).  Where mtgv_bank_topk would
 * not run the first pass whatever k is - F32 mode, b < 128, dim % 64 != 0, fewer than 4096 rows, no fp16 copy -
 * mtgv_bank_prepass_candidates returns status 1 with a message and writes nothing.  MTGV_MATCH_PREPASS plays no part. */
MTGV_API int mtgv_bank_prepass_layout(const mtgv_bank* h, int32_t* slots, int32_t* range_cols, int32_t* per_range);
MTGV_API int mtgv_bank_prepass_candidates(mtgv_bank* h, const float* q_dev, int32_t b, float* cand_scores_dev, int32_t* cand_cols_dev,
                                          int32_t* slots, int32_t* range_cols, void* stream);
/* merge ncand (score,id) candidates per query into the top k (multi-GPU shard merge); same threshold rule */
MTGV_API int mtgv_topk_merge(float* cand_scores_dev, const int64_t* cand_ids_dev, int32_t b, int32_t ncand, int32_t k,
                             float score_threshold, int64_t* ids_dev, float* scores_dev, void* stream);
/* The sharded match's exchange step without any arithmetic outside the library (mtgv/dist.py): the local
 * top-k of ALL ranks' queries over this rank's shard is written in the exchange format packed[b][k][2] int64 =
 * (global id or -1, float32 bit pattern of the score, zero-extended) - one buffer, so one all-gather carries ids and
 * scores; after the all-gather, gathered[n_ranks][b_total][k][2] is merged for this rank's own queries
 * [row0, row0 + b) (score desc, id asc; threshold rule as mtgv_bank_topk; n_ranks * k <= 4096).  Between the two calls
 * the caller issues only the collective (RCCL's own kernels). */
MTGV_API int mtgv_bank_topk_packed(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, int64_t* packed_dev,
                                   void* stream);
MTGV_API int mtgv_topk_merge_gathered(const int64_t* gathered_dev, int32_t n_ranks, int32_t b_total, int32_t k, int32_t row0, int32_t b,
                                      float score_threshold, int64_t* ids_dev, float* scores_dev, void* stream);
/* Row labels across the sharded exchange (version 108): mtgv_bank_topk_ex over a bank split by rows.  Group numbers are the
 * caller's and mean the same on every shard; the rows of one group may lie on several shards.
 *   mtgv_bank_topk_packed_ex   the labelled match (masks_dev, distinct as mtgv_bank_topk_ex; both absent: status 1) of ALL
 *     ranks' queries over this rank's shard - always the one-pass exact kernel; with distinct the shard's duplicates of a
 *     group are removed here already - written in the labelled exchange format packed[b][k][2] int64:
 *       word 0            global id (row + id_base), or -1
 *       word 1, low 32    float32 bit pattern of the score (as in the unlabelled format)
 *       word 1, high 32   the row's group as uint32 (group -1 = 0xFFFFFFFF)
 *     Pads are (id -1, -inf, group -1).  The message has the size of the unlabelled one, and mtgv_topk_merge_gathered reads
 *     it as it is (it takes the low half of word 1): a filter-only exchange needs no other merge.  No threshold here - it
 *     belongs to the merge.  An empty shard is not an error for this call: it writes b * k pads and returns 0, since a
 *     rank that failed would leave the others waiting in the collective.  (mtgv_bank_topk_packed keeps its zero high half
 *     and its error on an empty bank.)  The note on the first labelled call of mtgv_bank_topk_ex applies.
 *   mtgv_topk_merge_gathered_ex   distinct == 0: mtgv_topk_merge_gathered itself.  distinct != 0: gathered must be in the
 *     labelled format; the n_ranks * k candidates of a query are walked in order (score desc, global id asc), a picked
 *     candidate retires every other candidate of its non-negative group, the first k picks are the result, and the
 *     threshold is applied last (a representative below it becomes a pad and is not replaced).  n_ranks * k <= 4096.
 *     The result does not depend on the order of the ranks.
 * Together they return exactly what mtgv_bank_topk_ex returns over the whole bank, ids and score bits (DESIGN.md section
 * 6 has the argument).  Every rank must make the same choice of masks-or-not and of distinct.  masks_dev holds the masks
 * of all b queries, so with per-query filters the caller gathers them beside the queries (mtgv/dist.py). */
MTGV_API int mtgv_bank_topk_packed_ex(mtgv_bank* h, const float* q_dev, int32_t b, int32_t k, int64_t id_base, const uint64_t* masks_dev,
                                      int32_t distinct, int64_t* packed_dev, void* stream);
MTGV_API int mtgv_topk_merge_gathered_ex(const int64_t* gathered_dev, int32_t n_ranks, int32_t b_total, int32_t k, int32_t row0, int32_t b,
                                         float score_threshold, int32_t distinct, int64_t* ids_dev, float* scores_dev, void* stream);

/* ------------------------------------------------------------------------- */
/* Detector: YOLOv8 / 11 / 12 at scales n, s, m, -seg (forward + decode + NMS */
/* + mask logits) or -obb (forward + rotated decode + rotated NMS).           */
/* Replaces CardSegmenter.__call__ -> ultralytics YOLO predict                */
/* (mtgvision/od_export.py:141-160; model built in od_train.py:46-70).        */
/* ------------------------------------------------------------------------- */
typedef struct mtgv_detector mtgv_detector;

typedef struct {
  int32_t nc;        /* classes (3: od_train.py:46-50) */
  int32_t imgsz;     /* 640 */
  int32_t max_batch;
  float conf;        /* 0.25 */
  float iou;         /* 0.7 */
  int32_t max_det;   /* 300 */
  int32_t arch;      /* 0 or 8: YOLOv8; 11: YOLO11 (C3k2, C2PSA, depthwise class branch; od_train.py:20); 12 (version 109): YOLO12 -
                      * YOLO11's scale table, C3k2 and class branch, a backbone without SPPF and C2PSA whose nodes 6 and 8 are
                      * A2C2f blocks (four ABlocks each at n, s, m: area attention over 4 areas at P4 and 1 at P5, heads of 32
                      * channels, a depthwise 7x7 positional encoding, a 2-layer MLP of ratio 2), A2C2f without attention (C3k
                      * inside) in the neck, the head at node 21 on nodes 14, 17, 20.  Recalled from ultralytics 8.3.x and
                      * unpinned like the rest of the detector (least certain: the MLP ratio at scale m); a checkpoint that
                      * disagrees fails in mtgv_detector_set_param on the element count (status 1).  Anything else: status 2. */
  int32_t task;      /* 0: segment head (-seg); 1: OBB head (-obb, what od_train.py:19, :101 builds by default): no prototypes,
                      * one angle logit per anchor, rotated NMS.  (Added in version 101: the struct grew by this field.) */
  int32_t in_h, in_w; /* the input rectangle (added in version 102: the struct grew by these two fields).  Both 0: imgsz x imgsz.
                      * Otherwise each a multiple of 32 in [32, imgsz] (anything else: status 1) - what ultralytics'
                      * LetterBox(auto=True) feeds a .pt checkpoint: 480 x 640 for a webcam frame, 384 x 640 for 720p.  On such a
                      * handle anchors keep their order (P3's pixels row-major, then P4's, then P5's) with
                      * na = sum over s = 8, 16, 32 of (in_h / s)(in_w / s); boxes and rboxes are pixels of the in_h x in_w frame;
                      * mask_logits is (n, mask_rows, in_h / 4, in_w / 4); mtgv_detector_raw and mtgv_detector_flops follow. */
  int32_t scale;     /* the model size, od_train.py's --size (added in version 103: the struct grew by this field).  0: n (what a
                      * zero-initialised caller gets), 1: s, 2: m run on the GPU.  3 (l) and 4 (x) return status 2 with a message
                      * naming the scales that run: the library's 1e-4 contract cannot be tested at those widths yet.  Anything
                      * else: status 1.  (depth, width, max channels), recalled from ultralytics 8.3.x and unpinned like the rest
                      * of the detector: YOLOv8 n (.33, .25, 1024), s (.33, .50, 1024), m (.67, .75, 768); YOLO11 n (.50, .25,
                      * 1024), s (.50, .50, 1024), m (.50, 1.0, 512) with c3k = True in every C3k2.  Only layer widths and
                      * repeats change with the scale.  The anchors and what every anchor carries do not - 4 x 16 box bins, 32
                      * mask coefficients or one angle, nc classes - so mtgv_detector_raw and the mask stage keep their shapes;
                      * mtgv_detector_flops reports the scale's own count.  A state_dict of another scale fails in
                      * mtgv_detector_set_param on the element count (status 1). */
} mtgv_detector_cfg;
#define MTGV_TASK_SEGMENT 0
#define MTGV_TASK_OBB 1

MTGV_API int mtgv_detector_create(const mtgv_detector_cfg* cfg, mtgv_detector** out);
MTGV_API void mtgv_detector_destroy(mtgv_detector* h);
/* parameter by ultralytics state_dict key ("model.0.conv.weight", "model.0.bn.running_var", ...) */
MTGV_API int mtgv_detector_set_param(mtgv_detector* h, const char* key, const float* data_host, int64_t numel);
MTGV_API int mtgv_detector_missing_params(const mtgv_detector* h);
/* fold BatchNorm into the conv weights and repack; call once after all params are set */
MTGV_API int mtgv_detector_finalize(mtgv_detector* h);
/* frames_dev: (n, in_h, in_w, 3) uint8 (imgsz x imgsz unless the cfg names a rectangle), already letterboxed, 8-byte
 * aligned; flip_rgb reverses the channel order first (ultralytics treats ndarray input as BGR).
 * Outputs (device): n_det (n) int32; per frame up to max_det rows of
 *   boxes (n, max_det, 4) xyxy pixels, conf (n, max_det), cls (n, max_det) int32,
 *   keep_idx (n, max_det) int32 anchor index in [0, na) (8400 at 640 x 640),
 *   mask_logits (n, mask_rows, in_h / 4, in_w / 4) (160 x 160 at 640 x 640): coeffs @ protos cropped to the box (process_mask before
 *   the upsample) for the first min(n_det, mask_rows) detections of each frame; rows beyond
 *   n_det are left untouched; NULL skips the mask stage. */
MTGV_API int mtgv_detector_forward(mtgv_detector* h, const uint8_t* frames_dev, int32_t n, int32_t flip_rgb,
                                   int32_t* n_det_dev, float* boxes_dev, float* conf_dev, int32_t* cls_dev,
                                   int32_t* keep_idx_dev, float* mask_logits_dev, int32_t mask_rows, void* stream);
/* The forward of an OBB handle (task 1; mtgv_detector_forward on it, or this call on a segment handle, returns status 1):
 * backbone, neck and head as above without the prototype branch, then the OBB decode
 *   angle = (sigmoid(logit) - 0.25) pi;  xf = (r - l) / 2, yf = (b - t) / 2 from the DFL distances l, t, r, b;
 *   x = (xf cos(angle) - yf sin(angle) + ax) stride, y = (xf sin(angle) + yf cos(angle) + ay) stride,
 *   w = (l + r) stride, h = (t + b) stride
 * and mtgv_nms_rotated on the result (class-aware, max_wh 7680).  Outputs as above with rboxes (n, max_det, 5) =
 * x, y, w, h in pixels and the angle in radians, in place of boxes; there is no mask stage.  The arithmetic is
 * ultralytics 8.3.x's as recalled (OBB.forward, dist2rbox): unpinned, like the rest of the detector. */
MTGV_API int mtgv_detector_forward_obb(mtgv_detector* h, const uint8_t* frames_dev, int32_t n, int32_t flip_rgb, int32_t* n_det_dev,
                                       float* rboxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev, void* stream);
/* raw head outputs of the last forward: pred (n, 4+nc+32, na) and protos (n, 32, in_h / 4, in_w / 4) (8400 and 160 x 160
 * at 640 x 640); on an OBB handle pred (n, 4+nc+1, na) = xywh, class scores, angle, and protos_dev must be NULL */
MTGV_API int mtgv_detector_raw(mtgv_detector* h, int32_t n, float* pred_dev, float* protos_dev, void* stream);
MTGV_API int mtgv_detector_flops(const mtgv_detector* h, double* flops_per_frame);
/* The forward's internal fork-join (the prototype branch and the P3 / P4 head branches on library-owned streams, see the
 * concurrency contract above): mode 1 on, 0 off (every launch on the caller's stream), -1 the default - on unless the
 * environment says MTGV_DET_FORK=0.  A caller that already overlaps the detector with other work on a second stream turns it
 * off (mtgv.Pipeline.run_many does: branch streams share the runtime's few hardware queues with the caller's other streams,
 * and a long event wait queued in one of them holds up whatever shares it; od_export.py:147-150 has no counterpart). */
MTGV_API int mtgv_detector_set_fork(mtgv_detector* h, int32_t mode);
/* process_mask tail: bilinear x`scale` upsample (align_corners=False) of (n, mh, mw) logits, then > 0
 * -> (n, mh*scale, mw*scale) uint8 {0,1} */
MTGV_API int mtgv_mask_binarize(const float* logits_dev, int32_t n, int32_t mh, int32_t mw, int32_t scale, uint8_t* out_dev,
                                void* stream);

/* NMS alone on decoded predictions pred (n, 4+nc+nm, na) [xywh, class scores, coeffs] */
MTGV_API int mtgv_nms(const float* pred_dev, int32_t n, int32_t nc, int32_t nm, int32_t na, float conf, float iou,
                      int32_t max_det, float max_wh, int32_t* n_det_dev, float* boxes_dev, float* conf_dev, int32_t* cls_dev,
                      int32_t* keep_idx_dev, int32_t* workspace_dev, size_t workspace_bytes, void* stream);
MTGV_API size_t mtgv_nms_workspace_bytes(int32_t n, int32_t na);

/* Rotated NMS alone on OBB predictions pred (n, 4+nc+1, na) [xywh, class scores, angle]
 * (ultralytics 8.3.x non_max_suppression(rotated=True) -> nms_rotated, as recalled: unpinned).  Candidates: best class
 * score > conf, ordered score descending then anchor ascending; x and y get cls * max_wh added.  The rule is not the
 * greedy sweep: candidate j is kept iff no candidate i < j of that order has probiou(i, j) >= iou, whether or not i was
 * itself dropped; the first max_det kept are reported.  rboxes_dev (n, max_det, 5), conf_dev and keep_idx_dev are copies of
 * pred's values; slots beyond n_det are zeros.  iou > 0 and max_wh >= 7680; box sides <= 1024 px and centres within
 * [-512, 1536] (pairs of different classes are skipped on that ground).  One workgroup per image, all pairs of a class:
 * measured 0.7 ms at 900 candidates, 32 ms at 8400 dissimilar ones of one class (profiles/README.md). */
MTGV_API size_t mtgv_nms_rotated_workspace_bytes(int32_t n, int32_t na);
MTGV_API int mtgv_nms_rotated(const float* pred_dev, int32_t n, int32_t nc, int32_t na, float conf, float iou, int32_t max_det, float max_wh,
                              int32_t* n_det_dev, float* rboxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev,
                              int32_t* workspace_dev, size_t workspace_bytes, void* stream);
/* Test surface of the pair function of mtgv_nms_rotated (the same device function): ProbIoU of boxes a[i] and b[i],
 * (m, 5) x, y, w, h, angle each -> out (m).  With A = w^2/12, B = h^2/12: a = A cos^2 + B sin^2, b = A sin^2 + B cos^2,
 * c = (A - B) cos sin per box; D = (a1+a2)(b1+b2) - (c1+c2)^2; bd = clamp(t1 + t2 + t3, eps, 100) with
 * t1 = ((a1+a2)(y1-y2)^2 + (b1+b2)(x1-x2)^2) / (D + eps) / 4, t2 = (c1+c2)(x2-x1)(y1-y2) / (D + eps) / 2,
 * t3 = log(D / (4 sqrt(max(a1 b1 - c1^2, 0) max(a2 b2 - c2^2, 0)) + eps) + eps) / 2; probiou = 1 - sqrt(1 - exp(-bd) + eps);
 * eps = 1e-7, float32 throughout. */
MTGV_API int mtgv_op_probiou(const float* a_dev, const float* b_dev, int64_t m, float* out_dev, void* stream);

/* Test surface of the segment head's tail.  Raw head rows of the three pyramid levels (strides 8 / 16 / 32) of an h x w
 * input, per level (n, (h / stride)(w / stride), ct) floats, 16-byte aligned: 4 sides x 16 box bins at [0, 64), class logits
 * at [cls, cls + nc), mask coefficients at [coef, coef + nm); ct, cls and coef multiples of 4.  Anchors count P3's pixels
 * first (row-major), then P4's, then P5's: na = sum of (h / stride)(w / stride).  h = w = 0: the square imgsz x imgsz input;
 * otherwise both multiples of 32 (added in version 102: the struct grew by these two fields). */
typedef struct mtgv_head_rows {
  const float *r0, *r1, *r2;
  int32_t imgsz, ct, cls, coef;
  int32_t h, w;
} mtgv_head_rows;
/* the detector's decode pass: rows -> pred (n, 4+nc+nm, na) */
MTGV_API int mtgv_op_decode(const mtgv_head_rows* rows, int32_t n, int32_t nc, int32_t nm, float* pred_dev, void* stream);
/* NMS straight from the rows (what the detector's forward runs): bit-identical to mtgv_op_decode -> mtgv_nms; the boxes of
 * candidates only are decoded.  coef_dev (n, max_det, nm) may be null: the kept detections' coefficients, zeros beyond n_det */
MTGV_API int mtgv_op_nms_raw(const mtgv_head_rows* rows, int32_t n, int32_t nc, int32_t nm, float conf, float iou, int32_t max_det,
                             float max_wh, int32_t* n_det_dev, float* boxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev,
                             float* coef_dev, int32_t* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Mask -> oriented card quad.                                                */
/* Replaces the host geometry of InstanceSeg._orient                          */
/* (mtgvision/od_export.py:52-93: close the U-shaped mask, four corners,      */
/* corner 0 = the card's top-left).                                           */
/* ------------------------------------------------------------------------- */
/* masks_dev (n, h, w) uint8, non-zero = foreground (mtgv_mask_binarize output); boxes_dev (n, 4) xyxy float32 or NULL:
 * the quad reported for an empty mask.  quads_dev (n, 4, 2) float32 corners (x, y) in pixels of the mask grid, ordered
 * top-left, top-right, bottom-right, bottom-left of the card; ok_dev (n) int32: 1 = from the mask, 0 = empty mask.
 * The quad is the general quadrilateral cv2.approxPolyN(hull, 4) fits (od_export.py:72-74): the convex hull of the mask's
 * row extents, greedily contracted edge by edge (the edge whose removal adds the least area is replaced by the
 * intersection of its neighbours, first minimum wins) until four vertices remain - vertices may therefore lie outside
 * the mask, or outside the image; coordinates are truncated toward zero as the reference's astype(int) does.  "Up" is
 * mask centroid minus hull centroid: the ray from the quad's centre along it picks the card's top edge.  Fallbacks: a
 * hull of fewer than four vertices (point, line, triangle) reports the mask's bounding box; an empty mask reports
 * boxes_dev[n] (or zeros) with ok = 0. */
/* extents_dev: NULL, or (n, h, 2) int32 that receives every mask row's leftmost and rightmost foreground column (-1, -1 for
 * an empty row): the outline of the mask as the host needs it for `InstanceSeg.points` (od_export.py:152-153), 2 h
 * integers per card instead of the h x w mask. */
MTGV_API int mtgv_mask_quads(const uint8_t* masks_dev, int32_t n, int32_t h, int32_t w, const float* boxes_dev, float* quads_dev,
                             int32_t* ok_dev, int32_t* extents_dev, void* stream);
/* the same from the cropped mask logits (n, mh, mw) of the detector: a pixel of the (mh*scale, mw*scale) mask is foreground
 * where the bilinear interpolation of the logits is > 0 (what mtgv_mask_binarize writes) - the full-resolution mask is
 * never materialised.  Identical quads to mtgv_mask_binarize + mtgv_mask_quads. */
MTGV_API int mtgv_mask_quads_logits(const float* logits_dev, int32_t n, int32_t mh, int32_t mw, int32_t scale,
                                    const float* boxes_dev, float* quads_dev, int32_t* ok_dev, int32_t* extents_dev, void* stream);

/* Mask -> contour points: ultralytics `masks.xy` (ops.masks2segments behind od_export.py:152-153:
 * cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per mask), added in version 107.  unpinned: cv2 / ultralytics absent -
 * the specification is the host function mtgv.adapters._mask_segments, which the kernel reproduces point for point:
 *   - foreground: masks_dev (n, h, w) uint8 != 0.  Pixels outside the image are background.
 *   - blobs are 8-connected and numbered in raster order of their first pixel (scipy.ndimage.label, 3 x 3 structure); a blob
 *     inside another blob's hole is a blob of its own, holes are not reported.
 *   - one blob's trace starts at the leftmost pixel of its top row with back = 0; neighbour order W, NW, N, NE, E, SE, S, SW;
 *     from cur, the first set neighbour d in the order back, back + 1, ... (mod 8) becomes cur and back = (d + 5) % 8; the walk
 *     stops as soon as cur is the start pixel again, from whatever direction, or when no neighbour is set.  That rule cuts
 *     some shapes short - of an inverted V only the apex and one arm are visited - and the kernel cuts them the same way.
 *   - CHAIN_APPROX_SIMPLE: on the closed chain point i is kept iff p[i] - p[i-1] != p[i+1] - p[i] (cyclic); chains of at most
 *     two points are kept whole; trace order is preserved.
 *   - strategy 0 ("all"): the blobs' chains concatenated in blob order; 1 ("largest"): the chain with the most kept points,
 *     the first of equals.
 * points_dev (n, max_points, 2) int32 receives (x, y) in mask pixels, n_points_dev (n) the number written, n_blobs_dev (n) or
 * NULL the number of blobs, status_dev (n): 0 ok, 1 over a cap - more than max_points points (n_points = max_points, the
 * first max_points of the result are written), more than 4096 row runs or more than 1024 blobs in the mask (n_points = 0).
 * Nothing is written outside a mask's own slot, slots behind n_points are left as they were; an empty mask has 0 points,
 * 0 blobs, status 0.  One workgroup per mask with the mask as a bit image in LDS; every loop is bounded before it starts (a
 * trace by 8 x the mask's foreground pixels).  Deterministic: no atomic decides a position.  workspace_dev: at least
 * mtgv_mask_contours_workspace_bytes(n, h, w, max_points) bytes, 16-byte aligned.  Status 1 ("mask_contours: ...", checked
 * before any device call): n, h, w or max_points < 1, an unknown strategy, a mask too large for LDS (640 x 640 fits), a short
 * workspace, scale < 1.  Asynchronous on `stream`; library kernels only. */
MTGV_API size_t mtgv_mask_contours_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t max_points);
MTGV_API int mtgv_mask_contours(const uint8_t* masks_dev, int32_t n, int32_t h, int32_t w, int32_t strategy, int32_t max_points,
                                int32_t* points_dev, int32_t* n_points_dev, int32_t* n_blobs_dev, int32_t* status_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream);
/* the same from the cropped mask logits (n, mh, mw): foreground is what mtgv_mask_binarize writes for them (bilinear x`scale`,
 * align_corners = False, > 0); the (mh*scale, mw*scale) mask is never materialised (workspace: h = mh*scale, w = mw*scale).
 * Identical points to mtgv_mask_binarize + mtgv_mask_contours. */
MTGV_API int mtgv_mask_contours_logits(const float* logits_dev, int32_t n, int32_t mh, int32_t mw, int32_t scale, int32_t strategy,
                                       int32_t max_points, int32_t* points_dev, int32_t* n_points_dev, int32_t* n_blobs_dev,
                                       int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The K cards of every frame that go on to the crop stage: the K highest-confidence detections of the padded
 * mtgv_detector_forward outputs (n_det (frames), boxes (frames, max_det, 4), score-descending) or, where a frame has
 * fewer, pad_boxes_dev[k] (k, 4).  Writes sel_boxes_dev (frames*k, 4) xyxy, frame_idx_dev (frames*k) and, unless null,
 * quads_dev (frames*k, 4, 2): the boxes' corners in the order mtgv_warp_quads expects.  The glue between
 * `results.boxes` and `extract_dewarped` (mtgvision/od_export.py:152-160, server.py:139-183), batched. */
MTGV_API int mtgv_select_cards(const int32_t* n_det_dev, const float* boxes_dev, const float* pad_boxes_dev, int32_t frames,
                               int32_t max_det, int32_t k, float* sel_boxes_dev, float* quads_dev, int32_t* frame_idx_dev,
                               void* stream);

/* The OBB counterpart: the K cards of every frame from mtgv_detector_forward_obb's outputs (n_det (frames), rboxes
 * (frames, max_det, 5), conf, cls (frames, max_det), score-descending), as oriented quads.  Slot k of a frame is its k-th
 * detection of class card_cls, or pad_boxes_dev[k] where the frame has fewer.  The reference labels card, card_top and
 * card_bottom regions (od_datasets.py:244-257) "so we can compute this later" and never does; the rule is this library's:
 * h := the long side (w > h: swap, angle += pi/2), u = (-sin, cos) the long axis, v = (cos, sin); the first top_cls
 * detection in score order whose centre p lies inside the card (|d.v| <= w/2, |d.u| <= h/2, d = p - centre), accepted if
 * d.u != 0, gives up U = sign(d.u) u; otherwise a bottom_cls detection likewise gives U = -sign(d.u) u; otherwise U is
 * whichever of +-u has negative y (negative x when u.y == 0).  top_cls / bottom_cls = -1: class not used.  With
 * R = (-U.y, U.x) the corners are centre +- U h/2 +- R w/2 in the order mtgv_warp_quads expects (TL, TR, BR, BL).
 * Writes quads_dev (frames*k, 4, 2), sel_boxes_dev (frames*k, 4) the quads' axis-aligned bounds (the pad box itself for a
 * pad), frame_idx_dev (frames*k) and state_dev (frames*k) int32: 0 pad, 1 unoriented, 2 oriented. */
MTGV_API int mtgv_obb_cards(const int32_t* n_det_dev, const float* rboxes_dev, const float* conf_dev, const int32_t* cls_dev,
                            const float* pad_boxes_dev, int32_t frames, int32_t max_det, int32_t k, int32_t card_cls, int32_t top_cls,
                            int32_t bottom_cls, float* quads_dev, float* sel_boxes_dev, int32_t* frame_idx_dev, int32_t* state_dev,
                            void* stream);

/* ------------------------------------------------------------------------- */
/* Crop: perspective de-warp of card quads.                                   */
/* Replaces InstanceSeg.extract_dewarped (mtgvision/od_export.py:95-111).     */
/* ------------------------------------------------------------------------- */
/* frames_dev (nf, fh, fw, 3) uint8; quads_dev (nq, 4, 2) float32 source corners (x,y) in the
 * order dst corners [[0,0],[w,0],[w,h],[0,h]] are matched to; frame_idx_dev (nq) int32.
 * out_dev (nq, out_h, out_w, 3) uint8.  workspace_dev: mtgv_warp_workspace_bytes(nq) bytes. */
MTGV_API size_t mtgv_warp_workspace_bytes(int32_t nq);
MTGV_API int mtgv_warp_quads(const uint8_t* frames_dev, int32_t nf, int32_t fh, int32_t fw, const float* quads_dev,
                             const int32_t* frame_idx_dev, int32_t nq, int32_t out_h, int32_t out_w, double expand_ratio,
                             uint8_t* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same from source frames of their own sizes (mtgv_version >= 111): the crops are sampled from the frames the camera
 * delivered, not from their letterboxed copies.  src_dev: nf uint8 HWC RGB frames back to back, offsets_dev (nf) int64 byte
 * offset of each (any alignment), hw_dev (nf, 2) int32 height, width - the ragged layout of mtgv_make_cropped - plus
 * geo_dev (nf, 4) int32 = nh, nw, top, left and ratio_dev (nf) float64: each frame's letterbox into the detector's input
 * (mtgv.detector.fit_geometry; only top, left and the ratio are read here).  quads_dev (nq, 4, 2) float32 are pixels of
 * that input; quads_src_dev (nq, 4, 2) float32 receives every corner in the pixels of its own frame, in float64
 * x = (x_det - left) / ratio clipped to [0, w], y = (y_det - top) / ratio clipped to [0, h], rounded to float32
 * (ultralytics' scale_coords + clip_coords, mtgv.adapters: to_frame).  The homographies are solved from quads_src and each
 * crop is sampled from frame frame_idx_dev[q] with mtgv_warp_quads' arithmetic: for frames of one size the crops equal
 * mtgv_warp_quads(src, quads_src) bit for bit.  No byte outside a frame's own h * w * 3 is read.  A frame index outside
 * [0, nf) or a frame with h or w <= 0 gives a crop of zeros.  The caller guarantees offsets[i] + h * w * 3 <= the buffer. */
MTGV_API int mtgv_warp_quads_src(const uint8_t* src_dev, const int64_t* offsets_dev, const int32_t* hw_dev, const int32_t* geo_dev,
                                 const double* ratio_dev, int32_t nf, const float* quads_dev, const int32_t* frame_idx_dev, int32_t nq,
                                 int32_t out_h, int32_t out_w, double expand_ratio, uint8_t* out_dev, float* quads_src_dev,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Bank build: card image -> encoder input.                */
/* Replaces SyntheticBgFgMtgImages.make_cropped (mtgvision/encoder_datasets.py:733-753) */
/* as used by qdrant_populate.CardProcessor._get_card_point (qdrant_populate.py:84-90). */
/* ------------------------------------------------------------------------- */
/* images_dev: n uint8 HWC images of arbitrary sizes back to back; offsets_dev (n) byte offset of each;
 * hw_dev (n,2) int32 height,width.  Strips ceil(max(0.02 H, 0.02 W)) border pixels, area-resizes to
 * (out_h, out_w), clips: out_dev (n, out_h, out_w, 3) float32 in [0,1] (feed with MTGV_IN_NHWC_F32). */
MTGV_API int mtgv_make_cropped(const uint8_t* images_dev, const int64_t* offsets_dev, const int32_t* hw_dev, int32_t n,
                               int32_t out_h, int32_t out_w, float* out_dev, void* stream);

/* ultralytics LetterBox in front of the detector (behind CardSegmenter.__call__, mtgvision/od_export.py:147-150): the (h, w, 3)
 * uint8 frame at src_dev resampled bilinearly (align_corners = false form) to (nh, nw), placed at (top, left) of the
 * size x size x 3 uint8 image at dst_dev, the rest filled with pad_value (114 upstream).  The caller computes the geometry
 * (mtgv.detector.letterbox_geometry: r = min(size / h, size / w), nh = round(h r), ...). */
MTGV_API int mtgv_letterbox_u8(const uint8_t* src_dev, int32_t h, int32_t w, uint8_t* dst_dev, int32_t size, int32_t nh, int32_t nw,
                               int32_t top, int32_t left, int32_t pad_value, void* stream);
/* the same into a (dst_h, dst_w, 3) image, for n same-sized frames in one launch: src_dev (n, h, w, 3), dst_dev
 * (n, dst_h, dst_w, 3).  With mtgv.detector.rect_geometry this is LetterBox(auto=True), what ultralytics runs in front of a
 * .pt checkpoint: the pad only reaches the next multiple of the stride.  The resample arithmetic is mtgv_letterbox_u8's (which
 * is the n = 1, dst_h = dst_w case of the same kernel); a frame with (nh, nw) == (h, w) is copied exactly. */
MTGV_API int mtgv_letterbox_rect_u8(const uint8_t* src_dev, int32_t n, int32_t h, int32_t w, uint8_t* dst_dev, int32_t dst_h, int32_t dst_w,
                                    int32_t nh, int32_t nw, int32_t top, int32_t left, int32_t pad_value, void* stream);
/* the same for n frames of different sizes in one launch (mtgv_version >= 111): src_dev, offsets_dev (n) int64, hw_dev (n, 2)
 * int32 as for mtgv_make_cropped, geo_dev (n, 4) int32 = nh, nw, top, left of each frame (the host computes them:
 * mtgv.detector.fit_geometry).  Frame i goes to dst_dev[i] of (n, dst_h, dst_w, 3), pad included; byte for byte what
 * mtgv_letterbox_rect_u8 writes frame by frame.  The arrays live on the device and are not validated by the host: whatever
 * geo_dev holds, source positions are clamped into the frame and writes stay inside dst_dev[i]; a frame with h or w <= 0 is
 * all pad.  The caller guarantees offsets[i] + h * w * 3 <= the buffer. */
MTGV_API int mtgv_letterbox_ragged_u8(const uint8_t* src_dev, const int64_t* offsets_dev, const int32_t* hw_dev, const int32_t* geo_dev,
                                      int32_t n, uint8_t* dst_dev, int32_t dst_h, int32_t dst_w, int32_t pad_value, void* stream);
/* Tiled detection, the cut (mtgv_version >= 117): nt windows of the nf ragged frames, each letterboxed into its own
 * detector input, in one launch.  tiles_dev (nt, 5) int32 = frame, y0, x0, wh, ww (frame pixels), geo_dev (nt, 4) int32 =
 * nh, nw, top, left of each window's fit into (dst_h, dst_w) (mtgv.detector.fit_geometry(wh, ww, dst_h, dst_w)).  Output
 * pixel (y, x) of dst_dev[t] is what mtgv_letterbox_ragged_u8 writes for a contiguous copy of the window - the same float32
 * resample, the window's rows read w * 3 bytes apart in place; a window of the input's size is copied exactly.  The tables
 * are not validated by the host: a window is clamped into its frame, a frame index outside [0, nf) or an empty window is
 * all pad, writes stay inside dst_dev[t] and no byte outside a frame's own h * w * 3 is read.  nt <= 65535. */
MTGV_API int mtgv_letterbox_tiles_u8(const uint8_t* src_dev, const int64_t* offsets_dev, const int32_t* hw_dev, int32_t nf,
                                     const int32_t* tiles_dev, const int32_t* geo_dev, int32_t nt, uint8_t* dst_dev, int32_t dst_h, int32_t dst_w,
                                     int32_t pad_value, void* stream);
/* Tiled detection, the merge (mtgv_version >= 117): per-tile detector outputs -> the k cards of every frame in camera pixels
 * ("Tiled detection"; mtgv/tiles.py: merge_tiles_host is the rule in numpy, matched bit for bit).
 * n_det_dev (nt), boxes_dev (nt, max_det, 4) xyxy in the pixels of each tile's detector input, score-descending, conf_dev
 * (nt, max_det): mtgv_detector_forward's outputs with the tiles as frames.  quads_dev (nt * kt, 4, 2): the quads of the first
 * kt detections per tile (mtgv_mask_quads_logits), or NULL: the boxes' corners (TL, TR, BR, BL).  tiles_dev, geo_dev as for
 * mtgv_letterbox_tiles_u8, ratio_dev (nt) float64; tile_start_dev (frames + 1) int32: frame f owns tiles
 * [tile_start[f], tile_start[f + 1]); hw_dev (frames, 2) int32; pad_frac_dev (k, 4) float32.
 *   candidates  detection j < min(n_det[t], kt) of tile t
 *   mapping     float64 x = (x_det - left) / ratio + x0 clipped to [x0, x0 + ww], y likewise, rounded to float32
 *   cut rule    a window side that is no side of the frame is an inner side; dropped if bx0 < x0 + edge, bx1 > x0 + ww - edge
 *               (or the same in y) at an inner side, in float32
 *   order       conf descending, tile ascending, j ascending
 *   greedy      dropped if inter > ios_thr * min(area_a, area_b) against an earlier kept one (float32, strict)
 *   slots       the first k kept fill slots 0 .. n_sel - 1; slot >= n_sel is pad_frac[slot] * (w, h, w, h), conf 0, src_slot -1
 * Writes sel_boxes_src_dev (frames * k, 4), quads_src_dev (frames * k, 4, 2), frame_idx_dev, sel_conf_dev, src_slot_dev
 * (frames * k; t * kt + j) and n_sel_dev (frames).  Caps, checked from the arguments before anything touches a device
 * (status 1 with the numbers): k <= 64, kt <= max_det, frames <= 65535, max_tiles_per_frame * kt <= 1024.  The kernel
 * trusts tile_start no further than max_tiles_per_frame: a frame whose range is longer, negative or outside [0, nt] gets
 * n_sel = 0 and pads. */
MTGV_API int mtgv_tiles_merge(const int32_t* n_det_dev, const float* boxes_dev, const float* conf_dev, const float* quads_dev, int32_t nt,
                              int32_t max_det, int32_t kt, const int32_t* tiles_dev, const int32_t* geo_dev, const double* ratio_dev,
                              const int32_t* tile_start_dev, const int32_t* hw_dev, int32_t frames, int32_t max_tiles_per_frame,
                              const float* pad_frac_dev, int32_t k, float edge, float ios_thr, float* sel_boxes_src_dev, float* quads_src_dev,
                              int32_t* frame_idx_dev, float* sel_conf_dev, int32_t* src_slot_dev, int32_t* n_sel_dev, void* stream);
/* Tiled detection, the rotated merge (mtgv_version >= 119): the same for an OBB detector's oriented quads (DESIGN.md section 4,
 * "Tiled detection"; mtgv/tiles.py: merge_tiles_obb_host and quad_inter_host are the rule in numpy, matched bit for bit).
 * n_det_dev (nt), conf_dev, cls_dev (nt, max_det): mtgv_detector_forward's outputs with the tiles as frames; quads_dev
 * (nt * kt, 4, 2), state_dev (nt * kt): mtgv_obb_cards' outputs for them with k = kt.  The tables as for mtgv_tiles_merge.
 *   candidates  slot j < kt of tile t iff state[t * kt + j] is 1 or 2 and the tile has a j-th detection of class card_cls
 *               among its first min(max(n_det[t], 0), max_det); its confidence is that detection's
 *   mapping     every corner as in mtgv_tiles_merge; bounds = min / max of the mapped corners (float32 comparisons)
 *   cut rule    mtgv_tiles_merge's, on those bounds
 *   order       conf descending, tile ascending, j ascending
 *   greedy      b is dropped by an earlier kept a if inter > ios_thr * min(area_a, area_b) (float32, strict): area = half the
 *               absolute shoelace sum, inter = the area of intersection of the two convex quads, both with coordinates
 *               relative to a's corner 0; inter = 0 where the bounds do not overlap; a quad of zero area neither drops nor is
 *               dropped.  inter sums cross(p', q') over the parts of a's edges inside b (closed; an edge along an edge of b
 *               counts iff both run the same way) and of b's edges inside a (open), halved and clamped at 0
 *   orientation a kept a of state 1 takes the first candidate of the order that it dropped and that has state 2 as donor:
 *               u = (TL + TR) - (BR + BL), d = ua.x * ub.x + ua.y * ub.y; d != 0: state 2, oriented_by = the donor's slot;
 *               d < 0: a's corners are rolled by two
 *   slots       as for mtgv_tiles_merge; sel_boxes_src = the quad's bounds; a pad has state 0, oriented_by -1
 * Writes mtgv_tiles_merge's outputs plus state_out_dev and oriented_by_dev (frames * k) int32.  The same caps and the same
 * distrust of tile_start; a state outside {1, 2} is no candidate. */
MTGV_API int mtgv_tiles_merge_obb(const int32_t* n_det_dev, const float* conf_dev, const int32_t* cls_dev, const float* quads_dev,
                                  const int32_t* state_dev, int32_t nt, int32_t max_det, int32_t kt, const int32_t* tiles_dev,
                                  const int32_t* geo_dev, const double* ratio_dev, const int32_t* tile_start_dev, const int32_t* hw_dev,
                                  int32_t frames, int32_t max_tiles_per_frame, const float* pad_frac_dev, int32_t k, float edge, float ios_thr,
                                  int32_t card_cls, float* sel_boxes_src_dev, float* quads_src_dev, int32_t* frame_idx_dev, float* sel_conf_dev,
                                  int32_t* src_slot_dev, int32_t* n_sel_dev, int32_t* state_out_dev, int32_t* oriented_by_dev, void* stream);
/* test surface (mtgv_version >= 119): the pair function of mtgv_tiles_merge_obb on m pairs of quads a_dev, b_dev (m, 4, 2)
 * -> inter_dev, area_a_dev, area_b_dev (m) float32; the same device functions (mtgv/tiles.py: quad_inter_host) */
MTGV_API int mtgv_op_quad_inter(const float* a_dev, const float* b_dev, int64_t m, float* inter_dev, float* area_a_dev, float* area_b_dev,
                                void* stream);
/* fills the pad of n letterboxed (size, size, 3) uint8 frames with pad_value: every pixel outside the (nh, nw) rectangle
 * at (top, left), which someone else writes (mtgv.jpeg.JpegDecoder.decode_frames decodes a frame that already fits
 * straight into it) */
MTGV_API int mtgv_letterbox_pad_u8(uint8_t* frames_dev, int32_t n, int32_t size, int32_t nh, int32_t nw, int32_t top, int32_t left,
                                   int32_t pad_value, void* stream);
/* the same for (dst_h, dst_w, 3) frames (mtgv_letterbox_pad_u8 is its dst_h = dst_w case) */
MTGV_API int mtgv_letterbox_pad_rect_u8(uint8_t* frames_dev, int32_t n, int32_t dst_h, int32_t dst_w, int32_t nh, int32_t nw, int32_t top,
                                        int32_t left, int32_t pad_value, void* stream);

/* ------------------------------------------------------------------------- */
/* JPEG decode: the frames of mtgvision/server.py:272-280 (cv2.imdecode on the host) and the */
/* card scans of qdrant_populate.py:70-90 go from compressed bytes to RGB on the GPU.                            */
/* Baseline sequential Huffman 8-bit (SOF0 / SOF1); 1 component (returned as RGB, the channel replicated) or      */
/* YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; restart intervals; any size up to the handle's limits. */
/* Output equals libjpeg-turbo's default decode (islow IDCT, fancy upsampling, fixed-point YCbCr -> RGB).          */
/* ------------------------------------------------------------------------- */
typedef struct mtgv_jpeg_decoder mtgv_jpeg_decoder;
/* host only, no device needed: info[0..5] = h, w, components, sampling (444 / 422 / 420 / 400, 0 other), restart
 * interval (MCUs, 0 none), supported (1 / 0).  Returns 1 (ERR_INVALID) with a message for malformed input; for a
 * well-formed but unsupported file it returns 0 with info[5] = 0 and mtgv_last_error() naming the first unsupported
 * feature (progressive, arithmetic coding, lossless, 12-bit, CMYK / 4 components, other sampling factors ...). */
MTGV_API int mtgv_jpeg_info(const uint8_t* data, int64_t nbytes, int32_t* info);
/* Limits of one batch: max_images files, max_bytes compressed bytes in all, max_pixels pixels in all once every image
 * is padded to whole MCUs (8 or 16 pixels; a 640x480 frame needs 640 * 480).  The pinned staging buffer and every
 * device workspace are allocated here, never inside a decode.  Bound to the device current at creation. */
MTGV_API int mtgv_jpeg_decoder_create(int32_t max_images, int64_t max_bytes, int64_t max_pixels, mtgv_jpeg_decoder** out);
MTGV_API void mtgv_jpeg_decoder_destroy(mtgv_jpeg_decoder* h);
/* n JPEGs in host memory (file i at data_host + offsets[i], sizes[i] bytes) -> RGB uint8, image i written at
 * dst_dev + dst_offset[i] with rows dst_pitch[i] bytes apart (>= 3 w).  Every file is parsed first: malformed or
 * unsupported input returns 1 (ERR_INVALID) naming the image and the reason, before anything is launched.
 * status_dev (n) int32: 0 decoded, 1 corrupt entropy-coded data (that image's slot is then left undefined; nothing is
 * written outside it).  Asynchronous on `stream`: the host buffers may be reused when the call returns. */
MTGV_API int mtgv_jpeg_decode(mtgv_jpeg_decoder* h, const uint8_t* data_host, const int64_t* offsets, const int64_t* sizes,
                              int32_t n, uint8_t* dst_dev, const int64_t* dst_offset, const int64_t* dst_pitch,
                              int32_t* status_dev, void* stream);
/* Progressive files (version 106): SOF2, Huffman, 8-bit, the same component layouts, restart intervals, Huffman tables
 * redefined between scans, any scan script T.81 Annex G allows whose progression is complete (every coefficient of
 * every component is in some scan and the last scan over it has Al = 0; libjpeg would smooth an incomplete file, which
 * is not restated).  Output equals libjpeg-turbo's default decode, as for baseline.  Opt-in per call and per handle: */
#define MTGV_JPEG_PROGRESSIVE 1
/* mtgv_jpeg_info with flags: 0 is mtgv_jpeg_info; with MTGV_JPEG_PROGRESSIVE a progressive file inside the subset is
 * reported as supported.  info[0..5] as above, info[6] = progressive (0 / 1), info[7] = number of scans (1 when
 * info[6] = 0).  An illegal scan script is malformed input (1, the message names the SOS); an incomplete progression
 * and arithmetic coding (SOF10) are unsupported (0, info[5] = 0, the message names the reason). */
MTGV_API int mtgv_jpeg_info_ex(const uint8_t* data, int64_t nbytes, int32_t flags, int32_t* info);
/* mtgv_jpeg_decoder_create with flags.  With MTGV_JPEG_PROGRESSIVE, mtgv_jpeg_decode on this handle takes batches that
 * mix baseline and progressive files (a handle from mtgv_jpeg_decoder_create refuses progressive files as before);
 * baseline images are decoded exactly as on a plain handle.  max_scans: scans of all progressive files of one batch
 * (Pillow writes 10 per colour file, 6 per greyscale file), 0 selects 16 * max_images; a batch with more is refused
 * before any launch.  The extra workspace (scan records, two more Huffman tables per scan, restart-segment offsets:
 * about 2 * max_bytes more pinned and device memory) is allocated here, never inside a decode. */
MTGV_API int mtgv_jpeg_decoder_create_ex(int32_t max_images, int64_t max_bytes, int64_t max_pixels, int32_t flags, int64_t max_scans,
                                         mtgv_jpeg_decoder** out);

/* ------------------------------------------------------------------------- */
/* JPEG encode: the card thumbnails of mtgvision/server.py:222-225 (encode_rgb_im:           */
/* cv2.imencode(".jpg", ..., quality 50) on the host) are encoded on the GPU.  RGB uint8 in, baseline sequential   */
/* Huffman JPEG (SOF0) out: JFIF header, YCbCr 4:2:0 or 4:4:4, the Annex K tables scaled to quality 1..100 (clamped */
/* to 255), islow forward DCT, no restart markers.  The files are byte for byte libjpeg-turbo's with its defaults  */
/* (Pillow's Image.save(f, "JPEG", quality=q, subsampling=2 / 0)).  Anything else is refused with status 1.         */
/* ------------------------------------------------------------------------- */
typedef struct mtgv_jpeg_encoder mtgv_jpeg_encoder;
/* host only: worst-case file size of one h x w image (sampling 420 / 444), 0xFF stuffing included */
MTGV_API int mtgv_jpeg_encode_bound(int32_t h, int32_t w, int32_t sampling, int64_t* nbytes);
/* host only: the bytes from SOI through SOS exactly as the encoder writes them (623 bytes) */
MTGV_API int mtgv_jpeg_encode_header(int32_t h, int32_t w, int32_t quality, int32_t sampling, uint8_t* out_host, int64_t capacity,
                                     int64_t* nbytes);
/* Limits of one call: max_images images, max_pixels pixels in all once every image is padded to whole MCUs (multiples
 * of 16 for 4:2:0, of 8 for 4:4:4; a 192 x 128 crop needs 192 * 128).  Every device workspace is allocated (and the
 * bit-stream workspace cleared) here, never inside an encode.  Bound to the device current at creation. */
MTGV_API int mtgv_jpeg_encoder_create(int32_t max_images, int64_t max_pixels, mtgv_jpeg_encoder** out);
MTGV_API void mtgv_jpeg_encoder_destroy(mtgv_jpeg_encoder* h);
/* n contiguous height x width x 3 RGB uint8 images at src_dev -> n JPEG files back to back in out_dev; file i is
 * out_dev[out_offsets_dev[i], out_offsets_dev[i + 1]) (n + 1 int64 on the device, out_offsets_dev[0] = 0).  Quality
 * 1..100, sampling 420 / 444, sizes 1..65535, the handle's limits and out_capacity >= n * mtgv_jpeg_encode_bound are
 * checked before any launch (status 1, a "jpeg:" message).  Asynchronous on `stream`, library kernels only; nothing is
 * written past out_offsets_dev[n]. */
MTGV_API int mtgv_jpeg_encode(mtgv_jpeg_encoder* h, const uint8_t* src_dev, int32_t n, int32_t height, int32_t width, int32_t quality,
                              int32_t sampling, uint8_t* out_dev, int64_t out_capacity, int64_t* out_offsets_dev, void* stream);

/* ------------------------------------------------------------------------- */
/* Single ops (unit-test and composition surface; same kernels the handles use) */
/* ------------------------------------------------------------------------- */
/* out[M,N] = act(A[M,K] W[N,K]^T + bias) (+res);  act: 0 none 1 gelu 2 mish 3 silu 4 sigmoid */
MTGV_API int mtgv_op_linear(const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev, float* out_dev,
                            int32_t m, int32_t n, int32_t k, int32_t act, void* stream);
/* linear with the block's fused extras: rows are grouped in images of hw rows; a_scale (m/hw, k) and a_shift (k)
 * or NULL are applied to A on load (GRN apply); grn_part or NULL receives the per-row-unit sum(out^2) partials
 * (a buffer of mtgv_op_linear_ex_part_floats floats is large enough for any layout). */
MTGV_API int64_t mtgv_op_linear_ex_part_floats(int32_t m, int32_t n, int32_t k, int32_t act, int32_t hw);
/* layout of the partials the calling thread's last mtgv_op_linear_ex wrote: [ceil(m / unit_rows)][segmax][n] */
MTGV_API int mtgv_op_last_grn_layout(int32_t* unit_rows, int32_t* segmax);
MTGV_API int mtgv_op_linear_ex(const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev, float* out_dev,
                               int32_t m, int32_t n, int32_t k, int32_t act, int32_t hw, const float* a_scale_dev,
                               const float* a_shift_dev, float* grn_part_dev, void* stream);
/* NHWC conv, weight (cout, kh, kw, cin), zero padding */
MTGV_API int mtgv_op_conv2d(const float* x_dev, const float* w_dev, const float* bias_dev, float* out_dev, int32_t n, int32_t h,
                            int32_t w, int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                            int32_t act, void* stream);
/* One conv launch as the detector describes it (Detector::conv, conv_pair, proto), for single-layer tests of the
 * SP8 paths.  Tensors are NHWC views: a pointer to pixel 0, floats per pixel, first channel; fmt 0 = f32, 1 = SP8
 * (sp8.h: per 8 channels 8 fp16 hi halves, then 8 fp16 lo halves - same bytes per pixel, same offsets).  The output
 * grid is the conv's own ((h + 2 pad - kh) / stride + 1, likewise w) unless os > 1: then row (img, y, x) of that grid
 * is written to pixel (img, y os + oy, x os + ox) of an (oh os, ow os) grid - one phase of a ConvTranspose2d(k = s = os) -
 * or, with os_nq > 0, the cout = os os os_nq columns are os os groups of os_nq channels and group q goes to phase
 * (q / os, q % os): the whole ConvTranspose in one launch.  w2 != NULL chains a 1x1 layer [cout2][cout] behind the
 * activated output inside the same launch (act must be SiLU); only out2 is written and out may be NULL.  A chain the
 * kernel cannot run is status 1, never two launches. */
typedef struct {
  const void* x;       /* input: n images of h x w pixels, x_ct floats per pixel, channels [x_co, x_co + cin) */
  int32_t n, h, w, x_ct, x_co, cin, x_fmt;
  const float* wt;     /* [cout][kh][kw][cin] */
  const float* bias;   /* [cout] or NULL */
  int32_t cout, kh, kw, stride, pad, act;
  void* out;           /* channels [out_co, out_co + cout) of out_ct floats per pixel */
  int32_t out_ct, out_co, out_fmt;
  const void* res;     /* NULL, or a residual on the output grid: channels [res_co, res_co + cout) of res_ct */
  int32_t res_ct, res_co, res_fmt;
  int32_t os, oy, ox, os_nq; /* os <= 1: no scatter */
  const float* w2;     /* NULL, or the chained layer [cout2][cout] */
  const float* bias2;
  int32_t cout2, act2;
  void* out2;          /* channels [out2_co, out2_co + cout2) of out2_ct floats per pixel */
  int32_t out2_ct, out2_co, out2_fmt;
} mtgv_conv_ex;
/* path, unless NULL, receives {tile configuration, A mode, epilogue id, ring depth} of the launch that ran (the
 * values of gemm_sp_cfg.h); configuration -1 (the rest 0): the convert-on-load kernel. */
MTGV_API int mtgv_op_conv2d_ex(const mtgv_conv_ex* d, int32_t* path, void* stream);
/* The detector's mask stage alone (version 116; Detector::head_tail runs the same function): out[z][m][px] =
 * <coef[z][m], protos[z][px]> where pixel px = (py, px) of the mh x mw map lies inside box m scaled by crop_scale (x1 <= px < x2,
 * y1 <= py < y2, the products box * crop_scale rounded to f32), 0 outside, and 0 in every row m >= min(n_det[z], mask_rows).
 * coef (n, max_det, nm), protos NHWC (n, mh * mw, nm), n_det (n) int32, boxes (n, max_det, 4) xyxy, out (n, mask_rows, mh * mw),
 * all on the device, f32; nm a multiple of 4, 0 < mask_rows <= max_det.  form 0: the kernel the detector would choose for
 * these sizes; 1: the per-pixel kernel (one pass over the prototypes); 2: the batched GEMM behind a clearing memset.  Status 1,
 * and nothing launched, where the form cannot run: form 1 with nm != 32 or mask_rows > 16. */
MTGV_API int mtgv_op_mask_logits(const float* coef_dev, const float* protos_dev, const int32_t* n_det_dev, const float* boxes_dev,
                                 int32_t n, int32_t max_det, int32_t nm, int32_t mh, int32_t mw, float crop_scale, int32_t mask_rows,
                                 int32_t form, float* out_dev, void* stream);
/* The detector's stem alone (version 103): Conv(3 -> cout, k3, s2, p1) + SiLU straight from uint8 frames (n, h, w, 3), h even,
 * w a multiple of 8, frames 8-byte and out 128-byte aligned; w_dev [cout][3][3][4] with BatchNorm folded and a zero 4th
 * input channel, out (n, h / 2, w / 2, cout) in SP8 (out_sp8) or f32.  cout 16 runs scale n's kernel, 32 / 48 / 64 the wide
 * one; `wide` != 0 runs the wide kernel at 16 channels too (it must give scale n's bits).  Other widths: status 1. */
MTGV_API int mtgv_op_stem_u8(const uint8_t* frames_dev, const float* w_dev, const float* bias_dev, float* out_dev, int32_t n, int32_t h,
                             int32_t w, int32_t cout, int32_t flip_rgb, int32_t out_sp8, int32_t wide, void* stream);
/* YOLO12's area attention and its positional encoding alone (version 109; the detector's ABlocks run the same function), f32.
 * qkv (n, h * w, heads * 96): per head [q 32 | k 32 | v 32], tokens are the pixels row-major.  The h * w tokens of an image
 * are cut into `area` contiguous chunks of h * w / area tokens (not bands of whole rows) and softmax(q^T k / sqrt(32)) v runs
 * inside each chunk; out (n, h * w, heads * 32), channel head * 32 + d.  With pe_w49_dev ([49][heads * 32] tap-major, BatchNorm
 * folded, bias pe_bias_dev [heads * 32]) the depthwise 7x7 (zero padding 3 over the whole h x w map: it crosses the chunks) of
 * v is added; NULL: attention only.  Status 1, and nothing launched, when h * w % area != 0, heads < 1 or area < 1. */
MTGV_API int mtgv_op_area_attn(const float* qkv_dev, const float* pe_w49_dev, const float* pe_bias_dev, int32_t n, int32_t h, int32_t w,
                               int32_t heads, int32_t area, float* out_dev, void* stream);
/* YOLO11's C2PSA attention core and its positional encoding alone (version 114; Detector::c2psa runs the same two launches), f32.
 * qkv (n, h * w, heads * 128): per head [q 32 | k 32 | v 64], tokens are the pixels row-major; out (n, h * w, heads * 64), channel
 * head * 64 + d, receives softmax(q^T k / sqrt(32)) v per image and head.  With pe_w9_dev ([9][heads * 64] tap-major, BatchNorm
 * folded, bias pe_bias_dev [heads * 64]) the depthwise 3x3 (zero padding 1) of v over the h x w map is added: the attention
 * goes to a scratch buffer of the library's and the 3x3 runs as the detector launches it - input channel offset 64, g_size 64,
 * g_stride 128, the attention as addend.  NULL for both: attention only.  Status 1, and nothing launched, for null or
 * misaligned (16 bytes) tensors, sizes below 1, n or heads above 65535.  Synchronises the stream before it returns. */
MTGV_API int mtgv_op_psa_attn(const float* qkv_dev, const float* pe_w9_dev, const float* pe_bias_dev, int32_t n, int32_t h, int32_t w,
                              int32_t heads, float* out_dev, void* stream);
/* The detector's depthwise 3x3 alone (version 114; C2PSA's positional encoding and the Detect(legacy=False) class branch run
 * the same launch): stride 1, zero padding 1, BatchNorm folded into w9 [9][c] tap-major and bias [c], then act (0 none, 3 SiLU),
 * then the optional f32 addend (rows of add_ld floats, channel c at add[pixel * add_ld + c]).  x and out are NHWC views as in
 * mtgv_conv_ex (pixel 0, floats per pixel, first channel; fmt 0 f32, 1 SP8).  Output channel k reads input channel
 * x_co + (k / g_size) * g_stride + k % g_size; g_size 0: x_co + k.  Status 1, and nothing launched, for: null x, w9, bias or
 * out; a size below 1; c % 8 != 0; g_size neither 0 nor a multiple of 8; another act or format; a pointer that is not 16-byte
 * aligned; x_ct, x_co, g_stride (where there is more than one group), out_ct or out_co no multiple of 4 floats (8 on an SP8
 * side), add_ld no multiple of 4 or below c; channels that leave their pixel (x_co + the last channel read > x_ct,
 * out_co + c > out_ct).  Synchronises the stream before it returns. */
typedef struct {
  const void* x;       /* input: n images of h x w pixels, x_ct floats per pixel */
  int32_t n, h, w, x_ct, x_co, x_fmt;
  int32_t c, g_size, g_stride;
  const float* w9;
  const float* bias;
  int32_t act;
  const float* add;    /* NULL, or the addend */
  int32_t add_ld;
  void* out;           /* channels [out_co, out_co + c) of out_ct floats per pixel */
  int32_t out_ct, out_co, out_fmt;
} mtgv_dwconv3;
MTGV_API int mtgv_op_dwconv3(const mtgv_dwconv3* d, void* stream);
/* The detector's prototype branch behind cv1 (Detector::proto runs the same function): ConvTranspose2d(k2, s2, bias) ->
 * cv2 (3x3, BN folded, SiLU) -> cv3 (1x1, BN folded, SiLU), c -> c -> c -> nm channels.  pr1 is an SP8 view of n images of
 * h x w pixels; protos an f32 view of (2 h, 2 w) pixels.  Weights are host pointers: wt (c, c, 2, 2) and bt (c) as
 * ConvTranspose2d stores them, w2 [c][3][3][c], w3 [nm][c].  fold != 0: the ConvTranspose folded into cv2, four 2x2 phase
 * convs over pr1 (where the kernel has the launch; *folded says whether it ran); fold == 0: the layers as launches of
 * their own.  f16x3 operand mode only; synchronises the stream before it returns. */
typedef struct {
  const void* pr1;
  int32_t n, h, w, pr1_ct, pr1_co, c;
  const float *wt, *bt, *w2, *b2, *w3, *b3;
  int32_t nm;
  void* protos;
  int32_t protos_ct, protos_co;
  int32_t fold;
} mtgv_proto_tail;
MTGV_API int mtgv_op_proto_tail(const mtgv_proto_tail* d, int32_t* folded, void* stream);
/* The fused tail of a C2f block alone (version 112; Detector::csp_block runs the same launch, c2f_tail_kernel.h): the block's
 * last bottleneck and its closing 1x1 conv as one launch on SP8 activations,
 *   t = SiLU(w1 (*) y_last + b1), y_new = [y_last +] SiLU(w2 (*) t + b2), out = SiLU(w3 . [cat slices | y_new] + b3),
 * both 3x3 convs stride 1 with zero padding 1 (t is zero outside the frame).  cat is an SP8 view of n images of h x w pixels,
 * cat_ct floats per pixel: the 1 + nb slices of ch channels from channel cat_co on are read, y_last is the last of them; y_new
 * is never stored, so cat needs no room for it.  Weights and biases are device f32: w1 and w2 [ch][3][3][ch], w3
 * [cout][(2 + nb) ch].  out is an SP8 view, channels [out_co, out_co + cout) of out_ct floats per pixel.  There is a kernel
 * for ch = 16 with nb = 1 (w a multiple of 32) and ch = 32 with nb = 1 or 2 (w a multiple of 16), cout = 2 ch, h a multiple
 * of 8, h and w at least 80, channel counts and offsets in multiples of 8, 16-byte aligned pointers, every bias present,
 * f16x3 operand mode.  Anything else is status 1 with nothing launched: the call never falls back to the three conv
 * launches.  Synchronises the stream before it returns. */
typedef struct {
  const void* cat;
  int32_t cat_ct, cat_co;
  int32_t n, h, w, ch, nb, shortcut;
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int32_t cout;
  void* out;
  int32_t out_ct, out_co;
} mtgv_c2f_tail;
MTGV_API int mtgv_op_c2f_tail(const mtgv_c2f_tail* d, void* stream);
/* The weights of that fold, on the host: we [4 (phase 2 a + b)][cout][2][2][c] and bias9 [9 (3 row class + column class;
 * 0 first, 1 inner, 2 last)][cout] from wt (c, mid, 2, 2), bt (mid), w2 [cout][3][3][mid], b2 [cout].  Sums in double,
 * rounded to float once.  Needs no device. */
MTGV_API int mtgv_op_proto_fold_compose(const float* wt_host, const float* bt_host, const float* w2_host, const float* b2_host, int32_t c,
                                        int32_t mid, int32_t cout, float* we_host, float* bias9_host);
MTGV_API int mtgv_op_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, float* out_dev, int64_t rows,
                               int32_t c, float eps, void* stream);
/* depthwise 7x7 pad 3; weight (49, c) tap-major */
MTGV_API int mtgv_op_dwconv7(const float* x_dev, const float* w49_dev, const float* bias_dev, float* out_dev, int32_t n,
                             int32_t h, int32_t w, int32_t c, void* stream);
/* The fused depthwise 7x7 (pad 3, + bias) and LayerNorm over C alone (version 113; the launch that opens every block
 * of mtgv_op_block): NHWC x (n,h,w,c) f32, weight (49, c) tap-major, out (n,h,w,c) as f32 rows (out_fmt 0) or SP8 rows
 * (out_fmt 1, c % 8 == 0).  Runs the fused launch and synchronises the stream; where no fused kernel takes the shape
 * (c % 4 != 0, c > 1024, c / 4 below the strip width: 8 at w >= 8, 4 at w >= 4, else 2) or the format, status 1 and nothing launched -
 * never mtgv_op_dwconv7 + mtgv_op_layernorm.  form receives {kind, TW, TH, WL} of the kernel that ran: kind 0 row groups
 * (dwconv7_ln_rows_kernel<TW, TH, SP8, WL>), 1 row streaming (strip TW, TH rows a step), 2 whole image (TW = w, TH = the band
 * height); WL = 0 for kinds 1 and 2. */
MTGV_API int mtgv_op_dwconv7_ln(const float* x_dev, const float* w49_dev, const float* bias_dev, const float* ln_w_dev,
                                const float* ln_b_dev, float* out_dev, int32_t n, int32_t h, int32_t w, int32_t c, float eps,
                                int32_t out_fmt, int32_t form[4], void* stream);
/* The form that call (and the encoder) would run at this shape, by the launcher's own rule; MTGV_DW_ROWS and
 * MTGV_DW_IMAGE are read per call.  Status 1 for a shape the fused launch refuses.  Needs no device. */
MTGV_API int mtgv_op_dwconv7_ln_form(int32_t n, int32_t h, int32_t w, int32_t c, int32_t form[4]);
/* one ConvNeXt-V2 block on NHWC x (n,h,w,c): convnextv2.py:212-224.  params in reference layout
 * except dw weight (49,c).  ws_dev: workspace of mtgv_op_block_workspace_floats() floats. */
MTGV_API int mtgv_op_block(const float* x_dev, float* out_dev, int32_t n, int32_t h, int32_t w, int32_t c, int32_t act,
                           const float* dw_w49, const float* dw_b, const float* ln_w, const float* ln_b, const float* w1,
                           const float* b1, const float* gamma, const float* beta, const float* w2, const float* b2,
                           float* ws_dev, void* stream);
MTGV_API int64_t mtgv_op_block_workspace_floats(int32_t n, int32_t h, int32_t w, int32_t c);
MTGV_API int mtgv_op_l2norm(const float* x_dev, float* out_dev, int64_t rows, int32_t d, void* stream);

/* ---- tracker (version 104): the temporal logic of mtgvision/server.py:100-106, :133-207 for `streams` independent cameras,
 * state on the device.  Per stream it is mtgv/tracker.py's KalmanPointTracker (norfair.Tracker(mean_euclidean, 300,
 * hit_counter_max 5, initialization_delay 2) restated: parity with norfair itself is unpinned, as for the host class)
 * followed by TrackerCtx's gating: a track is embedded when it is new or update_wait_sec have passed, an exponentially
 * weighted mean of its embeddings queries the bank, the last top_k matches stay on the track.  Filter state is fp64 and the
 * arithmetic is the host class's, operation for operation (no FMA contraction): ids, due sets and filter state are equal.
 * Caps the host class does not have: at most max_tracks live tracks per stream - a detection that finds no free slot is
 * dropped and counted - at most cards_per_frame cards per frame, and every stream at most once per update.  max_tracks <= 64
 * and cards_per_frame <= 16 for mtgv_tracker_create; 256 and 64 for mtgv_tracker_create_ex with MTGV_TRACKER_WIDE (version
 * 110).  Ids are int32.  mtgv_tracker_gather_u8 takes at most 65535 rows: a step of frames * K rows above that is refused there.
 * Zero in a policy field selects the reference's value (300, 5, 2, 1, 0.5 s, 0.1).  To run without an initialisation delay
 * pass initialization_delay = -1 (an id at creation); a negative update_wait_sec makes every reported track due. */
typedef struct {
  int32_t streams;         /* S >= 1 */
  int32_t max_tracks;      /* T, 1..64 slots per stream (MTGV_TRACKER_WIDE: 1..256) */
  int32_t cards_per_frame; /* K, 1..16 (MTGV_TRACKER_WIDE: 1..64) */
  int32_t dim;             /* embedding size */
  int32_t top_k;           /* 1..8 matches kept per track */
  int32_t hit_counter_max, initialization_delay, period;
  double distance_threshold, update_wait_sec, ewma_weight;
} mtgv_tracker_cfg;
typedef struct mtgv_tracker mtgv_tracker;
/* Anything out of range: status 1, checked before the first HIP call (needs no device). */
MTGV_API int mtgv_tracker_create(const mtgv_tracker_cfg* cfg, mtgv_tracker** out);
#define MTGV_TRACKER_WIDE 1
/* flags 0: mtgv_tracker_create itself (T 1..64, K 1..16, the one-wave update kernel).
 * MTGV_TRACKER_WIDE: T 1..256, K 1..64, the multi-wave update kernel (one workgroup of ceil(T / 64) waves per stream) at
 * every size; the same arithmetic, the same results.  Unknown flag bits: status 1.  Checked before the first HIP call.
 * Every other mtgv_tracker_* call works on both kinds of handle; mtgv_tracker_get_state keeps its layout with the handle's T. */
MTGV_API int mtgv_tracker_create_ex(const mtgv_tracker_cfg* cfg, int32_t flags, mtgv_tracker** out);
/* A handle with an embed budget (version 115): flags as for mtgv_tracker_create_ex (0 or MTGV_TRACKER_WIDE), embed_budget
 * E in 1..65535, anything else status 1 before the first HIP call.  The layout of mtgv_tracker_cfg is unchanged.
 * A slot whose track is due (reported, and without an embedding or with more than update_wait_sec since its last one) is a
 * candidate; its key is the time it has waited, now - last_update in fp64 as the gate computes it, +inf for a track that was
 * never embedded.  mtgv_tracker_update takes the min(E, candidates) candidates with the largest key - ties go to the smaller
 * flat index f K + k - and reports them as due_idx (ascending) / n_due; only they get last_update = now.  (So a track
 * that was deferred before its first embed reads last_update = 0, the value of a new slot, in mtgv_tracker_get_state until
 * it is taken, where the host's TrackedData carries the clock of its first report; the gate never reads it without an
 * embedding, and the key of such a track is +inf.)  The others stay
 * due: their key grows with every step, so under a lasting overload a candidate is taken after at most
 * ceil(candidates / E) steps.  With E >= candidates the step is that of a handle without a budget, bit for bit.
 * n_due <= E always, so the embed and match stages can run on exactly E rows with no count read back: gather with
 * mtgv_tracker_gather_u8_pad, and mtgv_tracker_commit on this handle writes zeros into the rows [n_due, rows) of q (and
 * launches over all `rows` rows, at most 65535).  mtgv_tracker_store ignores rows that no slot ranks.
 * An update of more than 8192 flat slots (frames * K) on this handle: status 1, checked before any HIP call. */
MTGV_API int mtgv_tracker_create_budget(const mtgv_tracker_cfg* cfg, int32_t flags, int32_t embed_budget, mtgv_tracker** out);
MTGV_API void mtgv_tracker_destroy(mtgv_tracker* h);
/* forget the tracks of one stream, or of all (-1): ids start again at 1.  Asynchronous on `stream`. */
MTGV_API int mtgv_tracker_reset(mtgv_tracker* h, int32_t stream_or_minus_1, void* stream);
/* One step: frame f (quads (frames, K, 4, 2) f32, pixels) belongs to stream stream_of_frame_host[f] - distinct values in
 * [0, S), else status 1 - and was taken at now_host[f] seconds.  Slot k of frame f is a detection iff k < min(n_det[f], K)
 * (n_det given) and state[f][k] > 0 (state given); at least one of the two.  The valid slots in ascending k are the frame's
 * detection list.  Writes track_id (frames, K): the id of the initialised track matched to the slot, 0 none; due_idx
 * (frames * K): the flat indices f K + k of the slots whose track is due, ascending, -1 behind them; n_due: their count.
 * The host arrays are read before the call returns; nothing is copied and the stream is not synchronised.  due_idx_dev and
 * n_due_dev must stay valid until the step's commit / store have run. */
MTGV_API int mtgv_tracker_update(mtgv_tracker* h, const float* quads_dev, const int32_t* n_det_dev, const int32_t* state_dev, int32_t frames,
                                 const int32_t* stream_of_frame_host, const double* now_host, int32_t* track_id_dev, int32_t* due_idx_dev,
                                 int32_t* n_due_dev, void* stream);
/* mtgv_tracker_update on a handle with an embed budget (status 1 on any other), which also writes n_deferred_dev (1): the
 * candidates of the step that the budget left for later, candidates - n_due.  (mtgv_tracker_update itself works on such a
 * handle too and drops that count.) */
MTGV_API int mtgv_tracker_update_budget(mtgv_tracker* h, const float* quads_dev, const int32_t* n_det_dev, const int32_t* state_dev,
                                        int32_t frames, const int32_t* stream_of_frame_host, const double* now_host, int32_t* track_id_dev,
                                        int32_t* due_idx_dev, int32_t* n_due_dev, int32_t* n_deferred_dev, void* stream);
/* dst row r = src row due_idx[r] for r < min(n_due, max_rows), rows of row_bytes bytes; indices outside [0, src_rows) are
 * skipped.  n_due is read on the device: launched over max_rows rows, nothing written when it is 0. */
MTGV_API int mtgv_tracker_gather_u8(const uint8_t* src_dev, int64_t src_rows, int64_t row_bytes, const int32_t* due_idx_dev,
                                    const int32_t* n_due_dev, int32_t max_rows, uint8_t* dst_dev, void* stream);
/* mtgv_tracker_gather_u8 that also fills the rows [n_due, max_rows) of dst with zeros: every one of the max_rows rows is
 * written (a row whose index is outside [0, src_rows) excepted, as above), so dst can be embedded whole. */
MTGV_API int mtgv_tracker_gather_u8_pad(const uint8_t* src_dev, int64_t src_rows, int64_t row_bytes, const int32_t* due_idx_dev,
                                        const int32_t* n_due_dev, int32_t max_rows, uint8_t* dst_dev, void* stream);
/* z (rows, dim): the embeddings of the due slots in due_idx order.  avg = w z + (1 - w) avg in f32 (the first time avg = z,
 * then the same formula); q (rows, dim) receives the averaged vectors, the queries of the match.  n_due is read on the
 * device and min(n_due, rows) rows are processed: rows is what the buffers hold (n_due, or frames * K without the count).
 * On a handle of mtgv_tracker_create_budget only: rows [n_due, rows) of q are zeroed and rows is at most 65535 (status 1). */
MTGV_API int mtgv_tracker_commit(mtgv_tracker* h, const float* z_dev, float* q_dev, int32_t rows, void* stream);
/* ids / scores (rows, top_k): the matches of q, rows as in commit.  They are kept on the due tracks; then every slot of the step with a track id
 * emits its track's kept matches into out_ids (frames, K, top_k) / out_scores - a track that was not due its older ones - and
 * a slot without a track -1 / -inf.  rows 0 (nothing was due): ids_dev / scores_dev may be NULL. */
MTGV_API int mtgv_tracker_store(mtgv_tracker* h, const int64_t* ids_dev, const float* scores_dev, int32_t rows, int64_t* out_ids_dev,
                                float* out_scores_dev, void* stream);
/* Test surface: one stream's slots on the host (synchronises).  Any output may be NULL.  kal (40, T): rows 8 c + j = position,
 * velocity, pp, pv, vv (c) of corner coordinate j; ints (6, T): live, hit_counter, is_initializing, id, birth, has_z;
 * last_update (T); avg_z (T, dim); match_ids / match_scores (T, top_k); counters (4): next_id, next_birth, overflow, 0. */
MTGV_API int mtgv_tracker_get_state(mtgv_tracker* h, int32_t stream_index, double* kal_host, int32_t* ints_host, double* last_update_host,
                                    float* avg_z_host, int64_t* match_ids_host, float* match_scores_host, int32_t* counters_host, void* stream);
/* The selection kernel of a budget handle alone (version 115): one launch of one workgroup.  waited (n) fp64, slot i's key,
 * NaN for a slot that is no candidate; n in 1..8192, budget in 1..65535, else status 1.  Writes due_idx (n): the
 * min(budget, candidates) candidates with the largest key, ties to the smaller index, in ascending index, -1 behind them;
 * rank_of (n): a selected slot's position in due_idx, -1 otherwise; n_due (1); n_deferred (1) = candidates - n_due.  The
 * budget-th largest key is found exactly (a radix select over the keys as order-preserving 64-bit integers); mtgv/tracker.py's
 * select_due states the rule on the host. */
MTGV_API int mtgv_op_track_select(const double* waited_dev, int32_t n, int32_t budget, int32_t* due_idx_dev, int32_t* rank_of_dev,
                                  int32_t* n_due_dev, int32_t* n_deferred_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGV_H */
