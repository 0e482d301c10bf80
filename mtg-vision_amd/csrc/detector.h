// YOLOv8 / YOLO11 executor at scales n, s and m, -seg or -obb: conv stack on the implicit GEMM of gemm_launch (split-precision f16x3 or
// f32), decode, NMS, mask logits (segment) or rotated decode, rotated NMS (OBB).
// The architectures differ in their backbones only (backbone_v8 in detector.hip, backbone_v11 in detector_v11.hip,
// backbone_v12 in detector_v12.hip): the
// CSP block, the neck from the first upsample on, the head levels, the key expectations behind the backbone and the
// arena table are written once (detector.hip), the neck's node numbers shifted by one for YOLO11 (its node 10 is C2PSA)
// and by minus one for YOLO12 (it has no SPPF).
#pragma once
#include "common.h"
#include "gemm_f32.h"
#include "head_decode.h"
#include "mtgv.h"

#include <algorithm>
#include <map>
#include <math.h>
#include <string>
#include <vector>

namespace mtgv {

// ultralytics' width and depth scaling: channels min(c, max_ch) * width rounded up to a multiple of 8, repeats n * depth.
// The scales the executor runs (mtgv_detector_cfg.scale; recalled from ultralytics 8.3.x, unpinned - DESIGN.md section 3):
//        v8 (depth, width, max_ch)   11 (depth, width, max_ch)
//   n    0.33, 0.25, 1024            0.50, 0.25, 1024
//   s    0.33, 0.50, 1024            0.50, 0.50, 1024
//   m    0.67, 0.75,  768            0.50, 1.00,  512   (YOLO11 m: every C3k2 has c3k = True)
// YOLO12 (arch 12) has YOLO11's table and its c3k rule.
static inline int make_div8(double v) { return (int)(ceil(v / 8.0) * 8.0); }
struct DetScale {
  double depth, width;
  int max_ch;
  int chn(int c) const { return make_div8(std::min(c, max_ch) * width); }
  int rep(int n) const { return n > 1 ? std::max((int)lround(n * depth), 1) : n; }
};
static constexpr int kDetScales = 3;  // n, s, m
static inline DetScale det_scale(int arch, int scale) {
  static const DetScale v8[kDetScales] = {{0.33, 0.25, 1024}, {0.33, 0.50, 1024}, {0.67, 0.75, 768}};
  static const DetScale v11[kDetScales] = {{0.50, 0.25, 1024}, {0.50, 0.50, 1024}, {0.50, 1.00, 512}};
  return (arch == 11 || arch == 12 ? v11 : v8)[scale];
}

// raw head rows per anchor, four whole 128-byte lines: [0,64) box logits (4 sides x 16 bins), [64,96) mask coefficients,
// [96,96+nc) class logits; the rest of the 32 columns behind RAW_CLS is the zero padding of the chained class conv.
// OBB: the angle logit at RAW_COEF, the other 31 coefficient columns are the zero outputs of its padded branch.
// The rows do not change with the scale: 4 x 16 box bins, nm = 32 coefficients (or one angle) and nc classes at every width.
static constexpr int RAW_CT = 128, RAW_COEF = 64, RAW_CLS = 96;

struct ConvW {
  float* w = nullptr;  // [cout][k][k][cin] BN-folded
  float* b = nullptr;  // [cout]
  int cout = 0, cin = 0, k = 1;
};
struct View {
  float* p = nullptr;
  int H = 0, W = 0, ct = 0, co = 0, C = 0;
  int fmt = 0;  // 0: f32; 1: SP8 (sp8.h) - same bytes per element, channel offsets in multiples of 8
  bool f32 = false;  // arena buffer kept f32 in every forward (view() gives the others the forward's format)
  View slice(int off, int c) const {
    View v = *this;
    v.co = co + off;
    v.C = c;
    return v;
  }
};

// a constant vector on the device, registered as a B operand (operand_registry.h); row_k > 0: rows of row_k floats.
// The allocation is appended to `allocs` (the caller frees and unregisters it).
float* upload_operand(const std::vector<float>& v, int row_k, std::vector<float*>& allocs);
// the k x k / pad k/2 conv `w` from view `in` to view `out` of n frames (out.H x out.W: the grid the conv enumerates)
GemmArgs conv_desc(const ConvW& w, const View& in, const View& out, int stride, int act, int n);
// Conv(w1, SiLU) + 1x1 conv w2 (act2): one chained launch where the kernel takes the pair (SP8 input), else two launches.
// xflops: what the launch profiler adds to the pair's 2 M N K (GemmArgs::xflops; negative for zero rows that pad w2).
void conv_pair_launch(const ConvW& w1, const View& in, const View& mid, int stride, const ConvW& w2, const View& out2, int act2, int n,
                      hipStream_t s, double xflops = 0.0);

// model.0 straight from uint8 frames (detector.hip; kernels in detector_kernel.h): cout 16 on conv0_u8_kernel, 32 / 48 / 64
// on conv0_u8_wide_kernel (`wide`: that kernel at 16 channels too - test surface)
void stem_u8_launch(const uint8_t* frames, const float* w, const float* bias, float* out, int n, int H, int W, int cout, int flip, bool sp8,
                    bool wide, hipStream_t s);

// ---- Proto behind cv1 (detector_proto.hip): ConvTranspose2d(k2, s2, bias) -> cv2 (3x3 + BN + SiLU) -> cv3 (1x1 + BN + SiLU) ----
// There is no activation between the ConvTranspose and cv2, so the two are one linear map of the low-resolution map:
// output pixel (2i + a, 2j + b) of cv2 reads the 2x2 neighbourhood pr1[i + a - 1 .. i + a][j + b - 1 .. j + b] with
// weights that depend on the phase (a, b) only,
//   We[a, b][o][dy][dx][c] = sum over (ty, kh) in S(a, dy), (tx, kw) in S(b, dx), m of W2[o][ty][tx][m] * Wt[c][m][kh][kw]
//   S(a, dy) = {(ty, kh): ty in 0..2, r = a + ty - 1, floor(r / 2) - (a - 1) == dy, kh = r mod 2}
// and a bias that depends on which of cv2's 3x3 taps lie inside the upsampled frame (an upsampled pixel is outside
// exactly when its low-resolution source is, so pr1's own zero padding is cv2's):
//   bias9[3 rc + cc][o] = b2[o] + sum over taps (ty, tx) inside of W2[o][ty][tx][:] . bt,
//   rc = 0 first row (ty = 0 outside), 1 inner, 2 last row (ty = 2 outside); cc likewise for columns.
// Host code: wt [c][mid][2][2] and bt [mid] as ConvTranspose2d stores them, w2 [cout][3][3][mid] BN-folded, b2 [cout];
// we [4 (phase 2a + b)][cout][2][2][c], bias9 [9][cout].  Sums in double, rounded to float once.
void proto_fold_compose(const float* wt, const float* bt, const float* w2, const float* b2, int c, int mid, int cout, float* we,
                        float* bias9);
struct ProtoTailW {
  ConvW up[4], up_all;       // the ConvTranspose as four phase matrices [mid][c], and stacked (kh, kw, o) for one launch
  ConvW cv2, cv3;
  ConvW fold[4];             // proto_fold_compose's phases as 2x2 convs [cout][2][2][c] without bias; w == nullptr: no fold
  float* fold_bias = nullptr;  // [9][cout]
};
// Device copies (registered B operands, operand_registry.h) of everything above from the host ConvTranspose parameters
// and the uploaded cv2 / cv3; the fold where its launches exist: c, mid, cout of cv2 equal and a chain tile's width,
// cv3.cout % 32 == 0 and <= that width.  Allocations are appended to `allocs` (the caller frees and unregisters them).
ProtoTailW proto_tail_weights(const float* wt, const float* bt, int c, int mid, const ConvW& cv2, const ConvW& cv3,
                              std::vector<float*>& allocs);
// The launches behind cv1: with `fold` (SP8 activations and fold weights present) four phase launches pr1 -> protos
// (gemm_sp_kernel.h, EPI 96), pr2 and pr3 untouched; otherwise ConvTranspose pr1 -> pr2 (one launch, or four with
// MTGV_PROTO_UP1=0 / f32 activations), then cv2 + cv3 as a chained pair (or two launches) pr2 -> (pr3) -> protos.
// Returns whether the folded form ran.
bool proto_tail_launch(const ProtoTailW& w, const View& pr1, const View& pr2, const View& pr3, const View& protos, int n, bool fold,
                       hipStream_t s);

// The mask stage (process_mask / crop_mask): out[z][m][px] = <coef[z][m], protos[z][px]> inside box m * crop_scale, 0 outside
// and in rows m >= min(n_det[z], mask_rows).  coef [n][max_det][nm], protos NHWC [n][mh * mw][nm], boxes [n][max_det][4],
// out [n][mask_rows][mh * mw].  MASK_FORM_AUTO takes the per-pixel kernel where it can run, else the batched GEMM.
enum { MASK_FORM_AUTO = 0, MASK_FORM_PIXELS = 1, MASK_FORM_GEMM = 2 };
struct MaskLogitsArgs {
  const float* coef;
  const float* protos;
  const int* n_det;
  const float* boxes;
  int n, max_det, nm, mh, mw;
  float crop_scale;
  int mask_rows;
  float* out;
};
// mask_logits_kernel (detector_kernel.h) holds 16 rows of 32 coefficients
inline bool mask_logits_pixels_ok(int nm, int mask_rows) { return nm == 32 && mask_rows <= 16; }
void mask_logits_launch(const MaskLogitsArgs& a, int form, hipStream_t s);

class Detector {
 public:
  explicit Detector(const mtgv_detector_cfg& cfg);
  ~Detector();
  void set_param(const char* key, const float* host, int64_t numel);
  int missing() const;
  void finalize();
  void forward(const uint8_t* frames, int n, int flip, int* n_det, float* boxes, float* conf, int* cls, int* keep_idx,
               float* mask_logits, int mask_rows, hipStream_t s);
  // OBB handle: forward + rotated decode + rotated NMS; rboxes (n, max_det, 5) xywh + angle
  void forward_obb(const uint8_t* frames, int n, int flip, int* n_det, float* rboxes, float* conf, int* cls, int* keep_idx,
                   hipStream_t s);
  void raw(int n, float* pred, float* protos, hipStream_t s);
  double flops_per_frame() const { return flops_; }
  const mtgv_detector_cfg& cfg() const { return cfg_; }
  int na() const { return na_; }
  bool obb() const { return cfg_.task == MTGV_TASK_OBB; }
  int no() const { return 4 + cfg_.nc + (obb() ? 1 : nm_); }

 private:
  struct Raw {
    std::vector<int> shape;
    std::vector<float> data;
    bool set = false;
  };
  void expect(const std::string& key, std::vector<int> shape);
  void expect_conv_bn(const std::string& prefix, int cout, int cin, int k);
  // CSP block (C2f / C3k2) of node idx: cv1 -> two chunks of ch = cout * e channels, n inner modules each appended to the
  // concat, cv2 over the concat.  The inner module: C2f's Bottleneck(ch -> ch -> ch), C3k2's Bottleneck(ch -> ch / 2 -> ch)
  // or C3k(ch, ch, 2).  A2: YOLO12's A2C2f(a2 = False) - cv1 gives ONE chunk of ch = cout / 2 channels, the inner module is
  // C3k(ch, ch, 2), the concat is (1 + n) ch wide.
  enum class Csp { C2f, Half, C3k, A2 };
  struct CspInfo {
    int cout, n, ch; bool shortcut; Csp kind;
    int lead() const { return kind == Csp::A2 ? 1 : 2; }          // chunks cv1 writes
    bool c3k() const { return kind == Csp::C3k || kind == Csp::A2; }
  };
  void expect_csp(int idx, int cin, int cout, int n, bool shortcut, Csp kind, double e = 0.5);
  void expect_sppf(const std::string& prefix, int c);
  // nodes 10 + k .. 22 + k (k = 1 for YOLO11): the neck's four CSP blocks (`kind`, the P5 one `kind_p5`) and two stride-2
  // convs, then the head
  void expect_neck(int n, bool shortcut, Csp kind, Csp kind_p5);
  void expect_head(const int chs[3]);                               // head + Proto keys on features of chs channels
  std::pair<double, double> bn_affine(const std::string& prefix, int o) const;  // BatchNorm of channel o: (scale, bias)
  void free_weights();                                              // unregister and free every uploaded weight
  ConvW fold(const std::string& prefix, int cin_pad = 0);           // Conv+BN
  ConvW plain(const std::string& prefix, int cout_pad = 0);         // Conv2d with bias (cout_pad: zero rows up to that many)
  ConvW concat_out(const std::vector<ConvW>& parts);                // stack along cout (same cin and k)
  ConvW zero_pad(const ConvW& q, int cout, int cin);                // q with zero rows / input channels up to cout x cin
  float* upload(const std::vector<float>& v, int row_k = 0);  // row_k > 0: a GEMM B operand with rows of row_k floats
  void conv(const ConvW& w, const View& in, const View& out, int stride, int act, const View* res, int n, hipStream_t s);
  // Conv(w1, SiLU) followed by the 1x1 conv w2 (act2) with w1's output consumed on chip (gemm_sp_kernel.h, EPI 32): `mid` is
  // where w1's output would go in two launches (used when the pair cannot be chained: f32 mode, flop counting, shapes)
  void conv_pair(const ConvW& w1, const View& in, const View& mid, int stride, const ConvW& w2, const View& out2, int act2, int n,
                 hipStream_t s, double xflops = 0.0);
  void bottleneck(const std::string& prefix, const View& x, const View& tmp, const View& out, bool shortcut, int n, hipStream_t s);
  // pre: the stride-2 Conv in front of the block (input pre_in) where cv1 is its only consumer: `in` is then that conv's output
  void csp_block(int idx, const View& in, const View& out, int n, hipStream_t s, const ConvW* pre = nullptr, const View* pre_in = nullptr);
  // YOLO11 modules
  ConvW fold_dw(const std::string& prefix);                         // depthwise k x k Conv+BN -> weight [k * k][c], bias [c]
  void dwconv(const ConvW& w, const View& in, const View& out, int act, const float* add, int g_size, int g_stride, int n,
              hipStream_t s);
  void c3k(const std::string& prefix, const View& x, const View& kcat, const View& tmp, const View& out, bool shortcut, int n, hipStream_t s);
  void c2psa(int idx, const View& in, const View& out, int n, hipStream_t s);
  int chn(int c) const { return sc_.chn(c); }
  int rep(int n) const { return sc_.rep(n); }
  // YOLO12 modules (detector_v12.hip)
  struct A2Info { int cout, n, c, area; };                          // A2C2f(a2 = True): hidden width c = cout / 2, c / 32 heads
  void expect_a2c2f(int idx, int cin, int cout, int n, int area);
  View a2_view(const char* name, const View& like, int c) const;    // the shared attention buffer `name` as like's map, c wide
  void ablock(const std::string& prefix, const View& x, const View& y, int area, int n, hipStream_t s);
  void a2c2f(int idx, const View& in, const View& out, int n, hipStream_t s);
  int shift() const { return v11() ? 1 : v12() ? -1 : 0; }          // k: node i of the YOLOv8 neck and head is node i + k
  void build_v8();
  void build_v11();
  void build_v12();
  // activation arena: one entry per buffer of max_batch frames, carved in this order
  struct ArenaBuf { std::string name; int h, w, c; bool f32 = false, seg_only = false; };  // f32: View::f32; seg_only: not on an OBB handle
  std::vector<ArenaBuf> arena() const;
  void plan_arena(const std::vector<ArenaBuf>& all);
  // conv0, the architecture's backbone (returns its last node, a slice of concat 20 + k), the neck and the heads
  void forward_graph(const uint8_t* frames, int n, int flip, hipStream_t s);
  View backbone_v8(int n, hipStream_t s);
  View backbone_v11(int n, hipStream_t s);
  View backbone_v12(int n, hipStream_t s);
  void neck_and_heads(const View& top, int n, hipStream_t s);
  HeadRows head_rows() const;                                       // the arena's raw head rows (head_decode.h)
  void decode(int n, hipStream_t s);                                // decode_kernel / decode_obb_kernel: raw head rows -> pred
  void run_graph(const uint8_t* frames, int n, int flip, hipStream_t s);  // backbone, neck, head rows (+ prototype branch)
  void head_tail(int n, int* n_det, float* boxes, float* conf, int* cls, int* keep_idx, float* mask_logits, int mask_rows,
                 hipStream_t s);
  void conv0(const uint8_t* frames, int n, int flip, hipStream_t s);
  void sppf(const std::string& prefix, const View& in, const View& spp, const View& out, int n, hipStream_t s);
  void upsample2x(const View& in, const View& out, int n, hipStream_t s);
  void proto(const std::string& head, const View& p3, int n, hipStream_t s);
  void head_level(int l, int n, hipStream_t s);
  // the class branch of level l into the raw head rows rh: YOLOv8's on its slices of the head temporaries, YOLO11's
  // (Detect(legacy=False): depthwise / pointwise pairs) on the level's features f
  void head_cls_v8(int l, const View& t1, const View& t2, const View& rh, int n, hipStream_t s);
  void head_cls_v11(int l, const View& f, const View& rh, int n, hipStream_t s);
  void obb_flops_fix(const View& f);                                // count mode: the angle branch's real widths
  // Fork-join inside one forward (library-owned streams and events, library kernels only - the concurrency contract
  // of include/mtgv.h): the prototype branch and the P3 / P4 head branches leave the caller's stream as soon as their
  // input exists and rejoin it before decode / the mask product.  fork_after(s, i): side stream i starts after
  // everything enqueued on s so far; join_into(s, i): s continues after everything enqueued on side stream i so far.
  bool fork_enabled() const;
 public:
  void set_fork(int mode) { fork_mode_ = mode; }  // -1: environment (MTGV_DET_FORK, default on), 0: off, 1: on
 private:
  int fork_mode_ = -1;
  hipStream_t fork_after(hipStream_t s, int i);
  void join_into(hipStream_t s, int i);
  bool v11() const { return cfg_.arch == 11; }
  bool v12() const { return cfg_.arch == 12; }
  bool dwcls() const { return v11() || v12(); }                     // Detect(legacy=False): the depthwise class branch
  View view(const std::string& k) const;

  mtgv_detector_cfg cfg_;
  DetScale sc_{0.33, 0.25, 1024};
  int nm_ = 32, npr_ = 64, reg_max_ = 16, na_ = 0;
  // head widths on P3 features of ch0 channels (expect_head): box and class branches, the cv4 branch as the model has it
  // (hc4_) and as it runs (hc4p_: an OBB angle branch narrower than nm_ is zero-padded to nm_), attention heads of C2PSA
  int hc2_ = 64, hc3_ = 64, hc4_ = 32, hc4p_ = 32, psa_n_ = 1;
  std::map<std::string, Raw> raw_;
  bool finalized_ = false;
  std::vector<float*> dev_allocs_;
  double flops_ = 0;
  bool count_flops_ = false;

  // weights
  std::map<std::string, ConvW> cw_;
  std::map<int, CspInfo> csp_;
  std::map<int, A2Info> a2_;
  ConvW cls_dw1_[3], cls_pw1_[3], cls_dw2_[3], cls_pw2_[3];
  std::string head_ = "model.22";
  // head_first_: the first 3x3 convs of the branches that read the level's features, stacked (v8: box, class and
  // coefficient; v11: box and coefficient)
  ConvW head_first_[3], head_box2_[3], head_cls2_[3], head_coef2_[3], head_box3_[3], head_cls3_[3], head_coef3_[3];
  ConvW head_cls3_pad_[3];  // v8: head_cls3_ with zero rows up to 32 outputs (the chained form of the class branch)
  ProtoTailW proto_w_;  // the prototype branch behind cv1

  // activations (arena)
  DevBuf arena_;
  std::map<std::string, View> v_;
  int* nms_ws_ = nullptr;
  size_t nms_ws_bytes_ = 0;
  int last_n_ = 0;
  int pred_n_ = 0;             // frames of the last forward whose `pred` exists (0 after a MTGV_DET_HEAD_DIRECT forward)
  bool head_direct_ = true;    // MTGV_DET_HEAD_DIRECT of the forward in progress
  int fmt_ = 0;  // activation format of the forward in progress (0 f32, 1 SP8)
  static constexpr int NSIDE = 3;  // 0: prototype branch, 1: P3 head, 2: P4 head
  hipStream_t side_[NSIDE] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork_[NSIDE] = {nullptr, nullptr, nullptr}, ev_join_[NSIDE] = {nullptr, nullptr, nullptr};
  bool side_busy_[NSIDE] = {false, false, false};  // forked in the forward in progress and not joined yet
};

// Area attention + positional encoding of YOLO12's AAttn (detector_v12.hip), f32.  qkv (n, h * w, heads * 96), per head
// [q 32 | k 32 | v 32]; tokens are the pixels row-major, cut into `area` contiguous chunks of h * w / area; attention runs
// inside a chunk.  att (n, h * w, heads * 32) f32 receives softmax(q^T k / sqrt(32)) v.  With pe_w49 ([49][heads * 32], bias
// pe_bias) the depthwise 7x7 (zero padding 3 over the whole map) of the v channels is added and the sum written to channels
// [out_co, out_co + heads * 32) of out (out_ct floats per pixel, SP8 if out_sp8, else f32; out may be att itself).
void area_attn_launch(const float* qkv, const float* pe_w49, const float* pe_bias, int n, int h, int w, int heads, int area, float* att,
                      float* out, int out_ct, int out_co, bool out_sp8, hipStream_t s);

// C2PSA's attention core (detector_v11.hip: attn_kernel<32, 64, 16>), f32.  qkv (n, N, heads * 128), per head
// [q 32 | k 32 | v 64]; att (n, N, heads * 64) receives softmax(q^T k / sqrt(32)) v per image and head.  Refused with
// ERR_INVALID before any launch: null or misaligned tensors, non-positive sizes, n or heads above 65535 (grid dimensions).
// psa_attn_check is that refusal alone.
void psa_attn_check(const float* qkv, int n, int N, int heads, const float* att);
void psa_attn_launch(const float* qkv, int n, int N, int heads, float* att, hipStream_t s);

// Depthwise 3x3, stride 1, zero padding 1, + bias (+ SiLU) (+ f32 addend) on n images of H x W pixels (detector_v11.hip:
// dwconv3_kernel<IN_SP8, OUT_SP8>).  Views as in mtgv_conv_ex: pixel 0, floats per pixel, first channel; fmt 0 f32, 1 SP8.
// Output channel c reads input channel in_co + (c / g_size) g_stride + c % g_size (g_size 0: in_co + c); w9 [9][C] tap-major
// and bias [C] f32; act ACT_NONE or ACT_SILU; add nullptr or f32 rows of add_ld floats, added behind the activation.
// dwconv3_check is the launch's refusal alone (ERR_INVALID; the conditions are at its definition).
struct Dwconv3Args {
  const float* in;
  int in_ct, in_co, in_fmt, g_size, g_stride;
  const float *w9, *bias;
  int act;
  const float* add;
  int add_ld;
  float* out;
  int out_ct, out_co, out_fmt;
  int n, H, W, C;
};
void dwconv3_check(const Dwconv3Args& a);
void dwconv3_launch(const Dwconv3Args& a, hipStream_t s);

}  // namespace mtgv
