// YOLOv8-seg / -obb forward on the GPU, NHWC fp32.  Module graph: ultralytics yolov8-seg.yaml at
// scales n, s and m (detector.h: det_scale; third-party to the reference; call site mtgvision/od_export.py:141-160, model
// family od_train.py:46-70).  BatchNorm (eps 1e-3) is folded into the conv weights at
// finalize(); Concat is free (producers write channel slices of the consumer's buffer);
// every Conv+SiLU is one launch of the implicit GEMM (gemm_launch, gemm_f32.hip).
// This file also holds what YOLO11 and YOLO12 share with it: the CSP block (csp_block: C2f, C3k2 and A2C2f without attention), the neck and the head levels
// (neck_and_heads, head_level), their key expectations (expect_csp, expect_neck, expect_head) and the arena table (arena).
// The device kernels are in detector_kernel.h, the prototype branch behind cv1 in detector_proto.hip, the YOLO11
// backbone and the modules only it has in detector_v11.hip, YOLO12's (A2C2f with area attention) in detector_v12.hip.
#include "detector.h"
#include "detector_kernel.h"
#include "nms.h"
#include "rowops.h"
#include "gemm_sp.h"
#include "c2f_tail.h"
#include "operand_registry.h"

namespace mtgv {

// ---------------------------------------------------------------------------
// construction: expected ultralytics keys
// ---------------------------------------------------------------------------
void Detector::expect(const std::string& key, std::vector<int> shape) {
  Raw r;
  r.shape = shape;
  raw_[key] = r;
}
void Detector::expect_conv_bn(const std::string& p, int cout, int cin, int k) {
  expect(p + ".conv.weight", {cout, cin, k, k});
  expect(p + ".bn.weight", {cout});
  expect(p + ".bn.bias", {cout});
  expect(p + ".bn.running_mean", {cout});
  expect(p + ".bn.running_var", {cout});
}

Detector::Detector(const mtgv_detector_cfg& cfg) : cfg_(cfg) {
  MTGV_CHECK(cfg.nc >= 1 && cfg.nc <= 4, ERR_INVALID, "detector: nc=%d (1..4 supported)", cfg.nc);
  MTGV_CHECK(cfg.imgsz > 0 && cfg.imgsz % 32 == 0, ERR_INVALID, "detector: imgsz=%d must be a multiple of 32", cfg.imgsz);
  MTGV_CHECK(cfg.max_batch > 0, ERR_INVALID, "detector: max_batch=%d", cfg.max_batch);
  MTGV_CHECK(cfg.max_det > 0 && cfg.max_det <= 1024, ERR_INVALID, "detector: max_det=%d", cfg.max_det);
  MTGV_CHECK(cfg.arch == 0 || cfg.arch == 8 || cfg.arch == 11 || cfg.arch == 12, ERR_KEY, "detector: arch=%d (8: YOLOv8, 11: YOLO11, 12: YOLO12)",
             cfg.arch);
  MTGV_CHECK(cfg.task == MTGV_TASK_SEGMENT || cfg.task == MTGV_TASK_OBB, ERR_KEY, "detector: task=%d (0: segment, 1: OBB)", cfg.task);
  MTGV_CHECK(cfg.scale >= 0 && cfg.scale <= 4, ERR_INVALID, "detector: scale=%d (0: n, 1: s, 2: m)", cfg.scale);
  // l and x: spec.py knows their keys and the oracle runs them, but the 1e-4 contract cannot be tested at those widths yet
  MTGV_CHECK(cfg.scale < kDetScales, ERR_KEY, "detector: scale=%d (%s) is not supported: the scales that run are n, s, m (0, 1, 2)", cfg.scale,
             cfg.scale == 3 ? "l" : "x");
  sc_ = det_scale(cfg.arch, cfg.scale);
  npr_ = make_div8(std::min(256, sc_.max_ch) * sc_.width);
  // the input rectangle: in_h = in_w = 0 is the square imgsz x imgsz
  if (cfg.in_h == 0 && cfg.in_w == 0) cfg_.in_h = cfg_.in_w = cfg.imgsz;
  MTGV_CHECK(cfg_.in_h >= 32 && cfg_.in_w >= 32 && cfg_.in_h % 32 == 0 && cfg_.in_w % 32 == 0 && cfg_.in_h <= cfg.imgsz && cfg_.in_w <= cfg.imgsz,
             ERR_INVALID, "detector: in_h=%d in_w=%d must both be 0 (imgsz x imgsz) or multiples of 32 in [32, imgsz=%d]", cfg.in_h, cfg.in_w,
             cfg.imgsz);
  const int IH = cfg_.in_h, IW = cfg_.in_w;
  na_ = (IH / 8) * (IW / 8) + (IH / 16) * (IW / 16) + (IH / 32) * (IW / 32);
  // The branch streams of the forward's fork-join are created with the handle, not at the first forward: the HIP runtime maps
  // streams to its hardware queues in creation order, and branch streams created after an application's high-priority
  // stream (mtgv.Pipeline's embed stream) ended up sharing a queue with the caller's stream - the forward on ONE stream then
  // took 5.1 instead of 2.5 ms (tools/debug/one_stream_after_overlap.py).
  for (int i = 0; i < NSIDE; ++i) {
    HIP_OK(hipStreamCreateWithFlags(&side_[i], hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&ev_fork_[i], hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&ev_join_[i], hipEventDisableTiming));
  }
  head_ = "model." + std::to_string(22 + shift());
  if (v11()) build_v11();
  else if (v12()) build_v12();
  else build_v8();
}

static std::string node(int i) { return "model." + std::to_string(i); }

void Detector::expect_csp(int idx, int cin, int cout, int n, bool shortcut, Csp kind, double e) {
  const int ch = (int)(cout * e), c_ = ch / 2;
  const std::string p = node(idx);
  const CspInfo ci{cout, n, ch, shortcut, kind};
  auto bott = [&](const std::string& q, int c1, int cm, int c2) {
    expect_conv_bn(q + ".cv1", cm, c1, 3);
    expect_conv_bn(q + ".cv2", c2, cm, 3);
  };
  expect_conv_bn(p + ".cv1", ci.lead() * ch, cin, 1);
  expect_conv_bn(p + ".cv2", cout, (ci.lead() + n) * ch, 1);
  for (int j = 0; j < n; ++j) {
    const std::string m = p + ".m." + std::to_string(j);
    if (ci.c3k()) {
      expect_conv_bn(m + ".cv1", c_, ch, 1);
      expect_conv_bn(m + ".cv2", c_, ch, 1);
      expect_conv_bn(m + ".cv3", ch, 2 * c_, 1);
      for (int i = 0; i < 2; ++i) bott(m + ".m." + std::to_string(i), c_, c_, c_);
    } else {
      bott(m, ch, kind == Csp::Half ? c_ : ch, ch);
    }
  }
  csp_[idx] = ci;
}

void Detector::expect_sppf(const std::string& p, int c) {
  expect_conv_bn(p + ".cv1", c / 2, c, 1);
  expect_conv_bn(p + ".cv2", c, c / 2 * 4, 1);
}

void Detector::expect_neck(int n, bool shortcut, Csp kind, Csp kind_p5) {
  const int k = shift();
  const int c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  expect_csp(12 + k, c256 + c128, c128, n, shortcut, kind);            // on concat [up(9 + k), 6]
  expect_csp(15 + k, c128 + csp_.at(4).cout, c64, n, shortcut, kind);  // on concat [up(12 + k), 4]: P3
  expect_conv_bn(node(16 + k), c64, c64, 3);
  expect_csp(18 + k, c64 + c128, c128, n, shortcut, kind);             // on concat [16 + k, 12 + k]: P4
  expect_conv_bn(node(19 + k), c128, c128, 3);
  expect_csp(21 + k, c128 + c256, c256, n, shortcut, kind_p5);         // on concat [19 + k, 9 + k]: P5
  const int chs[3] = {c64, c128, c256};
  expect_head(chs);
}

// yolov8-seg.yaml / yolov8-obb.yaml
void Detector::build_v8() {
  const int c16 = chn(64), c32 = chn(128), c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  const int n3 = rep(3), n6 = rep(6);
  expect_conv_bn(node(0), c16, 3, 3);
  expect_conv_bn(node(1), c32, c16, 3);
  expect_csp(2, c32, c32, n3, true, Csp::C2f);
  expect_conv_bn(node(3), c64, c32, 3);
  expect_csp(4, c64, c64, n6, true, Csp::C2f);
  expect_conv_bn(node(5), c128, c64, 3);
  expect_csp(6, c128, c128, n6, true, Csp::C2f);
  expect_conv_bn(node(7), c256, c128, 3);
  expect_csp(8, c256, c256, n3, true, Csp::C2f);
  expect_sppf(node(9), c256);
  expect_neck(n3, false, Csp::C2f, Csp::C2f);
}

// Segment head (Detect + Segment + Proto) on features of chs[0..2] channels: the keys both architectures share; only
// the class branch cv3 differs.  OBB head (Detect + angle branch): cv4 carries ne = 1 angle logit through
// c4 = max(chs[0] / 4, ne) = 16 channels, and there is no Proto.
void Detector::expect_head(const int chs[3]) {
  const int c2 = std::max(std::max(16, chs[0] / 4), reg_max_ * 4);
  const int c3 = std::max(chs[0], std::min(cfg_.nc, 100));
  const int n4 = obb() ? 1 : nm_;
  const int c4 = std::max(chs[0] / 4, n4);
  hc2_ = c2, hc3_ = c3, hc4_ = c4, hc4p_ = std::max(c4, nm_);
  // (the box branch's final 1x1 fills the rows' 64 box columns, the class branch's chained form the 32 behind RAW_CLS)
  MTGV_CHECK(c2 % 8 == 0 && c3 % 8 == 0 && c4 % 8 == 0 && 4 * reg_max_ == RAW_COEF && RAW_COEF + nm_ == RAW_CLS, ERR_INVALID,
             "detector: unexpected head widths");
  const std::string H = head_;
  for (int l = 0; l < 3; ++l) {
    const std::string ls = std::to_string(l);
    expect_conv_bn(H + ".cv2." + ls + ".0", c2, chs[l], 3);
    expect_conv_bn(H + ".cv2." + ls + ".1", c2, c2, 3);
    expect(H + ".cv2." + ls + ".2.weight", {4 * reg_max_, c2, 1, 1});
    expect(H + ".cv2." + ls + ".2.bias", {4 * reg_max_});
    if (dwcls()) {
      // Detect(legacy=False): Sequential(DWConv(x, x, 3), Conv(x, c3, 1)), Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)), Conv2d
      expect_conv_bn(H + ".cv3." + ls + ".0.0", chs[l], 1, 3);
      expect_conv_bn(H + ".cv3." + ls + ".0.1", c3, chs[l], 1);
      expect_conv_bn(H + ".cv3." + ls + ".1.0", c3, 1, 3);
      expect_conv_bn(H + ".cv3." + ls + ".1.1", c3, c3, 1);
    } else {
      expect_conv_bn(H + ".cv3." + ls + ".0", c3, chs[l], 3);
      expect_conv_bn(H + ".cv3." + ls + ".1", c3, c3, 3);
    }
    expect(H + ".cv3." + ls + ".2.weight", {cfg_.nc, c3, 1, 1});
    expect(H + ".cv3." + ls + ".2.bias", {cfg_.nc});
    expect_conv_bn(H + ".cv4." + ls + ".0", c4, chs[l], 3);
    expect_conv_bn(H + ".cv4." + ls + ".1", c4, c4, 3);
    expect(H + ".cv4." + ls + ".2.weight", {n4, c4, 1, 1});
    expect(H + ".cv4." + ls + ".2.bias", {n4});
  }
  expect(H + ".dfl.conv.weight", {1, reg_max_, 1, 1});
  if (obb()) return;
  expect_conv_bn(H + ".proto.cv1", npr_, chs[0], 3);
  expect(H + ".proto.upsample.weight", {npr_, npr_, 2, 2});
  expect(H + ".proto.upsample.bias", {npr_});
  expect_conv_bn(H + ".proto.cv2", npr_, npr_, 3);
  expect_conv_bn(H + ".proto.cv3", nm_, npr_, 1);
}

void Detector::free_weights() {
  for (float* p : dev_allocs_) {
    operand_unregister(p);
    (void)hipFree(p);
  }
  dev_allocs_.clear();
}

Detector::~Detector() {
  free_weights();
  if (nms_ws_) (void)hipFree(nms_ws_);
  for (int i = 0; i < NSIDE; ++i) {
    if (side_[i]) (void)hipStreamDestroy(side_[i]);
    if (ev_fork_[i]) (void)hipEventDestroy(ev_fork_[i]);
    if (ev_join_[i]) (void)hipEventDestroy(ev_join_[i]);
  }
}

bool Detector::fork_enabled() const {
  if (count_flops_) return false;
  if (fork_mode_ >= 0) return fork_mode_ != 0;  // mtgv_detector_set_fork
  return env_int("MTGV_DET_FORK", 1) != 0;  // read per call: tests and tools compare both schedules in one process
}

hipStream_t Detector::fork_after(hipStream_t s, int i) {
  if (!fork_enabled()) return s;
  HIP_OK(hipEventRecord(ev_fork_[i], s));
  HIP_OK(hipStreamWaitEvent(side_[i], ev_fork_[i], 0));
  side_busy_[i] = true;
  return side_[i];
}

void Detector::join_into(hipStream_t s, int i) {
  if (!side_busy_[i]) return;
  HIP_OK(hipEventRecord(ev_join_[i], side_[i]));
  HIP_OK(hipStreamWaitEvent(s, ev_join_[i], 0));
  side_busy_[i] = false;
}

void Detector::set_param(const char* key, const float* host, int64_t numel) {
  auto it = raw_.find(key);
  MTGV_CHECK(it != raw_.end(), ERR_KEY, "unknown detector parameter key '%s'", key);
  int64_t want = 1;
  for (int d : it->second.shape) want *= d;
  MTGV_CHECK(numel == want, ERR_INVALID, "parameter %s: got %lld elements, expected %lld", key, (long long)numel, (long long)want);
  it->second.data.assign(host, host + numel);
  it->second.set = true;
  finalized_ = false;
}

int Detector::missing() const {
  int m = 0;
  for (auto& kv : raw_) m += kv.second.set ? 0 : 1;
  return m;
}

float* upload_operand(const std::vector<float>& v, int row_k, std::vector<float*>& allocs) {
  float* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, std::max<size_t>(v.size(), 4) * sizeof(float)));
  HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  allocs.push_back(d);
  operand_register(d, v.size(), row_k);  // weights become pre-split B operands for the f16x3 GEMMs (small vectors are skipped)
  operand_refresh(d, 0, v.size() % 4 == 0 ? v.size() : 0, nullptr);
  HIP_OK(hipStreamSynchronize(nullptr));
  return d;
}

float* Detector::upload(const std::vector<float>& v, int row_k) { return upload_operand(v, row_k, dev_allocs_); }

// BatchNorm2d(eps=1e-3) of prefix p in inference form, channel o: y = scale * x + bias, returned as (scale, bias)
std::pair<double, double> Detector::bn_affine(const std::string& p, int o) const {
  const double sc = (double)raw_.at(p + ".bn.weight").data[o] / sqrt((double)raw_.at(p + ".bn.running_var").data[o] + 1e-3);
  return {sc, (double)raw_.at(p + ".bn.bias").data[o] - (double)raw_.at(p + ".bn.running_mean").data[o] * sc};
}

// Conv2d(bias=False) + BatchNorm2d(eps=1e-3) -> weight [cout][k][k][cin_pad], bias [cout]
ConvW Detector::fold(const std::string& p, int cin_pad) {
  const Raw& w = raw_.at(p + ".conv.weight");
  const int cout = w.shape[0], cin = w.shape[1], k = w.shape[2];
  const int cp = cin_pad > 0 ? cin_pad : cin;
  std::vector<float> wf((size_t)cout * k * k * cp, 0.f), bf(cout);
  for (int o = 0; o < cout; ++o) {
    const auto [sc, bias] = bn_affine(p, o);
    bf[o] = (float)bias;
    for (int i = 0; i < cin; ++i)
      for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw)
          wf[(((size_t)o * k + kh) * k + kw) * cp + i] = (float)((double)w.data[(((size_t)o * cin + i) * k + kh) * k + kw] * sc);
  }
  return ConvW{upload(wf, k * k * cp), upload(bf), cout, cp, k};
}

ConvW Detector::plain(const std::string& p, int cout_pad) {
  const Raw& w = raw_.at(p + ".weight");
  const int cout = w.shape[0], cin = w.shape[1], k = w.shape[2];
  const int co = std::max(cout, cout_pad);
  std::vector<float> wf((size_t)co * k * k * cin, 0.f), bf(raw_.at(p + ".bias").data);
  bf.resize(co, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i)
      for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw)
          wf[(((size_t)o * k + kh) * k + kw) * cin + i] = w.data[(((size_t)o * cin + i) * k + kh) * k + kw];
  return ConvW{upload(wf, k * k * cin), upload(bf), co, cin, k};
}

// ConvWs that read the same input stacked along cout, rows and biases in the order given: one launch for all of them
ConvW Detector::concat_out(const std::vector<ConvW>& parts) {
  const int cin = parts.at(0).cin, k = parts[0].k;
  const size_t per = (size_t)k * k * cin;
  std::vector<float> w, b;
  for (const ConvW& q : parts) {
    MTGV_CHECK(q.cin == cin && q.k == k, ERR_RUNTIME, "detector: concat_out of convs with different inputs");
    const size_t wo = w.size(), bo = b.size();
    w.resize(wo + (size_t)q.cout * per), b.resize(bo + q.cout);
    HIP_OK(hipMemcpy(w.data() + wo, q.w, (size_t)q.cout * per * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b.data() + bo, q.b, (size_t)q.cout * sizeof(float), hipMemcpyDeviceToHost));
  }
  return ConvW{upload(w, (int)per), upload(b), (int)b.size(), cin, k};
}

// q with zero output rows (zero bias) up to `cout` and zero input channels up to `cin`: SiLU(0) = 0, so a padded
// channel stays zero through a Conv+SiLU chain and adds nothing to the real ones
ConvW Detector::zero_pad(const ConvW& q, int cout, int cin) {
  MTGV_CHECK(cout >= q.cout && cin >= q.cin, ERR_RUNTIME, "detector: zero_pad to a smaller conv");
  const int kk = q.k * q.k;
  std::vector<float> w0((size_t)q.cout * kk * q.cin), b(q.cout);
  HIP_OK(hipMemcpy(w0.data(), q.w, w0.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(b.data(), q.b, b.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> w((size_t)cout * kk * cin, 0.f);
  for (int o = 0; o < q.cout; ++o)
    for (int t = 0; t < kk; ++t)
      for (int i = 0; i < q.cin; ++i) w[((size_t)o * kk + t) * cin + i] = w0[((size_t)o * kk + t) * q.cin + i];
  b.resize(cout, 0.f);
  return ConvW{upload(w, kk * cin), upload(b), cout, cin, q.k};
}

// Carve the activation arena for max_batch frames: each buffer 256-byte aligned, in table order.  Cleared once: of the raw
// head rows' 32 columns behind RAW_CLS, those past the classes are written by the chained class conv only (as zeros).
void Detector::plan_arena(const std::vector<ArenaBuf>& all) {
  auto floats = [&](const ArenaBuf& b) { return ((size_t)cfg_.max_batch * b.h * b.w * b.c + 63) / 64 * 64; };
  std::vector<ArenaBuf> bufs;
  for (const ArenaBuf& b : all)
    if (!(obb() && b.seg_only)) bufs.push_back(b);  // OBB: no prototype branch, no mask coefficients
  size_t total = 0;
  for (const ArenaBuf& b : bufs) total += floats(b);
  arena_.alloc(total);
  v_.clear();
  float* p = arena_.p;
  for (const ArenaBuf& b : bufs) {
    View v;
    v.p = p, v.H = b.h, v.W = b.w, v.ct = b.c, v.C = b.c, v.f32 = b.f32;
    MTGV_CHECK(v_.emplace(b.name, v).second, ERR_RUNTIME, "detector: arena buffer '%s' listed twice", b.name.c_str());
    p += floats(b);
  }
  HIP_OK(hipMemset(arena_.p, 0, arena_.n * sizeof(float)));
}

// The arena table of every architecture (node numbers in the comments are YOLOv8's; k = 1 shifts the neck's for YOLO11, k = -1
// for YOLO12).
// The order is the carve order: it decides every buffer's address, so a buffer is added where it is first written.
std::vector<Detector::ArenaBuf> Detector::arena() const {
  const int IH = cfg_.in_h, IW = cfg_.in_w, k = shift();
  const int h2 = IH / 2, h4 = IH / 4, h8 = IH / 8, h16 = IH / 16, h32 = IH / 32;
  const int w2 = IW / 2, w4 = IW / 4, w8 = IW / 8, w16 = IW / 16, w32 = IW / 32;
  const int c16 = chn(64), c32 = chn(128), c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  std::vector<ArenaBuf> a;
  auto add = [&](std::initializer_list<ArenaBuf> l) { a.insert(a.end(), l); };
  auto cat = [&](int i) { return "cat" + std::to_string(i + k); };
  // CSP block `idx` on an h x w map: the concat of cv1's two chunks and the inner modules' outputs, C3k's own concat where
  // the inner module is one, and the bottlenecks' temporary (their hidden width: the chunk's, or half of it in C3k2)
  auto csp = [&](int idx, int h, int w) {
    const CspInfo& ci = csp_.at(idx);
    const std::string id = std::to_string(idx);
    a.push_back({"cat" + id, h, w, (ci.lead() + ci.n) * ci.ch});
    if (ci.c3k()) a.push_back({"kcat" + id, h, w, ci.ch});
    a.push_back({"tmp" + id, h, w, ci.kind == Csp::C2f ? ci.ch : ci.ch / 2});
  };
  auto rows = [&] { add({{"rawhead0", h8, w8, RAW_CT, true}, {"rawhead1", h16, w16, RAW_CT, true}, {"rawhead2", h32, w32, RAW_CT, true}}); };
  // backbone (nodes 4, 6 and the last one write into the neck's concats)
  add({{"l0", h2, w2, c16}, {"l1", h4, w4, c32}});
  csp(2, h4, w4);
  add({{"l2", h4, w4, csp_.at(2).cout}, {"l3", h8, w8, c64}});
  csp(4, h8, w8);
  add({{cat(14), h8, w8, c128 + csp_.at(4).cout},  // concat 14 = [up(12), 4]
       {"l5", h16, w16, c128}});
  if (v12()) {
    // A2C2f 6 and 8: their concats, and one set of attention buffers for all eight ABlocks, carved for P4 (four times P5's
    // pixels at no less than half its width) - qkv and the attention output in f32, the proj input and the MLP's hidden map
    const A2Info &a6 = a2_.at(6), &a8 = a2_.at(8);
    const int cw = std::max(a6.c, a8.c);
    add({{"cat6", h16, w16, (1 + a6.n) * a6.c}, {"a2qkv", h16, w16, 3 * cw, true}, {"a2att", h16, w16, cw, true}, {"a2y", h16, w16, cw},
         {"a2mlp", h16, w16, 2 * cw}});
    add({{cat(11), h16, w16, c256 + c128}, {"l7", h32, w32, c256}, {"cat8", h32, w32, (1 + a8.n) * a8.c}});
  } else {
    csp(6, h16, w16);
    add({{cat(11), h16, w16, c256 + c128},  // concat 11 = [up(9), 6]
         {"l7", h32, w32, c256}});
    csp(8, h32, w32);
    add({{"l8", h32, w32, c256}, {"sppcat", h32, w32, 2 * c256}});
  }
  if (v11()) {  // SPPF's own output and C2PSA (the attention core and the positional encoding read qkv and att in f32)
    const int pc = c256 / 2;  // C2PSA's hidden width: qkv is pc + 2 heads x 32 keys = 2 pc wide
    add({{"l9", h32, w32, c256}, {"psacat", h32, w32, 2 * pc}, {"qkv", h32, w32, 2 * pc, true}, {"att", h32, w32, pc, true},
         {"atty", h32, w32, pc}, {"ffn", h32, w32, 2 * pc}});
  }
  add({{cat(20), h32, w32, c128 + c256}});  // concat 20 = [19, 9]
  // neck
  csp(12 + k, h16, w16);
  add({{cat(17), h16, w16, c64 + c128}});  // concat 17 = [16, 12]
  csp(15 + k, h8, w8);
  add({{"p3", h8, w8, c64}});
  csp(18 + k, h16, w16);
  add({{"p4", h16, w16, c128}});
  csp(21 + k, h32, w32);
  add({{"p5", h32, w32, c256}});
  // head temporaries per level (the levels' branches run concurrently): the branches head_first_ stacks side by side (160
  // channels at YOLOv8 n, 96 at YOLO11 n), and YOLO11's class branch
  const int hs[3] = {h8, h16, h32}, ws[3] = {w8, w16, w32}, chs[3] = {c64, c128, c256};
  const int ht = hc2_ + (dwcls() ? 0 : hc3_) + hc4p_;
  for (int l = 0; l < 3; ++l) {
    const std::string ls = std::to_string(l);
    const int h = hs[l], w = ws[l];
    add({{"t1_" + ls, h, w, ht}, {"t2_" + ls, h, w, ht}});
    if (dwcls()) add({{"dwa_" + ls, h, w, chs[l]}, {"dwb_" + ls, h, w, hc3_}, {"dwc_" + ls, h, w, hc3_}, {"dwd_" + ls, h, w, hc3_}});
  }
  // (the raw head rows are carved in front of the prototype buffers for YOLOv8 and behind them for YOLO11)
  if (!dwcls()) rows();
  add({{"pr1", h8, w8, npr_, false, true}, {"pr2", h4, w4, npr_, false, true}, {"pr3", h4, w4, npr_, false, true},
       {"protos", h4, w4, nm_, true, true}});
  if (dwcls()) rows();
  add({{"pred", 1, na_, no(), true}, {"coef", 1, cfg_.max_det, nm_, true, true}});
  return a;
}

// activation view by name, in the format of the current forward (fmt_) unless the buffer is kept f32
View Detector::view(const std::string& k) const {
  View v = v_.at(k);
  v.fmt = v.f32 ? 0 : fmt_;
  return v;
}

void Detector::finalize() {
  MTGV_CHECK(missing() == 0, ERR_RUNTIME, "detector has %d unset parameters", missing());
  if (finalized_) return;
  free_weights();
  cw_.clear();
  // every Conv+BN key prefix
  for (auto& kv : raw_) {
    const std::string& k = kv.first;
    const std::string suf = ".conv.weight";
    if (k.size() > suf.size() && k.compare(k.size() - suf.size(), suf.size(), suf) == 0) {
      const std::string pre = k.substr(0, k.size() - suf.size());
      if (raw_.find(pre + ".bn.weight") == raw_.end()) continue;  // dfl.conv has no BatchNorm
      const Raw& wr = kv.second;
      if (wr.shape[1] == 1 && wr.shape[0] > 1 && (wr.shape[2] == 3 || wr.shape[2] == 7)) {
        cw_[pre] = fold_dw(pre);  // depthwise 3x3 (YOLO11 class branch, attention positional encoding), 7x7 (YOLO12's)
        continue;
      }
      cw_[pre] = fold(pre, pre == "model.0" ? 4 : 0);
    }
  }
  const std::string H = head_;
  for (int l = 0; l < 3; ++l) {
    const std::string ls = std::to_string(l);
    const std::string B = H + ".cv2." + ls, C = H + ".cv3." + ls, M = H + ".cv4." + ls;  // box, class, coefficient branches
    // OBB: the angle branch (max(ch0 / 4, 1) mid channels - 16 at scale n -, 1 output) zero-padded to the coefficient
    // branch's widths (at least nm_ = 32 mid channels, 32 outputs), so the head runs on the segment head's launches and the
    // angle logit lands in column RAW_COEF of the rows
    if (obb()) cw_[M + ".0"] = zero_pad(cw_.at(M + ".0"), hc4p_, cw_.at(M + ".0").cin);
    // the first 3x3 convs of the branches that start on the level's features as one conv (scale n: 64+64+32 outputs, box,
    // class and coefficient; YOLO11's class branch starts with a depthwise conv: 64+32)
    if (dwcls()) {
      head_first_[l] = concat_out({cw_.at(B + ".0"), cw_.at(M + ".0")});
      cls_dw1_[l] = cw_.at(C + ".0.0"), cls_pw1_[l] = cw_.at(C + ".0.1");
      cls_dw2_[l] = cw_.at(C + ".1.0"), cls_pw2_[l] = cw_.at(C + ".1.1");
    } else {
      head_first_[l] = concat_out({cw_.at(B + ".0"), cw_.at(C + ".0"), cw_.at(M + ".0")});
      head_cls2_[l] = cw_.at(C + ".1");
    }
    head_box2_[l] = cw_.at(B + ".1");
    head_coef2_[l] = obb() ? zero_pad(cw_.at(M + ".1"), hc4p_, hc4p_) : cw_.at(M + ".1");
    head_box3_[l] = plain(B + ".2");
    head_cls3_[l] = plain(C + ".2");
    // v8: the class branch's final 1x1 padded to a 32-column block (zero weights and bias past the classes), which the 3x3
    // before it can chain (gemm_sp_chain_ok wants N2 % 32 == 0)
    if (!dwcls()) head_cls3_pad_[l] = plain(C + ".2", 32);
    head_coef3_[l] = obb() ? zero_pad(plain(M + ".2"), nm_, hc4p_) : plain(M + ".2");
  }
  // DFL weights must be arange(16) (they are a fixed buffer upstream); the decode kernel hard-codes them
  {
    const auto& d = raw_.at(H + ".dfl.conv.weight").data;
    for (int i = 0; i < reg_max_; ++i) MTGV_CHECK(d[i] == (float)i, ERR_INVALID, "dfl.conv.weight is not arange(16)");
  }
  // the prototype branch behind cv1: the ConvTranspose's phase matrices, and its fold into cv2
  if (!obb()) {
    const Raw& w = raw_.at(H + ".proto.upsample.weight");
    proto_w_ = proto_tail_weights(w.data.data(), raw_.at(H + ".proto.upsample.bias").data.data(), w.shape[0], w.shape[1],
                                  cw_.at(H + ".proto.cv2"), cw_.at(H + ".proto.cv3"), dev_allocs_);
  }

  plan_arena(arena());
  if (nms_ws_) (void)hipFree(nms_ws_);
  nms_ws_bytes_ = nms_workspace_bytes(cfg_.max_batch, na_);
  HIP_OK(hipMalloc((void**)&nms_ws_, nms_ws_bytes_));
  finalized_ = true;

  // algorithmic FLOPs of one frame: run the plan once in counting mode
  count_flops_ = true;
  flops_ = 0;
  run_graph(nullptr, 1, 0, nullptr);
  count_flops_ = false;
}

GemmArgs conv_desc(const ConvW& w, const View& in, const View& out, int stride, int act, int n) {
  return conv_args({in.p, n, in.H, in.W, in.ct, in.co, in.C, in.fmt}, w.w, w.b, w.cout, w.k, w.k, stride, w.k / 2,
                   {out.p, out.H, out.W, out.ct, out.co, out.fmt}, act);
}

void Detector::conv(const ConvW& w, const View& in, const View& out, int stride, int act, const View* res, int n, hipStream_t s) {
  MTGV_CHECK(in.C == w.cin && out.C == w.cout, ERR_RUNTIME, "detector: conv channel mismatch (%d->%d vs %d->%d)", in.C, out.C, w.cin,
             w.cout);
  GemmArgs g = conv_desc(w, in, out, stride, act, n);
  if (res) g.res = res->p + res->co, g.ldr = res->ct, g.res_fmt = res->fmt;
  if (count_flops_) {
    flops_ += 2.0 * g.M * g.N * g.K;
    return;
  }
  gemm_launch(g, s);
}

void conv_pair_launch(const ConvW& w1, const View& in, const View& mid, int stride, const ConvW& w2, const View& out2, int act2, int n,
                      hipStream_t s, double xflops) {
  MTGV_CHECK(in.C == w1.cin && mid.C == w1.cout && w2.cin == w1.cout && w2.k == 1 && out2.C == w2.cout, ERR_RUNTIME,
             "detector: conv pair channel mismatch (%d->%d, %d->%d)", w1.cin, w1.cout, w2.cin, w2.cout);
  const bool chain = env_int("MTGV_DET_CHAIN", 1) != 0;  // read per call (A/B in one process); 0: two launches
  if (in.fmt == 1 && chain) {
    GemmArgs g = conv_desc(w1, in, mid, stride, ACT_SILU, n);
    g.Out = nullptr;  // only the second layer's output is stored
    g.W2 = w2.w, g.bias2 = w2.b, g.Out2 = out2.p, g.N2 = w2.cout, g.ldo2 = out2.ct, g.o_off2 = out2.co, g.out_fmt2 = out2.fmt, g.act2 = act2;
    g.xflops = xflops;
    if (gemm_sp_chain_ok(g)) {
      gemm_launch(g, s);
      return;
    }
  }
  gemm_launch(conv_desc(w1, in, mid, stride, ACT_SILU, n), s);
  GemmArgs g2 = conv_desc(w2, mid, out2, 1, act2, n);
  g2.xflops = xflops;
  gemm_launch(g2, s);
}

void Detector::conv_pair(const ConvW& w1, const View& in, const View& mid, int stride, const ConvW& w2, const View& out2, int act2, int n,
                         hipStream_t s, double xflops) {
  if (count_flops_ || fmt_ != 1) {
    conv(w1, in, mid, stride, ACT_SILU, nullptr, n, s);
    conv(w2, mid, out2, 1, act2, nullptr, n, s);
    return;
  }
  conv_pair_launch(w1, in, mid, stride, w2, out2, act2, n, s, xflops);
}

// Bottleneck(c1, c2, shortcut, k = (3, 3)): out = cv2(cv1(x)) (+ x).  `out` may be x itself (in place: every output
// element is read as the residual by the wave that later stores it).
void Detector::bottleneck(const std::string& p, const View& x, const View& tmp, const View& out, bool shortcut, int n, hipStream_t s) {
  conv(cw_.at(p + ".cv1"), x, tmp, 1, ACT_SILU, nullptr, n, s);
  conv(cw_.at(p + ".cv2"), tmp, out, 1, ACT_SILU, shortcut ? &x : nullptr, n, s);
}

// CSP block (C2f, C3k2, A2C2f without attention): cv1 -> 2 chunks (A2C2f: 1); n inner modules (+shortcut), each reading the chunk before it and appended to
// the concat; cv2 over the concat
void Detector::csp_block(int idx, const View& in, const View& out, int n, hipStream_t s, const ConvW* pre, const View* pre_in) {
  const CspInfo& ci = csp_.at(idx);
  const int ch = ci.ch, lead = ci.lead();
  const std::string id = std::to_string(idx), P = "model." + id;
  const View cat = view("cat" + id), tmp = view("tmp" + id);
  // pre: the stride-2 Conv in front of this block, whose only consumer is cv1 - the pair runs as one launch where it can
  if (pre != nullptr) conv_pair(*pre, *pre_in, in, 2, cw_.at(P + ".cv1"), cat.slice(0, lead * ch), ACT_SILU, n, s);
  else conv(cw_.at(P + ".cv1"), in, cat.slice(0, lead * ch), 1, ACT_SILU, nullptr, n, s);
  const bool fuse = env_int("MTGV_DET_C2F_FUSE", 1) != 0;  // read per call (A/B in one process); 0: three launches
  for (int j = 0; j < ci.n; ++j) {
    const View src = cat.slice((lead - 1 + j) * ch, ch);
    const View dst = cat.slice((lead + j) * ch, ch);
    const std::string M = P + ".m." + std::to_string(j);
    // the last bottleneck and cv2 as one launch where there is a kernel for the block (c2f_tail.h): tmp and dst stay on chip.
    // The shapes are those of C2f's Bottleneck(ch -> ch -> ch): a half-width bottleneck (cv1 has ch / 2 outputs) and C3k
    // (its cv1 and cv2 are 1x1) fail them by construction, so the inner module's kind need not be asked.
    const ConvW &w1 = cw_.at(M + ".cv1"), &w2 = cw_.at(M + ".cv2"), &w3 = cw_.at(P + ".cv2");
    const bool tail_shapes = w1.k == 3 && w1.cin == ch && w1.cout == ch && w2.k == 3 && w2.cin == ch && w2.cout == ch && w3.k == 1 &&
                             w3.cin == (lead + ci.n) * ch && w3.cout == out.C;  // (anything else: conv() below reports it)
    if (j == ci.n - 1 && fuse && tail_shapes && !count_flops_ && fmt_ == 1 && cat.fmt == 1 && out.fmt == 1) {
      C2fTailArgs a;
      a.cat = cat.p, a.cat_ct = cat.ct, a.cat_co = cat.co, a.n_img = n, a.H = cat.H, a.W = cat.W;
      a.ch = ch, a.nb = ci.n, a.shortcut = ci.shortcut;
      a.w1 = w1.w, a.b1 = w1.b, a.w2 = w2.w, a.b2 = w2.b, a.w3 = w3.w, a.b3 = w3.b, a.cout = w3.cout;
      a.out = out.p, a.out_ct = out.ct, a.out_co = out.co;
      if (c2f_tail_ok(a)) {
        c2f_tail_launch(a, s);
        return;
      }
    }
    if (ci.c3k()) c3k(M, src, view("kcat" + id), tmp, dst, ci.shortcut, n, s);
    else bottleneck(M, src, tmp, dst, ci.shortcut, n, s);
  }
  conv(cw_.at(P + ".cv2"), cat.slice(0, (lead + ci.n) * ch), out, 1, ACT_SILU, nullptr, n, s);
}

// The stem kernels (detector_kernel.h) on n frames of H x W: cout = 16 (scale n) is conv0_u8_kernel, 32 / 48 / 64 (s,
// YOLOv8 m, YOLO11 m) conv0_u8_wide_kernel; `wide` asks for the wide kernel at 16 channels too (test surface).
// w [cout][3][3][4] BN-folded with a zero 4th input channel, out (n, H / 2, W / 2, cout) dense, SP8 or f32.
void stem_u8_launch(const uint8_t* frames, const float* w, const float* bias, float* out, int n, int H, int W, int cout, int flip, bool sp8,
                    bool wide, hipStream_t s) {
  // (the kernels' whole-word loads and their two or four output columns per thread need W % 8 == 0)
  MTGV_CHECK(n > 0 && H >= 2 && H % 2 == 0 && W >= 8 && W % 8 == 0, ERR_INVALID, "stem: n=%d frames of %d x %d (H even, W a multiple of 8)", n, H, W);
  MTGV_CHECK(cout == 16 || cout == 32 || cout == 48 || cout == 64, ERR_INVALID, "stem: cout=%d (16, 32, 48, 64)", cout);
  MTGV_CHECK(((uintptr_t)frames & 7) == 0, ERR_INVALID, "detector: the frame buffer must be 8-byte aligned");
  MTGV_CHECK(((uintptr_t)out & 127) == 0, ERR_INVALID, "stem: the output must be 128-byte aligned");
  if (cout == 16 && !wide) {
    const long total = (long)n * (H / 2) * (W / 8);
    const auto kern = sp8 ? conv0_u8_kernel<true> : conv0_u8_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, w, bias, out, H, W, flip, total);
  } else {
    const long total = (long)n * (H / 2) * (W / 4);
    const unsigned grid = (unsigned)((total + 255) / 256);
#define STEM_GO(C_)                                                                                                            \
  hipLaunchKernelGGL((sp8 ? conv0_u8_wide_kernel<true, C_> : conv0_u8_wide_kernel<false, C_>), dim3(grid), dim3(256), 0, s, frames, w, \
                     bias, out, H, W, flip, total)
    if (cout == 16) STEM_GO(16);
    else if (cout == 32) STEM_GO(32);
    else if (cout == 48) STEM_GO(48);
    else STEM_GO(64);
#undef STEM_GO
  }
  HIP_OK(hipGetLastError());
}

// model.0 (Conv 3 -> 16 / 32 / 48 / 64, k3 s2) on its own kernel straight from the uint8 frame
void Detector::conv0(const uint8_t* frames, int n, int flip, hipStream_t s) {
  const int H = cfg_.in_h, W = cfg_.in_w;
  const ConvW& w0 = cw_.at("model.0");
  const View l0 = view("l0");
  MTGV_CHECK(l0.H == H / 2 && l0.W == W / 2 && l0.ct == w0.cout && l0.co == 0 && w0.cin == 4 && w0.k == 3, ERR_RUNTIME,
             "detector: unexpected model.0 geometry");
  if (count_flops_) {  // K = 27: the weights' zero 4th input channel is not counted
    flops_ += 2.0 * n * l0.H * l0.W * w0.cout * 27.0;
    return;
  }
  stem_u8_launch(frames, w0.w, w0.b, l0.p, n, H, W, w0.cout, flip, fmt_ == 1, false, s);
}


// head rows of n frames -> pred (n, 4 + nc + nm, na)
static void decode_launch(const HeadRows& rows, int n, int nc, int nm, float* pred, hipStream_t s) {
  const int na = head_rows_anchors(rows);
  const long tot = (long)n * na;
  hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, rows, pred, n, nc, nm, na);
  HIP_OK(hipGetLastError());
}

HeadRows Detector::head_rows() const {
  return HeadRows{v_.at("rawhead0").p, v_.at("rawhead1").p, v_.at("rawhead2").p, cfg_.imgsz, RAW_CT, RAW_CLS, RAW_COEF, cfg_.in_h, cfg_.in_w};
}

// the raw head rows of the first n frames -> pred
void Detector::decode(int n, hipStream_t s) {
  if (obb()) {
    const long tot = (long)n * na_;
    hipLaunchKernelGGL(decode_obb_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, head_rows(), v_.at("pred").p, n, cfg_.nc, na_);
    HIP_OK(hipGetLastError());
  } else {
    decode_launch(head_rows(), n, cfg_.nc, nm_, v_.at("pred").p, s);
  }
  pred_n_ = n;
}

// (decode ->) NMS -> mask logits of the kept detections
void Detector::head_tail(int n, int* n_det, float* boxes, float* conf, int* cls, int* keep_idx, float* mask_logits, int mask_rows,
                         hipStream_t s) {
  float* const coef = v_.at("coef").p;
  if (head_direct_) {
    // NMS reads the class logits of every anchor, and the box and the coefficients of candidates only, from the head
    // rows: no pass that decodes every anchor into `pred` (raw() runs it when a caller asks for `pred`)
    nms_rows_launch(head_rows(), n, cfg_.nc, nm_, cfg_.conf, cfg_.iou, cfg_.max_det, 7680.0f, n_det, boxes, conf, cls, keep_idx, coef, nms_ws_,
                    nms_ws_bytes_, s);
    pred_n_ = 0;
  } else {
    decode(n, s);
    nms_launch(v_.at("pred").p, n, cfg_.nc, nm_, na_, cfg_.conf, cfg_.iou, cfg_.max_det, 7680.0f, n_det, boxes, conf, cls, keep_idx, coef,
               nms_ws_, nms_ws_bytes_, s);
  }
  join_into(s, 0);  // the prototype branch ran beside the heads, decode and NMS (one workgroup per frame: 32 of 256 CUs)
  if (mask_logits != nullptr) {
    const View pr = view("protos");
    // the prototypes are a quarter of the input in both directions: one crop scale (pr.W / in_w, = pr.H / in_h)
    const float crop_scale = (float)pr.W / (float)cfg_.in_w;
    // (the FLOP count is of GEMM launches: it takes the batched GEMM at every size)
    mask_logits_launch({coef, pr.p, n_det, boxes, n, cfg_.max_det, nm_, pr.H, pr.W, crop_scale, mask_rows, mask_logits},
                       count_flops_ ? MASK_FORM_GEMM : MASK_FORM_AUTO, s);
  }
}

// masks = coeffs @ protos^T per image, cropped to the box (process_mask / crop_mask)
void mask_logits_launch(const MaskLogitsArgs& a, int form, hipStream_t s) {
  MTGV_CHECK(form == MASK_FORM_AUTO || form == MASK_FORM_PIXELS || form == MASK_FORM_GEMM, ERR_INVALID, "mask_logits: form=%d", form);
  MTGV_CHECK(a.coef && a.protos && a.n_det && a.boxes && a.out, ERR_INVALID, "mask_logits: null tensor");
  MTGV_CHECK(a.n > 0 && a.n <= 65535 && a.nm > 0 && a.mh > 0 && a.mw > 0 && a.mask_rows > 0 && a.mask_rows <= a.max_det, ERR_INVALID,
             "mask_logits: n=%d nm=%d map %d x %d mask_rows=%d max_det=%d", a.n, a.nm, a.mh, a.mw, a.mask_rows, a.max_det);
  const bool pixels_ok = mask_logits_pixels_ok(a.nm, a.mask_rows);
  MTGV_CHECK(form != MASK_FORM_PIXELS || pixels_ok, ERR_INVALID, "mask_logits: the per-pixel kernel needs nm == 32 and mask_rows <= 16 (nm=%d, mask_rows=%d)",
             a.nm, a.mask_rows);
  const int npx = a.mh * a.mw;
  if (form == MASK_FORM_PIXELS || (form == MASK_FORM_AUTO && pixels_ok)) {  // a handful of masks per frame: one pass over the prototypes
    hipLaunchKernelGGL(mask_logits_kernel, dim3((unsigned)((npx + 255) / 256), (unsigned)a.n), dim3(256), 0, s, a.coef, a.protos, a.n_det,
                       a.boxes, a.out, npx, a.mw, a.mask_rows, a.max_det, a.crop_scale);
    HIP_OK(hipGetLastError());
    return;
  }
  // the batched GEMM writes only the rows of kept detections: the rest is cleared first
  HIP_OK(hipMemsetAsync(a.out, 0, (size_t)a.n * a.mask_rows * npx * sizeof(float), s));
  GemmArgs g = linear_args(a.coef, a.nm, a.protos, nullptr, a.out, npx, a.mask_rows, npx, a.nm, ACT_NONE);
  g.batch = a.n;
  g.strideA = (long)a.max_det * a.nm;
  g.strideW = (long)npx * a.nm;
  g.strideO = (long)a.mask_rows * npx;
  g.m_count = a.n_det;
  g.crop_boxes = a.boxes;
  g.crop_rows = a.max_det;
  g.crop_scale = a.crop_scale;
  g.crop_w = a.mw;
  gemm_launch(g, s);
}

void Detector::forward(const uint8_t* frames, int n, int flip, int* n_det, float* boxes, float* conf, int* cls, int* keep_idx,
                       float* mask_logits, int mask_rows, hipStream_t s) {
  MTGV_CHECK(finalized_, ERR_RUNTIME, "detector: finalize() has not been called");
  MTGV_CHECK(!obb(), ERR_INVALID, "mtgv_detector_forward on an OBB handle (task 1): call mtgv_detector_forward_obb");
  MTGV_CHECK(n > 0 && n <= cfg_.max_batch, ERR_INVALID, "batch %d outside [1, %d]", n, cfg_.max_batch);
  MTGV_CHECK(frames && n_det && boxes && conf && cls && keep_idx, ERR_INVALID, "null tensor");
  MTGV_CHECK(mask_logits == nullptr || (mask_rows > 0 && mask_rows <= cfg_.max_det), ERR_INVALID, "mask_rows=%d", mask_rows);
  run_graph(frames, n, flip, s);
  head_tail(n, n_det, boxes, conf, cls, keep_idx, mask_logits, mask_rows, s);
  last_n_ = n;
}

// OBB: the same graph without the prototype branch, then decode every anchor and rotated NMS on `pred`
void Detector::forward_obb(const uint8_t* frames, int n, int flip, int* n_det, float* rboxes, float* conf, int* cls, int* keep_idx,
                           hipStream_t s) {
  MTGV_CHECK(finalized_, ERR_RUNTIME, "detector: finalize() has not been called");
  MTGV_CHECK(obb(), ERR_INVALID, "mtgv_detector_forward_obb on a segment handle (task 0): call mtgv_detector_forward");
  MTGV_CHECK(n > 0 && n <= cfg_.max_batch, ERR_INVALID, "batch %d outside [1, %d]", n, cfg_.max_batch);
  MTGV_CHECK(frames && n_det && rboxes && conf && cls && keep_idx, ERR_INVALID, "null tensor");
  run_graph(frames, n, flip, s);
  decode(n, s);
  nms_rotated_launch(v_.at("pred").p, n, cfg_.nc, na_, cfg_.conf, cfg_.iou, cfg_.max_det, 7680.0f, n_det, rboxes, conf, cls, keep_idx, nms_ws_,
                     nms_ws_bytes_, s);
  last_n_ = n;
}

void Detector::run_graph(const uint8_t* frames, int n, int flip, hipStream_t s) {
  // f16x3 on the LDS-DMA kernel: every intermediate activation is kept in SP8; the frame, the raw head rows and the
  // prototypes (decode / mask inputs) stay f32
  fmt_ = (!count_flops_ && gemm_sp_active()) ? 1 : 0;
  head_direct_ = env_int("MTGV_DET_HEAD_DIRECT", 1) != 0;  // read per call (A/B in one process); 0: class 3x3 + 1x1, decode, NMS on pred
  forward_graph(frames, n, flip, s);
}

// SPPF: cv1, three chained 5x5 max pools, cv2 over the concat
void Detector::sppf(const std::string& P, const View& in, const View& spp, const View& out, int n, hipStream_t s) {
  const int ch = spp.ct / 4;
  conv(cw_.at(P + ".cv1"), in, spp.slice(0, ch), 1, ACT_SILU, nullptr, n, s);
  const size_t pools_lds = (size_t)spp.H * spp.W * 64;  // two images of (hi, lo) pieces
  const bool pools1 = env_int("MTGV_SPPF_POOLS1", 1) != 0;  // read per call (A/B in one process); 0: three launches
  if (!count_flops_ && fmt_ == 1 && pools1 && pools_lds <= 64 * 1024 && ch % 8 == 0) {
    hipLaunchKernelGGL(sppf_pools_sp8_kernel, dim3((unsigned)(n * (ch / 8))), dim3(256), pools_lds, s, spp.p, spp.ct, ch, spp.H, spp.W);
    HIP_OK(hipGetLastError());
  } else if (!count_flops_)
    for (int i = 0; i < 3; ++i) {
      if (fmt_ == 1) {
        const long total = (long)n * spp.H * spp.W * (ch / 8);
        hipLaunchKernelGGL(maxpool5_sp8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, spp.p, spp.ct, i * ch, spp.p,
                           spp.ct, (i + 1) * ch, spp.H, spp.W, ch, total);
        HIP_OK(hipGetLastError());
      } else {
        maxpool5_launch(spp.p, spp.ct, i * ch, spp.p, spp.ct, (i + 1) * ch, n, spp.H, spp.W, ch, s);
      }
    }
  conv(cw_.at(P + ".cv2"), spp, out, 1, ACT_SILU, nullptr, n, s);
}

// nearest-neighbour 2x of `in` into the leading channels of `out` (whole elements move: either format)
void Detector::upsample2x(const View& in, const View& out, int n, hipStream_t s) {
  if (count_flops_) return;
  upsample2x_launch(in.p, in.ct, in.co, out.p, out.ct, out.co, n, in.H, in.W, in.C, s);
}

void Detector::forward_graph(const uint8_t* frames, int n, int flip, hipStream_t s) {
  conv0(frames, n, flip, s);
  neck_and_heads(v11() ? backbone_v11(n, s) : v12() ? backbone_v12(n, s) : backbone_v8(n, s), n, s);
}

// yolov8 nodes 1 .. 9 behind conv0; returns node 9
View Detector::backbone_v8(int n, hipStream_t s) {
  const int c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  auto V = [&](const char* k) -> View { return view(k); };
  const View l0 = V("l0");
  csp_block(2, V("l1"), V("l2"), n, s, &cw_.at("model.1"), &l0);  // model.1 (3x3 s2) + cv1 in one launch: l1 is never stored
  // (model.3 + node 4's cv1 measured 6 us SLOWER chained - 94 vs 61 + 27 - and stay two launches)
  conv(cw_.at("model.3"), V("l2"), V("l3"), 2, ACT_SILU, nullptr, n, s);
  const View n4 = V("cat14").slice(c128, c64);      // node 4 output lives in concat 14 = [up(12), 4]
  csp_block(4, V("l3"), n4, n, s);
  conv(cw_.at("model.5"), n4, V("l5"), 2, ACT_SILU, nullptr, n, s);
  const View n6 = V("cat11").slice(c256, c128);     // concat 11 = [up(9), 6]
  csp_block(6, V("l5"), n6, n, s);
  conv(cw_.at("model.7"), n6, V("l7"), 2, ACT_SILU, nullptr, n, s);
  csp_block(8, V("l7"), V("l8"), n, s);
  const View n9 = V("cat20").slice(c128, c256);     // concat 20 = [19, 9]
  sppf("model.9", V("l8"), V("sppcat"), n9, n, s);
  return n9;
}

// From the first upsample to the P5 head, on the backbone's last node `top` (9 + k, in concat 20 + k) and its nodes 4
// and 6 (in concats 14 + k and 11 + k).  Node numbers are YOLOv8's; YOLO11's are one higher, YOLO12's one lower.  A concat's slices are as wide
// as the views that fill them.
void Detector::neck_and_heads(const View& top, int n, hipStream_t s) {
  const int k = shift();
  auto cat = [&](int i) { return view("cat" + std::to_string(i + k)); };
  auto w = [&](int i) -> const ConvW& { return cw_.at("model." + std::to_string(i + k)); };
  const View cat11 = cat(11), cat14 = cat(14), cat17 = cat(17), cat20 = cat(20);
  const View p3 = view("p3"), p4 = view("p4"), p5 = view("p5");
  // top-down
  upsample2x(top, cat11, n, s);
  const View n12 = cat17.slice(p3.C, cat17.ct - p3.C);  // concat 17 = [16, 12]
  csp_block(12 + k, cat11, n12, n, s);
  upsample2x(n12, cat14, n, s);
  csp_block(15 + k, cat14, p3, n, s);
  // P3 exists: the prototype branch (0.5 ms of chip-filling launches) and the P3 head leave the caller's stream; the
  // rest of the neck - 100..400-tile launches that cannot fill 256 CUs on their own - runs beside them
  if (!obb()) proto(head_, p3, n, fork_after(s, 0));
  head_level(0, n, fork_after(s, 1));
  conv(w(16), p3, cat17.slice(0, p3.C), 2, ACT_SILU, nullptr, n, s);
  csp_block(18 + k, cat17, p4, n, s);
  head_level(1, n, fork_after(s, 2));
  conv(w(19), p4, cat20.slice(0, p4.C), 2, ACT_SILU, nullptr, n, s);
  csp_block(21 + k, cat20, p5, n, s);
  head_level(2, n, s);
  join_into(s, 1), join_into(s, 2);  // (the prototype branch is joined in head_tail, after decode + NMS)
}

// YOLOv8's class branch behind head_first_: 3x3 t1 -> t2, 1x1 t2 -> the rows' class columns
void Detector::head_cls_v8(int l, const View& t1, const View& t2, const View& rh, int n, hipStream_t s) {
  if (head_direct_ && !count_flops_ && fmt_ == 1) {  // (f32 activations chain nothing: the 1x1 keeps its nc columns)
    // one launch, the 1x1 padded to the 32 columns behind RAW_CLS (its nc outputs alone are no column block of the
    // chain); the launch profiler keeps counting the nc real outputs of the 1x1
    const double pad_flops = 2.0 * n * rh.H * rh.W * (double)(head_cls3_pad_[l].cout - cfg_.nc) * head_cls3_pad_[l].cin;
    conv_pair(head_cls2_[l], t1, t2, 1, head_cls3_pad_[l], rh.slice(RAW_CLS, 32), ACT_NONE, n, s, -pad_flops);
  } else {
    conv(head_cls2_[l], t1, t2, 1, ACT_SILU, nullptr, n, s);
    conv(head_cls3_[l], t2, rh.slice(RAW_CLS, cfg_.nc), 1, ACT_NONE, nullptr, n, s);
  }
}

// Head of level l (P3 / P4 / P5): the first 3x3 convs of the branches that start on the features as one launch
// (head_first_), then per branch 3x3 -> 1x1; YOLO11's class branch is a chain of its own on the features
void Detector::head_level(int l, int n, hipStream_t s) {
  const char* feats[3] = {"p3", "p4", "p5"};
  const std::string ls = std::to_string(l);
  const View f = view(feats[l]), t1 = view("t1_" + ls), t2 = view("t2_" + ls);
  const View rh = view("rawhead" + ls);
  conv(head_first_[l], f, t1, 1, ACT_SILU, nullptr, n, s);
  // every branch: the 3x3 and the final 1x1 as one launch.  head_first_ stacks the box branch first and the coefficient
  // branch last (64 and 32 channels at scale n), YOLOv8's class branch (64) between them.
  const int c2 = hc2_, c4 = hc4p_, o4 = head_first_[l].cout - c4;
  conv_pair(head_box2_[l], t1.slice(0, c2), t2.slice(0, c2), 1, head_box3_[l], rh.slice(0, 4 * reg_max_), ACT_NONE, n, s);
  // (the class branch is enqueued between the two pairs for YOLOv8 and behind them for YOLO11)
  if (!dwcls()) head_cls_v8(l, t1.slice(c2, hc3_), t2.slice(c2, hc3_), rh, n, s);
  conv_pair(head_coef2_[l], t1.slice(o4, c4), t2.slice(o4, c4), 1, head_coef3_[l], rh.slice(RAW_COEF, nm_), ACT_NONE, n, s);
  if (dwcls()) head_cls_v11(l, f, rh, n, s);
  obb_flops_fix(f);
}

// the OBB angle branch runs zero-padded to the coefficient branch's widths (hc4p_ mid channels, nm_ outputs); the
// algorithmic count is of the real c4 -> c4 -> 1 branch (c4 = 16 at scale n)
void Detector::obb_flops_fix(const View& f) {
  if (!count_flops_ || !obb()) return;
  const double px = (double)f.H * f.W;
  const int c4 = hc4_, c4p = hc4p_, ne = 1;
  flops_ -= 2.0 * px * (9.0 * f.C * (c4p - c4) + 9.0 * (c4p * c4p - c4 * c4) + (c4p * nm_ - c4 * ne));
}

void Detector::raw(int n, float* pred, float* protos, hipStream_t s) {
  MTGV_CHECK(n > 0 && n <= last_n_, ERR_INVALID, "raw: n=%d but the last forward had %d frames", n, last_n_);
  MTGV_CHECK(!obb() || protos == nullptr, ERR_INVALID, "raw: an OBB handle has no prototypes (protos_dev must be NULL)");
  if (pred && pred_n_ < n) decode(n, s);  // the last forward ran NMS straight from the head rows
  if (pred) HIP_OK(hipMemcpyAsync(pred, v_.at("pred").p, (size_t)n * no() * na_ * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (protos) {
    const View pr = v_.at("protos");
    const long hw = (long)pr.H * pr.W, total = (long)n * nm_ * hw;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pr.p, protos, nm_, hw, total);
    HIP_OK(hipGetLastError());
  }
}

}  // namespace mtgv

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace mtgv;
struct mtgv_detector {
  Detector impl;
  explicit mtgv_detector(const mtgv_detector_cfg& c) : impl(c) {}
};

extern "C" {
MTGV_API int mtgv_detector_create(const mtgv_detector_cfg* cfg, mtgv_detector** out) {
  return guarded([&] {
    MTGV_CHECK(cfg != nullptr && out != nullptr, ERR_INVALID, "null argument");
    *out = new mtgv_detector(*cfg);
  });
}
MTGV_API void mtgv_detector_destroy(mtgv_detector* h) { delete h; }
MTGV_API int mtgv_detector_set_param(mtgv_detector* h, const char* key, const float* data_host, int64_t numel) {
  return guarded([&] {
    MTGV_CHECK(h && key && data_host, ERR_INVALID, "null argument");
    h->impl.set_param(key, data_host, numel);
  });
}
MTGV_API int mtgv_detector_missing_params(const mtgv_detector* h) { return h ? h->impl.missing() : -1; }
MTGV_API int mtgv_detector_finalize(mtgv_detector* h) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.finalize();
  });
}
MTGV_API int mtgv_detector_forward(mtgv_detector* h, const uint8_t* frames_dev, int32_t n, int32_t flip_rgb, int32_t* n_det_dev,
                                   float* boxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev,
                                   float* mask_logits_dev, int32_t mask_rows, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.forward(frames_dev, n, flip_rgb, n_det_dev, boxes_dev, conf_dev, cls_dev, keep_idx_dev, mask_logits_dev, mask_rows,
                    (hipStream_t)stream);
  });
}
MTGV_API int mtgv_detector_forward_obb(mtgv_detector* h, const uint8_t* frames_dev, int32_t n, int32_t flip_rgb, int32_t* n_det_dev,
                                       float* rboxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.forward_obb(frames_dev, n, flip_rgb, n_det_dev, rboxes_dev, conf_dev, cls_dev, keep_idx_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_detector_raw(mtgv_detector* h, int32_t n, float* pred_dev, float* protos_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null handle");
    h->impl.raw(n, pred_dev, protos_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_mask_binarize(const float* logits_dev, int32_t n, int32_t mh, int32_t mw, int32_t scale, uint8_t* out_dev,
                                void* stream) {
  return guarded([&] {
    MTGV_CHECK(logits_dev && out_dev && n >= 0 && mh > 0 && mw > 0 && scale > 0, ERR_INVALID, "mask_binarize: bad argument");
    const long npx = (long)n * mh * scale * mw * scale;
    if (npx == 0) return;
    if ((mw * scale) % 16 == 0 && ((uintptr_t)out_dev % 16) == 0) {
      const long total = npx / 16;
      hipLaunchKernelGGL((mask_binarize_kernel<16>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits_dev,
                         out_dev, mh, mw, scale, total);
    } else {
      hipLaunchKernelGGL((mask_binarize_kernel<1>), dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits_dev,
                         out_dev, mh, mw, scale, npx);
    }
    HIP_OK(hipGetLastError());
  });
}
MTGV_API int mtgv_op_mask_logits(const float* coef_dev, const float* protos_dev, const int32_t* n_det_dev, const float* boxes_dev,
                                 int32_t n, int32_t max_det, int32_t nm, int32_t mh, int32_t mw, float crop_scale, int32_t mask_rows,
                                 int32_t form, float* out_dev, void* stream) {
  return guarded([&] {
    mask_logits_launch({coef_dev, protos_dev, n_det_dev, boxes_dev, n, max_det, nm, mh, mw, crop_scale, mask_rows, out_dev}, form,
                       (hipStream_t)stream);
  });
}
static HeadRows op_head_rows(const mtgv_head_rows* r) {
  MTGV_CHECK(r != nullptr && r->r0 && r->r1 && r->r2, ERR_INVALID, "null head rows");
  return HeadRows{r->r0, r->r1, r->r2, r->imgsz, r->ct, r->cls, r->coef, r->h, r->w};
}
MTGV_API int mtgv_op_decode(const mtgv_head_rows* rows, int32_t n, int32_t nc, int32_t nm, float* pred_dev, void* stream) {
  return guarded([&] {
    const HeadRows h = op_head_rows(rows);
    MTGV_CHECK(pred_dev && n > 0, ERR_INVALID, "decode: pred %p, n=%d", (void*)pred_dev, n);
    head_rows_check(h, nc, nm);
    decode_launch(h, n, nc, nm, pred_dev, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_nms_raw(const mtgv_head_rows* rows, int32_t n, int32_t nc, int32_t nm, float conf, float iou, int32_t max_det,
                             float max_wh, int32_t* n_det_dev, float* boxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev,
                             float* coef_dev, int32_t* workspace_dev, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    MTGV_CHECK(n_det_dev && boxes_dev && conf_dev && cls_dev && keep_idx_dev, ERR_INVALID, "null argument");
    nms_rows_launch(op_head_rows(rows), n, nc, nm, conf, iou, max_det, max_wh, n_det_dev, boxes_dev, conf_dev, cls_dev, keep_idx_dev, coef_dev,
                    workspace_dev, workspace_bytes, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_stem_u8(const uint8_t* frames_dev, const float* w_dev, const float* bias_dev, float* out_dev, int32_t n, int32_t h,
                             int32_t w, int32_t cout, int32_t flip_rgb, int32_t out_sp8, int32_t wide, void* stream) {
  return guarded([&] {
    MTGV_CHECK(frames_dev && w_dev && bias_dev && out_dev, ERR_INVALID, "null argument");
    stem_u8_launch(frames_dev, w_dev, bias_dev, out_dev, n, h, w, cout, flip_rgb, out_sp8 != 0, wide != 0, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_detector_set_fork(mtgv_detector* h, int32_t mode) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && mode >= -1 && mode <= 1, ERR_INVALID, "mtgv_detector_set_fork: handle %p, mode %d (-1, 0, 1)", (void*)h, mode);
    h->impl.set_fork(mode);
  });
}
MTGV_API int mtgv_detector_flops(const mtgv_detector* h, double* flops_per_frame) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr && flops_per_frame != nullptr, ERR_INVALID, "null argument");
    *flops_per_frame = h->impl.flops_per_frame();
  });
}
}
