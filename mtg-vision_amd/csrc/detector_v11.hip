// YOLO11-seg / -obb (scales n, s, m) on the GPU: the modules YOLOv8 does not have (ultralytics 8.3.x nn/modules: C3k2, C3k, C2PSA / PSABlock /
// Attention, DWConv, Detect(legacy=False) class branch - third-party to the reference, which trains this family by
// default: mtgvision/od_train.py:20, :55-56, :138-151).  Conv / C2f-skeleton / SPPF / Proto / decode / NMS / masks are
// shared with detector.hip; every 1x1 and 3x3 convolution runs on the split-precision implicit GEMM.
//   dwconv3_kernel   depthwise 3x3 + folded BN (+ SiLU) (+ f32 addend), f32 or SP8 in / out, channel-group gather
//   attn_kernel      softmax(q^T k / sqrt(kd)) v per (image, head): f32 VALU, online softmax, K / V staged in LDS
#include "act.h"
#include "detector.h"
#include "gemm_sp.h"
#include "rowops.h"
#include "sp8.h"

#include <math.h>

namespace mtgv {

// ---------------------------------------------------------------------------
// depthwise 3x3, stride 1, pad 1.  One thread = one pixel x 8 channels.
// input channel of output channel c: (c / g_size) * g_stride + c % g_size (+ the view's offset) - the positional
// encoding of Attention reads the v rows out of the qkv tensor that way.
// ---------------------------------------------------------------------------
template <bool IN_SP8, bool OUT_SP8>
__global__ __launch_bounds__(256) void dwconv3_kernel(const float* __restrict__ in, int ci_total, int ci_off, int g_size, int g_stride,
                                                     const float* __restrict__ w9, const float* __restrict__ bias,
                                                     const float* __restrict__ add, int add_ld, float* __restrict__ out,
                                                     int co_total, int co_off, int H, int W, int C, int act, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over N*H*W*(C/8)
  if (idx >= total) return;
  const int c8n = C >> 3;
  const int c = (int)(idx % c8n) * 8;
  long t = idx / c8n;
  const int x = (int)(t % W);
  t /= W;
  const int y = (int)(t % H);
  const long n = t / H;
  const int cin = (c / g_size) * g_stride + (c % g_size) + ci_off;
  f32x4 a0 = *reinterpret_cast<const f32x4*>(bias + c), a1 = *reinterpret_cast<const f32x4*>(bias + c + 4);
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int iy = y + kh - 1;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ix = x + kw - 1;
      if (ix < 0 || ix >= W) continue;
      const float* p = in + ((n * H + iy) * W + ix) * (long)ci_total + cin;
      f32x4 v0, v1;
      if (IN_SP8) {
        const sp_h8 hi = reinterpret_cast<const sp_h8*>(p)[0], lo = reinterpret_cast<const sp_h8*>(p)[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) v0[e] = (float)hi[e] + (float)lo[e], v1[e] = (float)hi[4 + e] + (float)lo[4 + e];
      } else {
        v0 = reinterpret_cast<const f32x4*>(p)[0], v1 = reinterpret_cast<const f32x4*>(p)[1];
      }
      const float* wp = w9 + (kh * 3 + kw) * C + c;
      const f32x4 w0 = reinterpret_cast<const f32x4*>(wp)[0], w1 = reinterpret_cast<const f32x4*>(wp)[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) a0[e] = __builtin_fmaf(v0[e], w0[e], a0[e]), a1[e] = __builtin_fmaf(v1[e], w1[e], a1[e]);
    }
  }
  if (act == ACT_SILU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a0[e] = act_silu(a0[e]), a1[e] = act_silu(a1[e]);
  }
  const long pix = (n * H + y) * W + x;
  if (add != nullptr) {
    const float* q = add + pix * add_ld + c;
    a0 = a0 + reinterpret_cast<const f32x4*>(q)[0], a1 = a1 + reinterpret_cast<const f32x4*>(q)[1];
  }
  float* o = out + pix * co_total + co_off + c;
  if (OUT_SP8) {
    sp_h8 hi, lo;
    sp8_split8(a0, a1, hi, lo);
    reinterpret_cast<sp_h8*>(o)[0] = hi, reinterpret_cast<sp_h8*>(o)[1] = lo;
  } else {
    reinterpret_cast<f32x4*>(o)[0] = a0, reinterpret_cast<f32x4*>(o)[1] = a1;
  }
}

// ---------------------------------------------------------------------------
// Attention core.  qkv (B, N, heads * (2 kd + hd)) f32, per head [q kd | k kd | v hd]; out (B, N, heads * hd) f32.
// Block = (query tile of 256, head, image); a thread owns one query: q in registers, keys / values stream through LDS
// in chunks of KC, softmax is the online form (running maximum and sum), one rescale per chunk.
// ---------------------------------------------------------------------------
template <int KD, int HD, int KC>
__global__ __launch_bounds__(256) void attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int heads,
                                                  float scale) {
  __shared__ __attribute__((aligned(16))) float ks[KC][KD];
  __shared__ __attribute__((aligned(16))) float vs[KC][HD];
  const int tid = threadIdx.x;
  const int qi = blockIdx.x * 256 + tid;
  const int head = blockIdx.y;
  const long img = blockIdx.z;
  const int ld = heads * (2 * KD + HD);
  const float* base = qkv + img * N * ld + head * (2 * KD + HD);
  float q[KD], acc[HD];
  const bool live = qi < N;
#pragma unroll
  for (int d = 0; d < KD; ++d) q[d] = live ? base[(long)qi * ld + d] * scale : 0.f;
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < N; k0 += KC) {
    __syncthreads();
    for (int i = tid; i < KC * (KD / 4); i += 256) {
      const int r = i / (KD / 4), c4 = i % (KD / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + r < N) v = *reinterpret_cast<const f32x4*>(base + (long)(k0 + r) * ld + KD + c4 * 4);
      *reinterpret_cast<f32x4*>(&ks[r][c4 * 4]) = v;
    }
    for (int i = tid; i < KC * (HD / 4); i += 256) {
      const int r = i / (HD / 4), c4 = i % (HD / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + r < N) v = *reinterpret_cast<const f32x4*>(base + (long)(k0 + r) * ld + 2 * KD + c4 * 4);
      *reinterpret_cast<f32x4*>(&vs[r][c4 * 4]) = v;
    }
    __syncthreads();
    const int kn = (N - k0) < KC ? (N - k0) : KC;
    float sc[KC];
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      float dsum = 0.f;
#pragma unroll
      for (int d = 0; d < KD; ++d) dsum = __builtin_fmaf(q[d], ks[j][d], dsum);
      sc[j] = j < kn ? dsum : -INFINITY;
      cm = fmaxf(cm, sc[j]);
    }
    const float mn = fmaxf(m, cm);
    const float f = __expf(m - mn);  // 0 on the first chunk (m = -inf)
    l *= f;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] *= f;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const float pj = __expf(sc[j] - mn);  // exp(-inf) = 0 for the padding keys
      l += pj;
#pragma unroll
      for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(pj, vs[j][d], acc[d]);
    }
    m = mn;
  }
  if (!live) return;
  const float inv = 1.0f / l;
  float* o = out + (img * N + qi) * (long)(heads * HD) + head * HD;
#pragma unroll
  for (int d = 0; d < HD; d += 4) {
    const f32x4 v = {acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
    *reinterpret_cast<f32x4*>(o + d) = v;
  }
}

// ---------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------
// depthwise Conv2d(c, c, 3, groups=c, bias=False) + BatchNorm2d(eps 1e-3) -> weight [9][c] (tap-major), bias [c]
ConvW Detector::fold_dw(const std::string& p) {
  const Raw& w = raw_.at(p + ".conv.weight");
  const int c = w.shape[0];
  std::vector<float> wf((size_t)9 * c), bf(c);
  for (int o = 0; o < c; ++o) {
    const auto [sc, bias] = bn_affine(p, o);
    bf[o] = (float)bias;
    for (int t = 0; t < 9; ++t) wf[(size_t)t * c + o] = (float)((double)w.data[(size_t)o * 9 + t] * sc);
  }
  return ConvW{upload(wf), upload(bf), c, c, 3};
}

void Detector::dwconv(const ConvW& w, const View& in, const View& out, int act, const float* add, int g_size, int g_stride, int n,
                      hipStream_t s) {
  MTGV_CHECK(out.C == w.cout && w.cout % 8 == 0, ERR_RUNTIME, "detector: depthwise conv channel mismatch");
  if (count_flops_) {
    flops_ += 2.0 * 9.0 * n * out.H * out.W * w.cout;
    return;
  }
  const int gs = g_size > 0 ? g_size : w.cout;
  const long total = (long)n * out.H * out.W * (w.cout / 8);
  const unsigned grid = (unsigned)((total + 255) / 256);
#define DW_GO(I_, O_)                                                                                                             \
  hipLaunchKernelGGL((dwconv3_kernel<I_, O_>), dim3(grid), dim3(256), 0, s, in.p, in.ct, in.co, gs, g_stride, w.w, w.b, add, w.cout, \
                     out.p, out.ct, out.co, out.H, out.W, w.cout, act, total)
  if (in.fmt == 1 && out.fmt == 1) DW_GO(true, true);
  else if (in.fmt == 1) DW_GO(true, false);
  else if (out.fmt == 1) DW_GO(false, true);
  else DW_GO(false, false);
#undef DW_GO
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// construction: expected ultralytics keys of yolo11{n,s,m}-seg / -obb
// ---------------------------------------------------------------------------
void Detector::build_v11() {
  auto P = [](int i) { return "model." + std::to_string(i); };
  const int c16 = chn(64), c32 = chn(128), c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  auto bott = [&](const std::string& p, int c1, int c_, int c2) {
    expect_conv_bn(p + ".cv1", c_, c1, 3);
    expect_conv_bn(p + ".cv2", c2, c_, 3);
  };
  const bool all_c3k = cfg_.scale >= 2;  // scales m, l, x: ultralytics sets c3k = True on every C3k2
  const int nrep = rep(2);
  MTGV_CHECK(nrep == 1, ERR_RUNTIME, "detector: C3k2 / C2PSA with %d inner modules", nrep);  // (l and x: 2)
  auto c3k2 = [&](int idx, int cin, int cout, bool c3k, double e) {
    c3k = c3k || all_c3k;
    const int ch = (int)(cout * e);
    const std::string p = P(idx);
    expect_conv_bn(p + ".cv1", 2 * ch, cin, 1);
    expect_conv_bn(p + ".cv2", cout, 3 * ch, 1);
    if (c3k) {
      const int c_ = ch / 2;
      expect_conv_bn(p + ".m.0.cv1", c_, ch, 1);
      expect_conv_bn(p + ".m.0.cv2", c_, ch, 1);
      expect_conv_bn(p + ".m.0.cv3", ch, 2 * c_, 1);
      for (int j = 0; j < 2; ++j) bott(p + ".m.0.m." + std::to_string(j), c_, c_, c_);
    } else {
      bott(p + ".m.0", ch, ch / 2, ch);
    }
    c3k2_[idx] = {cout, 1, ch, c3k};
  };
  expect_conv_bn(P(0), c16, 3, 3);
  expect_conv_bn(P(1), c32, c16, 3);
  c3k2(2, c32, c64, false, 0.25);
  expect_conv_bn(P(3), c64, c64, 3);
  c3k2(4, c64, c128, false, 0.25);
  expect_conv_bn(P(5), c128, c128, 3);
  c3k2(6, c128, c128, true, 0.5);
  expect_conv_bn(P(7), c256, c128, 3);
  c3k2(8, c256, c256, true, 0.5);
  expect_conv_bn(P(9) + ".cv1", c256 / 2, c256, 1);
  expect_conv_bn(P(9) + ".cv2", c256, c256 / 2 * 4, 1);
  {  // C2PSA(c256, n = 1): c = c256 / 2 (128 at scale n, 256 at s and m), heads = c / 64, key_dim = head_dim / 2
    const int c = c256 / 2, nh = std::max(c / 64, 1), kd = (c / nh) / 2;
    psa_n_ = nh;
    const std::string p = P(10);
    expect_conv_bn(p + ".cv1", 2 * c, c256, 1);
    expect_conv_bn(p + ".cv2", c256, 2 * c, 1);
    expect_conv_bn(p + ".m.0.attn.qkv", c + 2 * nh * kd, c, 1);
    expect_conv_bn(p + ".m.0.attn.proj", c, c, 1);
    expect_conv_bn(p + ".m.0.attn.pe", c, 1, 3);
    expect_conv_bn(p + ".m.0.ffn.0", 2 * c, c, 1);
    expect_conv_bn(p + ".m.0.ffn.1", c, 2 * c, 1);
    // (attn_kernel<32, 64> is the one instance: heads of 64 channels with 32-wide keys, any number of them)
    MTGV_CHECK(nh >= 1 && kd == 32 && c == nh * 64, ERR_INVALID, "detector: unexpected C2PSA geometry");
  }
  c3k2(13, c256 + c128, c128, false, 0.5);
  c3k2(16, c128 + c128, c64, false, 0.5);
  expect_conv_bn(P(17), c64, c64, 3);
  c3k2(19, c64 + c128, c128, false, 0.5);
  expect_conv_bn(P(20), c128, c128, 3);
  c3k2(22, c128 + c256, c256, true, 0.5);

  const int chs[3] = {c64, c128, c256};
  expect_head(chs);
}

// ---------------------------------------------------------------------------
// activation arena
// ---------------------------------------------------------------------------
std::vector<Detector::ArenaBuf> Detector::arena_v11() const {
  const int IH = cfg_.in_h, IW = cfg_.in_w;
  const int h2 = IH / 2, h4 = IH / 4, h8 = IH / 8, h16 = IH / 16, h32 = IH / 32;
  const int w2 = IW / 2, w4 = IW / 4, w8 = IW / 8, w16 = IW / 16, w32 = IW / 32;
  const int c16 = chn(64), c32 = chn(128), c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  const int pc = c256 / 2;  // C2PSA's hidden width: qkv is pc + 2 heads x 32 keys = 2 pc wide
  const int ht = hc2_ + hc4p_, c3 = hc3_;  // box + coefficient branches side by side (96 at scale n); class branch (64)
  std::vector<ArenaBuf> a;
  // C3k2 `idx` on an h x w map: the concat of cv1's two chunks and the inner module's output, C3k's own concat where the
  // inner module is one, and the bottlenecks' temporary (half the chunk width in both forms)
  auto c3k2 = [&](int idx, int h, int w) {
    static const char* const names[][3] = {{"cat2", "kcat2", "tmp2"},    {"cat4", "kcat4", "tmp4"},    {"cat6", "kcat6", "tmp6"},
                                           {"cat8", "kcat8", "tmp8"},    {"cat13", "kcat13", "tmp13"}, {"cat16", "kcat16", "tmp16"},
                                           {"cat19", "kcat19", "tmp19"}, {"cat22", "kcat22", "tmp22"}};
    static const int ids[] = {2, 4, 6, 8, 13, 16, 19, 22};
    const C3k2Info& ci = c3k2_.at(idx);
    for (size_t i = 0; i < sizeof(ids) / sizeof(ids[0]); ++i)
      if (ids[i] == idx) {
        a.push_back({names[i][0], h, w, 3 * ci.ch});
        if (ci.c3k) a.push_back({names[i][1], h, w, ci.ch});
        a.push_back({names[i][2], h, w, ci.ch / 2});
      }
  };
  auto add = [&](std::initializer_list<ArenaBuf> l) { a.insert(a.end(), l); };
  add({{"l0", h2, w2, c16}, {"l1", h4, w4, c32}});
  c3k2(2, h4, w4);
  add({{"l2", h4, w4, c64}, {"l3", h8, w8, c64}});
  c3k2(4, h8, w8);
  add({{"cat15", h8, w8, c128 + c128},  // concat 15 = [up(13), 4]
       {"l5", h16, w16, c128}});
  c3k2(6, h16, w16);
  add({{"cat12", h16, w16, c256 + c128},  // concat 12 = [up(10), 6]
       {"l7", h32, w32, c256}});
  c3k2(8, h32, w32);
  add({{"l8", h32, w32, c256}, {"sppcat", h32, w32, 2 * c256}, {"l9", h32, w32, c256},
       // (the attention core and the positional encoding read qkv and att in f32)
       {"psacat", h32, w32, 2 * pc}, {"qkv", h32, w32, 2 * pc, true}, {"att", h32, w32, pc, true}, {"atty", h32, w32, pc}, {"ffn", h32, w32, 2 * pc},
       {"cat21", h32, w32, c128 + c256}});  // concat 21 = [20, 10]
  c3k2(13, h16, w16);
  add({{"cat18", h16, w16, c64 + c128}});  // concat 18 = [17, 13]
  c3k2(16, h8, w8);
  add({{"p3", h8, w8, c64}});
  c3k2(19, h16, w16);
  add({{"p4", h16, w16, c128}});
  c3k2(22, h32, w32);
  add({{"p5", h32, w32, c256},
       // head temporaries per level (the levels' branches run concurrently): box + coefficient branches, class branch
       {"t1_0", h8, w8, ht}, {"t2_0", h8, w8, ht}, {"dwa_0", h8, w8, c64}, {"dwb_0", h8, w8, c3}, {"dwc_0", h8, w8, c3}, {"dwd_0", h8, w8, c3},
       {"t1_1", h16, w16, ht}, {"t2_1", h16, w16, ht}, {"dwa_1", h16, w16, c128}, {"dwb_1", h16, w16, c3}, {"dwc_1", h16, w16, c3}, {"dwd_1", h16, w16, c3},
       {"t1_2", h32, w32, ht}, {"t2_2", h32, w32, ht}, {"dwa_2", h32, w32, c256}, {"dwb_2", h32, w32, c3}, {"dwc_2", h32, w32, c3}, {"dwd_2", h32, w32, c3},
       {"pr1", h8, w8, npr_}, {"pr2", h4, w4, npr_}, {"pr3", h4, w4, npr_}, {"protos", h4, w4, nm_, true},
       {"rawhead0", h8, w8, RAW_CT, true}, {"rawhead1", h16, w16, RAW_CT, true}, {"rawhead2", h32, w32, RAW_CT, true},
       {"pred", 1, na_, no(), true}, {"coef", 1, cfg_.max_det, nm_, true}});
  return a;
}

// ---------------------------------------------------------------------------
// modules
// ---------------------------------------------------------------------------
// Bottleneck(c1, c2, shortcut, k = (3, 3)): out = cv2(cv1(x)) (+ x).  `out` may be x itself (in place: every output
// element is read as the residual by the wave that later stores it).
void Detector::bottleneck(const std::string& p, const View& x, const View& tmp, const View& out, bool shortcut, int n, hipStream_t s) {
  conv(cw_.at(p + ".cv1"), x, tmp, 1, ACT_SILU, nullptr, n, s);
  conv(cw_.at(p + ".cv2"), tmp, out, 1, ACT_SILU, shortcut ? &x : nullptr, n, s);
}

// C3k2: the C2f skeleton (cv1 -> two chunks, one inner module appended, cv2 over the concat); the inner module is
// Bottleneck(c, c, e = 0.5) or C3k(c, c, 2) = cv3(cat(m(cv1(x)), cv2(x))) with two Bottlenecks(c/2, c/2, e = 1)
void Detector::c3k2(int idx, const View& in, const View& out, int n, hipStream_t s) {
  const C3k2Info& ci = c3k2_.at(idx);
  const int ch = ci.ch;
  const std::string P = "model." + std::to_string(idx);
  const View cat = view("cat" + std::to_string(idx));
  const View tmp = view("tmp" + std::to_string(idx));
  conv(cw_.at(P + ".cv1"), in, cat.slice(0, 2 * ch), 1, ACT_SILU, nullptr, n, s);
  const View src = cat.slice(ch, ch), dst = cat.slice(2 * ch, ch);
  if (ci.c3k) {
    const View kcat = view("kcat" + std::to_string(idx));
    const int c_ = ch / 2;
    const std::string M = P + ".m.0";
    const View a = kcat.slice(0, c_);
    conv(cw_.at(M + ".cv1"), src, a, 1, ACT_SILU, nullptr, n, s);
    for (int j = 0; j < 2; ++j) bottleneck(M + ".m." + std::to_string(j), a, tmp, a, true, n, s);
    conv(cw_.at(M + ".cv2"), src, kcat.slice(c_, c_), 1, ACT_SILU, nullptr, n, s);
    conv(cw_.at(M + ".cv3"), kcat, dst, 1, ACT_SILU, nullptr, n, s);
  } else {
    bottleneck(P + ".m.0", src, tmp, dst, true, n, s);
  }
  conv(cw_.at(P + ".cv2"), cat.slice(0, 3 * ch), out, 1, ACT_SILU, nullptr, n, s);
}

// C2PSA(c1, c1, n = 1, e = 0.5): a, b = cv1(x).split; b = b + attn(b); b = b + ffn(b); cv2(cat(a, b))
void Detector::c2psa(int idx, const View& in, const View& out, int n, hipStream_t s) {
  const std::string P = "model." + std::to_string(idx);
  const View cat = view("psacat");
  const int c = cat.ct / 2;
  constexpr int KD = 32, HD = 64;
  const int NH = psa_n_;  // c / 64 heads: 2 at scale n, 4 at s and m
  conv(cw_.at(P + ".cv1"), in, cat, 1, ACT_SILU, nullptr, n, s);
  const View b = cat.slice(c, c);
  const std::string A = P + ".m.0.attn";
  const View qkv = view("qkv"), att = view("att"), y = view("atty");
  conv(cw_.at(A + ".qkv"), b, qkv, 1, ACT_NONE, nullptr, n, s);
  const int N = cat.H * cat.W;
  if (count_flops_) {
    flops_ += 2.0 * n * NH * (double)N * N * (KD + HD);
  } else {
    hipLaunchKernelGGL((attn_kernel<KD, HD, 16>), dim3((N + 255) / 256, NH, n), dim3(256), 0, s, qkv.p, att.p, N, NH,
                       1.0f / sqrtf((float)KD));
    HIP_OK(hipGetLastError());
  }
  // y = attn_out + pe(v): depthwise 3x3 over the v rows of qkv (head h: channels h*(2 KD + HD) + 2 KD ...)
  View vin = qkv;
  vin.co = 2 * KD;
  dwconv(cw_.at(A + ".pe"), vin, y, ACT_NONE, att.p, HD, 2 * KD + HD, n, s);
  conv(cw_.at(A + ".proj"), y, b, 1, ACT_NONE, &b, n, s);                       // b += proj(y)
  const View f = view("ffn");
  conv(cw_.at(P + ".m.0.ffn.0"), b, f, 1, ACT_SILU, nullptr, n, s);
  conv(cw_.at(P + ".m.0.ffn.1"), f, b, 1, ACT_NONE, &b, n, s);                  // b += ffn(b)
  conv(cw_.at(P + ".cv2"), cat, out, 1, ACT_SILU, nullptr, n, s);
}

void Detector::forward_v11(const uint8_t* frames, int n, int flip, hipStream_t s) {
  const int c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  auto V = [&](const char* k) -> View { return view(k); };
  conv0(frames, n, flip, s);
  conv(cw_.at("model.1"), V("l0"), V("l1"), 2, ACT_SILU, nullptr, n, s);
  c3k2(2, V("l1"), V("l2"), n, s);
  conv(cw_.at("model.3"), V("l2"), V("l3"), 2, ACT_SILU, nullptr, n, s);
  const View cat15 = V("cat15"), cat12 = V("cat12"), cat18 = V("cat18"), cat21 = V("cat21");
  const View n4 = cat15.slice(c128, c128);          // node 4 lives in concat 15 = [up(13), 4]
  c3k2(4, V("l3"), n4, n, s);
  conv(cw_.at("model.5"), n4, V("l5"), 2, ACT_SILU, nullptr, n, s);
  const View n6 = cat12.slice(c256, c128);          // concat 12 = [up(10), 6]
  c3k2(6, V("l5"), n6, n, s);
  conv(cw_.at("model.7"), n6, V("l7"), 2, ACT_SILU, nullptr, n, s);
  c3k2(8, V("l7"), V("l8"), n, s);
  sppf("model.9", V("l8"), V("sppcat"), V("l9"), n, s);
  const View n10 = cat21.slice(c128, c256);         // concat 21 = [20, 10]
  c2psa(10, V("l9"), n10, n, s);
  // top-down
  upsample2x(n10, cat12, n, s);
  const View n13 = cat18.slice(c64, c128);          // concat 18 = [17, 13]
  c3k2(13, cat12, n13, n, s);
  upsample2x(n13, cat15, n, s);
  c3k2(16, cat15, V("p3"), n, s);
  // the same fork-join as forward_v8: prototype branch and P3 / P4 heads beside the rest of the neck
  if (!obb()) proto(head_, V("p3"), n, fork_after(s, 0));
  head_level_v11(0, n, fork_after(s, 1));
  conv(cw_.at("model.17"), V("p3"), cat18.slice(0, c64), 2, ACT_SILU, nullptr, n, s);
  c3k2(19, cat18, V("p4"), n, s);
  head_level_v11(1, n, fork_after(s, 2));
  conv(cw_.at("model.20"), V("p4"), cat21.slice(0, c128), 2, ACT_SILU, nullptr, n, s);
  c3k2(22, cat21, V("p5"), n, s);
  head_level_v11(2, n, s);
  join_into(s, 1), join_into(s, 2);
}

// Segment head of level l: box + coefficient branches (first 3x3 convs merged), class branch of depthwise + pointwise pairs
void Detector::head_level_v11(int l, int n, hipStream_t s) {
  const char* feats[3] = {"p3", "p4", "p5"};
  const std::string ls = std::to_string(l);
  const View f = view(feats[l]), t1 = view("t1_" + ls), t2 = view("t2_" + ls);
  const View rh = view("rawhead" + ls);
  conv(head_first_[l], f, t1, 1, ACT_SILU, nullptr, n, s);
  const int c2 = hc2_, c4 = hc4p_;  // 64, 32 at scale n
  conv_pair(head_box2_[l], t1.slice(0, c2), t2.slice(0, c2), 1, head_box3_[l], rh.slice(0, 4 * reg_max_), ACT_NONE, n, s);
  conv_pair(head_coef2_[l], t1.slice(c2, c4), t2.slice(c2, c4), 1, head_coef3_[l], rh.slice(RAW_COEF, nm_), ACT_NONE, n, s);
  // class branch: (depthwise 3x3, 1x1) twice, then the plain 1x1
  const View da = view("dwa_" + ls), db = view("dwb_" + ls), dc = view("dwc_" + ls), dd = view("dwd_" + ls);
  dwconv(cls_dw1_[l], f, da, ACT_SILU, nullptr, 0, 0, n, s);
  conv(cls_pw1_[l], da, db, 1, ACT_SILU, nullptr, n, s);
  dwconv(cls_dw2_[l], db, dc, ACT_SILU, nullptr, 0, 0, n, s);
  conv(cls_pw2_[l], dc, dd, 1, ACT_SILU, nullptr, n, s);
  conv(head_cls3_[l], dd, rh.slice(RAW_CLS, cfg_.nc), 1, ACT_NONE, nullptr, n, s);
  obb_flops_fix(f);
}

}  // namespace mtgv
