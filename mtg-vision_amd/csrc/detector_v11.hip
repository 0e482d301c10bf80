// YOLO11-seg / -obb (scales n, s, m) on the GPU: the modules YOLOv8 does not have (ultralytics 8.3.x nn/modules: C3k2, C3k, C2PSA / PSABlock /
// Attention, DWConv, Detect(legacy=False) class branch - third-party to the reference, which trains this family by
// default: mtgvision/od_train.py:20, :55-56, :138-151).  Conv / the CSP block (C3k2 is C2f's skeleton with another inner
// module) / SPPF / the neck / the head levels / Proto / decode / NMS / masks and the arena table are shared with
// detector.hip; here are the YOLO11 backbone and its key expectations, the C3k inner module, C2PSA and the depthwise class
// branch.  Every 1x1 and 3x3 convolution runs on the split-precision implicit GEMM.
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
// depthwise Conv2d(c, c, k, groups=c, bias=False) + BatchNorm2d(eps 1e-3) -> weight [k * k][c] (tap-major), bias [c]; k = 3,
// or 7 (YOLO12's positional encoding)
ConvW Detector::fold_dw(const std::string& p) {
  const Raw& w = raw_.at(p + ".conv.weight");
  const int c = w.shape[0], k = w.shape[2], kk = k * k;
  std::vector<float> wf((size_t)kk * c), bf(c);
  for (int o = 0; o < c; ++o) {
    const auto [sc, bias] = bn_affine(p, o);
    bf[o] = (float)bias;
    for (int t = 0; t < kk; ++t) wf[(size_t)t * c + o] = (float)((double)w.data[(size_t)o * kk + t] * sc);
  }
  return ConvW{upload(wf), upload(bf), c, c, k};
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// What dwconv3_kernel can run, from its accesses.  A thread moves 8 channels as two 16-byte vectors: bias + c, w9 + tap C + c
// (C % 8 == 0), in + pixel in_ct + cin, add + pixel add_ld + c and out + pixel out_ct + out_co + c, c a multiple of 8.
// So every pointer is 16-byte aligned and in_ct, in_co, g_stride, add_ld, out_ct and out_co are multiples of 4 floats - of
// 8 on an SP8 side, whose 8-channel chunk (8 hi halves, then 8 lo halves) is one 32-byte unit of the format.  The 8 channels
// stay inside one group when g_size % 8 == 0, and inside their pixel when the last group ends within in_ct.
void dwconv3_check(const Dwconv3Args& a) {
  MTGV_CHECK(a.in != nullptr && a.w9 != nullptr && a.bias != nullptr && a.out != nullptr, ERR_INVALID, "dwconv3: null tensor");
  MTGV_CHECK(a.n > 0 && a.H > 0 && a.W > 0 && a.C > 0, ERR_INVALID, "dwconv3: n=%d h=%d w=%d c=%d", a.n, a.H, a.W, a.C);
  MTGV_CHECK(a.C % 8 == 0, ERR_INVALID, "dwconv3: c=%d is no multiple of 8", a.C);
  MTGV_CHECK((a.in_fmt == 0 || a.in_fmt == 1) && (a.out_fmt == 0 || a.out_fmt == 1), ERR_INVALID, "dwconv3: formats %d -> %d", a.in_fmt,
             a.out_fmt);
  MTGV_CHECK(a.act == ACT_NONE || a.act == ACT_SILU, ERR_INVALID, "dwconv3: activation %d (none or SiLU)", a.act);
  MTGV_CHECK(a.g_size == 0 || (a.g_size > 0 && a.g_size % 8 == 0 && a.g_stride >= 0), ERR_INVALID,
             "dwconv3: g_size=%d (0 or a multiple of 8) g_stride=%d", a.g_size, a.g_stride);
  const int gs = a.g_size > 0 ? a.g_size : a.C;
  const int qi = a.in_fmt == 1 ? 8 : 4, qo = a.out_fmt == 1 ? 8 : 4;
  const long last = (long)((a.C - 8) / gs) * a.g_stride + (a.C - 8) % gs + 8;  // one past the last input channel read, from in_co
  MTGV_CHECK(aligned16(a.in) && a.in_ct > 0 && a.in_ct % qi == 0 && a.in_co >= 0 && a.in_co % qi == 0 && (gs >= a.C || a.g_stride % qi == 0) &&
                 a.in_co + last <= a.in_ct,
             ERR_INVALID, "dwconv3: input view %d/%d fmt %d with g_size=%d g_stride=%d (16-byte alignment, channels inside the pixel)", a.in_ct,
             a.in_co, a.in_fmt, a.g_size, a.g_stride);
  MTGV_CHECK(aligned16(a.w9) && aligned16(a.bias), ERR_INVALID, "dwconv3: weights not 16-byte aligned");
  MTGV_CHECK(a.add == nullptr || (aligned16(a.add) && a.add_ld >= a.C && a.add_ld % 4 == 0), ERR_INVALID,
             "dwconv3: addend with add_ld=%d (16-byte alignment, at least c)", a.add_ld);
  MTGV_CHECK(aligned16(a.out) && a.out_ct % qo == 0 && a.out_co >= 0 && a.out_co % qo == 0 && a.out_co + a.C <= a.out_ct, ERR_INVALID,
             "dwconv3: output view %d/%d fmt %d (16-byte alignment, channels inside the pixel)", a.out_ct, a.out_co, a.out_fmt);
  MTGV_CHECK(((long)a.n * a.H * a.W * (a.C / 8) + 255) / 256 <= 0x7fffffffL, ERR_INVALID, "dwconv3: %d x %d x %d x %d is too large", a.n, a.H,
             a.W, a.C);
}

void dwconv3_launch(const Dwconv3Args& a, hipStream_t s) {
  dwconv3_check(a);
  const int gs = a.g_size > 0 ? a.g_size : a.C;
  const long total = (long)a.n * a.H * a.W * (a.C / 8);
  const unsigned grid = (unsigned)((total + 255) / 256);
#define DW_GO(I_, O_)                                                                                                                  \
  hipLaunchKernelGGL((dwconv3_kernel<I_, O_>), dim3(grid), dim3(256), 0, s, a.in, a.in_ct, a.in_co, gs, a.g_stride, a.w9, a.bias, a.add, \
                     a.add_ld, a.out, a.out_ct, a.out_co, a.H, a.W, a.C, a.act, total)
  if (a.in_fmt == 1 && a.out_fmt == 1) DW_GO(true, true);
  else if (a.in_fmt == 1) DW_GO(true, false);
  else if (a.out_fmt == 1) DW_GO(false, true);
  else DW_GO(false, false);
#undef DW_GO
  HIP_OK(hipGetLastError());
}

void psa_attn_check(const float* qkv, int n, int N, int heads, const float* att) {
  MTGV_CHECK(qkv != nullptr && att != nullptr, ERR_INVALID, "psa_attn: null tensor");
  MTGV_CHECK(n > 0 && N > 0 && heads > 0, ERR_INVALID, "psa_attn: n=%d tokens=%d heads=%d", n, N, heads);
  MTGV_CHECK(n <= 65535 && heads <= 65535, ERR_INVALID, "psa_attn: n=%d heads=%d are grid dimensions (at most 65535)", n, heads);
  // rows of heads * 128 and heads * 64 floats, read and written as 16-byte vectors
  MTGV_CHECK(aligned16(qkv) && aligned16(att), ERR_INVALID, "psa_attn: tensors not 16-byte aligned");
}

void psa_attn_launch(const float* qkv, int n, int N, int heads, float* att, hipStream_t s) {
  psa_attn_check(qkv, n, N, heads, att);
  constexpr int KD = 32, HD = 64;
  hipLaunchKernelGGL((attn_kernel<KD, HD, 16>), dim3((N + 255) / 256, heads, n), dim3(256), 0, s, qkv, att, N, heads, 1.0f / sqrtf((float)KD));
  HIP_OK(hipGetLastError());
}

void Detector::dwconv(const ConvW& w, const View& in, const View& out, int act, const float* add, int g_size, int g_stride, int n,
                      hipStream_t s) {
  MTGV_CHECK(out.C == w.cout && w.cout % 8 == 0, ERR_RUNTIME, "detector: depthwise conv channel mismatch");
  if (count_flops_) {
    flops_ += 2.0 * 9.0 * n * out.H * out.W * w.cout;
    return;
  }
  dwconv3_launch({in.p, in.ct, in.co, in.fmt, g_size, g_stride, w.w, w.b, act, add, w.cout, out.p, out.ct, out.co, out.fmt, n, out.H, out.W, w.cout},
                 s);
}

// ---------------------------------------------------------------------------
// construction: expected ultralytics keys of yolo11{n,s,m}-seg / -obb
// ---------------------------------------------------------------------------
void Detector::build_v11() {
  auto P = [](int i) { return "model." + std::to_string(i); };
  const int c16 = chn(64), c32 = chn(128), c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  const bool all_c3k = cfg_.scale >= 2;  // scales m, l, x: ultralytics sets c3k = True on every C3k2
  const int nrep = rep(2);
  MTGV_CHECK(nrep == 1, ERR_RUNTIME, "detector: C3k2 / C2PSA with %d inner modules", nrep);  // (l and x: 2)
  const Csp plain = all_c3k ? Csp::C3k : Csp::Half;  // a C3k2 the yaml gives c3k = False
  auto c3k2 = [&](int idx, int cin, int cout, Csp kind, double e) { expect_csp(idx, cin, cout, nrep, true, kind, e); };
  expect_conv_bn(P(0), c16, 3, 3);
  expect_conv_bn(P(1), c32, c16, 3);
  c3k2(2, c32, c64, plain, 0.25);
  expect_conv_bn(P(3), c64, c64, 3);
  c3k2(4, c64, c128, plain, 0.25);
  expect_conv_bn(P(5), c128, c128, 3);
  c3k2(6, c128, c128, Csp::C3k, 0.5);
  expect_conv_bn(P(7), c256, c128, 3);
  c3k2(8, c256, c256, Csp::C3k, 0.5);
  expect_sppf(P(9), c256);
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
  expect_neck(nrep, true, plain, Csp::C3k);  // nodes 13, 16, 19 (c3k = False) and 22 (True)
}

// ---------------------------------------------------------------------------
// modules
// ---------------------------------------------------------------------------
// C3k(c, c, 2), the inner module of a C3k2 with c3k = True: cv3(cat(m(cv1(x)), cv2(x))) with two Bottlenecks(c/2, c/2, e = 1)
// in place on the first half of kcat
void Detector::c3k(const std::string& M, const View& x, const View& kcat, const View& tmp, const View& out, bool shortcut, int n,
                   hipStream_t s) {
  const int c_ = kcat.ct / 2;
  const View a = kcat.slice(0, c_);
  conv(cw_.at(M + ".cv1"), x, a, 1, ACT_SILU, nullptr, n, s);
  for (int j = 0; j < 2; ++j) bottleneck(M + ".m." + std::to_string(j), a, tmp, a, shortcut, n, s);
  conv(cw_.at(M + ".cv2"), x, kcat.slice(c_, c_), 1, ACT_SILU, nullptr, n, s);
  conv(cw_.at(M + ".cv3"), kcat, out, 1, ACT_SILU, nullptr, n, s);
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
    psa_attn_launch(qkv.p, n, N, NH, att.p, s);
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

// yolo11 nodes 1 .. 10 behind conv0; returns node 10
View Detector::backbone_v11(int n, hipStream_t s) {
  const int c128 = chn(512), c256 = chn(1024);
  auto V = [&](const char* k) -> View { return view(k); };
  conv(cw_.at("model.1"), V("l0"), V("l1"), 2, ACT_SILU, nullptr, n, s);
  csp_block(2, V("l1"), V("l2"), n, s);
  conv(cw_.at("model.3"), V("l2"), V("l3"), 2, ACT_SILU, nullptr, n, s);
  const View n4 = V("cat15").slice(c128, c128);     // node 4 lives in concat 15 = [up(13), 4]
  csp_block(4, V("l3"), n4, n, s);
  conv(cw_.at("model.5"), n4, V("l5"), 2, ACT_SILU, nullptr, n, s);
  const View n6 = V("cat12").slice(c256, c128);     // concat 12 = [up(10), 6]
  csp_block(6, V("l5"), n6, n, s);
  conv(cw_.at("model.7"), n6, V("l7"), 2, ACT_SILU, nullptr, n, s);
  csp_block(8, V("l7"), V("l8"), n, s);
  sppf("model.9", V("l8"), V("sppcat"), V("l9"), n, s);
  const View n10 = V("cat21").slice(c128, c256);    // concat 21 = [20, 10]
  c2psa(10, V("l9"), n10, n, s);
  return n10;
}

// Detect(legacy=False)'s class branch on the level's features: (depthwise 3x3, 1x1) twice, then the plain 1x1
void Detector::head_cls_v11(int l, const View& f, const View& rh, int n, hipStream_t s) {
  const std::string ls = std::to_string(l);
  const View da = view("dwa_" + ls), db = view("dwb_" + ls), dc = view("dwc_" + ls), dd = view("dwd_" + ls);
  dwconv(cls_dw1_[l], f, da, ACT_SILU, nullptr, 0, 0, n, s);
  conv(cls_pw1_[l], da, db, 1, ACT_SILU, nullptr, n, s);
  dwconv(cls_dw2_[l], db, dc, ACT_SILU, nullptr, 0, 0, n, s);
  conv(cls_pw2_[l], dc, dd, 1, ACT_SILU, nullptr, n, s);
  conv(head_cls3_[l], dd, rh.slice(RAW_CLS, cfg_.nc), 1, ACT_NONE, nullptr, n, s);
}

}  // namespace mtgv

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace mtgv;
extern "C" {
// The positional encoding is not added in place.  dwconv3_kernel declares `add` and `out` __restrict__: with add == out the
// compiler may assume the two never overlap, and although a thread reads only the eight addend values it then replaces,
// that is an argument about the code it happens to generate, not about the kernel's source.  The detector keeps the two
// apart as well ("att" and "atty"), so the attention output goes to a scratch buffer this entry point owns (test surface:
// one per process, grown on demand, on the device of the first call) and the 3x3 reads it as the addend - the launch
// c2psa makes.
MTGV_API int mtgv_op_psa_attn(const float* qkv_dev, const float* pe_w9_dev, const float* pe_bias_dev, int32_t n, int32_t h, int32_t w,
                              int32_t heads, float* out_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(qkv_dev != nullptr && out_dev != nullptr, ERR_INVALID, "psa_attn: null argument");
    MTGV_CHECK(n > 0 && h > 0 && w > 0 && heads > 0 && (long)h * w <= (1 << 24), ERR_INVALID, "psa_attn: n=%d h=%d w=%d heads=%d", n, h, w, heads);
    MTGV_CHECK((pe_w9_dev == nullptr) == (pe_bias_dev == nullptr) && aligned16(pe_w9_dev) && aligned16(pe_bias_dev), ERR_INVALID,
               "psa_attn: positional encoding needs weights and bias, both 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int N = h * w;
    psa_attn_check(qkv_dev, n, N, heads, out_dev);
    if (pe_w9_dev == nullptr) {
      psa_attn_launch(qkv_dev, n, N, heads, out_dev, s);
    } else {
      constexpr int KD = 32, HD = 64;  // Detector::c2psa's arguments
      Dwconv3Args pe{qkv_dev, heads * (2 * KD + HD), 2 * KD, 0, HD, 2 * KD + HD, pe_w9_dev, pe_bias_dev, ACT_NONE, nullptr, heads * HD,
                     out_dev, heads * HD, 0, 0, n, h, w, heads * HD};
      dwconv3_check(pe);  // all but the addend: nothing is launched unless both launches can run
      static DevBuf att;
      att.ensure((size_t)n * N * heads * HD);
      pe.add = att.p;
      psa_attn_launch(qkv_dev, n, N, heads, att.p, s);
      dwconv3_launch(pe, s);
    }
    HIP_OK(hipStreamSynchronize(s));
  });
}
MTGV_API int mtgv_op_dwconv3(const mtgv_dwconv3* d, void* stream) {
  return guarded([&] {
    MTGV_CHECK(d != nullptr, ERR_INVALID, "dwconv3: null descriptor");
    dwconv3_launch({(const float*)d->x, d->x_ct, d->x_co, d->x_fmt, d->g_size, d->g_stride, d->w9, d->bias, d->act, d->add, d->add_ld,
                    (float*)d->out, d->out_ct, d->out_co, d->out_fmt, d->n, d->h, d->w, d->c},
                   (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}
}
