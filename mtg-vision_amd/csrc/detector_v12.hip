// YOLO12-seg / -obb (scales n, s, m) on the GPU: the modules the other two families do not have (ultralytics 8.3.x nn/modules/block.py:
// A2C2f, ABlock, AAttn - third-party to the reference, whose trainer builds this family with `--arch 12`:
// mtgvision/od_train.py:20, :55).  Recalled and unpinned like the rest of the detector.  There is no SPPF
// and no C2PSA: the backbone ends in node 8, the neck's node numbers are YOLOv8's minus one, the head is node 21.  Conv, C3k2,
// C3k, the neck (its A2C2f blocks without attention are a CSP kind of csp_block), the head levels with YOLO11's depthwise
// class branch, Proto, decode, NMS and masks are shared (detector.hip, detector_v11.hip); here are the YOLO12 backbone and its
// key expectations, A2C2f with attention, and the two kernels of AAttn.  Every 1x1 convolution (qkv, proj, the MLP) runs on
// the implicit GEMM, residual adds in its epilogue.
//   area_attn_kernel   softmax(q^T k / sqrt(32)) v per (image, area, head): f32 VALU, online softmax, K / V staged in LDS
//   pe7_kernel         depthwise 7x7 + folded BN of the v channels of qkv, plus the attention output; f32 or SP8 out
#include "detector.h"
#include "sp8.h"

#include <math.h>

namespace mtgv {

// ---------------------------------------------------------------------------
// Area attention core.  qkv (B, N, heads * 96) f32, per head [q 32 | k 32 | v 32]; out (B, N, heads * 32) f32.  The N tokens
// of an image are cut into `area` contiguous chunks of Na = N / area; (image, area) pairs are simply consecutive chunks of
// Na tokens, numbered by blockIdx.z.  Block = (query tile of 256, head, chunk); a thread owns one query: q in registers,
// the chunk's keys / values stream through LDS KC at a time, softmax is the online form (running maximum and sum), one
// rescale per KC keys.  Na is no multiple of anything: the last key group and the last query tile are ragged (keys past
// the chunk score -inf, threads past it load and store nothing).
// ---------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(256) void area_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int Na, int heads,
                                                       float scale) {
  constexpr int D = 32;
  __shared__ __attribute__((aligned(16))) float ks[KC][D];
  __shared__ __attribute__((aligned(16))) float vs[KC][D];
  const int tid = threadIdx.x;
  const int qi = blockIdx.x * 256 + tid;
  const int head = blockIdx.y;
  const long tok0 = (long)blockIdx.z * Na;  // first token of this chunk, counted over the whole batch
  const int ld = heads * 3 * D;
  const float* base = qkv + tok0 * ld + head * 3 * D;
  float q[D], acc[D];
  const bool live = qi < Na;
#pragma unroll
  for (int d = 0; d < D; d += 4) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) v = *reinterpret_cast<const f32x4*>(base + (long)qi * ld + d);
    q[d] = v[0] * scale, q[d + 1] = v[1] * scale, q[d + 2] = v[2] * scale, q[d + 3] = v[3] * scale;
  }
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < Na; k0 += KC) {
    __syncthreads();
    // K and V rows of KC keys: 2 x KC x 8 vectors of four
    for (int i = tid; i < 2 * KC * (D / 4); i += 256) {
      const int kv = i / (KC * (D / 4)), r = (i / (D / 4)) % KC, c4 = i % (D / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + r < Na) v = *reinterpret_cast<const f32x4*>(base + (long)(k0 + r) * ld + (1 + kv) * D + c4 * 4);
      *reinterpret_cast<f32x4*>(kv == 0 ? &ks[r][c4 * 4] : &vs[r][c4 * 4]) = v;
    }
    __syncthreads();
    const int kn = (Na - k0) < KC ? (Na - k0) : KC;
    float sc[KC];
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      float dsum = 0.f;
#pragma unroll
      for (int d = 0; d < D; ++d) dsum = __builtin_fmaf(q[d], ks[j][d], dsum);
      sc[j] = j < kn ? dsum : -INFINITY;
      cm = fmaxf(cm, sc[j]);
    }
    const float mn = fmaxf(m, cm);  // finite: every group has at least one key
    const float f = __expf(m - mn);  // 0 on the first group (m = -inf)
    l *= f;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] *= f;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const float pj = __expf(sc[j] - mn);  // exp(-inf) = 0 for the padding keys
      l += pj;
#pragma unroll
      for (int d = 0; d < D; ++d) acc[d] = __builtin_fmaf(pj, vs[j][d], acc[d]);
    }
    m = mn;
  }
  if (!live) return;
  const float inv = 1.0f / l;
  float* o = out + (tok0 + qi) * (long)(heads * D) + head * D;
#pragma unroll
  for (int d = 0; d < D; d += 4) {
    const f32x4 v = {acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
    *reinterpret_cast<f32x4*>(o + d) = v;
  }
}

// ---------------------------------------------------------------------------
// AAttn's positional encoding and the sum behind it: depthwise 7x7, stride 1, zero padding 3 over the whole H x W map (it
// crosses area boundaries), BatchNorm folded, on the v channels of qkv - channel c of C = heads * 32 is qkv channel
// (c / 32) * 96 + 64 + c % 32 - plus the attention output att (B, H, W, C) f32.  One thread = one pixel x 8 channels.
// w49 [49][C] tap-major.  out may be att (a thread reads only the eight att values it replaces).
// ---------------------------------------------------------------------------
template <bool OUT_SP8>
__global__ __launch_bounds__(256) void pe7_kernel(const float* __restrict__ qkv, const float* __restrict__ w49, const float* __restrict__ bias,
                                                 const float* att, float* out, int out_ct, int out_co, int H, int W, int C, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over B*H*W*(C/8)
  if (idx >= total) return;
  const int c8n = C >> 3;
  const int c = (int)(idx % c8n) * 8;
  long t = idx / c8n;
  const int x = (int)(t % W);
  t /= W;
  const int y = (int)(t % H);
  const long n = t / H;
  const int ld = 3 * C;
  const int cin = (c >> 5) * 96 + 64 + (c & 31);
  f32x4 a0 = *reinterpret_cast<const f32x4*>(bias + c), a1 = *reinterpret_cast<const f32x4*>(bias + c + 4);
  for (int kh = 0; kh < 7; ++kh) {
    const int iy = y + kh - 3;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) {
      const int ix = x + kw - 3;
      if (ix < 0 || ix >= W) continue;
      const float* p = qkv + ((n * H + iy) * W + ix) * (long)ld + cin;
      const f32x4 v0 = reinterpret_cast<const f32x4*>(p)[0], v1 = reinterpret_cast<const f32x4*>(p)[1];
      const float* wp = w49 + (kh * 7 + kw) * C + c;
      const f32x4 w0 = reinterpret_cast<const f32x4*>(wp)[0], w1 = reinterpret_cast<const f32x4*>(wp)[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) a0[e] = __builtin_fmaf(v0[e], w0[e], a0[e]), a1[e] = __builtin_fmaf(v1[e], w1[e], a1[e]);
    }
  }
  const long pix = (n * H + y) * W + x;
  const float* q = att + pix * C + c;
  a0 = a0 + reinterpret_cast<const f32x4*>(q)[0], a1 = a1 + reinterpret_cast<const f32x4*>(q)[1];
  float* o = out + pix * out_ct + out_co + c;
  if (OUT_SP8) {
    sp_h8 hi, lo;
    sp8_split8(a0, a1, hi, lo);
    reinterpret_cast<sp_h8*>(o)[0] = hi, reinterpret_cast<sp_h8*>(o)[1] = lo;
  } else {
    reinterpret_cast<f32x4*>(o)[0] = a0, reinterpret_cast<f32x4*>(o)[1] = a1;
  }
}

void area_attn_launch(const float* qkv, const float* pe_w49, const float* pe_bias, int n, int h, int w, int heads, int area, float* att,
                      float* out, int out_ct, int out_co, bool out_sp8, hipStream_t s) {
  MTGV_CHECK(qkv != nullptr && att != nullptr, ERR_INVALID, "area_attn: null tensor");
  MTGV_CHECK(n > 0 && h > 0 && w > 0 && heads >= 1 && area >= 1, ERR_INVALID, "area_attn: n=%d h=%d w=%d heads=%d area=%d", n, h, w, heads, area);
  const long N = (long)h * w;
  MTGV_CHECK(N % area == 0, ERR_INVALID, "area_attn: %d x %d = %ld tokens do not split into %d areas", h, w, N, area);
  MTGV_CHECK((long)n * area <= 65535 && N <= (1 << 24), ERR_INVALID, "area_attn: n=%d area=%d tokens=%ld out of range", n, area, N);
  MTGV_CHECK(pe_w49 == nullptr || (pe_bias != nullptr && out != nullptr), ERR_INVALID, "area_attn: positional encoding without bias or output");
  const int Na = (int)(N / area), C = heads * 32;
  hipLaunchKernelGGL((area_attn_kernel<16>), dim3((unsigned)((Na + 255) / 256), (unsigned)heads, (unsigned)(n * area)), dim3(256), 0, s, qkv, att,
                     Na, heads, 1.0f / sqrtf(32.0f));
  HIP_OK(hipGetLastError());
  if (pe_w49 == nullptr) return;
  const long total = (long)n * N * (C / 8);
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (out_sp8) hipLaunchKernelGGL((pe7_kernel<true>), dim3(grid), dim3(256), 0, s, qkv, pe_w49, pe_bias, att, out, out_ct, out_co, h, w, C, total);
  else hipLaunchKernelGGL((pe7_kernel<false>), dim3(grid), dim3(256), 0, s, qkv, pe_w49, pe_bias, att, out, out_ct, out_co, h, w, C, total);
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// construction: expected ultralytics keys of yolo12{n,s,m}-seg / -obb
// ---------------------------------------------------------------------------
// A2C2f(cin, cout, n, a2 = True, area), scales n, s, m (no residual gamma, MLP ratio 2): cv1 (1x1 cin -> c = cout / 2, ONE
// chunk), n modules of two ABlocks each, cv2 over the (1 + n) c concat
void Detector::expect_a2c2f(int idx, int cin, int cout, int n, int area) {
  const int c = cout / 2;
  MTGV_CHECK(c % 32 == 0 && c >= 32, ERR_INVALID, "detector: A2C2f hidden width %d is no multiple of 32", c);
  const std::string p = "model." + std::to_string(idx);
  expect_conv_bn(p + ".cv1", c, cin, 1);
  expect_conv_bn(p + ".cv2", cout, (1 + n) * c, 1);
  for (int j = 0; j < n; ++j)
    for (int b = 0; b < 2; ++b) {
      const std::string q = p + ".m." + std::to_string(j) + "." + std::to_string(b);
      expect_conv_bn(q + ".attn.qkv", 3 * c, c, 1);
      expect_conv_bn(q + ".attn.proj", c, c, 1);
      expect_conv_bn(q + ".attn.pe", c, 1, 7);
      expect_conv_bn(q + ".mlp.0", 2 * c, c, 1);
      expect_conv_bn(q + ".mlp.1", c, 2 * c, 1);
    }
  a2_[idx] = {cout, n, c, area};
}

void Detector::build_v12() {
  auto P = [](int i) { return "model." + std::to_string(i); };
  const int c16 = chn(64), c32 = chn(128), c64 = chn(256), c128 = chn(512), c256 = chn(1024);
  const bool all_c3k = cfg_.scale >= 2;  // scales m, l, x: ultralytics sets c3k = True on every C3k2
  const int n2 = rep(2), n4 = rep(4);
  MTGV_CHECK(n2 == 1 && n4 == 2, ERR_RUNTIME, "detector: YOLO12 repeats %d and %d", n2, n4);  // (l and x: 2 and 4)
  const Csp plain = all_c3k ? Csp::C3k : Csp::Half;
  expect_conv_bn(P(0), c16, 3, 3);
  expect_conv_bn(P(1), c32, c16, 3);
  expect_csp(2, c32, c64, n2, true, plain, 0.25);
  expect_conv_bn(P(3), c64, c64, 3);
  expect_csp(4, c64, c128, n2, true, plain, 0.25);
  expect_conv_bn(P(5), c128, c128, 3);
  expect_a2c2f(6, c128, c128, n4, 4);
  expect_conv_bn(P(7), c256, c128, 3);
  expect_a2c2f(8, c256, c256, n4, 1);
  expect_neck(n2, true, Csp::A2, Csp::C3k);  // nodes 11, 14, 17 (A2C2f, a2 = False) and 20 (C3k2 with C3k)
}

// ---------------------------------------------------------------------------
// modules
// ---------------------------------------------------------------------------
// A View has no image stride of its own: image i of a view starts at p + i * H * W * ct (conv_desc, the kernels here).  The
// arena carves max_batch * H * W * ct floats per buffer (plan_arena), so a view of the same buffer with another H, W and
// ct stays inside it for every n <= max_batch exactly when ONE image of the new shape is no larger than one of the carved
// shape - which is what is checked.  (Anything that gave View an explicit stride would have to set it here.)
View Detector::a2_view(const char* name, const View& like, int c) const {
  View v = view(name);
  MTGV_CHECK(v.co == 0 && v.C == v.ct && (long)like.H * like.W * c <= (long)v.H * v.W * v.ct, ERR_RUNTIME,
             "detector: attention buffer %s (%d x %d x %d per image) too small for %d x %d x %d", name, v.H, v.W, v.ct, like.H, like.W, c);
  v.H = like.H, v.W = like.W, v.ct = c, v.co = 0, v.C = c;
  return v;
}

// ABlock(c, heads = c / 32, mlp_ratio 2, area): y = x + proj(area_attn(qkv(x)) + pe(v)); y = y + mlp(y).  y may be x.
void Detector::ablock(const std::string& B, const View& x, const View& y, int area, int n, hipStream_t s) {
  const int c = x.C, heads = c / 32;
  const ConvW& pe = cw_.at(B + ".attn.pe");
  const ConvW& m0 = cw_.at(B + ".mlp.0");
  MTGV_CHECK(pe.k == 7 && pe.cout == c && heads * 32 == c, ERR_RUNTIME, "detector: unexpected ABlock geometry");
  const View qkv = a2_view("a2qkv", x, 3 * c), att = a2_view("a2att", x, c), t = a2_view("a2y", x, c), hid = a2_view("a2mlp", x, m0.cout);
  conv(cw_.at(B + ".attn.qkv"), x, qkv, 1, ACT_NONE, nullptr, n, s);
  const long N = (long)x.H * x.W;
  if (count_flops_) flops_ += 2.0 * n * heads * (double)N * (double)(N / area) * 64.0 + 2.0 * 49.0 * n * (double)N * c;
  else area_attn_launch(qkv.p, pe.w, pe.b, n, x.H, x.W, heads, area, att.p, t.p, t.ct, t.co, t.fmt == 1, s);
  conv(cw_.at(B + ".attn.proj"), t, y, 1, ACT_NONE, &x, n, s);
  conv(m0, y, hid, 1, ACT_SILU, nullptr, n, s);
  conv(cw_.at(B + ".mlp.1"), hid, y, 1, ACT_NONE, &y, n, s);
}

// A2C2f with attention (nodes 6 and 8): cv1 -> one chunk; module j (two ABlocks) reads chunk j and writes chunk j + 1
void Detector::a2c2f(int idx, const View& in, const View& out, int n, hipStream_t s) {
  const A2Info& ai = a2_.at(idx);
  const std::string id = std::to_string(idx), P = "model." + id;
  const View cat = view("cat" + id);
  conv(cw_.at(P + ".cv1"), in, cat.slice(0, ai.c), 1, ACT_SILU, nullptr, n, s);
  for (int j = 0; j < ai.n; ++j) {
    const View x = cat.slice(j * ai.c, ai.c), y = cat.slice((j + 1) * ai.c, ai.c);
    const std::string M = P + ".m." + std::to_string(j);
    ablock(M + ".0", x, y, ai.area, n, s);
    ablock(M + ".1", y, y, ai.area, n, s);
  }
  conv(cw_.at(P + ".cv2"), cat, out, 1, ACT_SILU, nullptr, n, s);
}

// yolo12 nodes 1 .. 8 behind conv0; returns node 8
View Detector::backbone_v12(int n, hipStream_t s) {
  const int c128 = chn(512), c256 = chn(1024);
  auto V = [&](const char* k) -> View { return view(k); };
  conv(cw_.at("model.1"), V("l0"), V("l1"), 2, ACT_SILU, nullptr, n, s);
  csp_block(2, V("l1"), V("l2"), n, s);
  conv(cw_.at("model.3"), V("l2"), V("l3"), 2, ACT_SILU, nullptr, n, s);
  const View n4 = V("cat13").slice(c128, c128);     // node 4 lives in concat 13 = [up(11), 4]
  csp_block(4, V("l3"), n4, n, s);
  conv(cw_.at("model.5"), n4, V("l5"), 2, ACT_SILU, nullptr, n, s);
  const View n6 = V("cat10").slice(c256, c128);     // concat 10 = [up(8), 6]
  a2c2f(6, V("l5"), n6, n, s);
  conv(cw_.at("model.7"), n6, V("l7"), 2, ACT_SILU, nullptr, n, s);
  const View n8 = V("cat19").slice(c128, c256);     // concat 19 = [18, 8]
  a2c2f(8, V("l7"), n8, n, s);
  return n8;
}

}  // namespace mtgv

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace mtgv;
extern "C" {
MTGV_API int mtgv_op_area_attn(const float* qkv_dev, const float* pe_w49_dev, const float* pe_bias_dev, int32_t n, int32_t h, int32_t w,
                               int32_t heads, int32_t area, float* out_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(qkv_dev != nullptr && out_dev != nullptr, ERR_INVALID, "area_attn: null argument");
    // attention into out, then the positional encoding added in place
    area_attn_launch(qkv_dev, pe_w49_dev, pe_bias_dev, n, h, w, heads, area, out_dev, out_dev, heads * 32, 0, false, (hipStream_t)stream);
  });
}
}
