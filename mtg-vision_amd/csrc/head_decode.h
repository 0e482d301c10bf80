// The per-anchor decode of the segment head's raw rows, defined once for its two users: decode_kernel
// (detector_kernel.h), which writes `pred` for every anchor, and the row form of nms_kernel (nms.hip), which decodes
// the candidates only.  The OBB head's decode (decode_obb_kernel) shares the DFL distances.  Both must give the same bits, so nothing here is left to the compiler's contraction: the
// function bodies are compiled with contraction off and the one fused operation - the expectation's accumulate, which
// is what decode_kernel compiled to when it was written in plain expressions - is spelled __builtin_fmaf.
#pragma once
#include "common.h"

#include <math.h>

namespace mtgv {

// Raw head rows of the three pyramid levels (strides 8 / 16 / 32) of an h x w input: per level [n][(h / stride)(w / stride)]
// rows of `ct` floats, 16-byte aligned; a row holds 4 sides x 16 box bins at [0, 64), class logits at [cls, cls + nc), mask
// coefficients at [coef, coef + nm).  ct, cls and coef are multiples of 4.  h = w = 0: the square imgsz x imgsz input.
struct HeadRows {
  const float *r0, *r1, *r2;
  int imgsz, ct, cls, coef;
  int h = 0, w = 0;
  __host__ __device__ int in_h() const { return h > 0 ? h : imgsz; }
  __host__ __device__ int in_w() const { return w > 0 ? w : imgsz; }
};

struct HeadAnchor {
  const float* row;
  int pix, gw;    // pixel index and width of the level's grid
  float stride;
};

// anchor a of image img: P3's pixels first, then P4's, then P5's (the order of `pred`)
__device__ __forceinline__ HeadAnchor head_anchor(const HeadRows& h, int img, int a) {
  const int ih = h.in_h(), iw = h.in_w();
  const int w0 = iw / 8, w1 = iw / 16, w2 = iw / 32;
  const int n0 = (ih / 8) * w0, n1 = (ih / 16) * w1, n2 = (ih / 32) * w2;
  HeadAnchor an;
  if (a < n0) {
    an.pix = a, an.gw = w0, an.stride = 8.f;
    an.row = h.r0 + ((long)img * n0 + an.pix) * h.ct;
  } else if (a < n0 + n1) {
    an.pix = a - n0, an.gw = w1, an.stride = 16.f;
    an.row = h.r1 + ((long)img * n1 + an.pix) * h.ct;
  } else {
    an.pix = a - n0 - n1, an.gw = w2, an.stride = 32.f;
    an.row = h.r2 + ((long)img * n2 + an.pix) * h.ct;
  }
  return an;
}

// DFL: per side the softmax over 16 bins and its expectation -> the distances l, t, r, b in grid units
__device__ __forceinline__ void head_dfl(const HeadAnchor& an, float d[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float v[16];
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // 16-byte loads (a lane's row shares no line with its neighbours')
      const f32x4 t = *reinterpret_cast<const f32x4*>(an.row + s * 16 + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[q * 4 + e] = t[e];
        mx = fmaxf(mx, t[e]);
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      v[i] = expf(v[i] - mx);
      sum = sum + v[i];
    }
    float e = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) e = __builtin_fmaf(v[i] / sum, (float)i, e);
    d[s] = e;
  }
}

// segment / detect box: ltrb around the anchor centre -> xywh * stride
__device__ __forceinline__ void head_box(const HeadAnchor& an, float xywh[4]) {
#pragma clang fp contract(off)
  float d[4];
  head_dfl(an, d);
  const float ax = (float)(an.pix % an.gw) + 0.5f, ay = (float)(an.pix / an.gw) + 0.5f;
  const float x1 = ax - d[0], y1 = ay - d[1], x2 = ax + d[2], y2 = ay + d[3];
  xywh[0] = (x1 + x2) / 2.f * an.stride;
  xywh[1] = (y1 + y2) / 2.f * an.stride;
  xywh[2] = (x2 - x1) * an.stride;
  xywh[3] = (y2 - y1) * an.stride;
}

// class score of a class logit
__device__ __forceinline__ float head_score(float logit) {
#pragma clang fp contract(off)
  return 1.0f / (1.0f + expf(-logit));
}

// OBB head (ultralytics 8.3.x OBB.forward + dist2rbox) [external - recalled]: the angle logit sits where the segment head
// keeps its first mask coefficient (row[h.coef]); angle = (sigmoid(logit) - 0.25) pi in [-pi/4, 3 pi/4); the box centre is
// the anchor centre plus the DFL box's own centre offset rotated by the angle.  xywhr: x, y, w, h in pixels, angle in rad.
__device__ __forceinline__ void head_rbox(const HeadAnchor& an, float angle_logit, float xywhr[5]) {
#pragma clang fp contract(off)
  float d[4];
  head_dfl(an, d);
  const float angle = (head_score(angle_logit) - 0.25f) * 3.14159274101257324f;
  const float cs = cosf(angle), sn = sinf(angle);
  const float ax = (float)(an.pix % an.gw) + 0.5f, ay = (float)(an.pix / an.gw) + 0.5f;
  const float xf = (d[2] - d[0]) / 2.f, yf = (d[3] - d[1]) / 2.f;
  xywhr[0] = (xf * cs - yf * sn + ax) * an.stride;
  xywhr[1] = (xf * sn + yf * cs + ay) * an.stride;
  xywhr[2] = (d[0] + d[2]) * an.stride;
  xywhr[3] = (d[1] + d[3]) * an.stride;
  xywhr[4] = angle;
}

}  // namespace mtgv
