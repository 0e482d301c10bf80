// OBB detections -> oriented card quads on the GPU: the OBB counterpart of mtgv_select_cards + the mask -> quad fit.
//
// The reference trains its OBB detector with three classes - card, card_top, card_bottom - because "we can't get exact
// orientation, even with rotated bounding box so we specify top and bottom regions with different classes so we can
// compute this later" (mtgvision/od_datasets.py:244-257), and never computes it.  The rule below is THIS PROJECT'S
// (DESIGN.md section 3), not the reference's.  For a detection (x, y, w, h, theta) of class card_cls:
//   1. if w > h: swap them, theta += pi / 2, so that h is the long side
//   2. u = (-sin theta, cos theta) is the long axis, v = (cos theta, sin theta) the short one
//   3. among the frame's detections of class top_cls, in score order, the first whose centre p lies inside the card
//      (|d.v| <= w / 2 and |d.u| <= h / 2, d = p - centre) is taken; it is accepted only if d.u != 0, and then
//      U = sign(d.u) u ("oriented")
//   4. otherwise the same search with bottom_cls and U = -sign(d.u) u
//   5. otherwise U is whichever of +-u has negative y (negative x if u.y == 0): the card is assumed upright ("unoriented")
//   6. R = (-U.y, U.x); TL = c + U h/2 - R w/2, TR = c + U h/2 + R w/2, BR = c - U h/2 + R w/2, BL = c - U h/2 - R w/2
// One thread per (frame, slot): the slot's card is the slot-th detection of card_cls in score order, or pad_boxes[slot]
// where the frame has fewer.  Single rounded float32 operations in the order written (contraction off), accurate
// sinf / cosf; oracle/obb_ref.py restates it operation for operation.
#include "common.h"
#include "mtgv.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mtgv {

// the first detection of class `want` (in score order) whose centre lies inside the card; returns d.u of it in `du`
__device__ __forceinline__ bool obb_inside_first(const float* rb, const int* cls, int nd, int want, float cx, float cy, float ux, float uy,
                                                 float vx, float vy, float hw, float hh, float& du) {
  if (want < 0) return false;
  for (int t = 0; t < nd; ++t) {
    if (cls[t] != want) continue;
    const float dx = rb[t * 5] - cx, dy = rb[t * 5 + 1] - cy;
    const float dv = dx * vx + dy * vy, d_u = dx * ux + dy * uy;
    if (fabsf(dv) <= hw && fabsf(d_u) <= hh) {
      du = d_u;
      return true;
    }
  }
  return false;
}

__global__ __launch_bounds__(256) void obb_cards_kernel(const int* __restrict__ n_det, const float* __restrict__ rboxes,
                                                       const int* __restrict__ cls, const float* __restrict__ pad, int F, int max_det,
                                                       int K, int card_cls, int top_cls, int bottom_cls, float* __restrict__ quads,
                                                       float* __restrict__ sel, int* __restrict__ frame_idx, int* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= F * K) return;
  const int f = i / K, k = i - f * K;
  const int nd = min(max(n_det[f], 0), max_det);
  const float* rb = rboxes + (long)f * max_det * 5;
  const int* cl = cls + (long)f * max_det;
  float* q = quads + (long)i * 8;
  frame_idx[i] = f;
  // the k-th detection of the card class
  int t = 0, seen = 0;
  for (; t < nd; ++t)
    if (cl[t] == card_cls && seen++ == k) break;
  if (t >= nd) {
    const float x1 = pad[k * 4], y1 = pad[k * 4 + 1], x2 = pad[k * 4 + 2], y2 = pad[k * 4 + 3];
    q[0] = x1, q[1] = y1, q[2] = x2, q[3] = y1, q[4] = x2, q[5] = y2, q[6] = x1, q[7] = y2;
    sel[i * 4 + 0] = x1, sel[i * 4 + 1] = y1, sel[i * 4 + 2] = x2, sel[i * 4 + 3] = y2;
    state[i] = 0;
    return;
  }
  const float cx = rb[t * 5], cy = rb[t * 5 + 1];
  float w = rb[t * 5 + 2], h = rb[t * 5 + 3], th = rb[t * 5 + 4];
  if (w > h) {
    const float tmp = w;
    w = h, h = tmp;
    th = th + 1.57079637050628662f;
  }
  const float cs = cosf(th), sn = sinf(th);
  const float ux = -sn, uy = cs, vx = cs, vy = sn;
  const float hw = w * 0.5f, hh = h * 0.5f;
  float Ux, Uy, du = 0.f;
  int st = 2;
  if (obb_inside_first(rb, cl, nd, top_cls, cx, cy, ux, uy, vx, vy, hw, hh, du) && du != 0.f) {
    const float sg = du > 0.f ? 1.f : -1.f;
    Ux = sg * ux, Uy = sg * uy;
  } else if (obb_inside_first(rb, cl, nd, bottom_cls, cx, cy, ux, uy, vx, vy, hw, hh, du) && du != 0.f) {
    const float sg = du > 0.f ? -1.f : 1.f;
    Ux = sg * ux, Uy = sg * uy;
  } else {
    const bool neg = uy < 0.f || (uy == 0.f && ux < 0.f);  // u itself points up (left when horizontal)
    const float sg = neg ? 1.f : -1.f;
    Ux = sg * ux, Uy = sg * uy;
    st = 1;
  }
  const float Rx = -Uy, Ry = Ux;
  const float ax = Ux * hh, ay = Uy * hh, bx = Rx * hw, by = Ry * hw;
  q[0] = cx + ax - bx, q[1] = cy + ay - by;
  q[2] = cx + ax + bx, q[3] = cy + ay + by;
  q[4] = cx - ax + bx, q[5] = cy - ay + by;
  q[6] = cx - ax - bx, q[7] = cy - ay - by;
  sel[i * 4 + 0] = fminf(fminf(q[0], q[2]), fminf(q[4], q[6]));
  sel[i * 4 + 1] = fminf(fminf(q[1], q[3]), fminf(q[5], q[7]));
  sel[i * 4 + 2] = fmaxf(fmaxf(q[0], q[2]), fmaxf(q[4], q[6]));
  sel[i * 4 + 3] = fmaxf(fmaxf(q[1], q[3]), fmaxf(q[5], q[7]));
  state[i] = st;
}

}  // namespace mtgv

using namespace mtgv;

extern "C" {
MTGV_API int mtgv_obb_cards(const int32_t* n_det_dev, const float* rboxes_dev, const float* conf_dev, const int32_t* cls_dev,
                            const float* pad_boxes_dev, int32_t frames, int32_t max_det, int32_t k, int32_t card_cls, int32_t top_cls,
                            int32_t bottom_cls, float* quads_dev, float* sel_boxes_dev, int32_t* frame_idx_dev, int32_t* state_dev,
                            void* stream) {
  return guarded([&] {
    MTGV_CHECK(frames >= 0 && max_det > 0 && k > 0 && card_cls >= 0, ERR_INVALID, "obb_cards: frames=%d max_det=%d k=%d card_cls=%d", frames,
               max_det, k, card_cls);
    if (frames == 0) return;
    (void)conf_dev;  // the detections arrive score-descending (mtgv_nms_rotated): their order is all the rule needs
    MTGV_CHECK(n_det_dev && rboxes_dev && cls_dev && pad_boxes_dev && quads_dev && sel_boxes_dev && frame_idx_dev && state_dev, ERR_INVALID,
               "obb_cards: null argument");
    hipLaunchKernelGGL(obb_cards_kernel, dim3((unsigned)((frames * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const int*)n_det_dev, rboxes_dev, (const int*)cls_dev, pad_boxes_dev, frames, max_det, k, card_cls, top_cls,
                       bottom_cls, quads_dev, sel_boxes_dev, (int*)frame_idx_dev, (int*)state_dev);
    HIP_OK(hipGetLastError());
  });
}
}
