// ProbIoU of two rotated boxes (x, y, w, h, theta), the overlap measure of ultralytics' rotated NMS
// (ultralytics 8.3.x utils/metrics.py batch_probiou, behind ops.nms_rotated) [external - recalled; unpinned]: each box
// is the Gaussian with its centre as mean and covariance [[a, c], [c, b]], and the measure is 1 - Hellinger distance
// derived from the Bhattacharyya distance bd of the two Gaussians.  Defined once for its two users, the rotated NMS
// kernel and mtgv_op_probiou (nms.hip).  Every operation is a single rounded float32 operation in the order written
// (contraction off), with the accurate sinf / cosf / logf / expf / sqrtf, so that the CPU restatement of the tests
// (oracle/obb_ref.py) differs by the math libraries' few ulp per transcendental only.
#pragma once
#include "common.h"

#include <math.h>

namespace mtgv {

static constexpr float PROBIOU_EPS = 1e-7f;

// covariance of a box: A = w^2 / 12, B = h^2 / 12 rotated by theta
__device__ __forceinline__ void probiou_cov(float w, float h, float theta, float& a, float& b, float& c) {
#pragma clang fp contract(off)
  const float A = w * w / 12.f, B = h * h / 12.f;
  const float cs = cosf(theta), sn = sinf(theta);
  const float cs2 = cs * cs, sn2 = sn * sn;
  a = A * cs2 + B * sn2;
  b = A * sn2 + B * cs2;
  c = (A - B) * cs * sn;
}

__device__ __forceinline__ float probiou_pair(float x1, float y1, float a1, float b1, float c1, float x2, float y2, float a2, float b2,
                                              float c2) {
#pragma clang fp contract(off)
  const float eps = PROBIOU_EPS;
  const float sa = a1 + a2, sb = b1 + b2, sc = c1 + c2;
  const float D = sa * sb - sc * sc;
  const float dy = y1 - y2, dx = x1 - x2;
  const float t1 = (sa * (dy * dy) + sb * (dx * dx)) / (D + eps) * 0.25f;
  const float t2 = (sc * (x2 - x1) * dy) / (D + eps) * 0.5f;
  const float d1 = fmaxf(a1 * b1 - c1 * c1, 0.f), d2 = fmaxf(a2 * b2 - c2 * c2, 0.f);
  const float t3 = 0.5f * logf(D / (4.f * sqrtf(d1 * d2) + eps) + eps);
  const float bd = fminf(fmaxf(t1 + t2 + t3, eps), 100.f);
  const float hd = sqrtf(1.f - expf(-bd) + eps);
  return 1.f - hd;
}

}  // namespace mtgv
