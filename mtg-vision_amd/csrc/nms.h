// Class-aware NMS, one workgroup per image (see nms.hip).
#pragma once
#include "common.h"
#include "head_decode.h"
#include "mtgv.h"

namespace mtgv {
size_t nms_workspace_bytes(int n, int na);
// coef_out (n, max_det, nm) may be null
void nms_launch(const float* pred, int n, int nc, int nm, int na, float conf, float iou, int max_det, float max_wh, int* n_det,
                float* boxes, float* conf_out, int* cls_out, int* keep_idx, float* coef_out, int* ws, size_t ws_bytes,
                hipStream_t s);
// rotated NMS on OBB predictions pred (n, 4 + nc + 1, na) = xywh, class scores, angle (nms.hip: nms_rotated_kernel);
// rboxes (n, max_det, 5) xywh + angle.  Workspace: nms_workspace_bytes(n, na).  iou > 0, max_wh >= 7680.
void nms_rotated_launch(const float* pred, int n, int nc, int na, float conf, float iou, int max_det, float max_wh, int* n_det,
                        float* rboxes, float* conf_out, int* cls_out, int* keep_idx, int* ws, size_t ws_bytes, hipStream_t s);
// the same on the segment head's raw rows (head_decode.h) of n images, na = head_rows_anchors(rows): bit-identical
// to decode_kernel -> nms_launch on those rows
int head_rows_anchors(const HeadRows& rows);
// the layout a HeadRows promises its kernels (head_decode.h), checked once for every launch that takes one
void head_rows_check(const HeadRows& rows, int nc, int nm);
void nms_rows_launch(const HeadRows& rows, int n, int nc, int nm, float conf, float iou, int max_det, float max_wh, int* n_det,
                     float* boxes, float* conf_out, int* cls_out, int* keep_idx, float* coef_out, int* ws, size_t ws_bytes,
                     hipStream_t s);
}  // namespace mtgv
