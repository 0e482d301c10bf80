"""The cases tests/test_yolo12_cpu.py and tests/test_gpu_yolo12.py share: YOLO12 at scales n, s, m, both tasks, in the style of
tests/scales_common.py.  Not a test module."""
import functools

import numpy as np

ARCH = "12"
SMALL_HW = (64, 96)   # P4 is 4 x 6 = 24 tokens, 6 per area; P5 is 2 x 3 = 6 tokens
SMALL_N = 3           # on a max_batch = 4 handle
# (scale, task, input_hw, frames)
FORWARD_CASES = [(s, t, SMALL_HW, SMALL_N) for s in "nsm" for t in ("seg", "obb")]
MID_CASES = [
    ("n", "seg", (96, 160), 1),   # P4 is 6 x 10: areas of 15 tokens, 1.5 rows each - the boundaries fall mid-row
    ("s", "seg", (96, 160), 1),
    ("s", "seg", (160, 224), 1),  # P4 is 10 x 14 = 140 tokens, 35 per area
]
BIG_CASES = [
    ("n", "seg", (640, 640), 2),  # 400 tokens per area: two query tiles of the attention kernel, the second ragged
    ("n", "seg", (480, 640), 1),  # 300 tokens per area
]
ALL_CASES = FORWARD_CASES + MID_CASES + BIG_CASES
# Weights: random_detector_state seed 4 (scales_common.WEIGHT_SEED), with the ABlock gains spec.random_detector_state documents.
WEIGHT_SEED = 4
CLS_BIAS = -0.9
# End to end (NMS, masks / rotated NMS), one case per task, chosen on the CPU (tests/test_yolo12_cpu.py checks the choice): in
# the float64 reference every class score is at least 1e-2 away from the 0.25 threshold, the float32 and float64 references
# keep identical anchors in the same order on all three frames, and more than 10 are kept per frame.
#   n seg: class bias -0.5, frame seed 0, IoU 0.7: kept 28, 29, 27 (nearest score 5.3e-2 from the threshold).
#   s obb: rotated NMS at IoU 0.7 keeps too few of the shape's 126 anchors (as scales_common.E2E_CASES found for YOLO11): IoU
#          0.9, class bias -0.5, frame seed 0: kept 28, 29, 30 (nearest score 2.8e-2 from the threshold).
E2E_CASES = {("n", "seg"): dict(bias=-0.5, seed=0, iou=0.7), ("s", "obb"): dict(bias=-0.5, seed=0, iou=0.9)}


def case_id(c):
    return f"12{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}"


def frame_seed(hw):
    return 1000 * hw[0] + hw[1]


@functools.lru_cache(maxsize=None)
def inputs(scale, task, hw, n, bias=CLS_BIAS, seed=None, iou=0.7):
    """(cfg, state dict, frames (n, h, w, 3) uint8) of a case"""
    from mtgv import spec

    cfg = spec.detector_scale_config(ARCH, scale, task=task, input_hw=hw, iou=iou)
    sd = spec.random_detector_state(cfg, WEIGHT_SEED, cls_bias=bias)
    frames = np.random.default_rng(frame_seed(hw) if seed is None else seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)
    return cfg, sd, frames


@functools.lru_cache(maxsize=None)
def reference(scale, task, hw, n, bias=CLS_BIAS, seed=None, iou=0.7, f32=False):
    """the reference's (detections, pred, protos) in float64 (or float32): computed once, left unchanged"""
    import torch

    import yolo12_ref as R

    cfg, sd, frames = inputs(scale, task, hw, n, bias, seed, iou)
    return R.detect(sd, cfg, frames, dtype=torch.float32 if f32 else torch.float64)
