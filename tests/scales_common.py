"""The cases tests/test_scales_cpu.py and tests/test_gpu_scales.py share: detector scales s and m of both architectures and
both tasks on a small rectangle, one mid-size case per architecture.  Not a test module."""
import functools

import numpy as np

SMALL_HW = (64, 96)  # P5 is 2 x 3, the stem writes W / 8 = 12 column groups per row
SMALL_N = 3          # on a max_batch = 4 handle: a multiple of nothing
MID_HW = (160, 224)  # P3 is 20 x 28 = 560 rows: no multiple of the GEMM's 128-row tile
# (arch, scale, task, input_hw, frames)
FORWARD_CASES = [(a, s, t, SMALL_HW, SMALL_N) for a in ("v8", "11") for s in ("s", "m") for t in ("seg", "obb")]
MID_CASES = [(a, "s", "seg", MID_HW, 1) for a in ("v8", "11")]
# Weights: random_detector_state seed 4.  Seed 3, the other detector tests' choice, is ill-conditioned at these widths: the
# oracle's own float32 forward is then 3.9e-5 (YOLOv8 m prototypes at 64 x 96) and 7.5e-5 (YOLO11 s at 160 x 224) away from
# float64, past a third of the 1e-4 the GPU is held to; with seed 4 every case stays below 2.4e-6 (1e-4 px on boxes).
WEIGHT_SEED = 4
CLS_BIAS = -0.9
# End to end (NMS, masks), chosen on the CPU.  Class bias -0.5 puts every score at least 3e-2 away from the 0.25 threshold
# (at -0.9 the nearest is 3e-5 away: a flip waiting to happen), and the float32 and float64 oracle keep identical anchors
# in the same order on all three frames.  Kept per frame: YOLOv8 s seg 23, 24, 23 (frame seed 3).  YOLO11 s OBB: rotated
# NMS at the default IoU 0.7 keeps at most 11 of the shape's 126 anchors at any bias or seed tried (bias 0 makes every
# anchor a candidate), so that case runs at IoU 0.9 and keeps 35, 41, 44 (frame seed 0).  max_det is 300.
E2E_CASES = {("v8", "s", "seg"): dict(bias=-0.5, seed=3, iou=0.7), ("11", "s", "obb"): dict(bias=-0.5, seed=0, iou=0.9)}


def case_id(c):
    return f"{c[0]}{c[1]}-{c[2]}-{c[3][0]}x{c[3][1]}"


def frame_seed(hw):
    return 1000 * hw[0] + hw[1]


@functools.lru_cache(maxsize=None)
def inputs(arch, scale, task, hw, n, bias=CLS_BIAS, seed=None, iou=0.7):
    """(cfg, state dict, frames (n, h, w, 3) uint8) of a case"""
    from mtgv import spec

    cfg = spec.detector_scale_config(arch, scale, task=task, input_hw=hw, iou=iou)
    sd = spec.random_detector_state(cfg, WEIGHT_SEED, cls_bias=bias)
    frames = np.random.default_rng(frame_seed(hw) if seed is None else seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)
    return cfg, sd, frames


@functools.lru_cache(maxsize=None)
def reference(arch, scale, task, hw, n, bias=CLS_BIAS, seed=None, iou=0.7, f32=False):
    """the oracle's (detections, pred, protos) in float64 (or float32): computed once, left unchanged"""
    import torch

    from oracle import detector_ref as D

    cfg, sd, frames = inputs(arch, scale, task, hw, n, bias, seed, iou)
    return D.detect(sd, cfg, frames, dtype=torch.float32 if f32 else torch.float64)
