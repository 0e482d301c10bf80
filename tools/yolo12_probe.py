#!/usr/bin/env python3
"""YOLO12 beside YOLO11 at batch 32, 640 x 640, default flags, in one process on one GPU:
    python tools/yolo12_probe.py [--out FILE]
  * yolo11n-seg and yolo12n-seg forward (ms, events around 30 forwards after 5 warm-up ones, alternated twice),
  * for yolo12n-seg the summed time of its eight area-attention launches and eight depthwise 7x7 launches: events around 200
    back-to-back calls of mtgv_op_area_attn itself (the C entry the ABlocks' launches go through; buffers allocated once,
    nothing else between the events) on the blocks' own shapes: 4 blocks at P4 (40 x 40 tokens, 2 heads, 4 areas) and 4
    at P5 (20 x 20, 4 heads, 1 area); without pe the call is the attention launch alone, with pe it is both launches, the
    7x7 is their difference,
  * the attention kernel's achieved FLOP/s (2 n heads N (N / area) 64 per launch) against the 157 TFLOP/s f32 vector peak.
A report, not a bar."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]
import torch

from mtgv import native, spec
from mtgv.detector import Detector

B = 32
PEAK_F32 = 157e12
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeit(fn, warm=5, it=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


fr = torch.randint(0, 256, (B, 640, 640, 3), device="cuda", dtype=torch.uint8)
dets = {}
for family in ("11", "12"):
    cfg = spec.detector_scale_config(family, "n")
    dets[family] = Detector(cfg, spec.random_detector_state(cfg, 4), max_batch=B)
say(f"tools/yolo12_probe.py, one process on {torch.cuda.get_device_name(0)}: batch {B}, 640 x 640, default flags (f16x3 GEMMs, fork on), mask_rows 8")
for rep in range(2):
    for family, det in dets.items():
        ms = timeit(lambda: det.forward(fr, True, 8))
        gf = det.flops_per_frame() / 1e9
        say(f"yolo{family}n-seg forward: {ms:.3f} ms  {B / ms * 1e3:.0f} frames/s  {gf:.2f} GFLOP/frame  {B * gf / ms:.1f} TFLOP/s (whole forward)")

total_attn = total_pe = 0.0
for name, h, w, heads, area, blocks in (("P4", 40, 40, 2, 4, 4), ("P5", 20, 20, 4, 1, 4)):
    c = heads * 32
    qkv = torch.randn((B, h * w, heads * 96), device="cuda")
    w49, bias = torch.randn((49, c), device="cuda") / 7, torch.randn((c,), device="cuda") * 0.1
    out = torch.empty((B, h * w, c), device="cuda")
    op, st = native.lib().mtgv_op_area_attn, native.stream()
    pq, pw, pb, po, null = native.ptr(qkv), native.ptr(w49), native.ptr(bias), native.ptr(out), native.c_vp(0)
    t_attn = timeit(lambda: native.check(op(pq, null, null, B, h, w, heads, area, po, st)), 10, 200)
    t_both = timeit(lambda: native.check(op(pq, pw, pb, B, h, w, heads, area, po, st)), 10, 200)
    flops = 2.0 * B * heads * (h * w) * (h * w // area) * 64
    t_pe = max(t_both - t_attn, 0.0)
    say(f"{name} block ({h} x {w} tokens, {heads} heads, {area} areas): attention {t_attn * 1e3:.1f} us = {flops / t_attn / 1e9:.2f} TFLOP/s "
        f"({100 * flops / (t_attn * 1e-3) / PEAK_F32:.1f} % of the {PEAK_F32 / 1e12:.0f} TFLOP/s f32 peak); attention + 7x7 {t_both * 1e3:.1f} us; 7x7 alone {t_pe * 1e3:.1f} us")
    total_attn += blocks * t_attn
    total_pe += blocks * t_pe
say(f"yolo12n-seg, eight blocks per forward of {B} frames: area attention {total_attn:.3f} ms + depthwise 7x7 {total_pe:.3f} ms = {total_attn + total_pe:.3f} ms")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
