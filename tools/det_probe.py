#!/usr/bin/env python3
"""Detector b=32 under the schedule switches (MTGV_DET_FORK, MTGV_PROTO_UP1), in one process: ms per forward.
    python tools/det_probe.py [yolov8n-seg|yolo11n-seg|yolov8n-obb|yolo11n-obb] [--default-only] [--scale n|s|m]
--scale (or the size letter in the model name: yolov8s-seg, yolo11m-obb) picks the model scale; the default-only line then also
gives mtgv_detector_flops and the algorithmic TFLOP/s.  An -obb model also times the batch-1 forward and the OBB stages alone: rotated NMS at a few hundred and at 8400 candidates,
mtgv_obb_cards for 32 x 8 slots.  --default-only: the default switches only (one line per model)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]
import torch
from mtgv import spec
from mtgv.detector import Detector

argv = sys.argv[1:]
opt_scale = None
if "--scale" in argv:
    i = argv.index("--scale")
    opt_scale = argv[i + 1]
    del argv[i : i + 2]
args = [a for a in argv if not a.startswith("--")]
arch = args[0] if args else "yolov8n-seg"
task = "obb" if arch.endswith("-obb") else "seg"
family = "v8" if arch.startswith("yolov8") else "11"
stem = "yolov8" if family == "v8" else "yolo11"
scale = opt_scale or arch[len(stem)]
arch = f"{stem}{scale}-{task}"
cfg = spec.detector_scale_config(family, scale, task=task)
det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=32)
fr = torch.randint(0, 256, (32, 640, 640, 3), device="cuda", dtype=torch.uint8)

def timeit(fn, warm=5, it=30):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it

if "--default-only" in sys.argv or task == "obb":
    for rep in range(2):
        ms = timeit(lambda: det.forward(fr, True, 8))
        gf = det.flops_per_frame() / 1e9
        print(f"{arch} b=32 defaults: {ms:.3f} ms  {32 / ms * 1e3:.0f} frames/s  {gf:.2f} GFLOP/frame  {32 * gf / ms:.1f} TFLOP/s", flush=True)
    ms1 = timeit(lambda: det.forward(fr[:1], True, 8))
    print(f"{arch} b=1 defaults: {ms1:.3f} ms", flush=True)
if task == "obb":
    import numpy as np
    from mtgv.crop import obb_cards
    from mtgv.detector import nms_rotated

    out = det.forward(fr, True)
    pred, _ = det.raw_outputs(32)
    print(f"{arch}: {float(out['n_det'].float().mean()):.0f} detections / frame of {float((pred[:, 4:4 + cfg.nc].amax(1) > cfg.conf).sum(1).float().mean()):.0f} candidates")
    print(f"nms_rotated b=32 on the forward's pred: {timeit(lambda: nms_rotated(pred, cfg.nc)):.3f} ms")
    print(f"nms_rotated b=1 on the forward's pred: {timeit(lambda: nms_rotated(pred[:1], cfg.nc)):.3f} ms")
    rng = np.random.default_rng(0)
    for spread, what in ((3.0, "heavily overlapping"), (640.0, "spread over the frame")):  # every anchor a candidate
        p = np.zeros((1, 4 + cfg.nc + 1, 8400), np.float32)
        p[0, :2] = 320 + rng.uniform(-spread / 2, spread / 2, (2, 8400))
        p[0, 2:4] = rng.uniform(20, 60, (2, 8400))
        p[0, 4] = rng.uniform(0.3, 0.9, 8400)
        p[0, -1] = rng.uniform(-0.7, 2.3, 8400)
        pt = torch.from_numpy(p).cuda()
        print(f"nms_rotated b=1, 8400 candidates of one class, {what}: {timeit(lambda: nms_rotated(pt, cfg.nc), 2, 5):.3f} ms "
              f"({int(nms_rotated(pt, cfg.nc)['n_det'][0])} kept)")
    pad = torch.rand((8, 4), device="cuda") * 600
    print(f"obb_cards 32 x 8 slots: {timeit(lambda: obb_cards(out['n_det'], out['rboxes'], out['conf'], out['cls'], pad, 8)) * 1e3:.1f} us (incl. 4 allocations)")
    sys.exit(0)
if "--default-only" in sys.argv:
    sys.exit(0)

for rep in range(2):
    for fork, up1, chain in (("0", "0", "0"), ("0", "1", "0"), ("0", "1", "1"), ("1", "0", "0"), ("1", "1", "0"), ("1", "1", "1")):
        os.environ["MTGV_DET_FORK"], os.environ["MTGV_PROTO_UP1"], os.environ["MTGV_SPPF_POOLS1"] = fork, up1, up1
        os.environ["MTGV_DET_CHAIN"] = chain
        ms = timeit(lambda: det.forward(fr, True, 8))
        print(f"{arch} b=32 fork={fork} up1={up1} chain={chain}: {ms:.3f} ms  {32 / ms * 1e3:.0f} frames/s", flush=True)
