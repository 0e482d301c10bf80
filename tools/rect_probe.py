#!/usr/bin/env python3
"""Detector forward at batch 32 on one stream, square against rectangular inputs: median ms of 50 forwards after 10
warm-ups per shape, and the per-launch GEMM table of one forward of each shape (which launches change form on a rectangle).
    python tools/rect_probe.py [yolov8n-seg|yolo11n-seg] [--shapes 640x640,480x640,384x640] [--tree DIR] [--csv DIR] [--jpeg]
--tree DIR: import mtgv from another checkout (a build of the parent commit: square shapes only), to compare two builds
with one script.  --csv DIR: write the launch tables there.  --jpeg: also time decode_frames of 32 JPEG frames of 640 x 480
with and without input_hw=(480, 640) (the saved pad pass); needs Pillow to make the frames (ImportError without it).
This is the record of how the figures of profiles/README.md "Rectangular detector input" were taken.  Note that --tree makes
the script import code from outside this repository: DIR must be a checkout of this project with its library built
(`python mtg-vision_amd/build.py` there); nothing else in the repository depends on it."""
import os, statistics, sys

args = sys.argv[1:]
def opt(name, default=None):
    return args[args.index(name) + 1] if name in args else default
ROOT = opt("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]
import torch
from mtgv import native, spec
from mtgv.detector import Detector

arch = args[0] if args and not args[0].startswith("--") else "yolov8n-seg"
shapes = [tuple(int(v) for v in s.split("x")) for s in opt("--shapes", "640x640,480x640,384x640").split(",")]
csv_dir = opt("--csv")
B = 32


def median_ms(fn, warm=10, it=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(it):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


print(f"{arch}, batch {B}, precision {native.get_gemm_precision()}, tree {ROOT}")
base = None
for h, w in shapes:
    kw = {} if (h, w) == (640, 640) else {"input_hw": (h, w)}
    cfg = spec.DetectorConfig(**kw) if arch.startswith("yolov8n") else spec.yolo11_config(**kw)
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=B)
    fr = torch.randint(0, 256, (B, h, w, 3), device="cuda", dtype=torch.uint8)
    for rep in range(2):
        med, best = median_ms(lambda: det.forward(fr, True, 8))
        if base is None:
            base = med
        print(f"{h}x{w} run {rep}: median {med:.3f} ms (min {best:.3f})  {B / med * 1e3:.0f} frames/s  ratio to the first square run "
              f"{med / base:.3f} (pixels {h * w / 409600:.3f})  {det.flops_per_frame() / 1e9:.3f} GFLOP/frame", flush=True)
    if csv_dir:
        os.makedirs(csv_dir, exist_ok=True)
        path = os.path.join(csv_dir, f"{arch}_{h}x{w}.csv")
        L = native.lib()
        native.check(L.mtgv_profile_gemm(1))
        det.forward(fr, True, 8)
        torch.cuda.synchronize()
        native.check(L.mtgv_profile_gemm_dump(path.encode()))
        native.check(L.mtgv_profile_gemm(0))
        print(f"  launch table: {path}")
    del det

if "--jpeg" in args:
    import io
    import numpy as np
    from PIL import Image
    from mtgv.jpeg import JpegDecoder

    rng = np.random.default_rng(0)
    datas = []
    for s in range(B):
        y, x = np.mgrid[0:480, 0:640]
        a = np.stack([x * 255 // 639, y * 255 // 479, (x * 3 + y * 5 + s * 8) % 256], -1).astype(np.uint8)
        a[100:300, 200:400] = rng.integers(0, 256, (200, 200, 3), dtype=np.uint8)
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", quality=80, subsampling=2)
        datas.append(b.getvalue())
    dec = JpegDecoder(B, 32 << 20, 32 << 20)
    sq = torch.empty((B, 640, 640, 3), dtype=torch.uint8, device="cuda")
    rc = torch.empty((B, 480, 640, 3), dtype=torch.uint8, device="cuda")
    for rep in range(2):
        m0, b0 = median_ms(lambda: dec.decode_frames(datas, out=sq))
        m1, b1 = median_ms(lambda: dec.decode_frames(datas, out=rc, input_hw=(480, 640)))
        print(f"decode_frames 32 x 640x480 JPEG run {rep}: into 640x640 + pad {m0:.3f} ms (min {b0:.3f}); into 480x640, no pad {m1:.3f} ms "
              f"(min {b1:.3f})", flush=True)
