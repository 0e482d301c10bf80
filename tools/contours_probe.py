#!/usr/bin/env python3
"""What `CardSegmenter(contours=...)` costs per frame, and the contour stage alone (csrc/contours.hip), on a 640 x 640
frame with 3 and with 8 synthetic card masks (rotated rectangles with a notch, the reference's U-shaped masks):

    (1) the contour kernel alone (HIP events around mtgv.crop.contours_from_logits_packed)
    (2) kernel + copies to the host, both ways: the counts, then the used slice of the point buffer / the padded buffer
    (3) CardSegmenter(contours=c)(frame) for c in "trace" (GPU), "trace_host" (every mask copied and traced in Python,
        what "trace" was before the kernel) and "outline"; the detector's forward runs for real, its detections are
        replaced by the synthetic cards so that every form sees the same masks
    (4) the kernel's registers, LDS and scratch from the compiler's resource report

Every time is the median of --runs calls after --warmup, wall clock around work that ends in a device synchronise
(HIP events for (1)).

    python tools/contours_probe.py [--runs 50 --warmup 5 --out profiles/contours_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mtg-vision_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def card_mask(centre, half, angle_deg, notch, size=640):
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    a = np.deg2rad(angle_deg)
    u = (xx - centre[0]) * np.cos(a) + (yy - centre[1]) * np.sin(a)
    v = -(xx - centre[0]) * np.sin(a) + (yy - centre[1]) * np.cos(a)
    m = (np.abs(u) <= half[0]) & (np.abs(v) <= half[1])
    bx, by = centre[0] - half[1] * np.sin(a), centre[1] + half[1] * np.cos(a)
    return m & ((xx - bx) ** 2 + (yy - by) ** 2 >= notch**2)


def card_masks(n):
    """n cards on a 640 x 640 frame: 3 large ones (120 x 170 half sizes: 240 x 340 px) or 8 smaller ones on a grid"""
    if n <= 3:
        spots = [((200.0, 220.0), (120.0, 170.0), 20.0, 30.0), ((450.0, 400.0), (110.0, 160.0), -35.0, 28.0), ((330.0, 320.0), (100.0, 150.0), 75.0, 25.0)]
        return np.stack([card_mask(*s) for s in spots[:n]])
    rng = np.random.default_rng(3)
    out = []
    for i in range(n):
        cx, cy = 100.0 + 145.0 * (i % 4), 170.0 + 300.0 * (i // 4)
        out.append(card_mask((cx, cy), (55.0, 78.0), float(rng.uniform(-80, 80)), 14.0))
    return np.stack(out)


def median_ms(fn, runs, warmup, events=False):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.asarray(ts)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def resource_report():
    """registers, LDS and scratch of the contour kernels as the compiler reports them"""
    import importlib.util

    s = importlib.util.spec_from_file_location("mtgv_build", os.path.join(ROOT, "mtg-vision_amd", "build.py"))
    mod = importlib.util.module_from_spec(s)
    s.loader.exec_module(mod)  # the product build's compiler and flags
    with tempfile.TemporaryDirectory() as d:
        cmd = [mod.HIPCC, *mod.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
               os.path.join(mod.CSRC, "contours.hip"), "-o", os.path.join(d, "contours.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return ["resource report: hipcc failed: " + r.stderr[-300:]]
    lines = []
    for b in re.split(r"Function Name: ", r.stderr)[1:]:
        def g(k):
            m = re.search(k + r": (\d+)", b)
            return m.group(1) if m else "?"

        kind = "logits" if "ILb1E" in b.split(" ")[0] else "mask"
        vgpr, sgpr, scratch = g("    VGPRs"), g("TotalSGPRs"), g(r"ScratchSize \[bytes/lane\]")
        lds, occ = g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")
        lines.append(f"mask_contours_kernel<{kind}>: VGPR {vgpr}  SGPR {sgpr}  scratch {scratch} B/lane  static LDS {lds} B (+ dynamic: bit image, "
                     f"48 KiB run table, row offsets; 108 KiB at 640 x 640)  occupancy {occ} waves/SIMD by registers")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contours_probe: no HIP device visible - times are measured on the GPU only")

    import mtgv.adapters as A
    from mtgv import spec
    from mtgv.crop import contours_from_logits_packed
    from mtgv.detector import Detections, Detector

    torch.cuda.set_device(0)
    cfg = spec.DetectorConfig()
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=1)
    real_detect = det.detect
    frame = np.random.default_rng(8).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    out = [f"contours_probe: {torch.cuda.get_device_name(0)}, median [p10, p90] of {a.runs} runs after {a.warmup}, ms"]
    real_detect(frame)
    t_det = median_ms(lambda: real_detect(frame), a.runs, a.warmup)
    out.append(f"detector alone, Detector.detect(frame):                    {t_det[0]:8.3f} [{t_det[1]:.3f}, {t_det[2]:.3f}]")
    for n in (3, 8):
        masks = card_masks(n)
        big = torch.from_numpy(np.where(masks, 4.0, -4.0).astype(np.float32))[:, None]
        logits = torch.nn.functional.avg_pool2d(big, 4)[:, 0].cuda().contiguous()
        boxes = torch.tensor([[0.0, 0.0, 640.0, 640.0]] * n, device="cuda")
        fake = Detections(boxes, torch.linspace(0.9, 0.5, n, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"),
                          torch.zeros(n, dtype=torch.int64, device="cuda"), logits)

        def detect(*args, **kw):
            real_detect(*args, **kw)  # the forward runs; its random-weight detections are replaced by the cards
            return fake

        det.detect = detect
        pts, counts = contours_from_logits_packed(logits)
        c = counts.cpu().numpy()
        out.append(f"--- {n} cards: points per card {c[0].tolist()}, blobs {c[1].tolist()}, status {c[2].tolist()}")

        def stage_slice():
            p, k = contours_from_logits_packed(logits)
            k = k.cpu().numpy()
            return p[:, : max(int(k[0].max()), 1)].cpu().numpy()

        def stage_padded():
            p, k = contours_from_logits_packed(logits)
            return p.cpu().numpy(), k.cpu().numpy()

        t = median_ms(lambda: contours_from_logits_packed(logits), a.runs, a.warmup, events=True)
        out.append(f"contour kernel alone (HIP events):                         {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}]")
        t = median_ms(stage_slice, a.runs, a.warmup)
        out.append(f"kernel + counts copy + used-slice copy:                    {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}]")
        t = median_ms(stage_padded, a.runs, a.warmup)
        out.append(f"kernel + padded buffer copy ({n} x 4096 x 2 int32) + counts:  {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}]")
        res = {}
        for mode in ("trace", "trace_host", "outline"):
            seg = A.CardSegmenter(detector=det, contours=mode)
            t = median_ms(lambda: seg(frame), a.runs, a.warmup)
            res[mode] = (t, seg(frame))
            out.append(f"CardSegmenter(contours={mode!r:13})(frame):               {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}]")
        same = len(res["trace"][1]) == len(res["trace_host"][1]) == n and all(
            g.points.tobytes() == w.points.tobytes() for g, w in zip(res["trace"][1], res["trace_host"][1]))
        out.append(f"trace == trace_host bit for bit: {same};  trace_host / trace = {res['trace_host'][0][0] / res['trace'][0][0]:.1f}x, "
                   f"contour stage (call minus detector): host {res['trace_host'][0][0] - t_det[0]:.3f} ms, device {res['trace'][0][0] - t_det[0]:.3f} ms")
        det.detect = real_detect
    if not a.no_resources:
        out += resource_report()
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
