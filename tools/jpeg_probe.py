#!/usr/bin/env python3
"""GPU JPEG decode probe (csrc/jpeg.hip): one batched decode of seeded inputs, timed with HIP events after warm-up.

    python tools/jpeg_probe.py [--reps 20] [--out profiles/jpeg_probe.txt] [--no-pipeline]

Inputs (Pillow-encoded from fixed seeds): 32 frames 640x480 4:2:0 at quality 50 / 80 / 95, and 256 card-like scans
488x680 (quality 90, 4:2:0).  Reports ms per batch, images/s and compressed MB/s for mtgv_jpeg_decode, Pillow on 16
threads for the same inputs, and Pipeline.run_many cards/s over JpegFrames next to HostFrames on the same frames.
The time of each kernel stage comes from a separate run under rocprofv3:

    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/jpeg_trace -o run -- python tools/jpeg_probe.py --reps 5 --no-pipeline
"""

from __future__ import annotations

import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]

import torch  # noqa: E402
from PIL import Image, features  # noqa: E402


def scene(h, w, seed):
    """a webcam-like frame: smooth background, a few flat card rectangles with texture, mild noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([128 + 60 * np.sin(x / 70 + seed), 110 + 50 * np.cos(y / 55), 90 + 40 * np.sin((x + y) / 90)], -1)
    for _ in range(6):
        y0, x0 = rng.integers(0, h - 100), rng.integers(0, w - 80)
        a[y0 : y0 + rng.integers(60, 200), x0 : x0 + rng.integers(40, 150)] = rng.integers(0, 256, 3)
    a += rng.normal(0, 6, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, q):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=q)
    return b.getvalue()


def pil_decode(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


def time_gpu(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def time_pil(datas, reps, pool):
    list(pool.map(pil_decode, datas))
    ts = []
    for _ in range(max(3, reps // 4)):
        t = time.perf_counter()
        list(pool.map(pil_decode, datas))
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    from mtgv.jpeg import JpegDecoder, _padded_pixels, jpeg_info

    lines = [f"# jpeg_probe: {torch.cuda.get_device_name(0)}, libjpeg-turbo {features.version('libjpeg_turbo')} (Pillow reference)"]
    sets = {f"frames 32x640x480 q{q}": [encode(scene(480, 640, 10 + i), q) for i in range(32)] for q in (50, 80, 95)}
    sets["cards 256x488x680 q90"] = [encode(scene(680, 488, 100 + i), 90) for i in range(256)]
    pool = ThreadPoolExecutor(16)
    dec = JpegDecoder(256, max(sum(map(len, d)) for d in sets.values()), max(sum(_padded_pixels(jpeg_info(x)) for x in d) for d in sets.values()))
    lines.append(f"{'input':28s} {'MB':>7s} {'gpu ms':>8s} {'(min)':>7s} {'img/s':>9s} {'MB/s':>8s} {'pil16 ms':>9s} {'pil img/s':>9s}")
    for name, datas in sets.items():
        mb = sum(map(len, datas)) / 1e6
        if name.startswith("frames"):
            out = torch.empty((32, 640, 640, 3), dtype=torch.uint8, device="cuda")
            fn = lambda: dec.decode_frames(datas, out=out, check=False)  # noqa: E731
        else:
            fn = lambda: dec.decode(datas, check=False)  # noqa: E731
        med, mn = time_gpu(fn, a.reps)
        pil = time_pil(datas, a.reps, pool)
        n = len(datas)
        lines.append(f"{name:28s} {mb:7.2f} {med:8.3f} {mn:7.3f} {n / med * 1e3:9.0f} {mb / med * 1e3:8.0f} {pil:9.2f} {n / pil * 1e3:9.0f}")
        print(lines[-1], flush=True)
    if not a.no_pipeline:
        from mtgv import spec
        from mtgv.detector import Detector, letterbox
        from mtgv.encoder import Encoder
        from mtgv.jpeg import JpegFrames
        from mtgv.matcher import Matcher
        from mtgv.pipeline import HostFrames, Pipeline

        F, K, steps = 32, 8, 30
        datas = sets["frames 32x640x480 q80"]
        det_cfg = spec.DetectorConfig()
        enc_cfg = spec.encoder_config("cnvnxt2ae_tiny")
        m = Matcher(768, capacity=100_000)
        m.add(np.random.default_rng(2).standard_normal((100_000, 768)).astype(np.float32))
        pipe = Pipeline(Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F),
                        Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1, quad_source="mask")
        host = torch.from_numpy(np.stack([letterbox(pil_decode(d))[0] for d in datas]))
        for label, make in (("HostFrames (decoded + letterboxed on the host, pinned)", lambda: HostFrames([host], "cuda")),
                            ("JpegFrames (GPU decode)", lambda: JpegFrames([datas], "cuda", decoder=dec))):
            src = make()
            pipe.run_many(src.leases(3))
            torch.cuda.synchronize()
            t = time.perf_counter()
            pipe.run_many(src.leases(steps))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            lines.append(f"Pipeline.run_many {label}: {steps * F * K / dt:.0f} cards/s ({dt / steps * 1e3:.2f} ms/step, "
                         f"MTGV_OVERLAP={os.environ.get('MTGV_OVERLAP', 'off')})")
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
