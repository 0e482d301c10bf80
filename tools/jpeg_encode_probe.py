#!/usr/bin/env python3
"""GPU JPEG encode probe (csrc/jpeg_enc.hip): batched encodes of seeded images, timed with HIP events after warm-up.

    python tools/jpeg_encode_probe.py [--reps 20] [--out profiles/jpeg_encode_probe.txt] [--no-pipeline]

Inputs (seeded): 256 card crops 192x128 at quality 50, 4:2:0 (one bench step's crops, the server's thumbnails) and 32
frames 640x480 at quality 80.  Reports ms per batch (median and min) and images/s for mtgv_jpeg_encode, Pillow on 16
threads for the same images, the output bytes, and Pipeline.run_many cards/s with thumbnails off and on (quality 50),
on one stream and with MTGV_OVERLAP=on, in the same process.  Every GPU file is checked against Pillow's bytes.  The
time of each kernel stage comes from a separate run under rocprofv3:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/jpeg_encode_probe.py --reps 5 --no-pipeline
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
    """smooth background, a few flat rectangles, mild noise (a de-warped card or a webcam frame)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([128 + 60 * np.sin(x / 70 + seed), 110 + 50 * np.cos(y / 55), 90 + 40 * np.sin((x + y) / 90)], -1)
    for _ in range(6):
        hh, ww = rng.integers(h // 8, h // 2), rng.integers(w // 8, w // 2)
        y0, x0 = rng.integers(0, h - hh), rng.integers(0, w - ww)
        a[y0 : y0 + hh, x0 : x0 + ww] = rng.integers(0, 256, 3)
    a += rng.normal(0, 6, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def pil_encode(a, q):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=q)
    return b.getvalue()


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


def time_pil(imgs, q, reps, pool):
    list(pool.map(lambda a: pil_encode(a, q), imgs))
    ts = []
    for _ in range(max(3, reps // 2)):
        t = time.perf_counter()
        list(pool.map(lambda a: pil_encode(a, q), imgs))
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    from mtgv.jpeg import JpegEncoder, jpeg_encode_bound, split_files

    lines = [f"# jpeg_encode_probe: {torch.cuda.get_device_name(0)}, libjpeg-turbo {features.version('libjpeg_turbo')} (Pillow reference)"]
    sets = {"crops 256x192x128 q50 4:2:0": (np.stack([scene(192, 128, 100 + i) for i in range(256)]), 50),
            "frames 32x640x480 q80 4:2:0": (np.stack([scene(480, 640, 10 + i) for i in range(32)]), 80)}
    pool = ThreadPoolExecutor(16)
    enc = JpegEncoder(256, 32 * 480 * 640)
    lines.append(f"{'input':30s} {'Mpx':>6s} {'gpu ms':>8s} {'(min)':>7s} {'img/s':>9s} {'pil16 ms':>9s} {'(min)':>7s} {'pil img/s':>9s} "
                 f"{'out MB':>7s}")
    for name, (imgs, q) in sets.items():
        dev = torch.from_numpy(imgs).cuda()
        n = len(imgs)
        cap = torch.empty(n * jpeg_encode_bound(imgs.shape[1], imgs.shape[2], 420), dtype=torch.uint8, device="cuda")
        files = split_files(*enc.encode_device(dev, q, 420, out=cap))
        want = [pil_encode(x, q) for x in imgs]
        assert files == want, f"{name}: GPU files differ from Pillow's"
        med, mn = time_gpu(lambda: enc.encode_device(dev, q, 420, out=cap), a.reps)  # noqa: B023
        pmed, pmn = time_pil(imgs, q, a.reps, pool)
        mpx = imgs.shape[0] * imgs.shape[1] * imgs.shape[2] / 1e6
        lines.append(f"{name:30s} {mpx:6.2f} {med:8.3f} {mn:7.3f} {n / med * 1e3:9.0f} {pmed:9.2f} {pmn:7.2f} {n / pmed * 1e3:9.0f} "
                     f"{sum(map(len, files)) / 1e6:7.3f}")
        print(lines[-1], flush=True)
    if not a.no_pipeline:
        from mtgv import spec
        from mtgv.detector import Detector
        from mtgv.encoder import Encoder
        from mtgv.matcher import Matcher
        from mtgv.pipeline import Pipeline

        F, K, steps = 32, 8, 30
        det_cfg = spec.DetectorConfig()
        enc_cfg = spec.encoder_config("cnvnxt2ae_tiny")
        m = Matcher(768, capacity=100_000)
        m.add(np.random.default_rng(2).standard_normal((100_000, 768)).astype(np.float32))
        det = Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F)
        emb = Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K)
        pipes = {"off": Pipeline(det, emb, m, K, 1, quad_source="mask"),
                 "q50": Pipeline(det, emb, m, K, 1, quad_source="mask", thumbnail_quality=50)}
        g = torch.Generator(device="cuda").manual_seed(7)
        frames = [torch.randint(0, 256, (F, 640, 640, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(4)]
        res = {}
        for rnd in range(2):  # the four configurations alternated twice; the better of the two rounds is kept
            for overlap in ("off", "on"):
                os.environ["MTGV_OVERLAP"] = overlap
                for th, pipe in pipes.items():
                    pipe.run_many(frames[:3])
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    outs = pipe.run_many(frames[i % 4] for i in range(steps))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t
                    if th == "q50":
                        o = outs[-1]
                        got = split_files(o["thumbs"], o["thumb_offsets"])
                        crops = o["crops"].cpu().numpy()
                        assert got[:8] == [pil_encode(c, 50) for c in crops[:8]], "pipeline thumbnails differ from Pillow's"
                    del outs
                    key = (overlap, th)
                    res[key] = max(res.get(key, 0.0), steps * F * K / dt)
        os.environ.pop("MTGV_OVERLAP", None)
        for (overlap, th), cps in res.items():
            lines.append(f"Pipeline.run_many F={F} K={K} AE-tiny, thumbnails {th:3s}, MTGV_OVERLAP={overlap:3s}: {cps:7.0f} cards/s "
                         f"({F * K / cps * 1e3:.2f} ms/step)")
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
