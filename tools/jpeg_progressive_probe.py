#!/usr/bin/env python3
"""Progressive JPEG decode probe (csrc/jpeg_prog.hip): the same 256 card-like scans (488x680, quality 90, 4:2:0, the set
of tools/jpeg_probe.py) saved as baseline and as progressive files, decoded in one batch each and run through
mtgv.bank.build_bank_jpeg, timed after warm-up.

    python tools/jpeg_progressive_probe.py [--reps 20] [--cards 2048] [--out profiles/jpeg_progressive_probe.txt] [--decode-only]

The time of each kernel (prog_zero, prog_scan once per level, prog_finish) comes from a separate run under rocprofv3:

    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/jpeg_prog_trace -o run -- python tools/jpeg_progressive_probe.py --reps 5 --decode-only
"""

from __future__ import annotations

import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from PIL import Image  # noqa: E402

from jpeg_probe import scene, time_gpu  # noqa: E402


def encode(a, q, progressive):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=q, progressive=progressive)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cards", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--decode-only", action="store_true")
    a = ap.parse_args()
    from mtgv.jpeg import JpegDecoder, _padded_pixels, jpeg_info

    imgs = [scene(680, 488, 100 + i) for i in range(256)]
    sets = {"baseline": [encode(x, 90, False) for x in imgs], "progressive": [encode(x, 90, True) for x in imgs]}
    lines = [f"# jpeg_progressive_probe: {torch.cuda.get_device_name(0)}, 256 scans 488x680 q90 4:2:0"]
    nbytes = max(sum(map(len, d)) for d in sets.values())
    pix = sum(_padded_pixels(jpeg_info(x)) for x in sets["baseline"])
    decs = {"baseline on a default handle": (JpegDecoder(256, nbytes, pix), "baseline"),
            "baseline on a progressive handle": (JpegDecoder(256, nbytes, pix, progressive=True), "baseline"),
            "progressive": (JpegDecoder(256, nbytes, pix, progressive=True), "progressive")}
    for name, (dec, key) in decs.items():
        datas = sets[key]
        med, mn = time_gpu(lambda: dec.decode(datas, check=False), a.reps)
        lines.append(f"decode 256 {name:34s} {sum(map(len, datas)) / 1e6:6.2f} MB  {med:8.3f} ms (min {mn:.3f})  {256 / med * 1e3:7.0f} img/s")
        print(lines[-1], flush=True)
    if not a.decode_only:
        from mtgv import spec
        from mtgv.adapters import VectorStoreQdrant
        from mtgv.bank import build_bank_jpeg
        from mtgv.encoder import Encoder

        cfg = spec.encoder_config(os.environ.get("ENC", "cnvnxt2ae_nano"))
        enc = Encoder(cfg, spec.random_encoder_state(cfg, 1), max_batch=256)
        for key, datas in sets.items():
            cards = [(f"{i:036d}", datas[i % 256]) for i in range(a.cards)]
            store = VectorStoreQdrant(capacity=2 * a.cards)
            build_bank_jpeg(cards[:256], enc, store, 256)
            store.drop_collection()
            torch.cuda.synchronize()
            t = time.perf_counter()
            added = build_bank_jpeg(cards, enc, store, 256)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            lines.append(f"build_bank_jpeg {key:12s}: {added} cards in {dt:.2f} s = {added / dt:.0f} cards/s end to end")
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
