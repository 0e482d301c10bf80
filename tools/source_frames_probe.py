#!/usr/bin/env python3
"""What cropping the cards from the camera's frames costs (`mtgv.pipeline.SourceFrames`), on a batch of 32 frames x 8 cards
from 1280 x 720 sources into the 640 x 640 detector input:

    (1) the letterbox: one mtgv_letterbox_ragged_u8 launch against the 32 mtgv_letterbox_rect_u8 launches (one per frame)
        it replaces in JpegDecoder.decode_frames, and against one same-size launch of all 32 for context
    (2) the de-warp of the 256 cards: mtgv_warp_quads_src from the sources against mtgv_warp_quads on the letterboxed copy
        (whose device code this library shares with its parent, instruction for instruction)
    (3) Pipeline.run on the SourceFrames against Pipeline.run on its letterboxed frames (the bench's models, quad_source
        "mask", a 20 000-row bank)

Every time is the median [p10, p90] of --runs calls after --warmup, HIP events around the calls (so Python's launch overhead
is inside: 32 launches cost 32 calls).

    python tools/source_frames_probe.py [--runs 50 --warmup 5 --out profiles/source_frames_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mtg-vision_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

F, K, H, W, S = 32, 8, 720, 1280, 640


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = np.asarray(ts)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def fmt(t):
    return f"{t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("source_frames_probe: no HIP device visible - times are measured on the GPU only")

    from mtgv import native as nv
    from mtgv import spec
    from mtgv.crop import warp_quads, warp_quads_src, warp_workspace
    from mtgv.detector import Detector, fit_geometry
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline, SourceFrames

    torch.cuda.set_device(0)
    L = nv.lib()
    g = torch.Generator(device="cuda").manual_seed(5)
    frames = torch.randint(0, 256, (F, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    sf = SourceFrames.from_frames(frames, size=S)
    r, nh, nw, top, left = fit_geometry(H, W, S, S)
    out = [f"source_frames_probe: {torch.cuda.get_device_name(0)}, {F} frames of {W} x {H} -> {S} x {S}, {K} cards per frame; "
           f"median [p10, p90] of {a.runs} runs after {a.warmup}, ms (HIP events)"]

    # (1) letterbox
    dst = torch.empty((F, S, S, 3), dtype=torch.uint8, device="cuda")

    def ragged():
        nv.check(L.mtgv_letterbox_ragged_u8(nv.ptr(sf.buf), nv.ptr(sf.offsets), nv.ptr(sf.hw), nv.ptr(sf.geo), F, nv.ptr(dst), S, S, 114, nv.stream()))

    def per_frame():
        for i in range(F):
            nv.check(L.mtgv_letterbox_rect_u8(nv.c_vp(frames.data_ptr() + i * H * W * 3), 1, H, W, nv.c_vp(dst.data_ptr() + i * S * S * 3), S, S, nh, nw,
                                              top, left, 114, nv.stream()))

    def same_size():
        nv.check(L.mtgv_letterbox_rect_u8(nv.ptr(frames), F, H, W, nv.ptr(dst), S, S, nh, nw, top, left, 114, nv.stream()))

    ragged()
    want = dst.clone()
    per_frame()
    same = torch.equal(want, dst) and torch.equal(want, sf.frames)
    t_r, t_p, t_s = median_ms(ragged, a.runs, a.warmup), median_ms(per_frame, a.runs, a.warmup), median_ms(same_size, a.runs, a.warmup)
    out.append(f"letterbox, one ragged launch:                              {fmt(t_r)}")
    out.append(f"letterbox, {F} per-frame launches:                          {fmt(t_p)}   (bytes equal: {same})")
    out.append(f"letterbox, one same-size launch of {F}:                     {fmt(t_s)}")

    # (2) de-warp: card-sized quads (about 128 x 192 px of the detector's input, turned a little) inside the image rectangle
    rng = np.random.default_rng(9)
    cx = rng.uniform(left + 90, left + nw - 90, (F * K, 1))
    cy = rng.uniform(top + 110, top + nh - 110, (F * K, 1))
    ang = rng.uniform(-0.3, 0.3, (F * K, 1))
    ux, uy = np.cos(ang), np.sin(ang)
    corners = []
    for sx, sy in ((-64, -96), (64, -96), (64, 96), (-64, 96)):
        corners.append(np.concatenate([cx + sx * ux - sy * uy, cy + sx * uy + sy * ux], 1))
    quads = torch.from_numpy(np.stack(corners, 1).astype(np.float32)).cuda()
    fidx = torch.arange(F, dtype=torch.int32, device="cuda").repeat_interleave(K)
    ws = warp_workspace(F * K, "cuda")
    t_src = median_ms(lambda: warp_quads_src(sf, quads, fidx, (192, 128), 0.05, ws), a.runs, a.warmup)
    t_box = median_ms(lambda: warp_quads(sf.frames, quads, fidx, (192, 128), 0.05, ws), a.runs, a.warmup)
    out.append(f"de-warp of {F * K} cards from the {W} x {H} sources (mtgv_warp_quads_src): {fmt(t_src)}")
    out.append(f"de-warp of {F * K} cards from the letterboxed copy (mtgv_warp_quads):      {fmt(t_box)}")

    # (3) the step
    det_cfg = spec.DetectorConfig()
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=20000)
    m.add(np.random.default_rng(2).standard_normal((20000, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F),
                    Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1, quad_source="mask")
    t_a = median_ms(lambda: pipe.run(sf), a.runs, a.warmup)
    t_b = median_ms(lambda: pipe.run(sf.frames), a.runs, a.warmup)
    t_c = median_ms(lambda: pipe.run(SourceFrames.from_frames(frames, size=S)), a.runs, a.warmup)
    out.append(f"Pipeline.run(SourceFrames), crops from the sources:            {fmt(t_a)}")
    out.append(f"Pipeline.run(frames), crops from the letterboxed copy:         {fmt(t_b)}")
    out.append(f"SourceFrames.from_frames + Pipeline.run (tables, letterbox):   {fmt(t_c)}")
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
