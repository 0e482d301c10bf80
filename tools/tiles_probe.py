#!/usr/bin/env python3
"""What tiled detection costs (`mtgv.tiles.TiledFrames`), on 4 frames of 1920 x 1080 cut into 640 x 640 windows with an
overlap of 128 plus the full-frame window (the host computes the tile count and prints it), a v8n detector, K = 32 cards per
frame, Kt = 16 per tile, mask quads:

    the cut                   one mtgv_letterbox_tiles_u8 launch for all tiles
    the detector forward      on the tiles, in chunks of the detector's max_batch
    per-tile select + quads   mtgv_select_cards + mtgv_mask_quads_logits with the tiles as frames
    the merge                 mtgv_tiles_merge
    the de-warp               mtgv_warp_quads_src with the identity geometry
    Pipeline.run(TiledFrames) the whole step, and Pipeline.run(SourceFrames) on the same four frames untiled for context

The OBB leg (a YOLO11n-obb detector, tile_merge={"rule": "rotated"}) measures the same four frames: the per-tile mtgv_obb_cards
launch, mtgv_tiles_merge_obb next to mtgv_tiles_merge on the same candidates (the card quads' bounds as boxes), the whole
step and the untiled step.

Every time is the median [p10, p90] of --runs calls after --warmup, HIP events around the calls (Python's launch overhead
is inside).  --untiled-only measures the untiled lines alone: the paths that exist without this module.

    python tools/tiles_probe.py [--runs 50 --warmup 5 --out profiles/tiles_probe.txt]
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

F, K, KT, H, W, S, OVERLAP = 4, 32, 16, 1080, 1920, 640, 128
MAX_BATCH = 36  # the tiles of the four frames in one forward (asserted below)


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


def obb_leg(frames, a, out):
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline, SourceFrames

    det_cfg = spec.yolo11_config(task="obb")
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=20000)
    m.add(np.random.default_rng(2).standard_normal((20000, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, spec.random_detector_state(det_cfg, 3, cls_bias=-0.9), max_batch=MAX_BATCH),
                    Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1, quad_source="obb",
                    **({} if a.untiled_only else {"cards_per_tile": KT, "tile_merge": {"rule": "rotated"}}))
    out.append(f"OBB leg: YOLO11n-obb, random weights (class bias -0.9), {K} cards per frame")
    sf = SourceFrames.from_frames(frames, size=S)
    t_u = median_ms(lambda: pipe.run(sf), a.runs, a.warmup)
    out.append(f"Pipeline.run(SourceFrames), the four frames untiled:      {fmt(t_u)}")
    if a.untiled_only:
        return
    from mtgv.crop import obb_cards
    from mtgv.tiles import TiledFrames, merge_tiles, merge_tiles_obb

    tf = TiledFrames.from_frames(frames, window_hw=(S, S), overlap=OVERLAP, with_full=True, size=S)
    nt = int(tf.tiles.shape[0])
    det = pipe.detector
    parts = [det.forward(tf.frames[i : i + det.max_batch]) for i in range(0, nt, det.max_batch)]
    d = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    t_fwd = median_ms(lambda: [det.forward(tf.frames[i : i + det.max_batch]) for i in range(0, nt, det.max_batch)], a.runs, a.warmup)
    cards = lambda: obb_cards(d["n_det"], d["rboxes"], d["conf"], d["cls"], pipe._pad_tile, KT, 0, 1, 2)  # noqa: E731
    q, sel, _, state = cards()
    t_c = median_ms(cards, a.runs, a.warmup)
    rot = lambda: merge_tiles_obb(tf, d["n_det"], d["conf"], d["cls"], q, state, KT, pipe._pad_frac, K, 2.0, 0.5, 0)  # noqa: E731
    mo = rot()
    t_r = median_ms(rot, a.runs, a.warmup)
    # the axis-aligned merge on the same candidates: every tile's card slots as its detections (bounds as boxes, quads as quads)
    n_card = (state.view(nt, KT) > 0).sum(1).to(torch.int32)
    boxes, conf = sel.view(nt, KT, 4).contiguous(), torch.linspace(0.9, 0.3, KT, device="cuda").repeat(nt, 1).contiguous()
    flat = lambda: merge_tiles(tf, n_card, boxes, conf, q, KT, pipe._pad_frac, K, 2.0, 0.5)  # noqa: E731
    fo = flat()
    t_f = median_ms(flat, a.runs, a.warmup)
    t_run = median_ms(lambda: pipe.run(tf), a.runs, a.warmup)
    out.append(f"card slots per tile {n_card.cpu().tolist()}")
    out.append(f"n_sel per frame: rotated {mo['n_sel'].cpu().tolist()} (oriented by a duplicate: {int((mo['oriented_by'] >= 0).sum())}), "
               f"axis-aligned on the bounds {fo['n_sel'].cpu().tolist()}")
    out.append(f"the detector forward on the {nt} tiles:                    {fmt(t_fwd)}")
    out.append(f"per-tile mtgv_obb_cards ({nt * KT} slots):                    {fmt(t_c)}")
    out.append(f"mtgv_tiles_merge_obb, one workgroup per frame:            {fmt(t_r)}")
    out.append(f"mtgv_tiles_merge on the same candidates:                  {fmt(t_f)}")
    out.append(f"Pipeline.run(TiledFrames):                                {fmt(t_run)}")
    out.append(f"rotated over axis-aligned merge: {t_r[0] / t_f[0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--untiled-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiles_probe: no HIP device visible - times are measured on the GPU only")

    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline, SourceFrames

    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(5)
    frames = torch.randint(0, 256, (F, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    det_cfg = spec.DetectorConfig()
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=20000)
    m.add(np.random.default_rng(2).standard_normal((20000, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=MAX_BATCH),
                    Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1, quad_source="mask",
                    **({} if a.untiled_only else {"cards_per_tile": KT}))
    out = [f"tiles_probe: {torch.cuda.get_device_name(0)}, {F} frames of {W} x {H}, detector input {S} x {S}, {K} cards per frame; "
           f"median [p10, p90] of {a.runs} runs after {a.warmup}, ms (HIP events)"]
    sf = SourceFrames.from_frames(frames, size=S)
    t_u = median_ms(lambda: pipe.run(sf), a.runs, a.warmup)
    out.append(f"Pipeline.run(SourceFrames), the four frames untiled:      {fmt(t_u)}")
    if not a.untiled_only:
        from mtgv.crop import mask_quads_from_logits, select_cards, warp_quads_src, warp_workspace
        from mtgv.tiles import TiledFrames, cut_tiles, merge_tiles

        tf = TiledFrames.from_frames(frames, window_hw=(S, S), overlap=OVERLAP, with_full=True, size=S)
        nt = int(tf.tiles.shape[0])
        assert nt == MAX_BATCH, nt
        out.insert(1, f"windows {S} x {S}, overlap {OVERLAP}, with the full frame: {nt} tiles ({nt // F} per frame), {KT} cards per tile, "
                      f"{nt // F * KT} candidates per frame; the cut moves {nt * S * S * 3 / 1e6:.1f} MB in and out")
        det = pipe.detector
        dst = torch.empty_like(tf.frames)
        t_cut = median_ms(lambda: cut_tiles(tf.buf, tf.offsets, tf.hw, tf.tiles, tf.geo, dst), a.runs, a.warmup)

        def forward():
            parts = [det.forward(tf.frames[i : i + det.max_batch], mask_rows=KT) for i in range(0, nt, det.max_batch)]
            return parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}

        d = forward()
        t_fwd = median_ms(forward, a.runs, a.warmup)

        def quads():
            sel, _, _ = select_cards(d["n_det"], d["boxes"], pipe._pad_tile, KT, want_quads=False)
            return mask_quads_from_logits(d["mask_logits"].view(nt * KT, *d["mask_logits"].shape[-2:]), sel)[0]

        q = quads()
        t_q = median_ms(quads, a.runs, a.warmup)
        merge = lambda: merge_tiles(tf, d["n_det"], d["boxes"], d["conf"], q, KT, pipe._pad_frac, K, 2.0, 0.5)  # noqa: E731
        mo = merge()
        t_m = median_ms(merge, a.runs, a.warmup)
        ws = warp_workspace(F * K, "cuda")
        t_w = median_ms(lambda: warp_quads_src(tf.sources(), mo["quads_src"], mo["frame_idx"], (192, 128), 0.05, ws), a.runs, a.warmup)
        t_run = median_ms(lambda: pipe.run(tf), a.runs, a.warmup)
        t_all = median_ms(lambda: pipe.run(TiledFrames.from_frames(frames, window_hw=(S, S), overlap=OVERLAP, with_full=True, size=S)), a.runs, a.warmup)
        out.append(f"n_det per tile {d['n_det'].cpu().tolist()}, n_sel per frame {mo['n_sel'].cpu().tolist()}")
        out.append(f"the cut, one launch for {nt} tiles:                        {fmt(t_cut)}")
        out.append(f"the detector forward on the {nt} tiles:                    {fmt(t_fwd)}")
        out.append(f"per-tile select + mask quads ({nt * KT} rows):              {fmt(t_q)}")
        out.append(f"the merge, one workgroup per frame:                       {fmt(t_m)}")
        out.append(f"the de-warp of {F * K} cards from the sources:               {fmt(t_w)}")
        out.append(f"Pipeline.run(TiledFrames):                                {fmt(t_run)}")
        out.append(f"TiledFrames.from_frames + Pipeline.run (tables, cut):     {fmt(t_all)}")
        out.append(f"cut + merge over the forward on the same tiles: {(t_cut[0] + t_m[0]) / t_fwd[0]:.3f}")
    obb_leg(frames, a, out)
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
