#!/usr/bin/env python3
"""What tracking costs and what its gating saves on the bench workload (32 streams x 8 cards, AE-tiny, 100k x 768 bank,
quad_source "mask", one stream, HIP events, after the settle steps bench.py uses):

    (1) Pipeline.run                                  the untracked baseline: every crop embedded and matched every step
    (2) TrackedPipeline.run, no wait and no delay     every detection due every step: the tracker's own overhead
    (3) TrackedPipeline.run, 1/30 s clock, 0.5 s wait the steady state of the reference's gating rule, with its due fraction

and the tracker's launches one by one.  The frames are bench.py's: four batches of uniform noise in rotation, so the cards
are whatever the random-weight detector sees in noise; the association is real work, the tracks are not real cards.

    python tools/track_probe.py [--steps 40 --settle-steps 160 --out FILE]
                                [--cards K --max-tracks T --wide auto|on|off]   the tracker's size and update kernel
                                [--synthetic]   and the launches again in a synthetic steady state: T live tracks per stream,
                                                disjoint sets of K cards in rotation, every detection matched
                                [--embed-budget E [E ...]]   (3) again with an embed budget: at most E embeds per step, the
                                                encoder and the matcher on exactly E rows, no read-back (line (4)); and
                                                update + selection beside update + compaction
                                [--overlap]     each budget also through TrackedPipeline.run_many with MTGV_OVERLAP=on (line (5))
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


def _timed(fn, n):
    """mean ms of fn(i) over n calls between two HIP events, and the last result"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        r = fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, r


def _synthetic(F, K, T, wide, crops, encoder, matcher):
    """the tracker's launches with every slot in use: T // K disjoint sets of K cards (700 px apart) shown in rotation to
    tracks that outlive the rotation, so each step matches K detections against T live tracks per stream in K rounds"""
    from mtgv.track import DeviceTracker

    n_sets = max(T // K, 1)
    trk = DeviceTracker(F, K, 768, 3, max_tracks=T, wide=wide, period=8, hit_counter_max=15, initialization_delay=10, update_wait_sec=0.0)
    sets = []
    for r in range(n_sets):
        c = np.arange(r * K, (r + 1) * K)
        ctr = np.stack([100 + 700.0 * (c % 32), 100 + 700.0 * (c // 32)], -1)[:, None, :]
        q = ctr + np.array([[-40, -60], [40, -60], [40, 60], [-40, 60]], np.float64)[None]
        sets.append(torch.from_numpy(np.broadcast_to(q.astype(np.float32), (F, K, 4, 2)).copy()).cuda())
    n_det = torch.full((F,), K, dtype=torch.int32, device="cuda")
    streams, t = list(range(F)), [0.0]

    def upd(i):
        t[0] += 1.0
        return trk.update(sets[i % n_sets], streams, t[0], n_det=n_det)

    for i in range(3 * n_sets):  # every track has its id
        upd(i)
    n = 50
    ms_upd, (tid, _, n_due_dev) = _timed(upd, n)
    n_due = int(n_due_dev.item())
    live = int(trk.state(0)["live"].sum())
    ms_gather, packed = _timed(lambda i: trk.gather(crops), n)
    z = encoder.encode(packed[:max(n_due, 1)])
    ms_commit, q = _timed(lambda i: trk.commit(z), n)
    ids, scores = matcher.match(q, 3)
    ms_store, _ = _timed(lambda i: trk.store(ids, scores), n)
    return (f"synthetic steady state, {live} live tracks per stream, {int((tid > 0).sum())} of {F * K} slots matched, n_due = {n_due} "
            f"(mean of {n} back-to-back calls): update + compaction {ms_upd * 1e3:.1f} us, gather {ms_gather * 1e3:.1f} us, "
            f"commit {ms_commit * 1e3:.1f} us, store {ms_store * 1e3:.1f} us")


def _budget(a, pipe, streams, batches, T, wide, E, quads, n_det):
    """(3)'s steady state with an embed budget E: one stream (4) and, with --overlap, run_many's three streams (5); then
    update + selection on (2)'s detections with every detection due"""
    from mtgv.track import DeviceTracker, TrackedPipeline

    F, K = a.frames, a.cards
    out_lines = []
    for label, overlap in [("(4) TrackedPipeline.run", False)] + ([("(5) TrackedPipeline.run_many", True)] if a.overlap else []):
        os.environ["MTGV_OVERLAP"] = "on" if overlap else "off"
        tp = TrackedPipeline(pipe, streams=F, top_k=3, max_tracks=T, wide=wide, embed_budget=E)
        clock, outs = [0.0], []

        def chunk(n):
            steps = []
            for i in range(n):
                clock[0] += 1.0 / 30.0
                steps.append((batches[i % 4], streams, clock[0]))
            return steps

        def run(n):
            outs.extend(tp.run_many(chunk(n)) if overlap else [tp.run(*st) for st in chunk(n)])

        _timed(lambda i: run(4), max(a.warmup, 20) // 4 + 1)
        del outs[:]
        ms, _ = _timed(lambda i: run(a.steps), 1)
        ms /= a.steps
        due = np.array([int(o["n_due"].item()) for o in outs])
        deferred = np.array([int(o["n_deferred"].item()) for o in outs])
        out_lines.append(f"{label}, embed_budget {E:3d}, {'three streams' if overlap else 'one stream   '} {ms:7.3f} ms/step  {F * K / ms * 1e3:9.0f} cards/s  "
                         f"embeds/step {due.mean():6.1f} of {E} rows (max {due.max()}), deferred/step {deferred.mean():5.1f} (max {deferred.max()})")
    os.environ["MTGV_OVERLAP"] = "off"
    trk = DeviceTracker(F, K, 768, 3, max_tracks=T, wide=wide, embed_budget=E, update_wait_sec=0.0, initialization_delay=0)
    t = [2e3]

    def upd(i):
        t[0] += 1.0
        return trk.update(quads, streams, t[0], n_det=n_det)

    _timed(upd, 5)
    ms_upd, (_, _, n_due_dev) = _timed(upd, 50)
    out_lines.append(f"    update + selection (2 launches) at {int(n_due_dev.item())} selected, {int(trk.n_deferred.item())} deferred: {ms_upd * 1e3:.1f} us "
                     f"(mean of 50 back-to-back calls, host call overhead included)")
    return out_lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--cards", type=int, default=8)
    ap.add_argument("--bank", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--settle-steps", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-tracks", type=int, default=64)
    ap.add_argument("--wide", choices=("auto", "on", "off"), default="auto", help="the multi-wave update kernel: by size, forced, refused")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--embed-budget", type=int, nargs="*", default=[], help="embed budgets E to time in the gated steady state")
    ap.add_argument("--overlap", action="store_true", help="also time TrackedPipeline.run_many with MTGV_OVERLAP=on for every budget")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline
    from mtgv.track import TrackedPipeline

    torch.cuda.set_device(0)
    F, K, T = a.frames, a.cards, a.max_tracks
    wide = {"auto": None, "on": True, "off": False}[a.wide]
    det_cfg = spec.DetectorConfig()
    enc_cfg = spec.encoder_config("cnvnxt2ae_tiny", (192, 128), "conv+linear")
    detector = Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F)
    encoder = Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K)
    matcher = Matcher(768, capacity=a.bank)
    for b0 in range(0, a.bank, 12_500):
        matcher.add(np.random.default_rng([2, b0 // 12_500]).standard_normal((min(a.bank, b0 + 12_500) - b0, 768), dtype=np.float32))
    pipe = Pipeline(detector, encoder, matcher, K, 1, quad_source="mask")
    g = torch.Generator(device="cuda").manual_seed(4)
    batches = [torch.randint(0, 256, (F, 640, 640, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(4)]
    streams = list(range(F))

    for _ in range(0, a.settle_steps, 8):  # bench.py's settle phase: steady load before anything is timed
        for i in range(8):
            pipe.run(batches[i % 4])
        torch.cuda.synchronize()

    lines = [f"# track_probe: {torch.cuda.get_device_name(0)}, {F} streams x {K} cards, {T} slots per stream, wide={a.wide}, AE-tiny, bank {a.bank} x 768, mask quads, "
             f"{a.steps} steps after {a.settle_steps} settle + {a.warmup} warm-up steps"]
    ms1, _ = _timed(lambda i: pipe.run(batches[i % 4]), a.warmup)
    ms1, _ = _timed(lambda i: pipe.run(batches[i % 4]), a.steps)
    lines.append(f"(1) Pipeline.run (untracked, top-1 as bench.py)      {ms1:7.3f} ms/step  {F * K / ms1 * 1e3:9.0f} cards/s  embeds/step {F * K}")
    pipe3 = Pipeline(detector, encoder, matcher, K, 3, quad_source="mask")  # the tracked runs keep three matches per track, as the reference
    _timed(lambda i: pipe3.run(batches[i % 4]), a.warmup)
    ms1, _ = _timed(lambda i: pipe3.run(batches[i % 4]), a.steps)
    lines.append(f"(1) Pipeline.run (untracked, top-3)                  {ms1:7.3f} ms/step  {F * K / ms1 * 1e3:9.0f} cards/s  embeds/step {F * K}")

    def tracked(label, **policy):
        tp = TrackedPipeline(pipe, streams=F, top_k=3, max_tracks=T, wide=wide, **policy)
        clock, due = [0.0], []

        def step(i):
            clock[0] += 1.0 / 30.0
            out = tp.run(batches[i % 4], streams, clock[0])
            due.append(out["n_due"])
            return out

        _timed(step, max(a.warmup, 20))  # tracks get their ids and the gating reaches its rhythm
        del due[:]
        ms, out = _timed(step, a.steps)
        tracked_slots = int((out["track_ids"] > 0).sum())
        lines.append(f"{label} {ms:7.3f} ms/step  {F * K / ms * 1e3:9.0f} cards/s  embeds/step {np.mean(due):6.1f} "
                     f"(due fraction {np.mean(due) / (F * K):.3f} of {F * K} slots, {tracked_slots} slots tracked in the last step)")
        return tp, ms

    # (2): no wait and no initialisation delay, so that every detection is a track with an id and due in every step
    tp2, ms2 = tracked("(2) TrackedPipeline.run, every detection due        ", update_wait_sec=0.0, initialization_delay=0)
    tp3, ms3 = tracked("(3) TrackedPipeline.run, 1/30 s clock, 0.5 s wait   ")

    # the tracker's launches one by one, on the state (2) left behind
    trk = tp2.tracker
    out = tp2.run(batches[0], streams, 1e3)
    quads, n_det, crops = out["quads"], out["n_det"], out["crops"]
    t = [2e3]

    def upd(i):
        t[0] += 1.0
        return trk.update(quads, streams, t[0], n_det=n_det)

    n = 50
    ms_upd, (_, _, n_due_dev) = _timed(upd, n)
    ms_read, n_due = _timed(lambda i: int(n_due_dev.item()), n)
    ms_gather, packed = _timed(lambda i: trk.gather(crops), n)
    z = encoder.encode(packed[:max(n_due, 1)])
    ms_commit, q = _timed(lambda i: trk.commit(z), n)
    ids, scores = matcher.match(q, 3)
    ms_store, _ = _timed(lambda i: trk.store(ids, scores), n)
    lines.append(f"tracker launches at n_due = {n_due} (mean of {n} back-to-back calls, host call overhead included): update + compaction (2 launches) "
                 f"{ms_upd * 1e3:.1f} us, n_due read-back {ms_read * 1e3:.1f} us, gather {ms_gather * 1e3:.1f} us, commit {ms_commit * 1e3:.1f} us, "
                 f"store {ms_store * 1e3:.1f} us; sum {(ms_upd + ms_read + ms_gather + ms_commit + ms_store) * 1e3:.1f} us; (2) - (1) = {(ms2 - ms1) * 1e3:.0f} us")
    for E in a.embed_budget:
        lines.extend(_budget(a, pipe, streams, batches, T, wide, E, quads, n_det))
    if a.synthetic:
        lines.append(_synthetic(F, K, T, wide, crops, encoder, matcher))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
