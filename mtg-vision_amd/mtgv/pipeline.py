"""detect -> crop -> embed -> match on one GPU without host round trips.

The reference runs this per frame and per card with batch 1 (mtgvision/server.py:133-207:
segmenter(frame) -> extract_dewarped -> encoder.predict -> vecs.query_nearby(k=3)).  Here a whole
batch of frames goes through each stage once; every stage's arithmetic is in libmtgv.so.
"""

from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from . import crop, native
from .crop import mask_quads_from_logits, obb_cards, select_cards, warp_quads, warp_workspace
from .detector import Detector, fit_geometry
from .encoder import Encoder
from .matcher import Matcher
from .tiles import TiledFrames, merge_tiles, merge_tiles_obb

# fixed quads (pixels of the 640x640 frame; scaled with a rectangular detector's input, Pipeline.__init__) used when a frame has fewer than K detections, so that
# cards/sec is well defined on synthetic frames
_PAD_BOXES = torch.tensor(
    [[40.0, 60.0, 168.0, 252.0], [200.0, 60.0, 328.0, 252.0], [360.0, 60.0, 488.0, 252.0], [500.0, 60.0, 628.0, 252.0],
     [40.0, 330.0, 168.0, 522.0], [200.0, 330.0, 328.0, 522.0], [360.0, 330.0, 488.0, 522.0], [500.0, 330.0, 628.0, 522.0]]
)


class HostFrames:
    """Frame batches that arrive in host memory, as the reference's do (one JPEG per websocket message decoded on the host,
    mtgvision/server.py:272-280): the batches are copied to the GPU on a third stream - hipMemcpyAsync from pinned memory,
    the copy engine, no kernel - into a small ring of device buffers while the previous batches are being processed.

        src = HostFrames(pinned_batches, device)
        outs = pipe.run_many(src.leases(n_steps))

    A lease's `tensor()` makes the consuming stream wait for its copy; `done()` (called by the pipeline after the last
    stage that reads the frames - the de-warp) lets the buffer be overwritten by the copy `depth` batches later."""

    def __init__(self, host_batches, device, depth: int = 3):
        assert depth >= 2 and len(host_batches) > 0
        self.host = [b if b.is_pinned() else b.pin_memory() for b in host_batches]
        self.device = torch.device(device)
        self.depth = depth
        self.s_copy = torch.cuda.Stream(self.device)
        self.bufs = [torch.empty(self.host[0].shape, dtype=self.host[0].dtype, device=self.device) for _ in range(depth)]
        self.copied = [torch.cuda.Event() for _ in range(depth)]
        self.released = [None] * depth
        self._issued = 0

    class _Lease:
        def __init__(self, src, slot):
            self.src, self.slot = src, slot

        def tensor(self) -> torch.Tensor:
            torch.cuda.current_stream(self.src.device).wait_event(self.src.copied[self.slot])
            return self.src.bufs[self.slot]

        def done(self) -> None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.src.device))
            self.src.released[self.slot] = ev

    def _issue(self, batch_index: int):
        j = self._issued % self.depth
        h = self.host[batch_index % len(self.host)]
        self._issued += 1
        with torch.cuda.stream(self.s_copy):
            if self.released[j] is not None:
                self.s_copy.wait_event(self.released[j])  # the batch that used this buffer has been de-warped
            self.bufs[j].copy_(h, non_blocking=True)
            self.copied[j].record(self.s_copy)
        return HostFrames._Lease(self, j)

    def leases(self, n: int):
        """n leases of host batches 0, 1, ... (cyclically); copies run one to two batches ahead of their consumer.  Copy
        i + 1 is issued when lease i is handed out (i >= 1): its buffer was last used by lease i - 2, whose done() the
        pipeline recorded one batch ago - so the event the copy has to wait for always exists by then."""
        ahead = [self._issue(b) for b in range(min(n, self.depth - 1))]
        issued = len(ahead)
        for i in range(n):
            if i > 0 and issued < n:
                ahead.append(self._issue(issued))
                issued += 1
            yield ahead.pop(0)


def _host_i64(a, shape) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.int64).reshape(shape)


@dataclass
class SourceFrames:
    """A batch of frames as the camera delivered them, beside the detector input made from them.  Handed to `Pipeline.run` /
    `run_many` / `TrackedPipeline.run` in place of the frame tensor, detection runs on `frames` and every card is cropped
    from its own source frame at that frame's resolution, as the reference crops from the caller's frame
    (mtgvision/od_export.py:95-111, server.py:173) - not from the letterboxed copy.

    buf (bytes,) uint8: the frames back to back, HWC RGB; offsets (n,) int64 byte offset of each; hw (n, 2) int32 height,
    width (the ragged layout of `JpegDecoder.decode` and mtgv_make_cropped); geo (n, 4) int32 = nh, nw, top, left and ratio
    (n,) float64: each frame's `fit_geometry` into the detector's input; frames (n, in_h, in_w, 3) uint8: that input.  All
    on the device."""

    buf: torch.Tensor
    offsets: torch.Tensor
    hw: torch.Tensor
    geo: torch.Tensor
    ratio: torch.Tensor
    frames: torch.Tensor

    @staticmethod
    def geometry(hw, input_hw):
        """host side: (geo (n, 4) int32 = nh, nw, top, left, ratio (n,) float64) of (n, 2) frame sizes into input_hw,
        `fit_geometry` per frame"""
        g = [fit_geometry(int(h), int(w), int(input_hw[0]), int(input_hw[1])) for h, w in np.asarray(hw).reshape(-1, 2)]
        geo = np.array([t[1:] for t in g], np.int32).reshape(len(g), 4)
        return geo, np.array([t[0] for t in g], np.float64)

    @classmethod
    def from_ragged(cls, buf: torch.Tensor, offsets, hw, size: int = 640, input_hw=None, pad_value: int = 114, out: torch.Tensor = None):
        """frames of their own sizes in one buffer (offsets, hw: host sequences or arrays; device tensors are read back) ->
        SourceFrames whose `frames` are all of them letterboxed into (size, size) or input_hw in one launch
        (mtgv_letterbox_ragged_u8; `out`: the tensor to write them to)."""
        native.require_gpu()
        assert buf.is_cuda and buf.dtype == torch.uint8 and buf.ndim == 1 and buf.is_contiguous(), f"{tuple(buf.shape)} {buf.dtype}"
        hw_h = _host_i64(hw, (-1, 2))
        n = hw_h.shape[0]
        off_h = _host_i64(offsets, (n,))
        oh, ow = (int(size), int(size)) if input_hw is None else (int(input_hw[0]), int(input_hw[1]))
        # the kernels trust these tables: every frame has pixels and lies inside the buffer
        assert n == 0 or ((hw_h > 0).all() and (off_h >= 0).all() and (off_h + hw_h[:, 0] * hw_h[:, 1] * 3 <= buf.numel()).all()), \
            f"frames (offsets {off_h.tolist()}, sizes {hw_h.tolist()}) outside a buffer of {buf.numel()} bytes"
        geo, ratio = cls.geometry(hw_h, (oh, ow))
        dev = buf.device
        if out is None:
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
        assert tuple(out.shape) == (n, oh, ow, 3) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev
        sf = cls(buf, torch.from_numpy(off_h).to(dev), torch.from_numpy(hw_h.astype(np.int32)).to(dev), torch.from_numpy(geo).to(dev),
                 torch.from_numpy(ratio).to(dev), out)
        if n and out.data_ptr() != buf.data_ptr():  # (from_frames: frames of the input's own size are the input)
            with torch.cuda.device(dev):
                native.check(native.lib().mtgv_letterbox_ragged_u8(native.ptr(buf), native.ptr(sf.offsets), native.ptr(sf.hw), native.ptr(sf.geo), n,
                                                                   native.ptr(out), oh, ow, int(pad_value), native.stream()))
        return sf

    @classmethod
    def from_frames(cls, frames: torch.Tensor, size: int = 640, input_hw=None, pad_value: int = 114):
        """(n, h, w, 3) uint8 same-sized frames on the device: the buffer is the tensor itself (offsets i * h * w * 3, no
        copy).  Frames that already have the detector's input size are that input, without a launch; others are letterboxed
        as in from_ragged."""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3 and frames.is_contiguous(), \
            f"{tuple(frames.shape)} {frames.dtype}"
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        oh, ow = (int(size), int(size)) if input_hw is None else (int(input_hw[0]), int(input_hw[1]))
        return cls.from_ragged(frames.view(-1), np.arange(n, dtype=np.int64) * (h * w * 3), [(h, w)] * n, input_hw=(oh, ow), pad_value=pad_value,
                               out=frames if (h, w) == (oh, ow) else None)


def _frames_of(item):
    """(tensor, lease or None, SourceFrames or None) of a batch handed to run / run_many: a device tensor, a SourceFrames,
    or a lease of HostFrames / JpegFrames (one that has `sources()` - JpegFrames(keep_source=True) - brings its SourceFrames)"""
    if isinstance(item, SourceFrames):
        return item.frames, None, item
    if hasattr(item, "tensor") and hasattr(item, "done"):
        return item.tensor(), item, (item.sources() if hasattr(item, "sources") else None)
    return item, None, None


def _no_tiles(batches, who: str):
    """the batches of a run_many, refusing a TiledFrames when its turn comes"""
    for b in batches:
        if isinstance(b[0] if isinstance(b, tuple) else b, TiledFrames):
            raise NotImplementedError(f"{who} does not take TiledFrames: the overlapped schedule for a tile batch is not built; call run per batch")
        yield b


@dataclass
class Cropped:
    """What `Pipeline.crop` hands on.  boxes (F, K, 4); crops (F * K, h, w, 3) uint8; quads (F * K, 4, 2): what the de-warp
    was given, pixels of the detector's input; quads_src: the same corners in camera pixels (SourceFrames only); card_state
    (F * K,) ("obb" only); thumbs, thumb_offsets: filled by `Pipeline._thumbnails` when the pipeline encodes them.
    TiledFrames only: boxes, quads and quads_src are all camera pixels, n_sel (F,) is the frames' card count (the step's
    n_det) and tile_slot (F * K,) each card's tile * cards_per_tile + detection, -1 for a pad."""

    boxes: torch.Tensor
    crops: torch.Tensor
    quads: torch.Tensor
    quads_src: Optional[torch.Tensor] = None
    card_state: Optional[torch.Tensor] = None
    thumbs: Optional[torch.Tensor] = None
    thumb_offsets: Optional[torch.Tensor] = None
    n_sel: Optional[torch.Tensor] = None
    tile_slot: Optional[torch.Tensor] = None

    def extras(self, det: dict, F: int, K: int) -> dict:
        """the optional parts as an output dict carries them; those that are no thumbnails go into its `det` as well"""
        out = {}
        if self.card_state is not None:
            out["quads"], out["card_state"] = self.quads.view(F, K, 4, 2), self.card_state.view(F, K)
        if self.quads_src is not None:
            out["quads_src"] = self.quads_src.view(F, K, 4, 2)
        det.update(out)
        if self.tile_slot is not None:  # (behind det.update: det keeps the per-tile n_det)
            out["n_det"], out["tile_slot"] = self.n_sel, self.tile_slot.view(F, K)
        if self.thumbs is not None:
            out["thumbs"], out["thumb_offsets"] = self.thumbs, self.thumb_offsets
        return out


class Pipeline:
    def __init__(self, detector: Detector, encoder: Encoder, matcher, cards_per_frame: int = 8, top_k: int = 1,
                 match_fn: Optional[Callable] = None, quad_source: str = "box", thumbnail_quality: Optional[int] = None,
                 match_opts: Optional[dict] = None, cards_per_tile: Optional[int] = None, tile_merge: Optional[dict] = None):
        """quad_source: "box" crops the detection boxes (the synthetic bench workload);
        "mask" crops the oriented quad fitted to each detection's mask, as the reference does
        (od_export.py:52-111: InstanceSeg._orient + extract_dewarped); "obb" (an OBB detector, spec.DetectorConfig(task="obb"))
        crops the oriented quad of each card-class rotated box, turned by the card_top / card_bottom detections inside it
        (crop.obb_cards, classes 0 / 1 / 2 as od_datasets.py:244-257 labels them) - the output gains `quads` (F, K, 4, 2) and
        `card_state` (F, K) (0 pad, 1 unoriented, 2 oriented).
        thumbnail_quality: when set, every step's crops are also encoded as 4:2:0 JPEG files at that quality on the GPU
        right after the de-warp, on the stream that made them (the thumbnails of mtgvision/server.py:222-225); the
        output gains `thumbs` (packed files, device) and `thumb_offsets` ((F * K + 1,) int64, device), file j being
        thumbs[thumb_offsets[j]:thumb_offsets[j + 1]].  None (default): no encode, no extra launch.
        match_opts: keyword arguments handed to `matcher.match` (threshold, filter, distinct), like TrackedPipeline's;
        None keeps the call as it is.  `matcher` may be a `mtgv.ShardedMatcher` (the row-sharded bank).
        cards_per_tile, tile_merge: read only by `run(TiledFrames)` - the detections kept per tile (None: cards_per_frame) and
        the merge rule's `edge` (pixels) and `ios` (mtgv.tiles.merge_tiles_host; None: edge 2.0, ios 0.5).  An "obb" pipeline
        takes TiledFrames only with tile_merge={"rule": "rotated"} (mtgv.tiles.merge_tiles_obb_host: the overlap of two
        oriented quads is the area of their intersection, and orientation is carried over from a dropped duplicate)."""
        assert quad_source in ("box", "mask", "obb"), quad_source
        task = getattr(getattr(detector, "cfg", None), "task", "seg")
        assert (quad_source == "obb") == (task == "obb"), f'quad_source "{quad_source}" with a {task} detector'
        self.quad_source = quad_source
        self.thumbnail_quality = None if thumbnail_quality is None else int(thumbnail_quality)
        self._jpeg = None
        if self.thumbnail_quality is not None:
            from .jpeg import JpegEncoder

            assert 1 <= self.thumbnail_quality <= 100, thumbnail_quality
            h, w = encoder.cfg.image_hw
            # the encoder takes at most encoder.max_batch crops per step
            self._jpeg = JpegEncoder(encoder.max_batch, encoder.max_batch * (-(-h // 16) * 16) * (-(-w // 16) * 16), detector.device)
        self.detector, self.encoder, self.matcher = detector, encoder, matcher
        self.K = int(cards_per_frame)
        self.top_k = int(top_k)
        # a caller-supplied match (bench.py: the sharded bank's local top-k + all-gathers + merge) may issue collectives, which
        # run on the process group's own normal-priority stream: run_many then keeps every stream at normal priority (below);
        # so does a matcher that says it issues them (ShardedMatcher)
        self._plain_match = match_fn is None and not getattr(matcher, "issues_collectives", False)
        assert match_fn is None or not match_opts, "match_opts go to matcher.match: a match_fn takes its own"
        opts = dict(match_opts or {})
        if match_fn is None and opts:
            match_fn = lambda z, k: matcher.match(z, k, **opts)  # noqa: E731
        self.match_fn = match_fn or (lambda z, k: matcher.match(z, k))
        reps = (self.K + _PAD_BOXES.shape[0] - 1) // _PAD_BOXES.shape[0]
        # a rectangular detector (cfg.input_hw): the pad boxes shrink with the frame, (in_w / imgsz, in_h / imgsz), and stay
        # inside it; a square handle keeps the numbers above
        dcfg = getattr(detector, "cfg", None)
        sx, sy = (dcfg.in_w / dcfg.imgsz, dcfg.in_h / dcfg.imgsz) if getattr(dcfg, "input_hw", None) is not None else (1.0, 1.0)
        pad = _PAD_BOXES * torch.tensor([sx, sy, sx, sy])
        self._pad = pad.repeat(reps, 1)[: self.K].to(detector.device).contiguous()
        self._warp_ws = None
        self.Kt = self.K if cards_per_tile is None else int(cards_per_tile)
        self.tile_merge = {"edge": 2.0, "ios": 0.5, **(tile_merge or {})}
        assert set(self.tile_merge) - {"rule"} == {"edge", "ios"}, f"tile_merge keys {sorted(self.tile_merge)}: expected edge, ios and optionally rule"
        if "rule" in self.tile_merge:
            assert self.tile_merge["rule"] == "rotated", f'tile_merge rule "{self.tile_merge["rule"]}": the only rule to choose is "rotated"'
            assert quad_source == "obb", f'tile_merge rule "rotated" with quad_source "{quad_source}": it merges the quads of an "obb" pipeline'
        # the tiled path's pads: fractions of each frame's own size, and the per-tile pad of select_cards
        self._pad_frac = (_PAD_BOXES / 640.0).repeat(reps, 1)[: self.K].to(detector.device).contiguous()
        treps = (self.Kt + _PAD_BOXES.shape[0] - 1) // _PAD_BOXES.shape[0]
        self._pad_tile = pad.repeat(treps, 1)[: self.Kt].to(detector.device).contiguous()

    def _embed_match(self, frames_u8: torch.Tensor, det, lease=None, src=None):
        return self._embed(det, self._thumbnails(self.crop(frames_u8, det, lease, src)))

    def _thumbnails(self, cropped: Cropped) -> Cropped:
        """fills thumbs, thumb_offsets: the crops as JPEG files, encoded on the current stream; nothing when off"""
        if self._jpeg is not None:
            cropped.thumbs, cropped.thumb_offsets = self._jpeg.encode_device(cropped.crops, self.thumbnail_quality, 420)
        return cropped

    def crop(self, frames_u8: torch.Tensor, det, lease=None, src=None) -> Cropped:
        """detections -> Cropped: the K best boxes, mask quadrilaterals or oriented boxes per frame, de-warped from frames_u8
        or, with `src` (SourceFrames), from the source frames.  `det` is read, not written."""
        F, K = frames_u8.shape[0], self.K
        if self.quad_source == "obb":
            quads, sel, frame_idx, state = obb_cards(det["n_det"], det["rboxes"], det["conf"], det["cls"], self._pad, K, 0, 1, 2)
            return self._warp(frames_u8, sel.view(F, K, 4), quads, frame_idx, lease, src, state)
        # the K highest-confidence detections per frame (NMS output is score-descending), pad boxes where a frame has
        # fewer; every step of the glue is a library kernel (no PyTorch arithmetic on the streams of the step)
        want_mask = self.quad_source == "mask"
        sel, quads, frame_idx = select_cards(det["n_det"], det["boxes"], self._pad, K, want_quads=not want_mask)
        if want_mask:
            # masks of the K best detections (logits are zero outside a detection's box and in rows beyond n_det):
            # interpolated to frame resolution, thresholded and fitted inside one kernel; an empty mask - no detection
            # in that slot, or nothing above threshold - falls back to the slot's box inside the kernel
            ml = det["mask_logits"]
            assert ml.shape[1] == K, f"mask rows {ml.shape[1]} != cards per frame {K}"
            quads, _ = mask_quads_from_logits(ml.view(F * K, *ml.shape[-2:]), sel)
        return self._warp(frames_u8, sel.view(F, K, 4), quads, frame_idx, lease, src)

    def _warp(self, frames_u8, boxes, quads, frame_idx, lease, src=None, state=None) -> Cropped:
        """the one place every quad_source's quads are de-warped.  With `src` the quads (pixels of the detector's input, like
        the boxes) are mapped into their source frames and the crops come from there; the record gains quads_src."""
        F, K = frames_u8.shape[0], self.K
        if self._warp_ws is None or self._warp_ws.numel() < 9 * F * K:
            self._warp_ws = warp_workspace(F * K, frames_u8.device)  # once per pipeline (the largest batch seen so far)
        if src is None:
            crops, quads_src = warp_quads(frames_u8, quads, frame_idx, self.encoder.cfg.image_hw, 0.05, self._warp_ws), None
        else:
            crops, quads_src = crop.warp_quads_src(src, quads, frame_idx, self.encoder.cfg.image_hw, 0.05, self._warp_ws)
        if lease is not None:
            lease.done()  # the de-warp is the last reader of the frames
        return Cropped(boxes, crops, quads, quads_src, state)

    def _embed(self, det, cropped: Cropped, match_stream=None):
        F, K = cropped.boxes.shape[0], self.K
        z = self.encoder.encode(cropped.crops)
        if match_stream is None:
            ids, scores = self.match_fn(z, self.top_k)
        else:  # the match on a stream of its own: the next batch's encoder does not queue behind it
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(z.device))
            with torch.cuda.stream(match_stream):
                match_stream.wait_event(ev)
                z.record_stream(match_stream)
                ids, scores = self.match_fn(z, self.top_k)
        out = {
            "ids": ids.view(F, K, self.top_k),
            "scores": scores.view(F, K, self.top_k),
            "n_det": det["n_det"],
            "boxes": cropped.boxes,
            "crops": cropped.crops,
            "z": z,
            "det": det,
        }
        out.update(cropped.extras(det, F, K))
        return out

    @staticmethod
    def overlap_enabled() -> bool:
        """Two-stream overlap is opt-in (MTGV_OVERLAP=on): while the split-precision GEMMs of one stream run, kernels of
        OTHER libraries that use packed-FP32 VALU instructions on another stream of the same GPU have been seen to lose
        lanes.  This library is built without those instructions, both streams of `run_many` launch
        library kernels only (output tensors are torch.empty, the glue between the stages is mtgv_select_cards) and
        tests/test_gpu_overlap.py guards the combination; an application that runs foreign kernels beside it keeps the
        default."""
        return os.environ.get("MTGV_OVERLAP", "off") == "on"

    def run_many(self, batches, flip_rgb: bool = True):
        """Process a sequence of frame batches with the detect + crop stages of batch i+1 (one stream) overlapped with the
        embed stage of batch i (a second stream) and its match (a third); with the library's own match the latter two run at
        high priority, with a caller-supplied (collective) match all three at normal priority - the comments below and
        DESIGN.md section 5 say why (round 4: +7 % cards/s over round 3's two equal-priority streams with the crops in front
        of the encoder, independent of the order in which the application created its handles).  The detector's late layers
        have too few tiles to fill 256 CUs on their own; they and the latency-bound crop kernels fill what the encoder's GEMMs
        of the previous batch leave idle.  Results are identical to `run` on each batch (same kernels, same order per stream).

        Opt-in: without MTGV_OVERLAP=on everything stays on the current stream (see overlap_enabled).  (History: with packed-FP32 VALU instructions in
        the library, kernels sharing a CU with the split-precision GEMM of the other stream sporadically lost a
        packed result in one 16-lane group; the library is built without those instructions - build.py, DESIGN.md
        section 5 - and tests/test_gpu_overlap.py guards the combination.)"""
        batches = _no_tiles(batches, "Pipeline.run_many")
        if not self.overlap_enabled():
            return [self.run(frames, flip_rgb) for frames in batches]
        crop_on_det, s_match, cur = self._overlap_streams()
        with self._det_fork_off():
            return self._run_overlapped(batches, flip_rgb, crop_on_det, s_match, cur)

    def _overlap_streams(self):
        """the streams of the overlapped schedules (run_many here and TrackedPipeline.run_many), created on first use:
        self._s_det, self._s_enc and the match stream, each waiting for the current stream
        -> (crop_on_det, s_match or None, the current stream)"""
        dev = self.detector.device
        if not hasattr(self, "_s_det"):
            # The embed + match stream runs at high priority: it is the longer chain (6 of a step's 8 ms), so its kernels get the
            # CUs as if alone and the detect + crop stream fills what they leave idle (tails, half-empty rounds, small launches)
            # instead of sharing every CU half and half.  MTGV_STREAM_PRIO=none|det: equal priorities / the other way round.
            # With a match that issues collectives (sharded bank) every stream stays at normal priority: a high-priority stream
            # that calls into the process group - whose own stream is a normal-priority one, queued with long event waits in
            # the hardware queues the detect stream uses - cost 19 % (world-size-1 RCCL run: 25.6k vs 31.7k cards/s; 32.0k replicated).
            prio = os.environ.get("MTGV_STREAM_PRIO", "enc" if self._plain_match else "none")
            self._s_det = torch.cuda.Stream(dev, priority=-1 if prio == "det" else 0)
            self._s_enc = torch.cuda.Stream(dev, priority=-1 if prio == "enc" else 0)
        crop_on_det = os.environ.get("MTGV_CROP_STAGE", "det") != "enc"
        # the match (normalise, first-pass GEMM, re-rank, merge: 0.16 ms, half of it latency-bound) on a third stream:
        # the next batch's encoder starts as soon as this batch's is done (MTGV_MATCH_STREAM=0: behind the encoder)
        s_match = None
        if os.environ.get("MTGV_MATCH_STREAM", "1") == "1":
            if not hasattr(self, "_s_match"):
                # (high priority like the embed stream: in the runtime's normal-priority pool its stream would share a hardware
                # queue with another normal stream - which one depends on the order in which the application created its
                # handles - and the match's wait for the encoder, queued long before it can be satisfied, then holds up
                # whatever sits behind it in that queue: measured 8.3 vs 9.3 ms per step, tools/debug/enqueue_time.py)
                mp = os.environ.get("MTGV_MATCH_PRIO", "-1" if self._plain_match else "0")
                self._s_match = torch.cuda.Stream(dev, priority=0 if mp == "0" else -1)
            s_match = self._s_match
            s_match.wait_stream(torch.cuda.current_stream(dev))
        cur = torch.cuda.current_stream(dev)
        self._s_det.wait_stream(cur)
        self._s_enc.wait_stream(cur)
        return crop_on_det, s_match, cur

    @contextlib.contextmanager
    def _det_fork_off(self):
        # The detector's own fork-join is for the one-stream schedule (its late layers alone on 256 CUs); here the embed stream
        # fills those gaps, and the branch streams would only add normal-priority streams to the few hardware queues:
        # 8.05 vs 8.3 ms per step with it off, whatever the handle creation order (MTGV_OVERLAP_DET_FORK=1: left on)
        fork_off = os.environ.get("MTGV_OVERLAP_DET_FORK", "0") != "1"
        if fork_off:
            self.detector.set_fork(0)
        try:
            yield
        finally:
            if fork_off:
                self.detector.set_fork(-1)

    def _run_overlapped(self, batches, flip_rgb, crop_on_det, s_match, cur):
        import itertools

        outs, pending = [], None
        for item in itertools.chain(batches, [None]):  # (lazily: a HostFrames lease is issued when its turn comes)
            nxt = None
            if item is not None:
                with torch.cuda.stream(self._s_det):
                    frames, lease, src = _frames_of(item)
                    det = self.detector.forward(frames, flip_rgb, mask_rows=self.K)
                    # the crop stage (card selection, mask -> quadrilateral, de-warp: latency-bound kernels of a few hundred
                    # workgroups) belongs to the detect stream: beside the other stream's GEMMs it costs next to nothing, in
                    # front of the encoder it would leave most of the GPU idle (MTGV_CROP_STAGE=enc: the round-3 split)
                    cropped = self.crop(frames, det, lease, src) if crop_on_det else None
                    ev = torch.cuda.Event()
                    ev.record(self._s_det)
                    if cropped is not None:  # behind the event: this batch's embed does not wait for its thumbnails
                        self._thumbnails(cropped)
                nxt = (frames, det, ev, lease, cropped, src)
            if pending is not None:
                pf, pdet, pev, please, pcrop, psrc = pending
                with torch.cuda.stream(self._s_enc):
                    self._s_enc.wait_event(pev)
                    for t in list(pdet.values()) + list(vars(pcrop).values() if pcrop is not None else ()):
                        if t is not None:
                            t.record_stream(self._s_enc)
                    outs.append(self._embed(pdet, pcrop, match_stream=s_match) if pcrop is not None
                                else self._embed_match(pf, pdet, please, psrc))
            pending = nxt
        cur.wait_stream(self._s_det)
        cur.wait_stream(self._s_enc)
        if s_match is not None:
            cur.wait_stream(s_match)
        for o in outs:
            for t in (o["ids"], o["scores"], o["z"], o["crops"], o["boxes"], o.get("thumbs"), o.get("thumb_offsets"), o.get("quads_src")):
                if t is not None:
                    t.record_stream(cur)
        return outs

    def run(self, frames_u8: torch.Tensor, flip_rgb: bool = True):
        """frames (F, in_h, in_w, 3) uint8 on the GPU (640 x 640 unless the detector's cfg.input_hw names a rectangle; the mask
        quads, the OBB quads and the de-warp work in the pixels of that frame) -> dict with ids (F, K, top_k) int64, scores, n_det (F,)
        and the intermediate crops / embeddings (device tensors).

        A `SourceFrames` (or a lease that has `sources()`) instead: detection runs on its `frames`, the quads go back into
        the camera's frames and the cards are cropped from those at their own resolution; the dict gains quads_src
        (F, K, 4, 2), the corners in camera pixels.  boxes (and an OBB detector's quads) stay pixels of the detector's input."""
        if isinstance(frames_u8, TiledFrames):
            det, cropped = self.detect_crop_tiled(frames_u8, flip_rgb)
            return self._embed(det, self._thumbnails(cropped))
        frames_u8, lease, src = _frames_of(frames_u8)
        det = self.detector.forward(frames_u8, flip_rgb, mask_rows=self.K)
        return self._embed_match(frames_u8, det, lease, src)

    def detect_crop_tiled(self, tf: TiledFrames, flip_rgb: bool = True):
        """The detect and crop stages of a `TiledFrames` batch -> (det, Cropped).  The detector runs on the tiles as if they
        were frames, in chunks of its max_batch (`det`: its outputs per tile, concatenated); the K best cards of every frame
        come out of mtgv_tiles_merge in camera pixels (mtgv.tiles.merge_tiles_host is the rule) and are de-warped from the
        source frames.  Output per frame: boxes (F, K, 4) and quads_src (F, K, 4, 2) in camera pixels, n_det = the merge's n_sel,
        tile_slot (F, K) = tile * cards_per_tile + detection of every card (-1: a pad).  An "obb" pipeline with the rotated rule
        runs crop.obb_cards per tile and mtgv_tiles_merge_obb instead (mtgv.tiles.merge_tiles_obb_host): its cards also carry
        quads (= quads_src) and card_state, and tile_slot counts a tile's card slots."""
        obb = self.quad_source == "obb"
        if obb and self.tile_merge.get("rule") != "rotated":
            raise NotImplementedError('quad_source "obb" takes TiledFrames only with the rotated overlap rule: Pipeline(..., tile_merge={"rule": "rotated"})')
        F, K, Kt = tf.n_frames, self.K, self.Kt
        nt, mb = int(tf.frames.shape[0]), self.detector.max_batch
        assert F > 0 and nt > 0, "a TiledFrames batch without frames"
        want_mask = self.quad_source == "mask"
        parts = [self.detector.forward(tf.frames[i : i + mb], flip_rgb, mask_rows=Kt if want_mask else 0) for i in range(0, nt, mb)]
        det = parts[0] if len(parts) == 1 else {k: (None if v is None else torch.cat([p[k] for p in parts])) for k, v in parts[0].items()}
        if obb:
            # the card slots of every tile, oriented where the tile saw a marker; the rotated rule merges them and carries
            # the orientation of a dropped duplicate over to the one it keeps
            quads, _, _, state = obb_cards(det["n_det"], det["rboxes"], det["conf"], det["cls"], self._pad_tile, Kt, 0, 1, 2)
            m = merge_tiles_obb(tf, det["n_det"], det["conf"], det["cls"], quads, state, Kt, self._pad_frac, K, self.tile_merge["edge"],
                                self.tile_merge["ios"], 0)
            return det, self._warp_tiled(tf, m, m["state"])
        quads = None  # "box": the merge takes the boxes' corners itself
        if want_mask:
            sel, _, _ = select_cards(det["n_det"], det["boxes"], self._pad_tile, Kt, want_quads=False)
            ml = det["mask_logits"]
            quads, _ = mask_quads_from_logits(ml.view(nt * Kt, *ml.shape[-2:]), sel)
        m = merge_tiles(tf, det["n_det"], det["boxes"], det["conf"], quads, Kt, self._pad_frac, K, self.tile_merge["edge"], self.tile_merge["ios"])
        return det, self._warp_tiled(tf, m)

    def _warp_tiled(self, tf: TiledFrames, m: dict, state=None) -> Cropped:
        """a merge's cards -> Cropped, de-warped from the source frames"""
        F, K = tf.n_frames, self.K
        if self._warp_ws is None or self._warp_ws.numel() < 9 * F * K:
            self._warp_ws = warp_workspace(F * K, tf.buf.device)
        # the quads are camera pixels already: an identity geometry makes mtgv_warp_quads_src read them as they are
        crops, quads_src = crop.warp_quads_src(tf.sources(), m["quads_src"], m["frame_idx"], self.encoder.cfg.image_hw, 0.05, self._warp_ws)
        return Cropped(m["sel_boxes_src"].view(F, K, 4), crops, quads_src, quads_src, card_state=state, n_sel=m["n_sel"], tile_slot=m["src_slot"])
