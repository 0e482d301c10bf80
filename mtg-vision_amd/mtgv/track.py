"""Card tracking on the GPU for many cameras at once, and a pipeline that embeds only the tracks that are due.

The reference does not embed every card of every frame (mtgvision/server.py:133-207): detections are associated with
tracks, a track is embedded when it is new or `update_wait_sec` have passed, an exponentially weighted mean of its
embeddings queries the bank and the last matches stay on the track.  `mtgv.tracker` has that on the host for one camera;
`DeviceTracker` is the same arithmetic (fp64 filter, same order of operations, same tie-breaks) for `streams` independent
cameras with all state on the device (csrc/track.hip), `TrackedPipeline` puts it between the crop and the embed stage of
`Pipeline`.

Limits the host tracker does not have: at most `max_tracks` (<= 256) live tracks per stream - a detection that finds no
free slot is dropped and counted (`state(s)["overflow"]`) - at most 64 cards per frame, every stream at most once per
step, int32 ids, and at most 65535 rows (frames * cards per frame) in a step that is gathered.  Up to 64 tracks and 16
cards run on the one-wave update kernel; anything larger (or `wide=True` at any size) on the multi-wave one, opt-in in
the C ABI (`mtgv_tracker_create_ex`, `MTGV_TRACKER_WIDE`), with the same results.  Like the host class it restates norfair's published algorithm: parity with norfair itself is unpinned.

Embed budget (`embed_budget=E`, opt-in): a step embeds at most E tracks, the longest-waiting of the due ones first
(`mtgv.tracker.select_due` is the rule), and the others stay due.  The device enforces it, so the encoder and the matcher
always run on exactly E rows and no count comes back to the host: `TrackedPipeline.run` then has no synchronisation and
`TrackedPipeline.run_many` can enqueue steps ahead.  A step of a budget handle has at most 8192 slots (frames * cards).
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import native
from .pipeline import SourceFrames, _no_tiles
from .tiles import TiledFrames

_POLICY = ("distance_threshold", "hit_counter_max", "initialization_delay", "period", "update_wait_sec", "ewma_weight")


def check_streams(stream_of_frame: Sequence[int], streams: int) -> np.ndarray:
    """the step's stream list as int32: every value in [0, streams), none twice (AssertionError otherwise)"""
    s = np.asarray(list(stream_of_frame), dtype=np.int64).reshape(-1)
    assert s.size >= 1, "a step needs at least one frame"
    assert ((s >= 0) & (s < streams)).all(), f"stream_of_frame {s.tolist()} outside [0, {streams})"
    assert len(set(s.tolist())) == s.size, f"stream_of_frame {s.tolist()}: a stream may appear once per step"
    return s.astype(np.int32)


def _policy_cfg(cfg: native.TrackerCfg, policy: dict) -> None:
    """mtgv_tracker_cfg reads 0 as `the reference's value`: absent keys stay 0, and the two fields where 0 is a policy of
    its own are sent in the form the header names for it"""
    unknown = set(policy) - set(_POLICY)
    assert not unknown, f"unknown tracker policy {sorted(unknown)}"
    for k, v in policy.items():
        if v is None:
            continue
        if k == "initialization_delay":
            v = -1 if int(v) == 0 else int(v)  # no delay: an id at creation
        elif k == "update_wait_sec":
            v = 5e-324 if float(v) == 0.0 else float(v)  # `now - last > 0`: the smallest positive double asks the same
        else:
            assert v != 0, f"{k} = 0"
        setattr(cfg, k, v)


class DeviceTracker:
    """`streams` independent `KalmanPointTracker`s + `TrackerCtx` gating with their state on the GPU.

    A step is update -> (read n_due) -> gather -> encode -> commit -> match -> store; every call is asynchronous on the
    current stream.  policy: distance_threshold, hit_counter_max, initialization_delay, period, update_wait_sec,
    ewma_weight (defaults: the reference's 300, 5, 2, 1, 0.5 s, 0.1).

    wide: None picks the wide handle (max_tracks <= 256, cards_per_frame <= 64, the multi-wave update kernel) iff
    max_tracks > 64 or cards_per_frame > 16; True forces it at any size; False is the narrow handle, refusals included.

    embed_budget: None, or E in 1..65535: `update` reports at most E due slots per step, those whose tracks have waited
    longest (never embedded first, ties to the smaller flat slot); the other candidates keep their last_update_time, stay
    due, and are counted in `n_deferred` ((1,) int32 on the device, kept after every update).  n_due <= E always, so
    `gather(pad=True)` and `commit` work on exactly E rows with zeros behind n_due and nothing has to be read back."""

    def __init__(self, streams: int, cards_per_frame: int, dim: int, top_k: int = 3, max_tracks: int = 64, device=None, wide: Optional[bool] = None,
                 embed_budget: Optional[int] = None, **policy):
        native.require_gpu()
        self.streams, self.K, self.dim, self.top_k, self.max_tracks = int(streams), int(cards_per_frame), int(dim), int(top_k), int(max_tracks)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        cfg = native.TrackerCfg()
        cfg.streams, cfg.max_tracks, cfg.cards_per_frame, cfg.dim, cfg.top_k = self.streams, self.max_tracks, self.K, self.dim, self.top_k
        _policy_cfg(cfg, policy)
        self.wide = (self.max_tracks > 64 or self.K > 16) if wide is None else bool(wide)
        self.embed_budget = None if embed_budget is None else int(embed_budget)
        self._h = native.c_vp(0)
        flags = native.TRACKER_WIDE if self.wide else 0
        with torch.cuda.device(self.device):
            if self.embed_budget is None:
                native.check(native.lib().mtgv_tracker_create_ex(C.byref(cfg), flags, C.byref(self._h)))
            else:
                native.check(native.lib().mtgv_tracker_create_budget(C.byref(cfg), flags, self.embed_budget, C.byref(self._h)))
        self._frames = 0
        self._due_idx = self._n_due = None
        self.n_deferred = None  # budget: (1,) int32 on the device, the candidates the last update left for later

    def reset(self, stream: int = -1) -> None:
        """forget the tracks of one stream, or of all (-1): ids start again at 1"""
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_tracker_reset(self._h, int(stream), native.stream()))
        self._frames = 0

    def update(self, quads: torch.Tensor, stream_of_frame: Sequence[int], now, n_det: Optional[torch.Tensor] = None,
               state: Optional[torch.Tensor] = None):
        """quads (F, K, 4, 2) float32 on the device, frame f from stream stream_of_frame[f] at now[f] seconds (or one
        clock for all); slot k of frame f is a detection iff k < n_det[f] (when given) and state[f, k] > 0 (when given).
        -> (track_ids (F, K) int32, 0 = no initialised track; due_idx (F * K,) int32, the flat slots whose track is due in
        ascending order, -1 behind them; n_due (1,) int32), all on the device.  With an embed budget due_idx / n_due are the
        selected slots (n_due <= embed_budget) and `self.n_deferred` holds the count of the candidates left for later."""
        sof = check_streams(stream_of_frame, self.streams)
        F = sof.size
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(now, dtype=np.float64), (F,)))
        assert n_det is not None or state is not None, "one of n_det and state must be given"
        assert quads.is_cuda and quads.dtype == torch.float32 and quads.numel() == F * self.K * 8, f"{tuple(quads.shape)} {quads.dtype}"
        assert n_det is None or (n_det.is_cuda and n_det.dtype == torch.int32 and n_det.numel() == F)
        assert state is None or (state.is_cuda and state.dtype == torch.int32 and state.numel() == F * self.K)
        dev = quads.device
        track_ids = torch.empty((F, self.K), dtype=torch.int32, device=dev)
        due_idx = torch.empty((F * self.K,), dtype=torch.int32, device=dev)
        n_due = torch.empty((1,), dtype=torch.int32, device=dev)
        args = [self._h, native.ptr(quads.contiguous()), native.ptr(None if n_det is None else n_det.contiguous()),
                native.ptr(None if state is None else state.contiguous()), F, sof.ctypes.data_as(native.c_vp), t.ctypes.data_as(native.c_vp),
                native.ptr(track_ids), native.ptr(due_idx), native.ptr(n_due)]
        with torch.cuda.device(dev):
            if self.embed_budget is None:
                native.check(native.lib().mtgv_tracker_update(*args, native.stream()))
            else:
                n_deferred = torch.empty((1,), dtype=torch.int32, device=dev)
                native.check(native.lib().mtgv_tracker_update_budget(*args, native.ptr(n_deferred), native.stream()))
                self.n_deferred = n_deferred
        self._frames, self._due_idx, self._n_due = F, due_idx, n_due  # commit / store read them on the device
        return track_ids, due_idx, n_due

    def gather(self, src: torch.Tensor, out: Optional[torch.Tensor] = None, pad: bool = False) -> torch.Tensor:
        """src (F * K, ...) uint8 -> the rows of the due slots packed in front ((F * K, ...); rows behind n_due are not
        written; `out`: a buffer of src's shape to pack into).  A library kernel that reads n_due on the device.
        pad=True (needs an embed budget E): -> (E, ...), every row written, zeros behind n_due (`out`: a buffer of that shape)."""
        assert self._frames > 0, "gather without an update"
        n = self._frames * self.K
        assert src.is_cuda and src.dtype == torch.uint8 and src.shape[0] == n, f"{tuple(src.shape)} {src.dtype}"
        assert not pad or self.embed_budget is not None, "gather(pad=True) needs a tracker with an embed_budget"
        src = src.contiguous()
        shape = (self.embed_budget, *src.shape[1:]) if pad else src.shape
        dst = torch.empty(shape, dtype=torch.uint8, device=src.device) if out is None else out
        assert dst.is_cuda and dst.dtype == torch.uint8 and tuple(dst.shape) == tuple(shape) and dst.is_contiguous()
        fn = native.lib().mtgv_tracker_gather_u8_pad if pad else native.lib().mtgv_tracker_gather_u8
        with torch.cuda.device(src.device):
            native.check(fn(native.ptr(src), n, src[0].numel(), native.ptr(self._due_idx), native.ptr(self._n_due), shape[0], native.ptr(dst),
                            native.stream()))
        return dst

    def commit(self, z: torch.Tensor) -> torch.Tensor:
        """z (rows, dim): embeddings of the due slots in due_idx order -> the tracks' averaged embeddings (rows, dim), the
        match queries (avg = w z + (1 - w) avg in float32; the first time avg = z, then the same formula).  With an embed
        budget every row of the result is written: zeros behind n_due."""
        assert self._frames > 0, "commit without an update"
        assert z.is_cuda and z.dtype == torch.float32 and z.ndim == 2 and z.shape[1] == self.dim and 1 <= z.shape[0], f"{tuple(z.shape)} {z.dtype}"
        z = z.contiguous()
        q = torch.empty_like(z)
        with torch.cuda.device(z.device):
            native.check(native.lib().mtgv_tracker_commit(self._h, native.ptr(z), native.ptr(q), z.shape[0], native.stream()))
        return q

    def store(self, ids: Optional[torch.Tensor] = None, scores: Optional[torch.Tensor] = None):
        """ids / scores (rows, top_k): the matches of commit's queries (None: nothing was due).  They are kept on the due
        tracks -> (ids (F, K, top_k) int64, scores float32): every slot's track's kept matches, -1 / -inf without a track."""
        assert self._frames > 0, "store without an update"
        rows = 0 if ids is None else ids.shape[0]
        if rows:
            assert ids.is_cuda and ids.dtype == torch.int64 and tuple(ids.shape) == (rows, self.top_k), f"{tuple(ids.shape)} {ids.dtype}"
            assert scores.is_cuda and scores.dtype == torch.float32 and tuple(scores.shape) == (rows, self.top_k)
            ids, scores = ids.contiguous(), scores.contiguous()
        dev = self._due_idx.device
        out_ids = torch.empty((self._frames, self.K, self.top_k), dtype=torch.int64, device=dev)
        out_scores = torch.empty((self._frames, self.K, self.top_k), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            native.check(native.lib().mtgv_tracker_store(self._h, native.ptr(ids if rows else None), native.ptr(scores if rows else None), rows,
                                                         native.ptr(out_ids), native.ptr(out_scores), native.stream()))
        return out_ids, out_scores

    def state(self, stream: int) -> dict:
        """one stream's slots on the host (synchronises; the test surface): per slot `live`, `hit_counter`,
        `is_initializing`, `id`, `birth`, `has_z`, `pos` / `vel` / `pp` / `pv` / `vv` (T, 8) float64, `last_update_time`,
        `avg_z` (T, dim), `match_ids` / `match_scores` (T, top_k); per stream `next_id`, `next_birth`, `overflow`"""
        T = self.max_tracks
        kal = np.empty((40, T), np.float64)
        ints = np.empty((6, T), np.int32)
        last = np.empty((T,), np.float64)
        avg = np.empty((T, self.dim), np.float32)
        mi = np.empty((T, self.top_k), np.int64)
        ms = np.empty((T, self.top_k), np.float32)
        ctr = np.empty((4,), np.int32)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_tracker_get_state(self._h, int(stream), *(a.ctypes.data_as(native.c_vp) for a in (kal, ints, last, avg, mi, ms, ctr)),
                                                             native.stream()))
        k = kal.reshape(5, 8, T).transpose(0, 2, 1)
        out = {n: ints[i].copy() for i, n in enumerate(("live", "hit_counter", "is_initializing", "id", "birth", "has_z"))}
        out.update({n: np.ascontiguousarray(k[i]) for i, n in enumerate(("pos", "vel", "pp", "pv", "vv"))})
        out.update(last_update_time=last, avg_z=avg, match_ids=mi, match_scores=ms, next_id=int(ctr[0]), next_birth=int(ctr[1]), overflow=int(ctr[2]))
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                native.lib().mtgv_tracker_destroy(self._h)
                self._h = native.c_vp(0)
        except Exception:
            pass


class TrackedPipeline:
    """detect -> crop -> track -> embed the due tracks -> match -> per-slot stable matches, for `streams` cameras.

    Wraps a `Pipeline` (its detector, crop stage, encoder and matcher; every `quad_source`) and a `DeviceTracker`.  Runs on
    the current stream.  Without an embed budget a step reads n_due back, and the overlapped schedule of `Pipeline.run_many`
    is not offered: that read would stall the stream that holds it.  With `embed_budget=E` the device picks at most E due
    tracks per step, the embed and match stages run on exactly E rows, nothing is read back and `run_many` enqueues steps
    ahead on the pipeline's three streams ("Embed budget")."""

    def __init__(self, pipeline, streams: int, top_k: int = 3, max_tracks: int = 64, match_opts: Optional[dict] = None,
                 wide: Optional[bool] = None, embed_budget: Optional[int] = None, **policy):
        """match_opts: keyword arguments for `Matcher.match` (`filter`, `distinct`, `threshold`): {"distinct": True} makes a
        track's top_k matches top_k different cards (the bank's rows carry groups).  None: the plain match.
        wide: as for `DeviceTracker` (None: by size, so 24 cards per frame or 128 tracks just work).
        embed_budget: None (a step embeds every due track and reads their number back), or E <= the encoder's max_batch: a
        step embeds at most E tracks, the longest-waiting first; the rest stay due (`DeviceTracker`)."""
        # (each rank has its own number of due tracks; the sharded exchange needs equal query counts on every rank)
        assert not getattr(pipeline.matcher, "issues_collectives", False), "TrackedPipeline does not run on a sharded bank"
        self.pipeline = pipeline
        self.top_k = int(top_k)
        self.match_opts = dict(match_opts) if match_opts else None
        self.embed_budget = None if embed_budget is None else int(embed_budget)
        assert self.embed_budget is None or 1 <= self.embed_budget <= pipeline.encoder.max_batch, \
            f"embed_budget {embed_budget} outside 1..{pipeline.encoder.max_batch} (the encoder's max_batch)"
        self.tracker = DeviceTracker(streams, pipeline.K, pipeline.encoder.cfg.z_size, self.top_k, max_tracks, pipeline.detector.device, wide=wide,
                                     embed_budget=self.embed_budget, **policy)
        # the embeddings committed by the last step: (n_due, dim), None when nothing was due; with an embed budget always
        # (embed_budget, dim), the rows behind n_due being the embedding of an all-zero crop
        self.last_z = None

    def run(self, frames_u8: torch.Tensor, stream_of_frame: Sequence[int], now, flip_rgb: bool = True) -> dict:
        """frames (F, in_h, in_w, 3) uint8 on the GPU, frame f from camera stream_of_frame[f] (distinct) at now[f] seconds
        (or one clock for all) -> dict: track_ids (F, K) int32 (0: no initialised track in the slot), ids / scores
        (F, K, top_k): each slot's track's kept matches (-1 / -inf without a track), n_due (int), due_idx (F * K,) int32,
        n_det, boxes, crops, det, quads (F, K, 4, 2) (+ card_state, thumbs, thumb_offsets where Pipeline.run has them).

        frames_u8 may be a `mtgv.pipeline.SourceFrames`: the cards are cropped from the camera's frames and the tracker is
        updated with the quads in camera pixels, the unit of the reference's norfair thresholds (server.py:100-106); the
        returned quads (and quads_src) are those.

        One synchronisation per step: the 4-byte read of n_due, which the encoder and the matcher need on the host as
        their batch size.  All crops (and thumbnails) are produced as in Pipeline.run; only the due ones are embedded.

        With an embed budget E there is no synchronisation: the encoder and the matcher always run on E rows (crop rows
        behind n_due are zeros, their queries zeros, their matches kept by nobody), n_due is a (1,) int32 device tensor
        and the dict gains n_deferred (1,) int32, the due tracks that the budget left for a later step."""
        p, trk = self.pipeline, self.tracker
        sof = check_streams(stream_of_frame, trk.streams)
        det, cropped, src, F = self._detect_crop(frames_u8, sof, flip_rgb)
        cropped = p._thumbnails(cropped)
        if self.embed_budget is not None:
            return self._finish(det, cropped, src, F, *self._match_store(*self._track_embed(det, cropped, src, sof, now)))
        K = p.K
        quads = cropped.quads if src is None else cropped.quads_src
        if p.quad_source == "obb":
            track_ids, due_idx, n_due_dev = trk.update(quads, sof, now, state=cropped.card_state)
        else:
            track_ids, due_idx, n_due_dev = trk.update(quads, sof, now, n_det=det["n_det"] if cropped.n_sel is None else cropped.n_sel)
        n_due = int(n_due_dev.item())  # the step's only synchronisation
        self.last_z = None
        if n_due > 0:
            z = p.encoder.encode(trk.gather(cropped.crops)[:n_due])
            q = trk.commit(z)
            hits = p.matcher.match(q, self.top_k) if self.match_opts is None else p.matcher.match(q, self.top_k, **self.match_opts)
            ids, scores = trk.store(*hits)
            self.last_z = z
        else:
            ids, scores = trk.store()
        out = {"track_ids": track_ids, "ids": ids, "scores": scores, "n_due": n_due, "due_idx": due_idx, "n_det": det["n_det"],
               "boxes": cropped.boxes, "crops": cropped.crops, "det": det}
        out.update(cropped.extras(det, F, K))
        out["quads"] = quads.view(F, K, 4, 2)  # every quad_source's, and what the tracker saw: camera pixels with sources
        return out

    # ---- a step in the pieces that run_many puts on different streams; run with a budget is the four in a row

    def _detect(self, frames_u8, sof, flip_rgb):
        """-> (det, the frame tensor, SourceFrames or None)"""
        src = frames_u8 if isinstance(frames_u8, SourceFrames) else None
        if src is not None:
            frames_u8 = src.frames
        assert sof.size == frames_u8.shape[0], f"{sof.size} streams named for {frames_u8.shape[0]} frames"
        return self.pipeline.detector.forward(frames_u8, flip_rgb, mask_rows=self.pipeline.K), frames_u8, src

    def _detect_crop(self, frames_u8, sof, flip_rgb):
        """-> (det, Cropped without thumbnails, SourceFrames or None, the number of frames)"""
        if isinstance(frames_u8, TiledFrames):  # its cards are camera pixels, like a SourceFrames': the tracker sees quads_src
            assert sof.size == frames_u8.n_frames, f"{sof.size} streams named for {frames_u8.n_frames} frames"
            det, cropped = self.pipeline.detect_crop_tiled(frames_u8, flip_rgb)
            return det, cropped, frames_u8, frames_u8.n_frames
        det, frames_u8, src = self._detect(frames_u8, sof, flip_rgb)
        return det, self.pipeline.crop(frames_u8, det, src=src), src, frames_u8.shape[0]

    def _track_embed(self, det, cropped, src, sof, now):
        """budget: update + selection, gather, encode, commit -> (track_ids, due_idx, n_due, n_deferred, z, q)"""
        p, trk = self.pipeline, self.tracker
        quads = cropped.quads if src is None else cropped.quads_src
        if p.quad_source == "obb":
            track_ids, due_idx, n_due = trk.update(quads, sof, now, state=cropped.card_state)
        else:
            track_ids, due_idx, n_due = trk.update(quads, sof, now, n_det=det["n_det"] if cropped.n_sel is None else cropped.n_sel)
        z = p.encoder.encode(trk.gather(cropped.crops, pad=True))
        return track_ids, due_idx, n_due, trk.n_deferred, z, trk.commit(z)

    def _match_store(self, track_ids, due_idx, n_due, n_deferred, z, q):
        p = self.pipeline
        hits = p.matcher.match(q, self.top_k) if self.match_opts is None else p.matcher.match(q, self.top_k, **self.match_opts)
        ids, scores = self.tracker.store(*hits)
        return track_ids, due_idx, n_due, n_deferred, z, ids, scores

    def _finish(self, det, cropped, src, F, track_ids, due_idx, n_due, n_deferred, z, ids, scores):
        K = self.pipeline.K
        self.last_z = z
        out = {"track_ids": track_ids, "ids": ids, "scores": scores, "n_due": n_due, "n_deferred": n_deferred, "due_idx": due_idx,
               "n_det": det["n_det"], "boxes": cropped.boxes, "crops": cropped.crops, "det": det}
        out.update(cropped.extras(det, F, K))
        out["quads"] = (cropped.quads if src is None else cropped.quads_src).view(F, K, 4, 2)
        return out

    def run_many(self, steps, flip_rgb: bool = True) -> list:
        """steps: [(frames, stream_of_frame, now), ...], each as for `run` -> the list of `run`'s dicts, bit for bit.
        Needs an embed budget: without one every step reads n_due back and nothing can be enqueued ahead.

        Opt-in like `Pipeline.run_many` (MTGV_OVERLAP=on; otherwise the steps run one after the other on the current
        stream), on the pipeline's three streams with their priorities:
          detect stream   detect + crop (+ thumbnails) of step i+1
          embed stream    update + selection, gather, encode, commit of step i
          match stream    match, store of step i
        The tracker's state has one writer at a time, in step order: update + selection of step i+1 wait for an event
        recorded behind the store of step i, because commit and store write avg_z / has_z / the kept matches into slots
        that the update may recycle.  So only detect + crop of the next step overlap the embed and match of this one.
        MTGV_CROP_STAGE=enc moves the crop stage (and the thumbnails) in front of the update on the embed stream, as it
        does in `Pipeline.run_many`; then only the detector overlaps."""
        assert self.embed_budget is not None, "TrackedPipeline.run_many needs an embed_budget: without one every step reads n_due back"
        steps = list(_no_tiles(steps, "TrackedPipeline.run_many"))
        p = self.pipeline
        if not p.overlap_enabled():
            return [self.run(frames, sof, now, flip_rgb) for frames, sof, now in steps]
        crop_on_det, s_match, cur = p._overlap_streams()
        s_match = p._s_enc if s_match is None else s_match  # (MTGV_MATCH_STREAM=0: behind the encoder)
        with p._det_fork_off():
            outs, pending, stored = [], None, None
            for item in steps + [None]:
                nxt = None
                if item is not None:
                    frames, sof, now = item
                    sof = check_streams(sof, self.tracker.streams)
                    with torch.cuda.stream(p._s_det):
                        det, frames, src = self._detect(frames, sof, flip_rgb)
                        cropped = p.crop(frames, det, src=src) if crop_on_det else None
                        ev = torch.cuda.Event()
                        ev.record(p._s_det)
                        if cropped is not None:  # behind the event: this step's embed does not wait for its thumbnails
                            cropped = p._thumbnails(cropped)
                    nxt = (det, cropped, frames, src, sof, now, ev)
                if pending is not None:
                    det, cropped, frames, src, sof, now, ev = pending
                    F = frames.shape[0]
                    with torch.cuda.stream(p._s_enc):
                        p._s_enc.wait_event(ev)
                        for t in list(det.values()) + list(vars(cropped).values() if cropped is not None else ()):
                            if t is not None:
                                t.record_stream(p._s_enc)
                        if cropped is None:  # MTGV_CROP_STAGE=enc
                            cropped = p._thumbnails(p.crop(frames, det, src=src))
                        if stored is not None:
                            p._s_enc.wait_event(stored)  # the tracker's state: one writer at a time, in step order
                        emb = self._track_embed(det, cropped, src, sof, now)
                        committed = torch.cuda.Event()
                        committed.record(p._s_enc)
                    with torch.cuda.stream(s_match):
                        s_match.wait_event(committed)
                        for t in emb:
                            t.record_stream(s_match)
                        res = self._match_store(*emb)
                        stored = torch.cuda.Event()
                        stored.record(s_match)
                    outs.append(self._finish(det, cropped, src, F, *res))
                pending = nxt
        for s in (p._s_det, p._s_enc, s_match):
            cur.wait_stream(s)
        for o in outs:
            for k in ("track_ids", "ids", "scores", "n_due", "n_deferred", "due_idx", "crops", "boxes", "quads", "thumbs", "thumb_offsets", "quads_src"):
                if o.get(k) is not None:
                    o[k].record_stream(cur)
        if outs:
            self.last_z.record_stream(cur)
        return outs
