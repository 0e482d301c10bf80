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
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import native
from .pipeline import SourceFrames

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
    max_tracks > 64 or cards_per_frame > 16; True forces it at any size; False is the narrow handle, refusals included."""

    def __init__(self, streams: int, cards_per_frame: int, dim: int, top_k: int = 3, max_tracks: int = 64, device=None, wide: Optional[bool] = None,
                 **policy):
        native.require_gpu()
        self.streams, self.K, self.dim, self.top_k, self.max_tracks = int(streams), int(cards_per_frame), int(dim), int(top_k), int(max_tracks)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        cfg = native.TrackerCfg()
        cfg.streams, cfg.max_tracks, cfg.cards_per_frame, cfg.dim, cfg.top_k = self.streams, self.max_tracks, self.K, self.dim, self.top_k
        _policy_cfg(cfg, policy)
        self.wide = (self.max_tracks > 64 or self.K > 16) if wide is None else bool(wide)
        self._h = native.c_vp(0)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_tracker_create_ex(C.byref(cfg), native.TRACKER_WIDE if self.wide else 0, C.byref(self._h)))
        self._frames = 0
        self._due_idx = self._n_due = None

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
        ascending order, -1 behind them; n_due (1,) int32), all on the device."""
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
        with torch.cuda.device(dev):
            native.check(native.lib().mtgv_tracker_update(
                self._h, native.ptr(quads.contiguous()), native.ptr(None if n_det is None else n_det.contiguous()),
                native.ptr(None if state is None else state.contiguous()), F, sof.ctypes.data_as(native.c_vp), t.ctypes.data_as(native.c_vp),
                native.ptr(track_ids), native.ptr(due_idx), native.ptr(n_due), native.stream()))
        self._frames, self._due_idx, self._n_due = F, due_idx, n_due  # commit / store read them on the device
        return track_ids, due_idx, n_due

    def gather(self, src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """src (F * K, ...) uint8 -> the rows of the due slots packed in front ((F * K, ...); rows behind n_due are not
        written; `out`: a buffer of src's shape to pack into).  A library kernel that reads n_due on the device."""
        assert self._frames > 0, "gather without an update"
        n = self._frames * self.K
        assert src.is_cuda and src.dtype == torch.uint8 and src.shape[0] == n, f"{tuple(src.shape)} {src.dtype}"
        src = src.contiguous()
        dst = torch.empty_like(src) if out is None else out
        assert dst.is_cuda and dst.dtype == torch.uint8 and dst.shape == src.shape and dst.is_contiguous()
        with torch.cuda.device(src.device):
            native.check(native.lib().mtgv_tracker_gather_u8(native.ptr(src), n, src[0].numel(), native.ptr(self._due_idx), native.ptr(self._n_due),
                                                             n, native.ptr(dst), native.stream()))
        return dst

    def commit(self, z: torch.Tensor) -> torch.Tensor:
        """z (rows, dim): embeddings of the due slots in due_idx order -> the tracks' averaged embeddings (rows, dim), the
        match queries (avg = w z + (1 - w) avg in float32; the first time avg = z, then the same formula)"""
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
    the current stream.  The overlapped schedule of `Pipeline.run_many` is not offered: the read-back of n_due would stall
    the stream that holds it."""

    def __init__(self, pipeline, streams: int, top_k: int = 3, max_tracks: int = 64, match_opts: Optional[dict] = None,
                 wide: Optional[bool] = None, **policy):
        """match_opts: keyword arguments for `Matcher.match` (`filter`, `distinct`, `threshold`): {"distinct": True} makes a
        track's top_k matches top_k different cards (the bank's rows carry groups).  None: the plain match.
        wide: as for `DeviceTracker` (None: by size, so 24 cards per frame or 128 tracks just work)."""
        # (each rank has its own number of due tracks; the sharded exchange needs equal query counts on every rank)
        assert not getattr(pipeline.matcher, "issues_collectives", False), "TrackedPipeline does not run on a sharded bank"
        self.pipeline = pipeline
        self.top_k = int(top_k)
        self.match_opts = dict(match_opts) if match_opts else None
        self.tracker = DeviceTracker(streams, pipeline.K, pipeline.encoder.cfg.z_size, self.top_k, max_tracks, pipeline.detector.device, wide=wide,
                                     **policy)
        self.last_z = None  # the embeddings committed by the last step (n_due, dim), None when nothing was due

    def run(self, frames_u8: torch.Tensor, stream_of_frame: Sequence[int], now, flip_rgb: bool = True) -> dict:
        """frames (F, in_h, in_w, 3) uint8 on the GPU, frame f from camera stream_of_frame[f] (distinct) at now[f] seconds
        (or one clock for all) -> dict: track_ids (F, K) int32 (0: no initialised track in the slot), ids / scores
        (F, K, top_k): each slot's track's kept matches (-1 / -inf without a track), n_due (int), due_idx (F * K,) int32,
        n_det, boxes, crops, det, quads (F, K, 4, 2) (+ card_state, thumbs, thumb_offsets where Pipeline.run has them).

        frames_u8 may be a `mtgv.pipeline.SourceFrames`: the cards are cropped from the camera's frames and the tracker is
        updated with the quads in camera pixels, the unit of the reference's norfair thresholds (server.py:100-106); the
        returned quads (and quads_src) are those.

        One synchronisation per step: the 4-byte read of n_due, which the encoder and the matcher need on the host as
        their batch size.  All crops (and thumbnails) are produced as in Pipeline.run; only the due ones are embedded."""
        p, trk = self.pipeline, self.tracker
        sof = check_streams(stream_of_frame, trk.streams)
        src = frames_u8 if isinstance(frames_u8, SourceFrames) else None
        if src is not None:
            frames_u8 = src.frames
        F, K = frames_u8.shape[0], p.K
        assert sof.size == F, f"{sof.size} streams named for {F} frames"
        det = p.detector.forward(frames_u8, flip_rgb, mask_rows=K)
        cropped = p._thumbnails(p.crop(frames_u8, det, src=src))
        quads = cropped.quads if src is None else cropped.quads_src
        if p.quad_source == "obb":
            track_ids, due_idx, n_due_dev = trk.update(quads, sof, now, state=cropped.card_state)
        else:
            track_ids, due_idx, n_due_dev = trk.update(quads, sof, now, n_det=det["n_det"])
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
