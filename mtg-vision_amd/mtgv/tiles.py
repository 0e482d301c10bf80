"""Tiled detection: the detector runs on overlapping windows (tiles) of large source frames instead of one letterbox per frame.

A 3840 x 2160 frame letterboxed into 640 x 640 leaves a card some 25 pixels tall.  Here the frame is cut into windows at, or
near, native resolution (`tile_grid`, `TiledFrames`, csrc/resize.hip: mtgv_letterbox_tiles_u8), the detector runs on the
windows as if they were frames, and one kernel (csrc/tiles.hip: mtgv_tiles_merge) maps the detections back into camera
pixels, drops the cards a window cut, removes the duplicates of the overlap and hands the K best per frame to the crop
stage.  `Pipeline.run(TiledFrames)` is the caller.  The rule is this library's; `merge_tiles_host` states it in numpy - the
specification the kernel is tested against, bit for bit; nothing on the GPU path calls it.  An OBB detector's oriented
quads are merged by the rotated rule (csrc/tiles_obb.hip: mtgv_tiles_merge_obb; `merge_tiles_obb_host`, `quad_inter_host`):
the overlap is the exact area of intersection of two convex quads, and a kept card takes its orientation from an oriented
duplicate.  `Pipeline(..., quad_source="obb", tile_merge={"rule": "rotated"})` turns it on.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import native
from .detector import fit_geometry

MAX_CANDIDATES = 1024  # per frame: tiles of the frame x cards per tile (the merge kernel's workgroup)
MAX_CARDS = 64  # K


def tile_grid(h: int, w: int, window_hw, overlap: int, with_full: bool = False) -> np.ndarray:
    """The windows of an (h, w) frame: (T, 4) int32 rows (y0, x0, wh, ww) in frame pixels, raster order.  Per axis the
    stride is window - overlap, the count max(1, ceil((size - overlap) / stride)), the origin min(i * stride,
    max(0, size - window)) - the last window is flush with the frame's edge - and the extent min(window, size).
    with_full: the whole frame (0, 0, h, w) is appended, the view that still sees a card larger than the overlap."""
    wh, ww = int(window_hw[0]), int(window_hw[1])
    overlap = int(overlap)
    assert 0 <= overlap < min(wh, ww), f"overlap {overlap} outside [0, {min(wh, ww)}) (window {wh} x {ww})"
    assert h > 0 and w > 0, f"frame {h} x {w}"

    def axis(size, window):
        stride = window - overlap
        n = max(1, -(-(size - overlap) // stride))
        return [min(i * stride, max(0, size - window)) for i in range(n)], min(window, size)

    ys, eh = axis(int(h), wh)
    xs, ew = axis(int(w), ww)
    rows = [(y, x, eh, ew) for y in ys for x in xs]
    if with_full:
        rows.append((0, 0, int(h), int(w)))
    return np.array(rows, np.int32).reshape(len(rows), 4)


def _host_i64(a, shape) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.int64).reshape(shape)


@dataclass
class _Sources:
    """what crop.warp_quads_src reads of a batch of source frames"""

    buf: torch.Tensor
    offsets: torch.Tensor
    hw: torch.Tensor
    geo: torch.Tensor
    ratio: torch.Tensor


@dataclass
class TiledFrames:
    """A batch of camera frames and the windows the detector is to see of them, handed to `Pipeline.run` /
    `TrackedPipeline.run` in place of a frame tensor or a `SourceFrames`.

    buf, offsets, hw: the frames, as `SourceFrames` has them.  tiles (NT, 5) int32 = frame, y0, x0, wh, ww, frame-major;
    tile_start (F + 1,) int32: frame f owns tiles[tile_start[f]:tile_start[f + 1]]; geo (NT, 4) int32 = nh, nw, top, left and
    ratio (NT,) float64: `fit_geometry(wh, ww, in_h, in_w)` per tile; frames (NT, in_h, in_w, 3) uint8: the detector inputs.
    All on the device; tiles_h, tile_start_h, hw_h are host copies (the merge's caps are checked from them)."""

    buf: torch.Tensor
    offsets: torch.Tensor
    hw: torch.Tensor
    tiles: torch.Tensor
    tile_start: torch.Tensor
    geo: torch.Tensor
    ratio: torch.Tensor
    frames: torch.Tensor
    tiles_h: Optional[np.ndarray] = None
    tile_start_h: Optional[np.ndarray] = None
    hw_h: Optional[np.ndarray] = None
    _identity: Optional[_Sources] = None

    @property
    def n_frames(self) -> int:
        return int(self.hw.shape[0])

    @property
    def max_tiles_per_frame(self) -> int:
        ts = self.tile_start_h
        return int((ts[1:] - ts[:-1]).max()) if ts.size > 1 else 0

    def sources(self) -> _Sources:
        """the frames with an identity geometry (top = left = 0, ratio = 1): mtgv_warp_quads_src reads quads that are
        camera pixels already as they are"""
        if self._identity is None:
            F, dev = self.n_frames, self.buf.device
            self._identity = _Sources(self.buf, self.offsets, self.hw, torch.zeros((F, 4), dtype=torch.int32, device=dev),
                                      torch.ones((F,), dtype=torch.float64, device=dev))
        return self._identity

    @classmethod
    def from_ragged(cls, buf: torch.Tensor, offsets, hw, window_hw=None, overlap: Optional[int] = None, with_full: bool = False,
                    size: int = 640, input_hw=None, pad_value: int = 114):
        """frames of their own sizes in one buffer (as for `SourceFrames.from_ragged`) -> their `tile_grid` windows cut
        into (size, size) or input_hw detector inputs in one launch.  window_hw None: the input's own size, so a tile is an
        exact copy of its window; overlap None: a fifth of the window's smaller side (128 at 640)."""
        native.require_gpu()
        assert buf.is_cuda and buf.dtype == torch.uint8 and buf.ndim == 1 and buf.is_contiguous(), f"{tuple(buf.shape)} {buf.dtype}"
        hw_h = _host_i64(hw, (-1, 2))
        n = hw_h.shape[0]
        off_h = _host_i64(offsets, (n,))
        oh, ow = (int(size), int(size)) if input_hw is None else (int(input_hw[0]), int(input_hw[1]))
        win = (oh, ow) if window_hw is None else (int(window_hw[0]), int(window_hw[1]))
        overlap = min(win) // 5 if overlap is None else int(overlap)
        # the kernels trust these tables: every frame has pixels and lies inside the buffer
        assert n == 0 or ((hw_h > 0).all() and (off_h >= 0).all() and (off_h + hw_h[:, 0] * hw_h[:, 1] * 3 <= buf.numel()).all()), \
            f"frames (offsets {off_h.tolist()}, sizes {hw_h.tolist()}) outside a buffer of {buf.numel()} bytes"
        grids = [tile_grid(int(h), int(w), win, overlap, with_full) for h, w in hw_h]
        tiles = np.concatenate([np.concatenate([np.full((len(g), 1), f, np.int32), g], 1) for f, g in enumerate(grids)] or
                               [np.zeros((0, 5), np.int32)]).astype(np.int32)
        tile_start = np.concatenate([[0], np.cumsum([len(g) for g in grids])]).astype(np.int32)
        return cls.from_tiles(buf, off_h, hw_h, tiles, tile_start, (oh, ow), pad_value)

    @classmethod
    def from_tiles(cls, buf: torch.Tensor, offsets, hw, tiles, tile_start, input_hw, pad_value: int = 114):
        """the same from a caller's own windows: tiles (NT, 5) = frame, y0, x0, wh, ww inside their frames, frame-major,
        tile_start (F + 1,)"""
        native.require_gpu()
        hw_h = _host_i64(hw, (-1, 2))
        n = hw_h.shape[0]
        off_h = _host_i64(offsets, (n,))
        tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 5)
        tile_start = np.ascontiguousarray(tile_start, np.int32).reshape(n + 1)
        nt = tiles.shape[0]
        oh, ow = int(input_hw[0]), int(input_hw[1])
        assert nt <= 65535, f"{nt} tiles in one batch (at most 65535)"
        assert tile_start[0] == 0 and tile_start[-1] == nt and (np.diff(tile_start) >= 0).all(), f"tile_start {tile_start.tolist()} for {nt} tiles"
        assert (np.repeat(np.arange(n), np.diff(tile_start)) == tiles[:, 0]).all(), "tiles are not frame-major"
        fh, fw = hw_h[tiles[:, 0], 0], hw_h[tiles[:, 0], 1]
        assert ((tiles[:, 1:3] >= 0).all() and (tiles[:, 3:] > 0).all() and (tiles[:, 1] + tiles[:, 3] <= fh).all()
                and (tiles[:, 2] + tiles[:, 4] <= fw).all()), "a window lies outside its frame"
        g = [fit_geometry(int(t[3]), int(t[4]), oh, ow) for t in tiles]
        geo = np.array([t[1:] for t in g], np.int32).reshape(nt, 4)
        ratio = np.array([t[0] for t in g], np.float64)
        dev = buf.device
        frames = torch.empty((nt, oh, ow, 3), dtype=torch.uint8, device=dev)
        tf = cls(buf, torch.from_numpy(off_h).to(dev), torch.from_numpy(hw_h.astype(np.int32)).to(dev), torch.from_numpy(tiles).to(dev),
                 torch.from_numpy(tile_start).to(dev), torch.from_numpy(geo).to(dev), torch.from_numpy(ratio).to(dev), frames,
                 tiles, tile_start, hw_h.astype(np.int32))
        cut_tiles(buf, tf.offsets, tf.hw, tf.tiles, tf.geo, frames, pad_value)
        return tf

    @classmethod
    def from_frames(cls, frames: torch.Tensor, window_hw=None, overlap: Optional[int] = None, with_full: bool = False, size: int = 640,
                    input_hw=None, pad_value: int = 114):
        """(n, h, w, 3) uint8 same-sized frames on the device: the buffer is the tensor itself (no copy)"""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3 and frames.is_contiguous(), \
            f"{tuple(frames.shape)} {frames.dtype}"
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        return cls.from_ragged(frames.view(-1), np.arange(n, dtype=np.int64) * (h * w * 3), [(h, w)] * n, window_hw, overlap, with_full, size,
                               input_hw, pad_value)


def cut_tiles(buf: torch.Tensor, offsets: torch.Tensor, hw: torch.Tensor, tiles: torch.Tensor, geo: torch.Tensor, out: torch.Tensor,
              pad_value: int = 114) -> torch.Tensor:
    """mtgv_letterbox_tiles_u8: the windows `tiles` (NT, 5) int32 of the ragged frames (buf, offsets (F,) int64, hw (F, 2)
    int32), each letterboxed by its geo row (NT, 4) int32 into out[t] of (NT, in_h, in_w, 3) uint8; one launch.  All device
    tensors; the kernel does not trust the tables (include/mtgv.h)."""
    native.require_gpu()
    nt, nf = int(tiles.shape[0]), int(offsets.shape[0])
    assert buf.is_cuda and buf.dtype == torch.uint8 and out.is_cuda and out.dtype == torch.uint8 and out.ndim == 4 and out.shape[0] == nt and out.shape[3] == 3
    assert offsets.dtype == torch.int64 and hw.dtype == torch.int32 and tiles.dtype == torch.int32 and geo.dtype == torch.int32
    assert tuple(hw.shape) == (nf, 2) and tuple(tiles.shape) == (nt, 5) and tuple(geo.shape) == (nt, 4)
    with torch.cuda.device(buf.device):
        native.check(native.lib().mtgv_letterbox_tiles_u8(native.ptr(buf), native.ptr(offsets), native.ptr(hw), nf, native.ptr(tiles), native.ptr(geo), nt,
                                                          native.ptr(out), int(out.shape[1]), int(out.shape[2]), int(pad_value), native.stream()))
    return out


def merge_tiles(tf: TiledFrames, n_det: torch.Tensor, boxes: torch.Tensor, conf: torch.Tensor, quads: Optional[torch.Tensor], kt: int,
                pad_frac: torch.Tensor, k: int, edge: float = 2.0, ios: float = 0.5, max_tiles_per_frame: Optional[int] = None) -> dict:
    """mtgv_tiles_merge: the per-tile detector outputs (n_det (NT,), boxes (NT, max_det, 4), conf (NT, max_det)) and, unless
    None, the quads of the first kt detections per tile (NT * kt, 4, 2) -> the k cards of every frame in camera pixels: dict of
    sel_boxes_src (F * k, 4), quads_src (F * k, 4, 2), frame_idx, sel_conf, src_slot (F * k,) and n_sel (F,).  The caps are
    checked by the library from max_tiles_per_frame (default: the host copy of tf.tile_start) before the launch."""
    native.require_gpu()
    F, nt, md = tf.n_frames, int(tf.tiles.shape[0]), int(boxes.shape[1])
    dev = boxes.device
    assert n_det.dtype == torch.int32 and boxes.dtype == torch.float32 and conf.dtype == torch.float32 and pad_frac.dtype == torch.float32
    assert tuple(n_det.shape) == (nt,) and tuple(boxes.shape) == (nt, md, 4) and tuple(conf.shape) == (nt, md) and tuple(pad_frac.shape) == (k, 4)
    assert quads is None or (quads.dtype == torch.float32 and quads.numel() == nt * kt * 8), "quads: (NT * kt, 4, 2) float32"
    out = {
        "sel_boxes_src": torch.empty((F * k, 4), dtype=torch.float32, device=dev),
        "quads_src": torch.empty((F * k, 4, 2), dtype=torch.float32, device=dev),
        "frame_idx": torch.empty((F * k,), dtype=torch.int32, device=dev),
        "sel_conf": torch.empty((F * k,), dtype=torch.float32, device=dev),
        "src_slot": torch.empty((F * k,), dtype=torch.int32, device=dev),
        "n_sel": torch.empty((F,), dtype=torch.int32, device=dev),
    }
    mt = tf.max_tiles_per_frame if max_tiles_per_frame is None else int(max_tiles_per_frame)
    with torch.cuda.device(dev):
        native.check(native.lib().mtgv_tiles_merge(
            native.ptr(n_det), native.ptr(boxes.contiguous()), native.ptr(conf.contiguous()), native.ptr(None if quads is None else quads.contiguous()),
            nt, md, int(kt), native.ptr(tf.tiles), native.ptr(tf.geo), native.ptr(tf.ratio), native.ptr(tf.tile_start), native.ptr(tf.hw), F, mt,
            native.ptr(pad_frac), int(k), float(edge), float(ios), *(native.ptr(out[n]) for n in ("sel_boxes_src", "quads_src", "frame_idx", "sel_conf",
                                                                                                      "src_slot", "n_sel")), native.stream()))
    return out


MERGE_OBB_OUTPUTS = ("sel_boxes_src", "quads_src", "frame_idx", "sel_conf", "src_slot", "n_sel", "state", "oriented_by")


def merge_tiles_obb(tf: TiledFrames, n_det: torch.Tensor, conf: torch.Tensor, cls: torch.Tensor, quads: torch.Tensor, state: torch.Tensor, kt: int,
                    pad_frac: torch.Tensor, k: int, edge: float = 2.0, ios: float = 0.5, card_cls: int = 0,
                    max_tiles_per_frame: Optional[int] = None) -> dict:
    """mtgv_tiles_merge_obb: the per-tile outputs of an OBB detector (n_det (NT,), conf, cls (NT, max_det)) and of
    crop.obb_cards on them with k = kt (quads (NT * kt, 4, 2), state (NT * kt,)) -> the k cards of every frame in camera
    pixels: `merge_tiles`' dict plus state and oriented_by (F * k,) int32.  `merge_tiles_obb_host` is the rule."""
    native.require_gpu()
    F, nt, md = tf.n_frames, int(tf.tiles.shape[0]), int(conf.shape[1])
    dev = conf.device
    assert n_det.dtype == torch.int32 and conf.dtype == torch.float32 and cls.dtype == torch.int32 and pad_frac.dtype == torch.float32
    assert tuple(n_det.shape) == (nt,) and tuple(conf.shape) == (nt, md) and tuple(cls.shape) == (nt, md) and tuple(pad_frac.shape) == (k, 4)
    assert quads.dtype == torch.float32 and quads.numel() == nt * kt * 8, "quads: (NT * kt, 4, 2) float32"
    assert state.dtype == torch.int32 and state.numel() == nt * kt, "state: (NT * kt,) int32"
    out = {
        "sel_boxes_src": torch.empty((F * k, 4), dtype=torch.float32, device=dev),
        "quads_src": torch.empty((F * k, 4, 2), dtype=torch.float32, device=dev),
        "frame_idx": torch.empty((F * k,), dtype=torch.int32, device=dev),
        "sel_conf": torch.empty((F * k,), dtype=torch.float32, device=dev),
        "src_slot": torch.empty((F * k,), dtype=torch.int32, device=dev),
        "n_sel": torch.empty((F,), dtype=torch.int32, device=dev),
        "state": torch.empty((F * k,), dtype=torch.int32, device=dev),
        "oriented_by": torch.empty((F * k,), dtype=torch.int32, device=dev),
    }
    mt = tf.max_tiles_per_frame if max_tiles_per_frame is None else int(max_tiles_per_frame)
    with torch.cuda.device(dev):
        native.check(native.lib().mtgv_tiles_merge_obb(
            native.ptr(n_det), native.ptr(conf.contiguous()), native.ptr(cls.contiguous()), native.ptr(quads.contiguous()), native.ptr(state.contiguous()),
            nt, md, int(kt), native.ptr(tf.tiles), native.ptr(tf.geo), native.ptr(tf.ratio), native.ptr(tf.tile_start), native.ptr(tf.hw), F, mt,
            native.ptr(pad_frac), int(k), float(edge), float(ios), int(card_cls), *(native.ptr(out[n]) for n in MERGE_OBB_OUTPUTS), native.stream()))
    return out


def quad_inter(a: torch.Tensor, b: torch.Tensor):
    """mtgv_op_quad_inter: the rotated merge's pair function on m pairs of quads (m, 4, 2) float32 on the device ->
    (inter, area_a, area_b), (m,) float32 each (`quad_inter_host` is the rule)"""
    native.require_gpu()
    assert a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and tuple(a.shape[1:]) == (4, 2), \
        f"{tuple(a.shape)} {tuple(b.shape)}"
    m = int(a.shape[0])
    inter, area_a, area_b = (torch.empty((m,), dtype=torch.float32, device=a.device) for _ in range(3))
    with torch.cuda.device(a.device):
        native.check(native.lib().mtgv_op_quad_inter(native.ptr(a.contiguous()), native.ptr(b.contiguous()), m, native.ptr(inter), native.ptr(area_a),
                                                     native.ptr(area_b), native.stream()))
    return inter, area_a, area_b


def _to_src(v, pad, ratio, origin, extent):
    """float32 coordinates of a tile's detector input -> camera pixels: float64 (v - pad) / ratio + origin, clipped to
    [origin, origin + extent] by comparisons (a NaN stays one), rounded to float32"""
    s = (np.asarray(v, np.float32).astype(np.float64) - np.float64(pad)) / np.float64(ratio) + np.float64(origin)
    lo, hi = np.float64(origin), np.float64(origin) + np.float64(extent)
    return np.where(s < lo, lo, np.where(s > hi, hi, s)).astype(np.float32)


def _order_key(conf, flat):
    """conf (float32) as order-preserving bits above the complement of the flat candidate index: descending keys are conf
    descending, then flat index ascending"""
    u = np.asarray(conf, np.float32).view(np.uint32).astype(np.uint64)
    ordb = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (ordb << np.uint64(32)) | (~np.asarray(flat, np.uint64) & np.uint64(0xFFFFFFFF))


def merge_tiles_host(n_det, boxes, conf, quads, tiles, geo, ratio, tile_start, hw, pad_frac, kt: int, k: int, edge: float = 2.0,
                     ios: float = 0.5, max_tiles_per_frame: Optional[int] = None) -> dict:
    """The merge rule on the host (numpy arrays in, numpy arrays out): what mtgv_tiles_merge computes, bit for bit.

    1. candidates: detection j < min(n_det[t], kt) of tile t.
    2. mapping: float64 x = (x_det - left) / ratio + x0 clipped to [x0, x0 + ww], y likewise, rounded to float32; the quads'
       corners likewise (quads None: the mapped box's corners TL, TR, BR, BL).
    3. cut rule: a window side is an inner side where it is no side of the frame (x0 > 0, x0 + ww < w, y0 > 0, y0 + wh < h); a
       candidate with bx0 < x0 + edge, bx1 > x0 + ww - edge (or the same in y) at an inner side is dropped (float32).
    4. order: conf descending, tile ascending, j ascending.
    5. greedy: a candidate is dropped if inter > ios * min(area_a, area_b) against an earlier kept one; inter =
       max(0, min(x1) - max(x0)) * max(0, min(y1) - max(y0)), float32 throughout, no division, strict.
    6. the first k kept fill slots 0 .. n_sel - 1; slot >= n_sel is pad_frac[slot] * (w, h, w, h) with its corners as quad,
       conf 0, src_slot -1.
    A frame whose tile_start range is longer than max_tiles_per_frame (default: the longest range), negative or outside
    [0, NT] has no candidates.  The caps (k <= 64, at most 1024 candidates per frame) are asserted."""
    n_det = np.asarray(n_det, np.int32)
    boxes, conf = np.asarray(boxes, np.float32), np.asarray(conf, np.float32)
    tiles, geo, ratio = np.asarray(tiles, np.int32).reshape(-1, 5), np.asarray(geo, np.int32).reshape(-1, 4), np.asarray(ratio, np.float64)
    tile_start, hw, pad_frac = np.asarray(tile_start, np.int64), np.asarray(hw, np.int32).reshape(-1, 2), np.asarray(pad_frac, np.float32)
    NT, F, kt, k = tiles.shape[0], hw.shape[0], int(kt), int(k)
    if quads is not None:
        quads = np.asarray(quads, np.float32).reshape(NT * kt, 4, 2)
    mt = int(np.diff(tile_start).max()) if max_tiles_per_frame is None and F else int(max_tiles_per_frame or 0)
    assert 1 <= k <= MAX_CARDS and 1 <= kt <= boxes.shape[1] and mt * kt <= MAX_CANDIDATES, f"k={k} kt={kt} tiles per frame {mt}"
    e32, thr = np.float32(edge), np.float32(ios)
    out = {"sel_boxes_src": np.zeros((F * k, 4), np.float32), "quads_src": np.zeros((F * k, 4, 2), np.float32),
           "frame_idx": np.repeat(np.arange(F, dtype=np.int32), k), "sel_conf": np.zeros((F * k,), np.float32),
           "src_slot": np.full((F * k,), -1, np.int32), "n_sel": np.zeros((F,), np.int32)}

    def corners(b):
        return np.array([[b[0], b[1]], [b[2], b[1]], [b[2], b[3]], [b[0], b[3]]], np.float32)

    for f in range(F):
        h, w = int(hw[f, 0]), int(hw[f, 1])
        ts, te = int(tile_start[f]), int(tile_start[f + 1])
        if ts < 0 or te < ts or te > NT or te - ts > mt:
            ts = te = 0
        cb, cc, cslot, cflat = [], [], [], []
        for tl, t in enumerate(range(ts, te)):
            _, y0, x0, wh, ww = (int(v) for v in tiles[t])
            nd = min(int(n_det[t]), kt)
            if nd <= 0:
                continue
            top, left, r = geo[t, 2], geo[t, 3], ratio[t]
            b = boxes[t, :nd]
            m = np.stack([_to_src(b[:, 0], left, r, x0, ww), _to_src(b[:, 1], top, r, y0, wh), _to_src(b[:, 2], left, r, x0, ww),
                          _to_src(b[:, 3], top, r, y0, wh)], 1)
            cut = np.zeros((nd,), bool)
            if x0 > 0:
                cut |= m[:, 0] < np.float32(x0) + e32
            if x0 + ww < w:
                cut |= m[:, 2] > np.float32(x0 + ww) - e32
            if y0 > 0:
                cut |= m[:, 1] < np.float32(y0) + e32
            if y0 + wh < h:
                cut |= m[:, 3] > np.float32(y0 + wh) - e32
            j = np.arange(nd)[~cut]
            cb.append(m[~cut]), cc.append(conf[t, j]), cslot.append(t * kt + j), cflat.append(tl * kt + j)
        n_sel = 0
        if cb and sum(len(x) for x in cb):
            cb, cc, cslot, cflat = np.concatenate(cb), np.concatenate(cc), np.concatenate(cslot), np.concatenate(cflat)
            order = np.argsort(_order_key(cc, cflat))[::-1]  # the keys are unique
            cb, cc, cslot = cb[order], cc[order], cslot[order]
            area = (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])
            alive = np.ones((len(cb),), bool)
            zero = np.float32(0)
            while n_sel < k and alive.any():
                p = int(np.argmax(alive))
                a = cb[p]
                iw = np.where(a[2] < cb[:, 2], a[2], cb[:, 2]) - np.where(a[0] > cb[:, 0], a[0], cb[:, 0])
                ih = np.where(a[3] < cb[:, 3], a[3], cb[:, 3]) - np.where(a[1] > cb[:, 1], a[1], cb[:, 1])
                inter = np.where(zero > iw, zero, iw) * np.where(zero > ih, zero, ih)
                alive &= ~(inter > thr * np.where(area[p] < area, area[p], area))
                alive[p] = False
                o = f * k + n_sel
                out["sel_boxes_src"][o], out["sel_conf"][o], out["src_slot"][o] = a, cc[p], cslot[p]
                if quads is None:
                    out["quads_src"][o] = corners(a)
                else:
                    t = int(cslot[p]) // kt
                    _, y0, x0, wh, ww = (int(v) for v in tiles[t])
                    q = quads[int(cslot[p])]
                    out["quads_src"][o, :, 0] = _to_src(q[:, 0], geo[t, 3], ratio[t], x0, ww)
                    out["quads_src"][o, :, 1] = _to_src(q[:, 1], geo[t, 2], ratio[t], y0, wh)
                n_sel += 1
        out["n_sel"][f] = n_sel
        for s in range(n_sel, k):
            pb = pad_frac[s] * np.array([w, h, w, h], np.float32)
            out["sel_boxes_src"][f * k + s], out["quads_src"][f * k + s] = pb, corners(pb)
    return out


# ---------------------------------------------------------------------------
# the rotated rule: oriented quads of an OBB detector (csrc/tiles_obb.hip: mtgv_tiles_merge_obb)
# ---------------------------------------------------------------------------
_F0, _F1, _HALF = np.float32(0), np.float32(1), np.float32(0.5)


def _min4(v):
    """min of (n, 4) float32 by comparisons, (v0 ? v1) ? (v2 ? v3): a NaN behaves as under np.where"""
    a, b = np.where(v[:, 0] < v[:, 1], v[:, 0], v[:, 1]), np.where(v[:, 2] < v[:, 3], v[:, 2], v[:, 3])
    return np.where(a < b, a, b)


def _max4(v):
    a, b = np.where(v[:, 0] > v[:, 1], v[:, 0], v[:, 1]), np.where(v[:, 2] > v[:, 3], v[:, 2], v[:, 3])
    return np.where(a > b, a, b)


def quad_bounds(q) -> np.ndarray:
    """(n, 4, 2) float32 quads -> (n, 4) bounds x0, y0, x1, y1"""
    q = np.asarray(q, np.float32).reshape(-1, 4, 2)
    return np.stack([_min4(q[:, :, 0]), _min4(q[:, :, 1]), _max4(q[:, :, 0]), _max4(q[:, :, 1])], 1)


def _shoelace(x, y):
    """the doubled signed area: s = 0, then s = s + (x_i * y_i+1 - x_i+1 * y_i) for i = 0 .. 3"""
    s = np.zeros(x.shape[0], np.float32)
    for i in range(4):
        j = (i + 1) & 3
        s = s + (x[:, i] * y[:, j] - x[:, j] * y[:, i])
    return s


def _edge_sum(px, py, qx, qy, sq, same, closed: bool):
    """sum over P's four edges of cross(p', q'), p' -> q' being the part of the edge inside Q's four half-planes (sq: the sign
    of Q's winding).  closed: a point on a boundary line is inside, and an edge that lies along an edge of Q counts iff the
    two run the same way (same: the product of the two windings' signs); open: neither."""
    n = px.shape[0]
    ex = [qx[:, (k + 1) & 3] - qx[:, k] for k in range(4)]
    ey = [qy[:, (k + 1) & 3] - qy[:, k] for k in range(4)]
    d = [[sq * (ex[k] * (py[:, i] - qy[:, k]) - ey[k] * (px[:, i] - qx[:, k])) for i in range(4)] for k in range(4)]
    tot = np.zeros(n, np.float32)
    for e in range(4):
        e1 = (e + 1) & 3
        dx, dy = px[:, e1] - px[:, e], py[:, e1] - py[:, e]
        t0, t1, ok = np.zeros(n, np.float32), np.ones(n, np.float32), np.ones(n, bool)
        for k in range(4):
            dp, dq = d[k][e], d[k][e1]
            line = ~((ex[k] == _F0) & (ey[k] == _F0))  # a zero-length edge of Q bounds nothing
            along = (dp == _F0) & (dq == _F0)
            if closed:
                inp, inq = dp >= _F0, dq >= _F0
                along_out = along & ~(same * (dx * ex[k] + dy * ey[k]) > _F0)
            else:
                inp, inq = dp > _F0, dq > _F0
                along_out = along
            rest = line & ~along
            ok &= ~(line & along_out) & ~(rest & ~inp & ~inq)
            cross = rest & (inp != inq)
            t = dp / (dp - dq)
            t1 = np.where(cross & inp & (t < t1), t, t1)
            t0 = np.where(cross & ~inp & (t > t0), t, t0)
        x0, y0 = px[:, e] + t0 * dx, py[:, e] + t0 * dy
        x1, y1 = px[:, e] + t1 * dx, py[:, e] + t1 * dy
        tot = np.where(ok & (t0 < t1), tot + (x0 * y1 - x1 * y0), tot)
    return tot


def quad_inter_host(a, b):
    """The pair function of the rotated merge on m pairs of quads (m, 4, 2) -> (inter, area_a, area_b), float32 (m,): what
    mtgv_op_quad_inter computes, bit for bit.  Single rounded float32 operations in the order written.

    All coordinates are first taken relative to a's corner 0 (one subtraction each).  area = |s| / 2 of the shoelace sum s.
    inter = 0 where the bounds of the two quads (`quad_bounds` of the absolute corners) do not overlap - min(x1) - max(x0) > 0
    and the same in y - or either s is 0.  Otherwise the boundary of the intersection of two convex quads is made of the
    parts of a's edges inside b and the parts of b's edges inside a: with both windings made positive by their signs,
    inter = max(0, (sign_a * sum_a + sign_b * sum_b) / 2), every sum being `_edge_sum`: an edge p -> q is cut to the
    parameter interval [t0, t1] that lies inside the other quad's four half-planes (d = the signed distance numerators of p
    and q, t = dp / (dp - dq) where they differ in side) and adds cross(p', q') of what is left.  a's edges are tested closed and
    b's open, so a shared piece of boundary counts once; an edge of a that runs along an edge of b counts only where the two
    run the same way (identical quads: the area; quads that touch from outside: 0)."""
    a, b = np.asarray(a, np.float32).reshape(-1, 4, 2), np.asarray(b, np.float32).reshape(-1, 4, 2)
    with np.errstate(all="ignore"):
        ba, bb = quad_bounds(a), quad_bounds(b)
        iw = np.where(ba[:, 2] < bb[:, 2], ba[:, 2], bb[:, 2]) - np.where(ba[:, 0] > bb[:, 0], ba[:, 0], bb[:, 0])
        ih = np.where(ba[:, 3] < bb[:, 3], ba[:, 3], bb[:, 3]) - np.where(ba[:, 1] > bb[:, 1], ba[:, 1], bb[:, 1])
        o = a[:, :1]
        ra, rb = a - o, b - o
        ax, ay, bx, by = ra[:, :, 0], ra[:, :, 1], rb[:, :, 0], rb[:, :, 1]
        sa, sb = _shoelace(ax, ay), _shoelace(bx, by)
        area_a, area_b = np.abs(sa) * _HALF, np.abs(sb) * _HALF
        sga, sgb = np.where(sa > _F0, _F1, -_F1), np.where(sb > _F0, _F1, -_F1)
        same = sga * sgb
        s = (sga * _edge_sum(ax, ay, bx, by, sgb, same, True) + sgb * _edge_sum(bx, by, ax, ay, sga, same, False)) * _HALF
        full = (iw > _F0) & (ih > _F0) & ~(sa == _F0) & ~(sb == _F0)
        inter = np.where(full & (s > _F0), s, _F0)
    return inter.astype(np.float32), area_a.astype(np.float32), area_b.astype(np.float32)


def merge_tiles_obb_host(n_det, conf, cls, quads, state, tiles, geo, ratio, tile_start, hw, pad_frac, kt: int, k: int, edge: float = 2.0,
                         ios: float = 0.5, card_cls: int = 0, max_tiles_per_frame: Optional[int] = None) -> dict:
    """The rotated merge rule on the host (numpy arrays in and out): what mtgv_tiles_merge_obb computes, bit for bit.  The
    inputs are what the untiled OBB path produces with the tiles as frames: n_det (NT,), conf, cls (NT, max_det) of
    Detector.forward, quads (NT * kt, 4, 2) and state (NT * kt,) of crop.obb_cards(..., k=kt).

    1. candidates: slot j < kt of tile t iff state[t * kt + j] is 1 or 2 and the tile has a j-th detection of class card_cls
       among its first min(max(n_det[t], 0), max_det) (obb_cards' own scan); its confidence is that detection's.
    2. mapping: every corner through `_to_src`; bounds = min / max of the mapped corners by float32 comparisons.
    3. cut rule: rule 3 of `merge_tiles_host` on those bounds.
    4. order: conf descending, tile ascending, j ascending (the same 64-bit key).
    5. greedy: a later candidate b is dropped by a kept a if inter > ios * min(area_a, area_b) (`quad_inter_host`: float32,
       strict, no division in the comparison); a quad of zero area neither drops nor is dropped.
    6. orientation: a kept a of state 1 that dropped candidates of state 2 takes the first of them in the order as its donor:
       with u = (TL + TR) - (BR + BL) of each and d = ua.x * ub.x + ua.y * ub.y, d != 0 makes a's state 2 and oriented_by the
       donor's slot, d < 0 also rolls a's corners by two (TL, TR, BR, BL <- BR, BL, TL, TR).
    7. the first k kept fill slots 0 .. n_sel - 1 (sel_boxes_src: the quad's bounds); slot >= n_sel is pad_frac[slot] *
       (w, h, w, h) with its corners as quad, conf 0, state 0, src_slot -1, oriented_by -1.
    Caps and distrust are `merge_tiles_host`'s."""
    n_det, conf, cls = np.asarray(n_det, np.int32), np.asarray(conf, np.float32), np.asarray(cls, np.int32)
    tiles, geo, ratio = np.asarray(tiles, np.int32).reshape(-1, 5), np.asarray(geo, np.int32).reshape(-1, 4), np.asarray(ratio, np.float64)
    tile_start, hw, pad_frac = np.asarray(tile_start, np.int64), np.asarray(hw, np.int32).reshape(-1, 2), np.asarray(pad_frac, np.float32)
    NT, F, kt, k, md = tiles.shape[0], hw.shape[0], int(kt), int(k), conf.shape[1]
    quads, state = np.asarray(quads, np.float32).reshape(NT * kt, 4, 2), np.asarray(state, np.int32).reshape(NT * kt)
    mt = int(np.diff(tile_start).max()) if max_tiles_per_frame is None and F else int(max_tiles_per_frame or 0)
    assert 1 <= k <= MAX_CARDS and 1 <= kt <= md and mt * kt <= MAX_CANDIDATES, f"k={k} kt={kt} tiles per frame {mt}"
    e32, thr = np.float32(edge), np.float32(ios)
    out = {"sel_boxes_src": np.zeros((F * k, 4), np.float32), "quads_src": np.zeros((F * k, 4, 2), np.float32),
           "frame_idx": np.repeat(np.arange(F, dtype=np.int32), k), "sel_conf": np.zeros((F * k,), np.float32),
           "src_slot": np.full((F * k,), -1, np.int32), "n_sel": np.zeros((F,), np.int32), "state": np.zeros((F * k,), np.int32),
           "oriented_by": np.full((F * k,), -1, np.int32)}
    for f in range(F):
        h, w = int(hw[f, 0]), int(hw[f, 1])
        ts, te = int(tile_start[f]), int(tile_start[f + 1])
        if ts < 0 or te < ts or te > NT or te - ts > mt:
            ts = te = 0
        cq, cc, cslot, cflat = [], [], [], []
        for tl, t in enumerate(range(ts, te)):
            _, y0, x0, wh, ww = (int(v) for v in tiles[t])
            nd = min(max(int(n_det[t]), 0), md)
            cards = np.flatnonzero(cls[t, :nd] == card_cls)
            st = state[t * kt : (t + 1) * kt]
            j = np.arange(kt)[((st == 1) | (st == 2)) & (np.arange(kt) < len(cards))]
            if j.size == 0:
                continue
            q = quads[t * kt + j]
            m = np.stack([_to_src(q[:, :, 0], geo[t, 3], ratio[t], x0, ww), _to_src(q[:, :, 1], geo[t, 2], ratio[t], y0, wh)], 2)
            bd = quad_bounds(m)
            cut = np.zeros((len(j),), bool)
            if x0 > 0:
                cut |= bd[:, 0] < np.float32(x0) + e32
            if x0 + ww < w:
                cut |= bd[:, 2] > np.float32(x0 + ww) - e32
            if y0 > 0:
                cut |= bd[:, 1] < np.float32(y0) + e32
            if y0 + wh < h:
                cut |= bd[:, 3] > np.float32(y0 + wh) - e32
            j = j[~cut]
            cq.append(m[~cut]), cc.append(conf[t, cards[j]]), cslot.append(t * kt + j), cflat.append(tl * kt + j)
        n_sel = 0
        if cq and sum(len(x) for x in cq):
            cq, cc, cslot, cflat = np.concatenate(cq), np.concatenate(cc), np.concatenate(cslot), np.concatenate(cflat)
            order = np.argsort(_order_key(cc, cflat))[::-1]  # the keys are unique
            cq, cc, cslot = cq[order], cc[order], cslot[order]
            cst = state[cslot]
            alive = np.ones((len(cq),), bool)
            while n_sel < k and alive.any():
                p = int(np.argmax(alive))
                alive[p] = False
                inter, area_a, area_b = quad_inter_host(np.broadcast_to(cq[p], cq.shape), cq)
                drop = alive & ~(area_a == _F0) & ~(area_b == _F0) & (inter > thr * np.where(area_a < area_b, area_a, area_b))
                alive &= ~drop
                o = f * k + n_sel
                qa, sta, by = cq[p], int(cst[p]), -1
                donors = np.flatnonzero(drop & (cst == 2))
                if sta == 1 and donors.size:
                    qb = cq[donors[0]]
                    ua, ub = (qa[0] + qa[1]) - (qa[2] + qa[3]), (qb[0] + qb[1]) - (qb[2] + qb[3])
                    d = ua[0] * ub[0] + ua[1] * ub[1]
                    if d != _F0:
                        sta, by = 2, int(cslot[donors[0]])
                    if d < _F0:
                        qa = qa[[2, 3, 0, 1]]
                out["sel_boxes_src"][o], out["quads_src"][o], out["sel_conf"][o], out["src_slot"][o] = quad_bounds(cq[p])[0], qa, cc[p], cslot[p]
                out["state"][o], out["oriented_by"][o] = sta, by
                n_sel += 1
        out["n_sel"][f] = n_sel
        for s in range(n_sel, k):
            pb = pad_frac[s] * np.array([w, h, w, h], np.float32)
            out["sel_boxes_src"][f * k + s] = pb
            out["quads_src"][f * k + s] = np.array([[pb[0], pb[1]], [pb[2], pb[1]], [pb[2], pb[3]], [pb[0], pb[3]]], np.float32)
    return out
