"""Host side of the detect stage: YOLOv8 / YOLO11 / YOLO12 (scales n, s, m: `spec.detector_scale_config`) forward + decode + NMS on the GPU - the segment family with mask
logits, the OBB family (`DetectorConfig(task="obb")`) with rotated boxes and rotated NMS.

`Detector.detect(frame)` is the north-star name; the reference's boundary is
`CardSegmenter(model_path)(rgb_im) -> list[InstanceSeg]` (mtgvision/od_export.py:141-160), which
`mtgv.adapters.CardSegmenter` provides on top of this class.  All arithmetic is in libmtgv.so.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Mapping, Optional, Union

import numpy as np
import torch

from . import native, spec


@dataclass
class Detections:
    """Raw per-frame detector output (score-descending)."""

    boxes_xyxy: torch.Tensor  # (n, 4) float32, pixels of the letterboxed frame (640 x 640, or the handle's in_h x in_w)
    conf: torch.Tensor  # (n,) float32
    cls: torch.Tensor  # (n,) int64
    keep_idx: torch.Tensor  # (n,) int64 anchor index in [0, num_anchors)
    mask_logits: Optional[torch.Tensor]  # (n, in_h / 4, in_w / 4) float32 (160 x 160 at 640 x 640), zero outside the box


@dataclass
class ObbDetections:
    """Raw per-frame output of an OBB detector (score-descending)."""

    rboxes: torch.Tensor  # (n, 5) float32: x, y, w, h in pixels of the letterboxed frame, angle in radians [-pi/4, 3pi/4)
    conf: torch.Tensor  # (n,) float32
    cls: torch.Tensor  # (n,) int64
    keep_idx: torch.Tensor  # (n,) int64 anchor index


def letterbox_geometry(h: int, w: int, size: int = 640):
    """ultralytics LetterBox geometry: (ratio, nh, nw, top, left) - scale to fit, centre (round(d - 0.1) like upstream):
    `fit_geometry` on a square"""
    return fit_geometry(h, w, size, size)


def rect_geometry(h: int, w: int, size: int = 640, stride: int = 32):
    """ultralytics LetterBox(auto=True) geometry, what the predictor runs in front of a .pt checkpoint [external - recalled
    from ultralytics 8.3.x, unpinned like the rest of the detector]: scale to fit `size`, then pad only up to the next
    multiple of `stride`.  (ratio, nh, nw, top, left, out_h, out_w): the (nh, nw) image sits at (top, left) of an
    (out_h, out_w) input - 480 x 640 for a 640 x 480 webcam frame, 384 x 640 for 720p."""
    r = min(size / h, size / w)
    nh, nw = int(round(h * r)), int(round(w * r))
    dh, dw = ((size - nh) % stride) / 2, ((size - nw) % stride) / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return r, nh, nw, top, left, nh + top + bottom, nw + left + right


def fit_geometry(h: int, w: int, out_h: int, out_w: int):
    """an (h, w) frame scaled to fit and centred in an (out_h, out_w) input: (ratio, nh, nw, top, left).  Equals
    `rect_geometry` whenever (out_h, out_w) is that frame shape's own rectangle."""
    r = min(out_h / h, out_w / w)
    nh, nw = min(int(round(h * r)), out_h), min(int(round(w * r)), out_w)
    return r, nh, nw, int(round((out_h - nh) / 2 - 0.1)), int(round((out_w - nw) / 2 - 0.1))


def letterbox_device(frame: torch.Tensor, size=640, pad_value: int = 114):
    """(H, W, 3) uint8 frame on the GPU, or (n, H, W, 3) same-sized frames -> ((n, out_h, out_w, 3) uint8 letterboxed images
    on the GPU, ratio, (left, top)): one library kernel (resize.hip: letterbox_u8_kernel) instead of a host resample + pad.
    `size` = (out_h, out_w), or one int for a square: scaled to fit and centred (`fit_geometry`)."""
    native.require_gpu()
    assert frame.is_cuda and frame.dtype == torch.uint8 and frame.ndim in (3, 4) and frame.shape[-1] == 3, f"{tuple(frame.shape)} {frame.dtype}"
    h, w = int(frame.shape[-3]), int(frame.shape[-2])
    out_h, out_w = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size), int(size))
    n = int(frame.shape[0]) if frame.ndim == 4 else 1
    r, nh, nw, top, left = fit_geometry(h, w, out_h, out_w)
    out = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=frame.device)
    with torch.cuda.device(frame.device):
        native.check(native.lib().mtgv_letterbox_rect_u8(native.ptr(frame.contiguous()), n, h, w, native.ptr(out), out_h, out_w, nh, nw, top,
                                                         left, pad_value, native.stream()))
    return out, r, (left, top)


def letterbox(frame: np.ndarray, size: int = 640, pad_value: int = 114):
    """ultralytics LetterBox for non-.pt backends: scale to fit, centre, pad to size x size with 114.

    Returns (image (size,size,3) uint8, ratio, (pad_left, pad_top)).  Frames that already fit
    (e.g. the 640x480 webcam frames of server.py / od_cam.py) are only padded; other sizes are
    resized bilinearly on the host (cv2.resize is not available here: that resample is unpinned).
    """
    h, w = frame.shape[:2]
    r, nh, nw, top, left = letterbox_geometry(h, w, size)
    img = frame
    if (nh, nw) != (h, w):
        t = torch.from_numpy(np.ascontiguousarray(frame)).permute(2, 0, 1)[None].float()
        t = torch.nn.functional.interpolate(t, (nh, nw), mode="bilinear", align_corners=False)
        img = t[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy()
    out = np.full((size, size, 3), pad_value, np.uint8)
    out[top : top + nh, left : left + nw] = img
    return out, r, (left, top)


def _padded_outputs(n: int, max_det: int, box_name: str, box_width: int, dev):
    """the padded output tensors of a forward or an NMS: n_det (n,) int32, `box_name` (n, max_det, box_width) float32, conf
    (n, max_det) float32, cls and keep_idx (n, max_det) int32.  Uninitialised: the library writes every element (slots
    beyond n_det as zeros), so there are no fill kernels here."""
    return {
        "n_det": torch.empty((n,), dtype=torch.int32, device=dev),
        box_name: torch.empty((n, max_det, box_width), dtype=torch.float32, device=dev),
        "conf": torch.empty((n, max_det), dtype=torch.float32, device=dev),
        "cls": torch.empty((n, max_det), dtype=torch.int32, device=dev),
        "keep_idx": torch.empty((n, max_det), dtype=torch.int32, device=dev),
    }


class Detector:
    def __init__(
        self,
        cfg: Optional[spec.DetectorConfig] = None,
        state_dict: Optional[Mapping[str, Union[np.ndarray, torch.Tensor]]] = None,
        max_batch: int = 32,
        device=None,
    ):
        native.require_gpu()
        # (no cfg: the family and scale of the state dict, spec.detector_config_for_state; neither: yolov8n-seg)
        self.cfg = cfg or (spec.DetectorConfig() if state_dict is None else spec.detector_config_for_state(state_dict))
        self.max_batch = int(max_batch)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        c = native.DetectorCfg()
        c.nc, c.imgsz, c.max_batch = self.cfg.nc, self.cfg.imgsz, self.max_batch
        c.conf, c.iou, c.max_det = self.cfg.conf, self.cfg.iou, self.cfg.max_det
        c.arch = {"11": 11, "12": 12}.get(self.cfg.arch, 8)
        c.task = 1 if self.cfg.task == "obb" else 0
        c.scale = spec.SCALE_NAMES.index(self.cfg.scale)  # (l and x: the library refuses them, status 2)
        if self.cfg.input_hw is not None:  # (0, 0: the square imgsz x imgsz)
            c.in_h, c.in_w = self.cfg.in_h, self.cfg.in_w
        self._h = native.c_vp(0)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_detector_create(C.byref(c), C.byref(self._h)))
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, state_dict: Mapping[str, Union[np.ndarray, torch.Tensor]]):
        """ultralytics `model.state_dict()` keys (model.<i>....); `num_batches_tracked` is ignored."""
        want = spec.detector_param_shapes(self.cfg)
        L = native.lib()
        with torch.cuda.device(self.device):
            for key, shape in want.items():
                if key not in state_dict:
                    raise KeyError(f"missing parameter {key}")
                a = state_dict[key]
                a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
                a = np.ascontiguousarray(a, dtype=np.float32)
                assert tuple(a.shape) == tuple(shape), f"{key}: shape {tuple(a.shape)} != {tuple(shape)}"
                native.check(L.mtgv_detector_set_param(self._h, key.encode(), a.ctypes.data_as(native.c_vp), a.size))
            native.check(L.mtgv_detector_finalize(self._h))
        return self

    # ---- batched device API (what the pipeline uses) ---------------------------
    def forward(self, frames_u8: torch.Tensor, flip_rgb: bool = True, mask_rows: int = 0):
        """frames (n, in_h, in_w, 3) uint8 on the GPU (640 x 640 unless cfg.input_hw names a rectangle) -> dict of padded
        device tensors.

        n_det (n,) int32; boxes (n, max_det, 4); conf (n, max_det); cls, keep_idx (n, max_det) int32;
        mask_logits (n, mask_rows, in_h / 4, in_w / 4) if mask_rows > 0.
        An OBB detector returns n_det, rboxes (n, max_det, 5) xywh + angle, conf, cls, keep_idx; it has no masks and
        ignores mask_rows."""
        H, W, md = self.cfg.in_h, self.cfg.in_w, self.cfg.max_det
        assert frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.ndim == 4 and tuple(frames_u8.shape[1:]) == (H, W, 3), (
            f"frames {tuple(frames_u8.shape)} {frames_u8.dtype}: expected (n, {H}, {W}, 3) uint8 on the GPU"
        )
        n = frames_u8.shape[0]
        assert 0 < n <= self.max_batch, f"batch {n} outside [1, {self.max_batch}]"
        dev = self.device
        if self.cfg.task == "obb":
            return self._forward_obb(frames_u8, n, flip_rgb)
        out = _padded_outputs(n, md, "boxes", 4, dev)
        # mask rows beyond n_det are written too (zeros)
        out["mask_logits"] = torch.empty((n, mask_rows, H // 4, W // 4), dtype=torch.float32, device=dev) if mask_rows > 0 else None
        with torch.cuda.device(dev):
            native.check(
                native.lib().mtgv_detector_forward(
                    self._h, native.ptr(frames_u8.contiguous()), n, 1 if flip_rgb else 0, native.ptr(out["n_det"]), native.ptr(out["boxes"]),
                    native.ptr(out["conf"]), native.ptr(out["cls"]), native.ptr(out["keep_idx"]), native.ptr(out["mask_logits"]), int(mask_rows), native.stream(),
                )
            )
        return out

    def _forward_obb(self, frames_u8: torch.Tensor, n: int, flip_rgb: bool):
        dev = self.device
        out = _padded_outputs(n, self.cfg.max_det, "rboxes", 5, dev)
        with torch.cuda.device(dev):
            native.check(
                native.lib().mtgv_detector_forward_obb(
                    self._h, native.ptr(frames_u8.contiguous()), n, 1 if flip_rgb else 0, native.ptr(out["n_det"]), native.ptr(out["rboxes"]),
                    native.ptr(out["conf"]), native.ptr(out["cls"]), native.ptr(out["keep_idx"]), native.stream(),
                )
            )
        return out

    def set_fork(self, mode: int):
        """the forward's internal fork-join: 1 on, 0 off, -1 the default (on unless MTGV_DET_FORK=0); mtgv_detector_set_fork"""
        native.check(native.lib().mtgv_detector_set_fork(self._h, int(mode)))

    def raw_outputs(self, n: int):
        """pred (n, 4+nc+32, na) and protos (n, 32, in_h / 4, in_w / 4) of the last forward (parity tests; 8400 and
        160 x 160 at 640 x 640); an OBB detector gives (pred (n, 4+nc+1, na), None)."""
        pred = torch.empty((n, self.cfg.no, self.cfg.num_anchors), dtype=torch.float32, device=self.device)
        if self.cfg.task == "obb":
            with torch.cuda.device(self.device):
                native.check(native.lib().mtgv_detector_raw(self._h, n, native.ptr(pred), native.c_vp(0), native.stream()))
            return pred, None
        protos = torch.empty((n, self.cfg.nm, self.cfg.in_h // 4, self.cfg.in_w // 4), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_detector_raw(self._h, n, native.ptr(pred), native.ptr(protos), native.stream()))
        return pred, protos

    # ---- single-frame API -------------------------------------------------------
    def detect(self, frame: np.ndarray, flip_rgb: bool = True, masks: bool = True):
        """One HWC uint8 frame (any size) -> Detections (ObbDetections from an OBB detector) in the coordinates of the
        letterboxed input (640 x 640; a rectangular handle: the frame scaled to fit its in_h x in_w, centred)."""
        assert frame.ndim == 3 and frame.shape[-1] == 3 and frame.dtype == np.uint8, f"{frame.shape} {frame.dtype}"
        # the raw frame goes to the GPU as it is; scale-to-fit + pad there (the host `letterbox` only supplies the geometry
        # to callers that map coordinates back, e.g. CardSegmenter)
        size = self.cfg.imgsz if self.cfg.input_hw is None else (self.cfg.in_h, self.cfg.in_w)
        x, _, _ = letterbox_device(torch.from_numpy(np.ascontiguousarray(frame)).to(self.device), size)
        if self.cfg.task == "obb":
            out = self.forward(x, flip_rgb)
            n = int(out["n_det"][0].item())
            return ObbDetections(out["rboxes"][0, :n], out["conf"][0, :n], out["cls"][0, :n].long(), out["keep_idx"][0, :n].long())
        out = self.forward(x, flip_rgb, self.cfg.max_det if masks else 0)
        n = int(out["n_det"][0].item())
        return Detections(
            out["boxes"][0, :n], out["conf"][0, :n], out["cls"][0, :n].long(), out["keep_idx"][0, :n].long(),
            out["mask_logits"][0, :n] if masks else None,
        )

    __call__ = detect

    def flops_per_frame(self) -> float:
        f = C.c_double(0)
        native.check(native.lib().mtgv_detector_flops(self._h, C.byref(f)))
        return f.value

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                native.lib().mtgv_detector_destroy(self._h)
                self._h = native.c_vp(0)
        except Exception:
            pass


def nms(pred: torch.Tensor, nc: int, conf: float = 0.25, iou: float = 0.7, max_det: int = 300, max_wh: float = 7680.0):
    """Stand-alone NMS kernel on decoded predictions (n, 4+nc+nm, A) -> padded tensors like Detector.forward."""
    native.require_gpu()
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.ndim == 3
    pred = pred.contiguous()
    n, no, na = pred.shape
    nm = no - 4 - nc
    dev = pred.device
    L = native.lib()
    ws = torch.empty((int(L.mtgv_nms_workspace_bytes(n, na)) + 3) // 4, dtype=torch.int32, device=dev)
    out = _padded_outputs(n, max_det, "boxes", 4, dev)
    with torch.cuda.device(dev):
        native.check(
            L.mtgv_nms(native.ptr(pred), n, nc, nm, na, conf, iou, max_det, max_wh, native.ptr(out["n_det"]), native.ptr(out["boxes"]),
                       native.ptr(out["conf"]), native.ptr(out["cls"]), native.ptr(out["keep_idx"]), native.ptr(ws), ws.numel() * 4, native.stream())
        )
    return out


def nms_rotated(pred: torch.Tensor, nc: int, conf: float = 0.25, iou: float = 0.7, max_det: int = 300, max_wh: float = 7680.0):
    """Stand-alone rotated NMS kernel on OBB predictions (n, 4+nc+1, A) [xywh, class scores, angle] -> padded tensors like
    an OBB Detector.forward: n_det, rboxes (n, max_det, 5), conf, cls, keep_idx."""
    native.require_gpu()
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.ndim == 3 and pred.shape[1] == 4 + nc + 1, f"{tuple(pred.shape)}"
    pred = pred.contiguous()
    n, _, na = pred.shape
    dev = pred.device
    L = native.lib()
    ws = torch.empty((int(L.mtgv_nms_rotated_workspace_bytes(n, na)) + 3) // 4, dtype=torch.int32, device=dev)
    out = _padded_outputs(n, max_det, "rboxes", 5, dev)
    with torch.cuda.device(dev):
        native.check(
            L.mtgv_nms_rotated(native.ptr(pred), n, nc, na, conf, iou, max_det, max_wh, native.ptr(out["n_det"]), native.ptr(out["rboxes"]),
                               native.ptr(out["conf"]), native.ptr(out["cls"]), native.ptr(out["keep_idx"]), native.ptr(ws), ws.numel() * 4, native.stream())
        )
    return out


def probiou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """ProbIoU of the box pairs a[i], b[i] ((m, 5) x, y, w, h, angle each): the pair function of `nms_rotated` (test surface)"""
    native.require_gpu()
    assert a.is_cuda and a.dtype == torch.float32 and a.ndim == 2 and a.shape[1] == 5 and a.shape == b.shape and b.dtype == torch.float32
    a, b = a.contiguous(), b.to(a.device).contiguous()
    out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        native.check(native.lib().mtgv_op_probiou(native.ptr(a), native.ptr(b), a.shape[0], native.ptr(out), native.stream()))
    return out


def area_attn(qkv: torch.Tensor, h: int, w: int, heads: int, area: int, pe_w49: Optional[torch.Tensor] = None,
              pe_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """YOLO12's area attention alone (mtgv_op_area_attn, what the detector's ABlocks run; test surface): qkv (n, h * w, heads * 96)
    float32, per head [q 32 | k 32 | v 32] -> (n, h * w, heads * 32): softmax(q^T k / sqrt(32)) v inside each of the `area`
    contiguous token chunks, plus - with pe_w49 ([49][heads * 32]) and pe_bias - the depthwise 7x7 of v over the h x w map."""
    native.require_gpu()
    assert qkv.is_cuda and qkv.dtype == torch.float32 and qkv.ndim == 3 and tuple(qkv.shape[1:]) == (h * w, heads * 96), f"{tuple(qkv.shape)}"
    assert (pe_w49 is None) == (pe_bias is None)
    if pe_w49 is not None:
        assert pe_w49.is_cuda and pe_bias.is_cuda and tuple(pe_w49.shape) == (49, heads * 32) and tuple(pe_bias.shape) == (heads * 32,)
        pe_w49, pe_bias = pe_w49.float().contiguous(), pe_bias.float().contiguous()
    qkv = qkv.contiguous()
    out = torch.empty((qkv.shape[0], h * w, heads * 32), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        native.check(native.lib().mtgv_op_area_attn(native.ptr(qkv), native.ptr(pe_w49), native.ptr(pe_bias), qkv.shape[0], h, w, heads, area,
                                                    native.ptr(out), native.stream()))
    return out


def psa_attn(qkv: torch.Tensor, h: int, w: int, heads: int, pe_w9: Optional[torch.Tensor] = None,
             pe_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """YOLO11's C2PSA attention core alone (mtgv_op_psa_attn, the launches Detector::c2psa makes; test surface): qkv
    (n, h * w, heads * 128) float32, per head [q 32 | k 32 | v 64] -> (n, h * w, heads * 64): softmax(q^T k / sqrt(32)) v per image
    and head, plus - with pe_w9 ([9][heads * 64]) and pe_bias - the depthwise 3x3 of v over the h x w map."""
    native.require_gpu()
    assert qkv.is_cuda and qkv.dtype == torch.float32 and qkv.ndim == 3 and tuple(qkv.shape[1:]) == (h * w, heads * 128), f"{tuple(qkv.shape)}"
    assert (pe_w9 is None) == (pe_bias is None)
    if pe_w9 is not None:
        assert pe_w9.is_cuda and pe_bias.is_cuda and tuple(pe_w9.shape) == (9, heads * 64) and tuple(pe_bias.shape) == (heads * 64,)
        pe_w9, pe_bias = pe_w9.float().contiguous(), pe_bias.float().contiguous()
    qkv = qkv.contiguous()
    out = torch.empty((qkv.shape[0], h * w, heads * 64), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        native.check(native.lib().mtgv_op_psa_attn(native.ptr(qkv), native.ptr(pe_w9), native.ptr(pe_bias), qkv.shape[0], h, w, heads,
                                                   native.ptr(out), native.stream()))
    return out


def dwconv3(x: torch.Tensor, w9: torch.Tensor, bias: torch.Tensor, *, x_co: int = 0, x_fmt: int = 0, g_size: int = 0, g_stride: int = 0,
            act: int = 0, add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_co: int = 0, out_fmt: int = 0) -> torch.Tensor:
    """The detector's depthwise 3x3 alone (mtgv_op_dwconv3, the launch of C2PSA's positional encoding and of the
    Detect(legacy=False) class branch; test surface): x (n, h, w, x_ct) float32-typed (fmt 1: SP8 bytes), w9 [9][c] tap-major,
    bias [c]; output channel k reads input channel x_co + (k // g_size) * g_stride + k % g_size (g_size 0: x_co + k); act 0
    none or 3 SiLU; add (n, h, w, add_ld) float32 is added behind the activation.  Writes channels [out_co, out_co + c) of
    out (n, h, w, out_ct) - a new (n, h, w, c) tensor if none is given - and returns it."""
    native.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and w9.ndim == 2 and w9.shape[0] == 9
    n, h, w, x_ct = x.shape
    c = w9.shape[1]
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape[:3]) == (n, h, w) and tuple(bias.shape) == (c,)
    assert add is None or (add.is_cuda and add.dtype == torch.float32 and tuple(add.shape[:3]) == (n, h, w))
    d = native.Dwconv3()
    d.x, d.n, d.h, d.w, d.x_ct, d.x_co, d.x_fmt = x.data_ptr(), n, h, w, x_ct, x_co, x_fmt
    d.c, d.g_size, d.g_stride = c, g_size, g_stride
    keep = (w9.float().contiguous(), bias.float().contiguous())
    d.w9, d.bias, d.act = keep[0].data_ptr(), keep[1].data_ptr(), act
    if add is not None:
        d.add, d.add_ld = add.data_ptr(), add.shape[3]
    d.out, d.out_ct, d.out_co, d.out_fmt = out.data_ptr(), out.shape[3], out_co, out_fmt
    assert x.is_contiguous() and out.is_contiguous() and (add is None or add.is_contiguous())
    with torch.cuda.device(x.device):
        native.check(native.lib().mtgv_op_dwconv3(C.byref(d), native.stream()))
    return out


def binarize_masks(mask_logits: torch.Tensor, scale: int = 4) -> torch.Tensor:
    """(n, mh, mw) cropped logits -> (n, mh * scale, mw * scale) uint8 {0,1}: bilinear x`scale` (align_corners=False), > 0.
    (160 x 160 -> 640 x 640 for a square handle, in_h / 4 x in_w / 4 -> in_h x in_w for a rectangular one.)"""
    native.require_gpu()
    assert mask_logits.is_cuda and mask_logits.dtype == torch.float32 and mask_logits.ndim == 3
    n, mh, mw = mask_logits.shape
    out = torch.empty((n, mh * scale, mw * scale), dtype=torch.uint8, device=mask_logits.device)
    with torch.cuda.device(mask_logits.device):
        native.check(native.lib().mtgv_mask_binarize(native.ptr(mask_logits.contiguous()), n, mh, mw, scale, native.ptr(out), native.stream()))
    return out
