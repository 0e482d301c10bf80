"""ORACLE for rectangular detector inputs (test infrastructure, never shipped or measured as the product).

oracle/detector_ref.py's `backbone_neck`, `_conv`, `_branch`, `_branch_dw`, `preprocess` and `nms_single` take any map
shape and are imported.  Only `make_anchors`, `head` and `mask_logits` assume a square; they are restated here for one
(gh, gw) grid per level (`cfg.grids`), operation for operation as the oracle writes them, so that a square `cfg` gives
the oracle's bits (tests/test_rect_cpu.py pins that).  The OBB head is tests/obb_ref.py's with the same anchors.

Every function computes in the dtype of its inputs: float32 is the oracle's arithmetic, float64 the yardstick.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import obb_ref
from mtgv import spec
from oracle import detector_ref as D
from oracle import resize_ref


def make_anchors(cfg: spec.DetectorConfig):
    """anchor centres (2, A) and strides (1, A): grid (x + 0.5, y + 0.5), row-major per level, P3 first"""
    pts, st = [], []
    for s, (gh, gw) in zip((8, 16, 32), cfg.grids):
        sy, sx = torch.meshgrid(torch.arange(gh, dtype=torch.float32) + 0.5, torch.arange(gw, dtype=torch.float32) + 0.5, indexing="ij")
        pts.append(torch.stack((sx, sy), -1).view(-1, 2))
        st.append(torch.full((gh * gw, 1), float(s)))
    return torch.cat(pts).T.contiguous(), torch.cat(st).T.contiguous()


def head(feats, p, cfg: spec.DetectorConfig):
    """Segment head on feature maps of any (gh, gw): pred (B, 4 + nc + nm, A), protos (B, nm, in_h / 4, in_w / 4)"""
    for f, (gh, gw) in zip(feats, cfg.grids):
        assert tuple(f.shape[2:]) == (gh, gw), (tuple(f.shape), cfg.grids)
    pre = f"model.{cfg.head_index}"
    eps = cfg.bn_eps
    b = feats[0].shape[0]
    cls_branch = D._branch_dw if cfg.arch == "11" else D._branch
    x = D._conv(feats[0], p, f"{pre}.proto.cv1", 3, eps=eps)
    x = F.conv_transpose2d(x, p[f"{pre}.proto.upsample.weight"], p[f"{pre}.proto.upsample.bias"], stride=2)
    x = D._conv(x, p, f"{pre}.proto.cv2", 3, eps=eps)
    protos = D._conv(x, p, f"{pre}.proto.cv3", 1, eps=eps)
    mc = torch.cat([D._branch(f, p, f"{pre}.cv4.{l}", eps).view(b, cfg.nm, -1) for l, f in enumerate(feats)], 2)
    xs = [torch.cat((D._branch(f, p, f"{pre}.cv2.{l}", eps), cls_branch(f, p, f"{pre}.cv3.{l}", eps)), 1) for l, f in enumerate(feats)]
    x_cat = torch.cat([xi.view(b, 4 * cfg.reg_max + cfg.nc, -1) for xi in xs], 2)
    box, cls = x_cat.split((4 * cfg.reg_max, cfg.nc), 1)
    a = box.shape[-1]
    w = p[f"{pre}.dfl.conv.weight"].view(1, cfg.reg_max, 1, 1)
    dist = (box.view(b, 4, cfg.reg_max, a).transpose(2, 1).softmax(1) * w).sum(1)  # (b, 4, a) l, t, r, b
    anchors, strides = make_anchors(cfg)
    anchors, strides = anchors.to(dist.dtype), strides.to(dist.dtype)
    lt, rb = dist.chunk(2, 1)
    x1y1 = anchors.unsqueeze(0) - lt
    x2y2 = anchors.unsqueeze(0) + rb
    dbox = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * strides
    return torch.cat((dbox, cls.sigmoid(), mc), 1), protos


def head_obb(feats, p, cfg: spec.DetectorConfig):
    """OBB head (tests/obb_ref.py: head) with the anchors of cfg.grids: pred (B, 4 + nc + 1, A)"""
    pre = f"model.{cfg.head_index}"
    eps = cfg.bn_eps
    b = feats[0].shape[0]
    cls_branch = D._branch_dw if cfg.arch == "11" else D._branch
    logit = torch.cat([D._branch(f, p, f"{pre}.cv4.{l}", eps).view(b, cfg.ne, -1) for l, f in enumerate(feats)], 2)
    angle = (logit.sigmoid() - 0.25) * torch.pi
    xs = [torch.cat((D._branch(f, p, f"{pre}.cv2.{l}", eps), cls_branch(f, p, f"{pre}.cv3.{l}", eps)), 1) for l, f in enumerate(feats)]
    x_cat = torch.cat([xi.view(b, 4 * cfg.reg_max + cfg.nc, -1) for xi in xs], 2)
    box, cls = x_cat.split((4 * cfg.reg_max, cfg.nc), 1)
    a = box.shape[-1]
    w = p[f"{pre}.dfl.conv.weight"].view(1, cfg.reg_max, 1, 1)
    dist = F.conv2d(box.view(b, 4, cfg.reg_max, a).transpose(2, 1).softmax(1), w).view(b, 4, a)  # l, t, r, b
    anchors, strides = make_anchors(cfg)
    anchors, strides = anchors.to(dist.dtype), strides.to(dist.dtype)
    l_, t_, r_, b_ = dist.unbind(1)
    ang = angle[:, 0]
    cs, sn = torch.cos(ang), torch.sin(ang)
    xf, yf = (r_ - l_) / 2, (b_ - t_) / 2
    x = (xf * cs - yf * sn + anchors[0]) * strides[0]
    y = (xf * sn + yf * cs + anchors[1]) * strides[0]
    wh = torch.stack(((l_ + r_) * strides[0], (t_ + b_) * strides[0]), 1)
    return torch.cat((torch.stack((x, y), 1), wh, cls.sigmoid(), angle), 1)


def forward(params, cfg: spec.DetectorConfig, frames_u8, flip_rgb=True, dtype=torch.float32):
    """(B, in_h, in_w, 3) uint8 frames -> (pred, protos) (segment) or pred (OBB), torch tensors of `dtype`"""
    assert tuple(np.asarray(frames_u8).shape[1:]) == (cfg.in_h, cfg.in_w, 3), (np.asarray(frames_u8).shape, cfg.input_hw)
    p = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(dtype) for k, v in params.items()}
    with torch.no_grad():
        feats = D.backbone_neck(D.preprocess(frames_u8, flip_rgb, dtype), p, cfg)
        return head_obb(feats, p, cfg) if cfg.task == "obb" else head(feats, p, cfg)


def mask_logits(pred_img: np.ndarray, protos_img: np.ndarray, det: dict, nc: int, in_h: int, in_w: int) -> np.ndarray:
    """process_mask up to the crop for an in_h x in_w input: (n, mh, mw) float32 logits, zero outside the box (scaled
    to mask units per direction, x in [x1, x2), y in [y1, y2)).  As in the oracle the product is summed in float64 and
    rounded once, whichever dtype pred and protos_img come in."""
    c, mh, mw = protos_img.shape
    coef = np.asarray(pred_img, np.float32)[4 + nc :, det["keep_idx"]].T  # (n, nm)
    m = (coef.astype(np.float64) @ protos_img.reshape(c, -1).astype(np.float64)).reshape(-1, mh, mw).astype(np.float32)
    b = det["boxes"].astype(np.float32).copy()
    b[:, [0, 2]] *= np.float32(mw / in_w)
    b[:, [1, 3]] *= np.float32(mh / in_h)
    r = np.arange(mw, dtype=np.float32)[None, None, :]
    cc = np.arange(mh, dtype=np.float32)[None, :, None]
    inside = (r >= b[:, 0, None, None]) & (r < b[:, 2, None, None]) & (cc >= b[:, 1, None, None]) & (cc < b[:, 3, None, None])
    return m * inside


def detect(params, cfg: spec.DetectorConfig, frames_u8, flip_rgb=True, dtype=torch.float32):
    """the full detector on a batch: (list of per-image dicts, pred, protos) like oracle.detector_ref.detect; OBB:
    (list of dicts of obb_ref.nms_rotated_single, pred, None).  NMS runs on pred rounded to float32 in either dtype."""
    if cfg.task == "obb":
        pred = forward(params, cfg, frames_u8, flip_rgb, dtype).numpy()
        p32 = pred.astype(np.float32)
        return [obb_ref.nms_rotated_single(p32[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh) for i in range(len(p32))], pred, None
    pred, protos = forward(params, cfg, frames_u8, flip_rgb, dtype)
    pred, protos = pred.numpy(), protos.numpy()
    p32 = pred.astype(np.float32)
    out = []
    for i in range(pred.shape[0]):
        d = D.nms_single(p32[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        d["mask_logits"] = mask_logits(p32[i], protos[i], d, cfg.nc, cfg.in_h, cfg.in_w)
        out.append(d)
    return out, pred, protos


def letterbox(frame: np.ndarray, size: int = 640, stride: int = 32, pad_value: int = 114):
    """the expected LetterBox(auto=True) image of `frame`: oracle/resize_ref.letterbox holds the same resampled (nh, nw)
    image (r, nh and nw are the square letterbox's); it is cut out and placed at (top, left) of a pad_value-filled
    (out_h, out_w) image.  Returns (image, geometry of mtgv.detector.rect_geometry)."""
    from mtgv.detector import letterbox_geometry, rect_geometry

    h, w = frame.shape[:2]
    geo = rect_geometry(h, w, size, stride)
    r, nh, nw, top, left, out_h, out_w = geo
    r0, nh0, nw0, top0, left0 = letterbox_geometry(h, w, size)
    assert (r0, nh0, nw0) == (r, nh, nw)
    sq = resize_ref.letterbox(frame, size)
    out = np.full((out_h, out_w, 3), pad_value, np.uint8)
    out[top : top + nh, left : left + nw] = sq[top0 : top0 + nh, left0 : left0 + nw]
    return out, geo
