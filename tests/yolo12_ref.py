"""REFERENCE for YOLO12 (test infrastructure, like oracle/: never shipped or measured as the product).  Not a test module.

A float64-capable torch restatement of what oracle/detector_ref.py does not have: A2C2f, ABlock, AAttn (area attention) and
the YOLO12 graph walk.  Everything else is detector_ref's own code: `_conv`, `_c3k`, `_c3k2`, `preprocess`, `head`,
`nms_single`, `mask_logits`.  detector_ref.head keys its class branch and its index on arch "11", so it is handed a
`dataclasses.replace(cfg, arch="11")` config and the head's parameters renamed model.21. -> model.23.; detector_ref's
`backbone_neck` skips node kinds it does not know and is not used.

PARITY UNPINNED like the rest of the detector: recalled from ultralytics 8.3.x (nn/modules/block.py: AAttn, ABlock, A2C2f;
cfg/models/12/yolo12-seg.yaml), which is not installed here.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from mtgv import spec
from oracle import detector_ref as D
from oracle import obb_ref

HEAD_DIM = 32


def area_attention(qkv, heads, area):
    """qkv (B, 3 c, H, W), channel h * 96 + [0, 32) q, + [32, 64) k, + [64, 96) v of head h -> (attention output (B, c, H, W)
    before the positional encoding, v (B, c, H, W)).  Tokens are the pixels row-major; with area > 1 the sequence is cut into
    `area` contiguous chunks of N / area tokens and attention runs inside each chunk."""
    b, c3, h, w = qkv.shape
    c, n = c3 // 3, h * w
    assert c == heads * HEAD_DIM and n % area == 0
    t = qkv.flatten(2).transpose(1, 2)  # (B, N, 3c)
    t = t.reshape(b * area, n // area, heads, 3 * HEAD_DIM)
    q, k, v = t.permute(0, 2, 3, 1).split([HEAD_DIM, HEAD_DIM, HEAD_DIM], dim=2)  # (B * area, heads, 32, N / area)
    attn = ((q.transpose(-2, -1) @ k) * (HEAD_DIM**-0.5)).softmax(dim=-1)
    x = v @ attn.transpose(-2, -1)  # (B * area, heads, 32, N / area)
    x = x.permute(0, 3, 1, 2).reshape(b, n, c)  # chunks back in order, channel h * 32 + d
    v = v.permute(0, 3, 1, 2).reshape(b, n, c)
    to_map = lambda y: y.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return to_map(x), to_map(v)


def _pe(v, p, prefix, eps):
    """Conv(c, c, 7, pad 3, groups=c, act=False) on v as the whole map: it crosses area boundaries"""
    c = v.shape[1]
    x = F.conv2d(v, p[f"{prefix}.conv.weight"], None, stride=1, padding=3, groups=c)
    return F.batch_norm(x, p[f"{prefix}.bn.running_mean"], p[f"{prefix}.bn.running_var"], p[f"{prefix}.bn.weight"], p[f"{prefix}.bn.bias"], False, 0.0, eps)


def _aattn(x, p, prefix, area, eps):
    heads = x.shape[1] // HEAD_DIM
    qkv = D._conv(x, p, f"{prefix}.qkv", 1, eps=eps, act=False)
    y, v = area_attention(qkv, heads, area)
    return D._conv(y + _pe(v, p, f"{prefix}.pe", eps), p, f"{prefix}.proj", 1, eps=eps, act=False)


def _ablock(x, p, prefix, area, eps):
    x = x + _aattn(x, p, f"{prefix}.attn", area, eps)
    return x + D._conv(D._conv(x, p, f"{prefix}.mlp.0", 1, eps=eps), p, f"{prefix}.mlp.1", 1, eps=eps, act=False)


def _a2c2f(x, p, prefix, n, a2, area, residual, eps):
    y = [D._conv(x, p, f"{prefix}.cv1", 1, eps=eps)]
    for j in range(n):
        t = y[-1]
        if a2:
            for b in range(2):
                t = _ablock(t, p, f"{prefix}.m.{j}.{b}", area, eps)
        else:
            t = D._c3k(t, p, f"{prefix}.m.{j}", 2, True, eps)
        y.append(t)
    out = D._conv(torch.cat(y, 1), p, f"{prefix}.cv2", 1, eps=eps)
    if a2 and residual:
        return x + p[f"{prefix}.gamma"].view(1, -1, 1, 1) * out
    return out


def backbone_neck(x, p, cfg: spec.DetectorConfig):
    outs = {}
    graph, feats = spec.detector_graph(cfg)
    eps = cfg.bn_eps
    for idx, kind, a in graph:
        pre = f"model.{idx}"
        if kind == "Conv":
            x = D._conv(x, p, pre, a[1], a[2], eps)
        elif kind == "C3k2":
            x = D._c3k2(x, p, pre, a[1], a[2], eps)
        elif kind == "A2C2f":
            x = _a2c2f(x, p, pre, a[1], a[2], a[3], a[4], eps)
        elif kind == "Upsample":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        elif kind == "Concat":
            x = torch.cat([outs[s] for s in a], 1)
        else:
            raise KeyError(kind)
        outs[idx] = x
    return [outs[f] for f in feats]


def _head_args(p, cfg):
    """detector_ref.head's view of a YOLO12 head: YOLO11's class branch at YOLO11's index"""
    assert cfg.arch == "12"
    old, new = f"model.{cfg.head_index}.", "model.23."
    return {(new + k[len(old):] if k.startswith(old) else k): v for k, v in p.items()}, dataclasses.replace(cfg, arch="11")


def forward(params, cfg: spec.DetectorConfig, frames_u8, flip_rgb=True, dtype=torch.float32):
    """(B, in_h, in_w, 3) uint8 frames -> (pred, protos) (segment) or pred (OBB), torch tensors of `dtype`"""
    assert tuple(np.asarray(frames_u8).shape[1:]) == (cfg.in_h, cfg.in_w, 3), (np.asarray(frames_u8).shape, cfg.in_h, cfg.in_w)
    p = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(dtype) for k, v in params.items()}
    with torch.no_grad():
        feats = backbone_neck(D.preprocess(frames_u8, flip_rgb, dtype), p, cfg)
        hp, hcfg = _head_args(p, cfg)
        return D.head(feats, hp, hcfg)


def detect(params, cfg: spec.DetectorConfig, frames_u8, flip_rgb=True, dtype=torch.float32):
    """detector_ref.detect's return shapes: (per-image dicts, pred, protos or None); NMS and the mask crop on pred rounded to float32"""
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
        d["mask_logits"] = D.mask_logits(p32[i], protos[i], d, cfg.nc, (cfg.in_h, cfg.in_w))
        out.append(d)
    return out, pred, protos


def flops_per_frame(cfg: spec.DetectorConfig) -> float:
    """Algorithmic FLOPs of one frame, counted from spec.detector_graph and the head's shapes independently of the library:
    2 x (output pixels) x cout x cin x k x k per conv (the stem's cin is 3), attention as 2 heads N (N / area) 64 per block,
    depthwise convs as 2 k^2 pixels c; decode, NMS, upsampling and the mask product are not counted."""
    total = 0.0
    hw = {-1: (cfg.in_h, cfg.in_w)}
    chans = {-1: 3}
    graph, feats = spec.detector_graph(cfg)

    def conv(px, cout, cin, k=1):
        nonlocal total
        total += 2.0 * px * cout * cin * k * k

    def c3k(px, c):
        c_ = c // 2
        conv(px, c_, c), conv(px, c_, c), conv(px, c, 2 * c_)
        for _ in range(2):
            conv(px, c_, c_, 3), conv(px, c_, c_, 3)

    prev, (h, w) = 3, (cfg.in_h, cfg.in_w)
    for idx, kind, a in graph:
        if kind == "Conv":
            h, w = h // a[2], w // a[2]
            conv(h * w, a[0], prev, a[1])
            prev = a[0]
        elif kind == "C3k2":
            cout, n, k, e = a
            ch, px = int(cout * e), h * w
            conv(px, 2 * ch, prev), conv(px, cout, (2 + n) * ch)
            for _ in range(n):
                if k:
                    c3k(px, ch)
                else:
                    conv(px, ch // 2, ch, 3), conv(px, ch, ch // 2, 3)
            prev = cout
        elif kind == "A2C2f":
            cout, n, a2, area, _, ratio = a
            ch, px = cout // 2, h * w
            conv(px, ch, prev), conv(px, cout, (1 + n) * ch)
            for _ in range(n):
                if not a2:
                    c3k(px, ch)
                    continue
                for _ in range(2):
                    conv(px, 3 * ch, ch), conv(px, ch, ch)
                    total += 2.0 * (ch // HEAD_DIM) * px * (px // area) * 64  # q^T k and attn v, 32 wide each
                    total += 2.0 * 49 * px * ch
                    conv(px, int(ch * ratio), ch), conv(px, ch, int(ch * ratio))
            prev = cout
        elif kind == "Upsample":
            h, w = 2 * h, 2 * w
        elif kind == "Concat":
            prev = sum(chans[s] for s in a)
            h, w = hw[a[0]]
        else:
            raise KeyError(kind)
        chans[idx], hw[idx] = prev, (h, w)
    ch = [chans[f] for f in feats]
    c2, c3 = max(16, ch[0] // 4, cfg.reg_max * 4), max(ch[0], min(cfg.nc, 100))
    obb = cfg.task == "obb"
    n4 = cfg.ne if obb else cfg.nm
    c4 = max(ch[0] // 4, n4)
    for f, cl in zip(feats, ch):
        px = hw[f][0] * hw[f][1]
        conv(px, c2, cl, 3), conv(px, c2, c2, 3), conv(px, 4 * cfg.reg_max, c2)
        total += 2.0 * 9 * px * cl + 2.0 * 9 * px * c3  # the class branch's two depthwise 3x3
        conv(px, c3, cl), conv(px, c3, c3), conv(px, cfg.nc, c3)
        conv(px, c4, cl, 3), conv(px, c4, c4, 3), conv(px, n4, c4)
    if not obb:
        px = hw[feats[0]][0] * hw[feats[0]][1]
        conv(px, cfg.npr, ch[0], 3)
        conv(px, 4 * cfg.npr, cfg.npr)  # ConvTranspose2d(k2, s2): every input pixel feeds four outputs
        conv(4 * px, cfg.npr, cfg.npr, 3), conv(4 * px, cfg.nm, cfg.npr)
    return total
