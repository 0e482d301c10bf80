"""Export surface of the detector: a plain `torch.nn.Module` with the ultralytics state_dict keys (model.<i>....),
built from the same graph tables as the GPU executor (`spec.detector_graph`), for `torch.jit.trace` and - where the
`onnx` package exists - `torch.onnx.export`.

The reference exports its trained detector with `YOLO(pt).export(format="onnx", nms=True)` and
`.export(format="coreml", nms=False)` (mtgvision/od_export.py:163-176); ultralytics and coremltools are absent here, so
this module mirrors the `nms=False` form: frames (B, 3, in_h, in_w) float in [0, 1] (640 x 640 unless cfg.input_hw names a
rectangle) -> (pred (B, 4 + nc + nm, A) decoded boxes / class scores / mask coefficients, protos (B, nm, in_h / 4, in_w / 4)).
NMS and mask assembly stay outside the graph
(`mtgv.detector.nms`, `Detector.forward`).  With `task="obb"` (what od_train.py builds by default) the head is `OBB` and
the only output is pred (B, 4 + nc + 1, A) = xywh, class scores, angle (`mtgv.detector.nms_rotated` outside the graph).

NOT on the recognition path: `mtgv.Detector` never calls it and there is no fallback to it.  Checked on CPU against
oracle/detector_ref.py (tests/test_export_cpu.py).
"""

from __future__ import annotations

from typing import Mapping

import numpy as np
import torch
from torch import nn

from . import spec


class Conv(nn.Module):
    """ultralytics Conv: Conv2d(bias=False, padding=k//2) + BatchNorm2d(eps 1e-3) + SiLU"""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
        self.act = nn.SiLU() if act else nn.Identity()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 3)
        self.cv2 = Conv(c_, c2, 3)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv2(self.cv1(x)) if self.add else self.cv2(self.cv1(x))


class C2f(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=False, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, e=1.0) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        for m in self.m:
            y.append(m(y[-1]))
        return self.cv2(torch.cat(y, 1))


class C3k(nn.Module):
    def __init__(self, c1, c2, n=2, shortcut=True, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1)
        self.cv2 = Conv(c1, c_, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, e=1.0) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class C3k2(C2f):
    def __init__(self, c1, c2, n=1, c3k=False, e=0.5):
        super().__init__(c1, c2, n, True, e)
        self.m = nn.ModuleList(C3k(self.c, self.c, 2, True) if c3k else Bottleneck(self.c, self.c, True) for _ in range(n))


class SPPF(nn.Module):
    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1)
        self.cv2 = Conv(c_ * 4, c2, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

    def forward(self, x):
        y = [self.cv1(x)]
        for _ in range(3):
            y.append(self.m(y[-1]))
        return self.cv2(torch.cat(y, 1))


class Attention(nn.Module):
    def __init__(self, dim, num_heads, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim**-0.5
        self.qkv = Conv(dim, dim + 2 * self.key_dim * num_heads, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x):
        b, c, h, w = x.shape
        n = h * w
        q, k, v = self.qkv(x).view(b, self.num_heads, self.key_dim * 2 + self.head_dim, n).split([self.key_dim, self.key_dim, self.head_dim], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * self.scale).softmax(dim=-1)
        y = (v @ attn.transpose(-2, -1)).view(b, c, h, w) + self.pe(v.reshape(b, c, h, w))
        return self.proj(y)


class PSABlock(nn.Module):
    def __init__(self, c, num_heads):
        super().__init__()
        self.attn = Attention(c, num_heads)
        self.ffn = nn.Sequential(Conv(c, 2 * c, 1), Conv(2 * c, c, 1, act=False))

    def forward(self, x):
        x = x + self.attn(x)
        return x + self.ffn(x)


class C2PSA(nn.Module):
    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, max(self.c // 64, 1)) for _ in range(n)))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), 1)
        return self.cv2(torch.cat((a, self.m(b)), 1))


class AAttn(nn.Module):
    """YOLO12's area attention: heads of 32 channels, qkv channel h * 96 + [q 32 | k 32 | v 32]; the H * W tokens (row-major)
    are cut into `area` contiguous chunks and attention runs inside a chunk; the depthwise 7x7 positional encoding runs on v
    as the whole map.  [external - recalled from ultralytics 8.3.x nn/modules/block.py, unpinned]"""

    def __init__(self, dim, num_heads, area=1):
        super().__init__()
        self.area, self.num_heads, self.head_dim = area, num_heads, dim // num_heads
        self.qkv = Conv(dim, dim * 3, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 7, 1, g=dim, act=False)

    def forward(self, x):
        b, c, h, w = x.shape
        n, hd, nh = h * w, self.head_dim, self.num_heads
        qkv = self.qkv(x).flatten(2).transpose(1, 2)  # (b, n, 3c)
        if self.area > 1:
            qkv = qkv.reshape(b * self.area, n // self.area, c * 3)
        bb, nn_, _ = qkv.shape
        q, k, v = qkv.view(bb, nn_, nh, hd * 3).permute(0, 2, 3, 1).split([hd, hd, hd], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * (hd**-0.5)).softmax(dim=-1)
        y = (v @ attn.transpose(-2, -1)).permute(0, 3, 1, 2)  # (bb, nn, heads, hd)
        v = v.permute(0, 3, 1, 2)
        y = y.reshape(b, h, w, c).permute(0, 3, 1, 2)
        v = v.reshape(b, h, w, c).permute(0, 3, 1, 2)
        return self.proj(y + self.pe(v.contiguous()))


class ABlock(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=1.2, area=1):
        super().__init__()
        self.attn = AAttn(dim, num_heads, area)
        hidden = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(Conv(dim, hidden, 1), Conv(hidden, dim, 1, act=False))

    def forward(self, x):
        x = x + self.attn(x)
        return x + self.mlp(x)


class A2C2f(nn.Module):
    """cv1 gives ONE chunk of c_ = c2 // 2 channels; n modules - two ABlocks (a2) or C3k(c_, c_, 2) - each appended to the
    concat; cv2 over (1 + n) c_.  residual (scales l, x): x + gamma * out on the a2 blocks."""

    def __init__(self, c1, c2, n=1, a2=True, area=1, residual=False, mlp_ratio=2.0):
        super().__init__()
        c_ = c2 // 2
        assert c_ % 32 == 0, "the hidden width of A2C2f is a multiple of 32"
        self.cv1 = Conv(c1, c_, 1)
        self.cv2 = Conv((1 + n) * c_, c2, 1)
        self.gamma = nn.Parameter(0.01 * torch.ones(c2)) if a2 and residual else None
        self.m = nn.ModuleList(
            nn.Sequential(*(ABlock(c_, c_ // 32, mlp_ratio, area) for _ in range(2))) if a2 else C3k(c_, c_, 2, True) for _ in range(n)
        )

    def forward(self, x):
        y = [self.cv1(x)]
        for m in self.m:
            y.append(m(y[-1]))
        y = self.cv2(torch.cat(y, 1))
        return x + self.gamma.view(1, -1, 1, 1) * y if self.gamma is not None else y


class _DFL(nn.Module):
    def __init__(self, c1=16, as_sum=False):
        """as_sum (YOLO12's Segment head only; YOLOv8 and YOLO11 keep the conv): the same 1x1 conv written as the expectation
        sum(softmax * weight) - the form, and so the float32 summation order, of the Segment decode the YOLO12 mirror is
        checked against to 1e-5 (tests/yolo12_ref.py -> oracle/detector_ref.py: _head_segment; its OBB decode has the conv)"""
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.c1 = c1
        self.as_sum = as_sum

    def forward(self, x):
        b, _, a = x.shape
        if self.as_sum:
            return (x.view(b, 4, self.c1, a).transpose(2, 1).softmax(1) * self.conv.weight.view(1, self.c1, 1, 1)).sum(1)
        return self.conv(x.view(b, 4, self.c1, a).transpose(2, 1).softmax(1)).view(b, 4, a)


class _Proto(nn.Module):
    def __init__(self, c1, c_, c2):
        super().__init__()
        self.cv1 = Conv(c1, c_, 3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, 3)
        self.cv3 = Conv(c_, c2, 1)

    def forward(self, x):
        return self.cv3(self.cv2(self.upsample(self.cv1(x))))


def _make_anchors(cfg: spec.DetectorConfig):
    """anchor centres (2, A) in grid units and strides (1, A): the pixels of cfg.grids row-major, P3 first"""
    pts, st = [], []
    for s, (gh, gw) in zip((8, 16, 32), cfg.grids):
        sy, sx = torch.meshgrid(torch.arange(gh, dtype=torch.float32) + 0.5, torch.arange(gw, dtype=torch.float32) + 0.5, indexing="ij")
        pts.append(torch.stack((sx, sy), -1).view(-1, 2))
        st.append(torch.full((gh * gw, 1), float(s)))
    return torch.cat(pts).T.contiguous(), torch.cat(st).T.contiguous()


class _Detect(nn.Module):
    """what the two heads share: the box branch cv2, the class branch cv3 (either architecture's), the DFL, a cv4 branch
    with `n4` outputs per anchor, and the anchors and strides of cfg.grids.  `proto` (Segment's) is registered between dfl
    and cv4, where the upstream state_dict has it."""

    def __init__(self, cfg: spec.DetectorConfig, ch, n4, proto=None):
        super().__init__()
        self.cfg, self.n4 = cfg, n4
        nc, rm = cfg.nc, cfg.reg_max
        c2 = max(16, ch[0] // 4, rm * 4)
        c3 = max(ch[0], min(nc, 100))
        c4 = max(ch[0] // 4, n4)
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * rm, 1)) for x in ch)
        if cfg.arch in ("11", "12"):
            self.cv3 = nn.ModuleList(
                nn.Sequential(nn.Sequential(Conv(x, x, 3, g=x), Conv(x, c3, 1)), nn.Sequential(Conv(c3, c3, 3, g=c3), Conv(c3, c3, 1)), nn.Conv2d(c3, nc, 1))
                for x in ch
            )
        else:
            self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1)) for x in ch)
        self.dfl = _DFL(rm, as_sum=cfg.arch == "12" and proto is not None)
        if proto is not None:
            self.proto = proto
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, n4, 1)) for x in ch)
        anchors, strides = _make_anchors(cfg)
        self.anchors: torch.Tensor
        self.strides: torch.Tensor
        self.register_buffer("anchors", anchors, persistent=False)
        self.register_buffer("strides", strides, persistent=False)

    def logits(self, feats):
        """(lt, rb) DFL distances (B, 2, A) each, class logits (B, nc, A), cv4 outputs (B, n4, A): levels concatenated, P3 first"""
        cfg = self.cfg
        b = feats[0].shape[0]
        extra = torch.cat([self.cv4[i](f).view(b, self.n4, -1) for i, f in enumerate(feats)], 2)
        x = torch.cat([torch.cat((self.cv2[i](f), self.cv3[i](f)), 1).view(b, 4 * cfg.reg_max + cfg.nc, -1) for i, f in enumerate(feats)], 2)
        box, cls = x.split((4 * cfg.reg_max, cfg.nc), 1)
        lt, rb = self.dfl(box).chunk(2, 1)
        return lt, rb, cls, extra


class Segment(_Detect):
    """Segment head (Detect + prototypes + mask coefficients), inference form"""

    def __init__(self, cfg: spec.DetectorConfig, ch):
        super().__init__(cfg, ch, cfg.nm, proto=_Proto(ch[0], cfg.npr, cfg.nm))

    def forward(self, feats):
        protos = self.proto(feats[0])
        lt, rb, cls, mc = self.logits(feats)
        x1y1, x2y2 = self.anchors.unsqueeze(0) - lt, self.anchors.unsqueeze(0) + rb
        dbox = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * self.strides
        return torch.cat((dbox, cls.sigmoid(), mc), 1), protos


class OBB(_Detect):
    """OBB head (Detect + one angle logit per anchor), inference form: pred (B, 4 + nc + 1, A) = xywh in pixels, class
    sigmoids, angle in radians.  [external - recalled from ultralytics 8.3.x OBB.forward / dist2rbox; unpinned]"""

    def __init__(self, cfg: spec.DetectorConfig, ch):
        super().__init__(cfg, ch, cfg.ne)

    def forward(self, feats):
        lt, rb, cls, angle = self.logits(feats)
        angle = (angle.sigmoid() - 0.25) * torch.pi
        cos, sin = torch.cos(angle), torch.sin(angle)
        xf, yf = ((rb - lt) / 2).split(1, 1)
        xy = torch.cat((xf * cos - yf * sin, xf * sin + yf * cos), 1) + self.anchors.unsqueeze(0)
        dbox = torch.cat((xy, lt + rb), 1) * self.strides
        return torch.cat((dbox, cls.sigmoid(), angle), 1)


class DetectorModule(nn.Module):
    """`self.model` is an nn.ModuleList indexed like ultralytics' `model.model`: same state_dict keys."""

    def __init__(self, cfg: spec.DetectorConfig):
        super().__init__()
        self.cfg = cfg
        graph, feats = spec.detector_graph(cfg)
        self.graph, self.feats = graph, feats
        mods, chans, prev = [], {-1: 3}, 3
        for idx, kind, a in graph:
            if kind == "Conv":
                m, prev = Conv(prev, a[0], a[1], a[2]), a[0]
            elif kind == "C2f":
                m, prev = C2f(prev, a[0], a[1], a[2]), a[0]
            elif kind == "C3k2":
                m, prev = C3k2(prev, a[0], a[1], a[2], a[3]), a[0]
            elif kind == "C2PSA":
                m, prev = C2PSA(prev, a[0], a[1]), a[0]
            elif kind == "A2C2f":
                m, prev = A2C2f(prev, *a), a[0]
            elif kind == "SPPF":
                m, prev = SPPF(prev, a[0]), a[0]
            elif kind == "Upsample":
                m = nn.Upsample(scale_factor=2, mode="nearest")
            elif kind == "Concat":
                m, prev = nn.Identity(), sum(chans[s] for s in a)
            else:
                raise KeyError(kind)
            chans[idx] = prev
            mods.append(m)
        mods.append((OBB if cfg.task == "obb" else Segment)(cfg, [chans[f] for f in feats]))
        self.model = nn.ModuleList(mods)

    def forward(self, x):
        outs = {}
        for (idx, kind, a), m in zip(self.graph, self.model):
            x = torch.cat([outs[s] for s in a], 1) if kind == "Concat" else m(x)
            outs[idx] = x
        return self.model[-1]([outs[f] for f in self.feats])


def to_torch_module(cfg: spec.DetectorConfig, state_dict: Mapping) -> DetectorModule:
    m = DetectorModule(cfg).eval()
    want = spec.detector_param_shapes(cfg)
    sd = {k: torch.as_tensor(np.asarray(state_dict[k]) if not isinstance(state_dict[k], torch.Tensor) else state_dict[k]).float() for k in want}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m


def export_torchscript(cfg: spec.DetectorConfig, state_dict: Mapping, path: str):
    """`torch.jit.trace` of the detector on a (1, 3, in_h, in_w) example, saved to `path`"""
    m = to_torch_module(cfg, state_dict)
    ts = torch.jit.trace(m, torch.rand((1, 3, cfg.in_h, cfg.in_w)))
    ts.save(path)
    return ts


def export_onnx(cfg: spec.DetectorConfig, state_dict: Mapping, path: str):
    """ONNX export (od_export.py:167-171) when the `onnx` package is importable (it is not in the build image)."""
    import importlib.util

    if importlib.util.find_spec("onnx") is None:
        raise RuntimeError("the onnx package is not installed")
    m = to_torch_module(cfg, state_dict)
    ex = torch.rand((1, 3, cfg.in_h, cfg.in_w))
    outs = ["pred"] if cfg.task == "obb" else ["pred", "protos"]
    torch.onnx.export(m, ex, path, input_names=["images"], output_names=outs, dynamic_axes={k: {0: "n"} for k in ["images"] + outs})
