"""Rectangular detector inputs on the GPU (`DetectorConfig(input_hw=...)`, mtgv_detector_cfg.in_h / in_w) against
oracle/detector_ref.py: forward, NMS, end to end, mask logits, the rectangular letterbox, and the callers (Detector.detect,
JpegDecoder.decode_frames, CardSegmenter(rect=True), Pipeline).

Square-assumption bugs are swaps of H and W, a grid width used as a height, and an image stride of S x S.  The small
shapes, 96 x 160 and 160 x 96 (grids 12 x 20, 6 x 10, 3 x 5 and transposed: both sides different, H / 32 and W / 32 odd and
coprime) at batch 3 of 4, expose all of them; 480 x 640 and 640 x 480 are what a webcam frame gives (640 x 480 puts the odd
width 15 at P5, under upsample2x, the pools and the attention)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import detector_ref as D
from oracle import obb_ref, resize_ref

pytestmark = pytest.mark.gpu

SMALL = [(96, 160), (160, 96)]
FULL = [(480, 640), (640, 480)]
# Full size: frame seeds and YOLO11's class bias were chosen on the CPU, out of seeds 1000 H + W + 0 .. 13: the oracle in float32
# and in float64 keep identical anchor sets, in the same order, on both frames of every case, the kept counts lie inside
# (10, max_det), and of the candidates the seed with the class score nearest to the 0.25 threshold furthest away was taken.
#   v8 (cls_bias default, -2.1)  480 x 640 seed 480649: kept 212, 149, nearest score 2.4e-5 away
#                                640 x 480 seed 640489: kept 158, 216, 2.0e-5
#   YOLO11 cls_bias -1.7         480 x 640 seed 480641: kept 111, 108, 3.4e-5
#                                640 x 480 seed 640481: kept 30, 60, 1.1e-4
#   (YOLO11 at -0.9 .. -1.5 saturates max_det on noise frames; at -2.1 a frame keeps one detection, at -2.5 none)
FULL_BIAS = {"v8": None, "11": -1.7}
FULL_SEED = {("v8", (480, 640)): 480649, ("v8", (640, 480)): 640489, ("11", (480, 640)): 480641, ("11", (640, 480)): 640481}


def _seed(hw):
    return 1000 * hw[0] + hw[1]


def _cfg(arch, task, hw, **kw):
    from mtgv import spec

    kw = dict(task=task, input_hw=hw, **kw)
    return spec.yolo11_config(**kw) if arch == "11" else spec.DetectorConfig(**kw)


_DETS64 = {}  # the float64 reference's detections of every case (NMS on its pred rounded to float32)


@functools.lru_cache(maxsize=None)
def _case(arch, task, hw, n, bias, seed):
    """(cfg, frames, detector, float64 reference (pred, protos), float32 reference detections): each computed once and
    left unchanged"""
    from mtgv import spec
    from mtgv.detector import Detector

    cfg = _cfg(arch, task, hw)
    sd = spec.random_detector_state(cfg, 3) if bias is None else spec.random_detector_state(cfg, 3, cls_bias=bias)
    frames = np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)
    det = Detector(cfg, sd, max_batch=n + 1 if n == 3 else n)
    dets64, pred64, protos64 = D.detect(sd, cfg, frames, dtype=torch.float64)
    dets32, _, _ = D.detect(sd, cfg, frames)
    _DETS64[arch, task, hw, n] = dets64
    return cfg, frames, det, (pred64, protos64), dets32


def _small(arch, task, hw):
    return _case(arch, task, hw, 3, -0.9, _seed(hw))


def _full(arch, hw):
    return _case(arch, "seg", hw, 2, FULL_BIAS[arch], FULL_SEED[arch, hw])


def _with_mode(mode, fn):
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision(mode)
    try:
        return fn()
    finally:
        native.set_gemm_precision(before)


# ---------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------
def _check_forward(case, mode, tag):
    """raw outputs against the float64 reference: class scores, coefficients / angle and prototypes within 1e-4 (the
    project's figure, BASELINE.json), box coordinates within max(in_h, in_w) * 1e-4 px"""
    cfg, frames, det, (ref_pred, ref_protos), _ = case
    n = len(frames)

    def run():
        det.forward(torch.from_numpy(frames).cuda(), True, 0)
        return det.raw_outputs(n)

    pred, protos = _with_mode(mode, run)
    assert tuple(pred.shape) == (n, cfg.no, cfg.num_anchors)
    pred = pred.cpu().numpy().astype(np.float64)
    nc = cfg.nc
    box_err = np.abs(pred[:, :4] - ref_pred[:, :4]).max()
    cls_err = np.abs(pred[:, 4 : 4 + nc] - ref_pred[:, 4 : 4 + nc]).max()
    rest_err = np.abs(pred[:, 4 + nc :] - ref_pred[:, 4 + nc :]).max()
    if cfg.task == "obb":
        assert protos is None
        proto_err = 0.0
    else:
        assert tuple(protos.shape) == (n, cfg.nm, cfg.in_h // 4, cfg.in_w // 4)
        proto_err = np.abs(protos.cpu().numpy().astype(np.float64) - ref_protos).max()
    print(f"{tag} {mode}: box {box_err:.2e}px cls {cls_err:.2e} coef/angle {rest_err:.2e} protos {proto_err:.2e}")
    assert np.isfinite(pred).all()
    assert cls_err < 1e-4 and rest_err < 1e-4 and proto_err < 1e-4
    assert box_err < max(cfg.in_h, cfg.in_w) * 1e-4


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("hw", SMALL)
@pytest.mark.parametrize("task", ["seg", "obb"])
@pytest.mark.parametrize("arch", ["v8", "11"])
def test_forward_small(arch, task, hw, mode):
    _check_forward(_small(arch, task, hw), mode, f"{arch} {task} {hw}")


# ---------------------------------------------------------------------------
# 2. NMS
# ---------------------------------------------------------------------------
def _forward_np(case, mask_rows=0):
    cfg, frames, det, _, _ = case
    out = det.forward(torch.from_numpy(frames).cuda(), True, mask_rows)
    pred, protos = det.raw_outputs(len(frames))
    o = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
    return o, pred.cpu().numpy(), None if protos is None else protos.cpu().numpy()


def _check_nms_and_end_to_end(case, tag):
    """(2) the NMS kernel is bit-exact on the predictions it was given; (3) end to end against the float32 reference, the
    pattern of tests/test_gpu_detector.py: at most one threshold flip per frame (a condition, not a measurement: the
    reference's decisions are far from every threshold on these inputs), order moves at most 1 + flips, k > 10"""
    from oracle import detector_ref as D

    cfg, frames, det, _, ref_dets = case
    o, pred, _ = _forward_np(case)
    bkey = "rboxes" if cfg.task == "obb" else "boxes"
    for i in range(len(frames)):
        k = int(o["n_det"][i])
        if cfg.task == "obb":
            same_in = obb_ref.nms_rotated_single(pred[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        else:
            same_in = D.nms_single(pred[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        assert k == len(same_in["keep_idx"])
        np.testing.assert_array_equal(o["keep_idx"][i, :k], same_in["keep_idx"])
        np.testing.assert_array_equal(o["cls"][i, :k], same_in["cls"])
        np.testing.assert_array_equal(o[bkey][i, :k], same_in[bkey])
        ref = ref_dets[i]
        got_idx, ref_idx = o["keep_idx"][i, :k], ref["keep_idx"]
        common = np.intersect1d(got_idx, ref_idx)
        flips = max(k, len(ref_idx)) - len(common)
        print(f"{tag} frame {i}: kept {k} (reference {len(ref_idx)}), threshold flips {flips}")
        assert k > 10 and flips <= 1
        assert k < cfg.max_det and got_idx.max() < cfg.num_anchors
        gi = {a: j for j, a in enumerate(got_idx)}
        ri = {a: j for j, a in enumerate(ref_idx)}
        gsel = np.asarray([gi[a] for a in common])
        rsel = np.asarray([ri[a] for a in common])
        assert (np.diff(o["conf"][i, :k]) <= 0).all()
        assert np.abs(gsel - rsel).max() <= 1 + flips
        np.testing.assert_array_equal(o["cls"][i, :k][gsel], ref["cls"][rsel])
        assert np.abs(o["conf"][i, :k][gsel] - ref["conf"][rsel]).max() < 1e-4
        if cfg.task == "obb":
            assert np.abs(o[bkey][i, :k][gsel][:, :4] - ref[bkey][rsel][:, :4]).max() < max(cfg.in_h, cfg.in_w) * 1e-4
            assert np.abs(o[bkey][i, :k][gsel][:, 4] - ref[bkey][rsel][:, 4]).max() < 1e-4
        else:
            assert np.abs(o[bkey][i, :k][gsel] - ref[bkey][rsel]).max() < max(cfg.in_h, cfg.in_w) * 1e-4
            # boxes are pixels of the in_h x in_w frame: kept boxes of noise frames reach into both halves of either axis
            b = o[bkey][i, :k]
            cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
            assert cx.max() > cfg.in_w / 2 and cy.max() > cfg.in_h / 2 and cx.max() < cfg.in_w + 64 and cy.max() < cfg.in_h + 64


@pytest.mark.parametrize("hw", SMALL)
@pytest.mark.parametrize("task", ["seg", "obb"])
@pytest.mark.parametrize("arch", ["v8", "11"])
def test_nms_and_end_to_end_small(arch, task, hw):
    _check_nms_and_end_to_end(_small(arch, task, hw), f"{arch} {task} {hw}")


def _synthetic_rows(grids, n, nc, nm, seed):
    """raw head rows (n, gh * gw, 128) per level in the detector's layout: box logits peaked on bin 2 of every side (a box
    4 strides wide centred on its anchor), random class logits and coefficients"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for gh, gw in grids:
        r = torch.zeros((n, gh * gw, 128))
        r[..., :64] = torch.randn((n, gh * gw, 64), generator=g) * 0.1
        r[..., :64].view(n, gh * gw, 4, 16)[..., 2] += 14.0
        r[..., 96 : 96 + nc] = torch.randn((n, gh * gw, nc), generator=g) * 2.0 - 2.0
        r[..., 64 : 64 + nm] = torch.randn((n, gh * gw, nm), generator=g)
        rows.append(r.cuda().contiguous())
    return rows


def _decode_and_nms_raw(rows, imgsz, h, w, n, nc, nm, na, max_det=300):
    from mtgv import native as nv
    from mtgv.detector import nms

    L = nv.lib()
    hr = nv.HeadRows(rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), imgsz, 128, 96, 64, h, w)
    pred = torch.full((n, 4 + nc + nm, na), float("nan"), device="cuda")
    nv.check(L.mtgv_op_decode(C.byref(hr), n, nc, nm, nv.ptr(pred), nv.stream()))
    ref = nms(pred, nc, 0.25, 0.7, max_det, 7680.0)
    ws = torch.empty((int(L.mtgv_nms_workspace_bytes(n, na)) + 3) // 4, dtype=torch.int32, device="cuda")
    got = {
        "n_det": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
        "boxes": torch.full((n, max_det, 4), float("nan"), device="cuda"),
        "conf": torch.full((n, max_det), float("nan"), device="cuda"),
        "cls": torch.full((n, max_det), -7, dtype=torch.int32, device="cuda"),
        "keep_idx": torch.full((n, max_det), -7, dtype=torch.int32, device="cuda"),
    }
    nv.check(L.mtgv_op_nms_raw(C.byref(hr), n, nc, nm, 0.25, 0.7, max_det, 7680.0, nv.ptr(got["n_det"]), nv.ptr(got["boxes"]),
                               nv.ptr(got["conf"]), nv.ptr(got["cls"]), nv.ptr(got["keep_idx"]), None, nv.ptr(ws), ws.numel() * 4, nv.stream()))
    torch.cuda.synchronize()
    return pred, ref, got


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("hw", SMALL)
def test_head_rows_on_a_rectangle(hw):
    """mtgv_op_decode -> mtgv_nms equals mtgv_op_nms_raw bit for bit with h, w set, and every anchor's box sits on its own
    grid position: level by level, x over the grid's width, y over its height"""
    from mtgv import spec

    cfg = spec.DetectorConfig(input_hw=hw)
    n, nc, nm, na = 2, 3, 32, cfg.num_anchors
    rows = _synthetic_rows(cfg.grids, n, nc, nm, _seed(hw))
    pred, ref, got = _decode_and_nms_raw(rows, 640, hw[0], hw[1], n, nc, nm, na)
    anchors, strides = D.make_anchors(cfg)
    centres = (anchors * strides).numpy()  # (2, na) pixels
    p = pred.cpu().numpy()
    assert np.isfinite(p).all()
    # a peaked DFL puts every side at 2 bins up to exp(-14): centre = anchor centre, width = height = 4 strides
    assert np.abs(p[:, 0] - centres[0]).max() < 1e-2 and np.abs(p[:, 1] - centres[1]).max() < 1e-2
    assert np.abs(p[:, 2] - 4 * strides.numpy()[0]).max() < 1e-2 and np.abs(p[:, 3] - 4 * strides.numpy()[0]).max() < 1e-2
    a0 = 0
    for lvl, (gh, gw) in enumerate(cfg.grids):  # rows, class scores and coefficients come from the level's own rows
        sl = slice(a0, a0 + gh * gw)
        np.testing.assert_array_equal(p[:, 4 + nc :, sl], rows[lvl][..., 64 : 64 + nm].cpu().numpy().transpose(0, 2, 1))
        a0 += gh * gw
    assert int(ref["n_det"].min()) > 5
    for key in ("n_det", "boxes", "conf", "cls", "keep_idx"):
        assert torch.equal(_bits(got[key]), _bits(ref[key])), f"{hw}: {key} differs between the row form and decode -> nms"


def test_head_rows_zero_hw_is_the_square():
    """a HeadRows with h = w = 0 behaves as before: the square imgsz grid, the bits of h = w = imgsz; bad shapes: status 1"""
    from mtgv import native as nv
    from mtgv import spec

    cfg = spec.DetectorConfig(imgsz=96)
    n, nc, nm, na = 2, 3, 32, cfg.num_anchors
    rows = _synthetic_rows(cfg.grids, n, nc, nm, 7)
    p0, r0, g0 = _decode_and_nms_raw(rows, 96, 0, 0, n, nc, nm, na)
    p1, r1, g1 = _decode_and_nms_raw(rows, 96, 96, 96, n, nc, nm, na)
    assert torch.equal(_bits(p0), _bits(p1)) and int(r0["n_det"].min()) > 5
    for key in ("n_det", "boxes", "conf", "cls", "keep_idx"):
        assert torch.equal(_bits(g0[key]), _bits(r0[key])) and torch.equal(_bits(g1[key]), _bits(g0[key]))
    hr = nv.HeadRows(rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), 96, 128, 96, 64, 96, 0)
    with pytest.raises(AssertionError, match="head rows"):
        nv.check(nv.lib().mtgv_op_decode(C.byref(hr), n, nc, nm, nv.ptr(p0), nv.stream()))
    hr = nv.HeadRows(rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), 96, 128, 96, 64, 100, 96)
    with pytest.raises(AssertionError, match="head rows"):
        nv.check(nv.lib().mtgv_op_decode(C.byref(hr), n, nc, nm, nv.ptr(p0), nv.stream()))


# ---------------------------------------------------------------------------
# 4. mask logits
# ---------------------------------------------------------------------------
def _check_masks(case, mask_rows, tag):
    """(k, in_h / 4, in_w / 4): within 1e-4 of the reference's, within 2e-5 of the oracle's mask_logits on the GPU's own pred and
    protos, not all zero; rows beyond n_det are zeros"""
    from oracle import detector_ref as D

    cfg, frames, det, _, ref_dets = case
    o, pred, protos = _forward_np(case, mask_rows)
    mh, mw = cfg.in_h // 4, cfg.in_w // 4
    assert o["mask_logits"].shape == (len(frames), mask_rows, mh, mw)
    for i in range(len(frames)):
        k = int(o["n_det"][i])
        kk = min(k, mask_rows)
        same_in = D.nms_single(pred[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        first = {key: v[:kk] for key, v in same_in.items()}
        ml = o["mask_logits"][i, :kk]
        same = D.mask_logits(pred[i], protos[i], first, cfg.nc, (cfg.in_h, cfg.in_w))
        own_err = np.abs(ml - same).max()
        ref = ref_dets[i]
        ri = {a: j for j, a in enumerate(ref["keep_idx"])}
        pairs = [(j, ri[a]) for j, a in enumerate(same_in["keep_idx"][:kk]) if a in ri]
        gsel, rsel = np.asarray([p[0] for p in pairs]), np.asarray([p[1] for p in pairs])
        ref_err = np.abs(ml[gsel] - ref["mask_logits"][rsel]).max()
        print(f"{tag} mask_rows {mask_rows} frame {i}: {kk} masks, vs own pred {own_err:.2e}, vs reference {ref_err:.2e}")
        assert len(pairs) >= kk - 1 and kk > 10
        assert own_err < 2e-5 and ref_err < 1e-4
        assert (ml != 0).any() and (o["mask_logits"][i, kk:] == 0).all()
        # the crop follows the box in both directions: no logit outside the box scaled by 1/4
        b = same_in["boxes"][:kk] / 4
        ys, xs = np.arange(mh)[None, :, None], np.arange(mw)[None, None, :]
        outside = (xs < np.floor(b[:, 0])[:, None, None]) | (xs > np.ceil(b[:, 2])[:, None, None]) | (ys < np.floor(b[:, 1])[:, None, None]) | (
            ys > np.ceil(b[:, 3])[:, None, None])
        assert (ml[np.broadcast_to(outside, ml.shape)] == 0).all()


@pytest.mark.parametrize("mask_rows", [16, 300])  # <= 16: mask_logits_kernel; above: the batched GEMM with the crop epilogue
@pytest.mark.parametrize("hw", SMALL)
@pytest.mark.parametrize("arch", ["v8", "11"])
def test_mask_logits_small(arch, hw, mask_rows):
    _check_masks(_small(arch, "seg", hw), mask_rows, f"{arch} {hw}")


# ---------------------------------------------------------------------------
# 5. full size, batch 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", FULL)
@pytest.mark.parametrize("arch", ["v8", "11"])
def test_full_size(arch, hw):
    case = _full(arch, hw)
    cfg, frames, det, _, ref_dets = case
    assert all(10 < len(d["keep_idx"]) < cfg.max_det for d in ref_dets)
    # what the named seeds were chosen for: the reference keeps the same anchors, in the same order, in float32 and float64
    for d32, d64 in zip(ref_dets, _DETS64[arch, "seg", hw, 2]):
        np.testing.assert_array_equal(d32["keep_idx"], d64["keep_idx"])
    _check_forward(case, "f16x3", f"{arch} {hw}")
    _check_nms_and_end_to_end(case, f"{arch} {hw}")
    _check_masks(case, cfg.max_det, f"{arch} {hw}")
    if arch == "v8" and hw == (480, 640):
        # exactly 0.75 of the square graph's 11_342_592_000: every layer's M scales with the pixel count
        assert det.flops_per_frame() == 8_506_944_000.0


# ---------------------------------------------------------------------------
# 6. unchanged square
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [640, 224])
@pytest.mark.parametrize("arch,task", [("v8", "seg"), ("11", "seg"), ("v8", "obb")])
def test_square_handle_is_unchanged(arch, task, S):
    """input_hw=(S, S) and input_hw=None are the same handle: bit-identical n_det, boxes, keep_idx, mask_logits and raw outputs
    on the same frames.  640 is the size whose launches are the full-size forms (the fused C2f tail, the 160-column head
    tile on 80-wide maps, 400 attention tokens, the pools out of LDS); 224 (28 / 14 / 7 maps) takes their fallbacks."""
    from mtgv import spec
    from mtgv.detector import Detector

    frames = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (3, S, S, 3), dtype=np.uint8)).cuda()
    outs = []
    for hw in (None, (S, S)):
        cfg = _cfg(arch, task, hw, imgsz=S)
        det = Detector(cfg, spec.random_detector_state(cfg, 3, cls_bias=-0.9), max_batch=4)
        o = det.forward(frames, True, 0 if task == "obb" else cfg.max_det)
        pred, _ = det.raw_outputs(3)
        outs.append((o, pred, det.flops_per_frame()))
    (a, pa, fa), (b, pb, fb) = outs
    assert fa == fb and int(a["n_det"].min()) > 10
    assert torch.equal(_bits(pa), _bits(pb))
    for key in a:
        assert torch.equal(_bits(a[key]), _bits(b[key])), key


# ---------------------------------------------------------------------------
# 7. letterbox
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(480, 640), (720, 1280), (1080, 810), (300, 200), (33, 1000), (640, 640)])
def test_letterbox_rect_kernel_bit_exact(h, w):
    """mtgv_letterbox_rect_u8 on a batch of 3 same-sized frames against resize_ref.letterbox_rect, every byte"""
    from mtgv import native as nv
    from mtgv.detector import letterbox_device, rect_geometry

    frames = np.random.default_rng(h * 7 + w).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    r, nh, nw, top, left, out_h, out_w = rect_geometry(h, w)
    src = torch.from_numpy(frames).cuda()
    dst = torch.full((3, out_h, out_w, 3), 7, dtype=torch.uint8, device="cuda")
    nv.check(nv.lib().mtgv_letterbox_rect_u8(nv.ptr(src), 3, h, w, nv.ptr(dst), out_h, out_w, nh, nw, top, left, 114, nv.stream()))
    got = dst.cpu().numpy()
    for i in range(3):
        ref, geo = resize_ref.letterbox_rect(frames[i])
        np.testing.assert_array_equal(got[i], ref)
        if (nh, nw) == (h, w):
            np.testing.assert_array_equal(got[i, top : top + nh, left : left + nw], frames[i])
    # the Python form on top of it, and the pad-only entry point: the same bytes around an image someone else wrote
    got2, r2, (left2, top2) = letterbox_device(src, (out_h, out_w))
    assert (r2, left2, top2) == (r, left, top) and torch.equal(got2, dst)
    pad = torch.full((3, out_h, out_w, 3), 7, dtype=torch.uint8, device="cuda")
    nv.check(nv.lib().mtgv_letterbox_pad_rect_u8(nv.ptr(pad), 3, out_h, out_w, nh, nw, top, left, 114, nv.stream()))
    pad = pad.cpu().numpy()
    inner = np.zeros((out_h, out_w), bool)
    inner[top : top + nh, left : left + nw] = True
    assert (pad[:, inner] == 7).all() and (pad[:, ~inner] == 114).all()
    with pytest.raises(AssertionError, match="letterbox"):  # an image taller than its frame
        nv.check(nv.lib().mtgv_letterbox_rect_u8(nv.ptr(src), 3, h, w, nv.ptr(dst), out_h, out_w, out_h + 1, nw, top, left, 114, nv.stream()))


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_rect_errors():
    from mtgv import native as nv
    from mtgv import spec
    from mtgv.detector import Detector

    def create(in_h, in_w, imgsz=640):
        c = nv.DetectorCfg()
        c.nc, c.imgsz, c.max_batch, c.conf, c.iou, c.max_det, c.arch, c.task = 3, imgsz, 1, 0.25, 0.7, 300, 8, 0
        c.in_h, c.in_w = in_h, in_w
        h = nv.c_vp(0)
        try:
            nv.check(nv.lib().mtgv_detector_create(C.byref(c), C.byref(h)))
        finally:
            if h.value:
                nv.lib().mtgv_detector_destroy(h)

    create(0, 0)
    create(96, 160)
    for in_h, in_w in ((100, 640), (480, 0), (0, 640), (672, 640), (640, 672), (-32, 640)):
        with pytest.raises(AssertionError, match="in_h"):
            create(in_h, in_w)
    cfg = spec.DetectorConfig(input_hw=(96, 160))
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=2)
    for shape in ((1, 160, 96, 3), (1, 640, 640, 3), (1, 96, 160, 4), (96, 160, 3)):
        with pytest.raises(AssertionError, match="expected"):
            det.forward(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    with pytest.raises(AssertionError):
        det.forward(torch.zeros((3, 96, 160, 3), dtype=torch.uint8, device="cuda"))  # beyond max_batch


# ---------------------------------------------------------------------------
# 8. callers
# ---------------------------------------------------------------------------
def _noise_720p(seed):
    """a 720 x 1280 frame of 2 x 2 blocks of noise: its half-size bilinear resample (align_corners = False: the mean of two
    equal pixels in each direction) is the 360 x 640 noise itself, so the detector sees noise, not its blur"""
    small = np.random.default_rng(seed).integers(0, 256, (360, 640, 3), dtype=np.uint8)
    return np.ascontiguousarray(small.repeat(2, axis=0).repeat(2, axis=1))


def test_detect_equals_forward_on_a_fitting_frame():
    """Detector.detect on a 480 x 640 frame through a (480, 640) handle: the letterbox is the identity, so it equals forward
    on the raw frame, bit for bit; a 720 x 1280 frame through a (384, 640) handle equals forward on resize_ref's letterbox_rect"""
    cfg, frames, det, _, _ = _full("v8", (480, 640))
    d = det.detect(frames[0])
    o = det.forward(torch.from_numpy(frames[:1]).cuda(), True, cfg.max_det)
    k = int(o["n_det"][0])
    assert k > 10 and d.mask_logits.shape == (k, 120, 160)
    assert torch.equal(d.keep_idx, o["keep_idx"][0, :k].long()) and torch.equal(_bits(d.boxes_xyxy), _bits(o["boxes"][0, :k]))
    assert torch.equal(_bits(d.mask_logits), _bits(o["mask_logits"][0, :k]))

    from mtgv import spec
    from mtgv.detector import Detector

    cfg2 = spec.DetectorConfig(input_hw=(384, 640))
    det2 = Detector(cfg2, spec.random_detector_state(cfg2, 3), max_batch=1)
    frame = _noise_720p(720 * 7 + 1280)
    img, geo = resize_ref.letterbox_rect(frame)
    assert img.shape == (384, 640, 3) and np.array_equal(img[12:372], frame[::2, ::2]) and (img[:12] == 114).all()
    d2 = det2.detect(frame, masks=False)
    pred_detect, _ = det2.raw_outputs(1)
    o2 = det2.forward(torch.from_numpy(img[None]).cuda(), True, 0)
    pred_forward, _ = det2.raw_outputs(1)
    k2 = int(o2["n_det"][0])
    assert torch.equal(_bits(pred_detect), _bits(pred_forward))
    assert k2 > 10 and torch.equal(d2.keep_idx, o2["keep_idx"][0, :k2].long()) and torch.equal(_bits(d2.boxes_xyxy), _bits(o2["boxes"][0, :k2]))


def test_decode_frames_into_a_rectangle():
    """decode_frames(input_hw=(480, 640)) of 640 x 480 JPEGs is Pillow's decode, every byte: the frame is decoded straight
    into the detector's input and no pad is written anywhere; other sizes are scaled to fit and centred"""
    import io

    pytest.importorskip("PIL")
    from PIL import Image

    from mtgv.detector import letterbox_device
    from mtgv.jpeg import JpegDecoder, JpegFrames

    def jpeg(h, w, seed):
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255 // (w - 1)), (y * 255 // (h - 1)), (x * 3 + y * 5 + seed * 40) % 256], -1).astype(np.uint8)
        a[h // 4 : h // 2, w // 3 : w // 2] = np.random.default_rng(seed).integers(0, 256, (h // 2 - h // 4, w // 2 - w // 3, 3), dtype=np.uint8)
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", quality=85, subsampling=2)
        return b.getvalue()

    def pil(d):
        return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))

    dec = JpegDecoder(8, 8 << 20, 8 << 20)
    datas = [jpeg(480, 640, s) for s in range(3)]
    out = torch.full((3, 480, 640, 3), 7, dtype=torch.uint8, device="cuda")
    got = dec.decode_frames(datas, out=out, input_hw=(480, 640))
    assert got.data_ptr() == out.data_ptr()
    for i, d in enumerate(datas):
        np.testing.assert_array_equal(got[i].cpu().numpy(), pil(d))
    # the square form of the same frames is this image between two pads of 80 rows
    sq = dec.decode_frames(datas)
    assert torch.equal(sq[:, 80:560], got) and (sq[:, :80] == 114).all() and (sq[:, 560:] == 114).all()
    # other sizes: 720p into (384, 640) is resampled, a 320 x 640 frame is decoded in place between two pads of 32 rows
    mixed = [jpeg(720, 1280, 5), jpeg(320, 640, 6), jpeg(384, 640, 7)]
    got = dec.decode_frames(mixed, input_hw=(384, 640))
    for i, d in enumerate(mixed):
        ref, _, _ = letterbox_device(torch.from_numpy(pil(d)).cuda(), (384, 640))
        assert torch.equal(got[i], ref[0]), i
    assert (got[1, :32] == 114).all() and (got[1, 352:] == 114).all() and np.array_equal(got[1, 32:352].cpu().numpy(), pil(mixed[1]))
    # the lease form feeds a rectangular detector's batches
    src = JpegFrames([datas[:2]], "cuda", input_hw=(480, 640), decoder=dec)
    lease = next(iter(src.leases(1)))
    t = lease.tensor()
    torch.cuda.synchronize()
    assert tuple(t.shape) == (2, 480, 640, 3) and np.array_equal(t[1].cpu().numpy(), pil(datas[1]))


def _card_mask(quad, h, w):
    """binary mask of a convex quadrilateral with a bite out of its bottom edge (the reference's U-shaped card masks)"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.ones((h, w), bool)
    q = np.asarray(quad, np.float64)
    for i in range(4):
        a, b = q[i], q[(i + 1) % 4]
        m &= (b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0]) >= 0
    c = (q[2] + q[3]) / 2
    m &= ~(((xx - c[0]) ** 2 + (yy - c[1]) ** 2) < 24**2)
    return m


def test_card_segmenter_rect(monkeypatch):
    """CardSegmenter(rect=True): one lazily built handle per rectangle, points in the caller's frame"""
    from mtgv import spec
    from mtgv.adapters import CardSegmenter
    from mtgv.detector import Detections, Detector

    cfg = spec.DetectorConfig()
    sd = spec.random_detector_state(cfg, 3)
    seg = CardSegmenter(state_dict=sd, contours=False, rect=True)
    assert seg.yolo is None and len(seg._rect_handles) == 0
    with pytest.raises(AssertionError):
        CardSegmenter(detector=_full("v8", (480, 640))[2], rect=True)
    rng = np.random.default_rng(21)
    for (h, w), key in (((480, 640), (480, 640)), ((720, 1280), (384, 640)), ((480, 640), (480, 640))):
        frame = _noise_720p(5) if h == 720 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        cards = seg(frame)
        assert seg.yolo.cfg.input_hw == key and list(seg._rect_handles)[-1] == key
        assert len(cards) > 5
        for c in cards:
            p = np.asarray(c.points)
            assert p.shape == (4, 2) and p[:, 0].min() >= 0 and p[:, 0].max() <= w and p[:, 1].min() >= 0 and p[:, 1].max() <= h
        allp = np.concatenate([np.asarray(c.points) for c in cards])
        assert allp[:, 0].max() > w / 2 and allp[:, 1].max() > h / 2  # (frame coordinates, not the network's)
    assert list(seg._rect_handles) == [(384, 640), (480, 640)]  # two handles, the last used last
    # the least recently used handle is dropped beyond RECT_HANDLES
    for h, w in ((640, 480), (200, 300), (300, 200)):
        seg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    assert len(seg._rect_handles) == CardSegmenter.RECT_HANDLES and (384, 640) not in seg._rect_handles

    # A frame with a few drawn card rectangles.  Random weights know no cards, so the detections are drawn too: every handle
    # reports the same three cards, each in the coordinates of its own letterboxed input (the pattern of
    # tests/test_gpu_adapters.py: test_card_segmenter_outline_from_the_device).  The square and the rectangular segmenter
    # must then agree on the number of cards and on where they are in the caller's 480 x 640 frame.
    quads = [[(60, 40), (200, 60), (180, 260), (40, 240)], [(300, 200), (420, 190), (440, 380), (310, 400)], [(480, 60), (600, 70), (590, 250), (470, 240)]]

    def fake_detect(self, frame, flip_rgb=True, masks=True):
        H, W = self.cfg.in_h, self.cfg.in_w
        top = (H - 480) // 2  # 80 rows of pad in the square input, none in the rectangle
        qs = [[(x, y + top) for x, y in q] for q in quads]
        big = torch.from_numpy(np.where(np.stack([_card_mask(q, H, W) for q in qs]), 4.0, -4.0).astype(np.float32))[:, None]
        logits = torch.nn.functional.avg_pool2d(big, 4)[:, 0].cuda().contiguous()
        boxes = torch.tensor([[min(p[0] for p in q), min(p[1] for p in q), max(p[0] for p in q), max(p[1] for p in q)] for q in qs],
                             dtype=torch.float32, device="cuda")
        z = torch.zeros(3, dtype=torch.int64, device="cuda")
        return Detections(boxes, torch.tensor([0.9, 0.8, 0.7], device="cuda"), z, z, logits)

    monkeypatch.setattr(Detector, "detect", fake_detect)
    frame = np.zeros((480, 640, 3), np.uint8)
    for contours in (False, "trace"):
        sq = CardSegmenter(state_dict=sd, contours=contours)(frame)
        rc = CardSegmenter(state_dict=sd, contours=contours, rect=True)(frame)
        assert len(sq) == len(rc) == 3
        for a, b, q in zip(sq, rc, quads):
            ca, cb = np.asarray(a.xyxyxyxy, float), np.asarray(b.xyxyxyxy, float)
            assert np.abs(ca - cb).max() <= 1.5, (ca, cb)
            assert np.abs(cb - np.asarray(q, float)).max() <= 6.0, (cb, q)  # the drawn corners (mask grid: 4 px), corner 0 top-left
    # a rectangular handle handed over as detector= maps back with its own geometry (no pad rows here), not the square's
    own = CardSegmenter(detector=Detector(spec.DetectorConfig(input_hw=(480, 640)), None, max_batch=1), contours=False)(frame)
    assert len(own) == 3
    for b, q in zip(own, quads):
        assert np.abs(np.asarray(b.xyxyxyxy, float) - np.asarray(q, float)).max() <= 6.0, (b.xyxyxyxy, q)


@pytest.mark.parametrize("quad_source", ["mask", "obb"])
def test_pipeline_on_a_rectangle(quad_source):
    """Pipeline with a (480, 640) detector, F = 2, K = 4: the crops are warp_quads of the quads it reports, in the frame's own
    pixels; with nothing detected every slot is a pad box, scaled into the rectangle"""
    from mtgv import spec
    from mtgv.crop import mask_quads_from_logits, warp_quads
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline

    F, K = 2, 4
    task = "obb" if quad_source == "obb" else "seg"
    cfg = spec.DetectorConfig(task=task, input_hw=(480, 640))
    ecfg = spec.EncoderConfig("ae", (192, 128), 3, 48, (1, 1, 1, 1), (8, 16, 32, 64), "pool+linear", True)
    enc = Encoder(ecfg, spec.random_encoder_state(ecfg, 1), max_batch=F * K)
    m = Matcher(48, capacity=16)
    m.add(np.random.default_rng(1).standard_normal((16, 48)).astype(np.float32))
    frames = torch.from_numpy(np.random.default_rng(480640).integers(0, 256, (F, 480, 640, 3), dtype=np.uint8)).cuda()
    pipe = Pipeline(Detector(cfg, spec.random_detector_state(cfg, 3, cls_bias=-0.9), max_batch=F), enc, m, K, 1, quad_source=quad_source)
    o = pipe.run(frames)
    torch.cuda.synchronize()
    assert int(o["n_det"].min()) >= K and o["crops"].shape == (F * K, 192, 128, 3) and o["ids"].shape == (F, K, 1)
    fidx = torch.arange(F, dtype=torch.int32, device="cuda").repeat_interleave(K)
    if quad_source == "obb":
        quads = o["quads"].reshape(F * K, 4, 2)
        assert (o["card_state"] > 0).any()
    else:
        ml = o["det"]["mask_logits"]
        assert tuple(ml.shape) == (F, K, 120, 160)
        assert torch.equal(o["boxes"], o["det"]["boxes"][:, :K])
        quads, ok = mask_quads_from_logits(ml.reshape(F * K, 120, 160), o["boxes"].reshape(F * K, 4))
        assert int(ok.sum()) > 0
    assert torch.equal(o["crops"], warp_quads(frames, quads, fidx, (192, 128), 0.05))
    b = o["boxes"].reshape(-1, 4)
    # the frame's own pixels.  A box's centre is its anchor's, inside the frame, plus the DFL offset ((r - l) / 2, (b - t) / 2)
    # stride - at most 7.5 bins x 32 px = 240 px per axis, turned by the angle on an OBB handle: 240 sqrt(2) < 340 px.  (The
    # sides themselves reach 30 bins x 32 px with random weights, so the boxes' bounds say nothing.)
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    assert cx.min() > -340 and cx.max() < 640 + 340 and cy.min() > -340 and cy.max() < 480 + 340
    assert (o["crops"].float().std(dim=(1, 2, 3)) > 1).all()  # crops of noise, not of a border

    # nothing detected: the pad boxes, today's numbers scaled by (in_w / imgsz, in_h / imgsz) = (1, 0.75)
    quiet = Pipeline(Detector(cfg, spec.random_detector_state(cfg, 3, cls_bias=-12.0), max_batch=F), enc, m, K, 1, quad_source=quad_source)
    q = quiet.run(frames)
    torch.cuda.synchronize()
    assert (q["n_det"] == 0).all()
    pb = q["boxes"].cpu()
    want = torch.tensor([[40.0, 45.0, 168.0, 189.0], [200.0, 45.0, 328.0, 189.0], [360.0, 45.0, 488.0, 189.0], [500.0, 45.0, 628.0, 189.0]])
    assert torch.equal(pb[0], want) and torch.equal(pb[1], want)
    assert pb[..., 0].min() >= 0 and pb[..., 1].min() >= 0 and pb[..., 2].max() <= 640 and pb[..., 3].max() <= 480
    # (all eight pad boxes: the second row ends at 522 * 0.75 = 391.5 <= 480)
    p8 = Pipeline(Detector(cfg, None, max_batch=1), enc, m, 8, 1, quad_source=quad_source)._pad.cpu()
    assert p8[:, 3].max() == 391.5 and p8[:, 2].max() == 628.0
    # a square handle keeps today's numbers
    sq_cfg = spec.DetectorConfig(task=task)
    assert Pipeline(Detector(sq_cfg, None, max_batch=1), enc, m, 8, 1, quad_source=quad_source)._pad.cpu()[:, 3].max() == 522.0
