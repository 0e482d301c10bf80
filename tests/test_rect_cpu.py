"""Rectangular detector inputs, the parts that need no GPU: LetterBox(auto=True) geometry, the config's grids and anchor
count, the export mirror on a rectangle, and the oracle (oracle/detector_ref.py) on a square and on a rectangle."""
import numpy as np
import pytest
import torch

from oracle import detector_ref as D
from oracle import resize_ref

# frame (h, w) -> r, (nh, nw), top, left, (out_h, out_w): hand-derived from the formula in rect_geometry's docstring
GEOMETRY = [
    ((480, 640), 1.0, (480, 640), 0, 0, (480, 640)),
    ((720, 1280), 0.5, (360, 640), 12, 0, (384, 640)),
    ((1080, 810), 640 / 1080, (640, 480), 0, 0, (640, 480)),
    ((300, 200), 640 / 300, (640, 427), 0, 10, (640, 448)),
    ((33, 1000), 0.64, (21, 640), 5, 0, (32, 640)),
    ((640, 640), 1.0, (640, 640), 0, 0, (640, 640)),
]


@pytest.mark.parametrize("hw,r,nhw,top,left,out", GEOMETRY)
def test_rect_geometry(hw, r, nhw, top, left, out):
    from mtgv.detector import fit_geometry, letterbox_geometry, rect_geometry

    g = rect_geometry(*hw)
    assert g == (r, nhw[0], nhw[1], top, left, out[0], out[1])
    assert g[5] % 32 == 0 and g[6] % 32 == 0 and max(g[5], g[6]) == 640
    assert g[3] + g[1] <= g[5] and g[4] + g[2] <= g[6]
    # the scale and the resampled size are the square letterbox's, and a handle made for this frame shape letterboxes alike
    assert letterbox_geometry(*hw)[:3] == g[:3]
    assert fit_geometry(hw[0], hw[1], g[5], g[6]) == g[:5]
    assert rect_geometry(*hw, size=640, stride=32) == g


def test_config_square_is_unchanged():
    from mtgv import spec

    for cfg in (spec.DetectorConfig(), spec.yolo11_config(), spec.DetectorConfig(task="obb"), spec.DetectorConfig(imgsz=224)):
        S = cfg.imgsz
        assert cfg.input_hw is None and (cfg.in_h, cfg.in_w) == (S, S)
        assert cfg.grids == ((S // 8, S // 8), (S // 16, S // 16), (S // 32, S // 32))
        assert cfg.num_anchors == sum((S // s) ** 2 for s in (8, 16, 32))
    assert spec.DetectorConfig().num_anchors == 8400
    same = spec.DetectorConfig(input_hw=(640, 640))
    assert same.num_anchors == 8400 and same.grids == spec.DetectorConfig().grids
    # the parameter set does not depend on the input shape
    assert spec.detector_param_shapes(spec.DetectorConfig(input_hw=(480, 640))) == spec.detector_param_shapes(spec.DetectorConfig())


def test_config_rectangle():
    from mtgv import spec

    cfg = spec.DetectorConfig(input_hw=(480, 640))
    assert (cfg.in_h, cfg.in_w) == (480, 640) and cfg.grids == ((60, 80), (30, 40), (15, 20)) and cfg.num_anchors == 6300
    assert spec.yolo11_config(input_hw=(96, 160)).num_anchors == 315
    assert spec.DetectorConfig(task="obb", input_hw=(160, 96)).grids == ((20, 12), (10, 6), (5, 3))
    for bad in ((100, 640), (0, 640), (672, 640), (480,), (480, 640, 3)):
        with pytest.raises(AssertionError):
            spec.DetectorConfig(input_hw=bad)


@pytest.mark.parametrize("arch", ["v8", "11"])
@pytest.mark.parametrize("task", ["seg", "obb"])
def test_export_mirror_on_a_rectangle(arch, task):
    """export_detector's module (anchors from cfg.grids) against the oracle at 96 x 160, float32 both: the two run the same
    torch ops on the same weights, so only the fusion order of a few sums can differ"""
    from mtgv import spec
    from mtgv.export_detector import _make_anchors, to_torch_module

    kw = dict(task=task, input_hw=(96, 160))
    cfg = spec.yolo11_config(**kw) if arch == "11" else spec.DetectorConfig(**kw)
    sd = spec.random_detector_state(cfg, 3, cls_bias=-0.9)
    frames = np.random.default_rng(1000 * 96 + 160).integers(0, 256, (2, 96, 160, 3), dtype=np.uint8)
    assert all(torch.equal(a, b) for a, b in zip(_make_anchors(cfg), D.make_anchors(cfg)))
    ref = D.forward(sd, cfg, frames, flip_rgb=False)
    m = to_torch_module(cfg, sd)
    with torch.no_grad():
        got = m(torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255.0)
    # everything but the box is the same torch ops on the same numbers: the existing export test's 2e-5.  The box differs
    # by the order in which the DFL expectation's 16 products are summed (a conv against a product and sum): a side's
    # distance is <= 15 bins, where float32 is spaced 9.5e-7, and two orders of 16 terms differ by 8 spacings at the most
    # = 7.6e-6 bins; a box coordinate combines two sides and is scaled by the stride, <= 32: 2 x 32 x 7.6e-6 = 4.9e-4 px
    # (8 float32 spacings at the 512 .. 960 px the widest boxes reach).  Observed: 0.9e-4 .. 1.8e-4 px.
    pred, ref_pred = (got, ref) if task == "obb" else (got[0], ref[0])
    assert tuple(pred.shape) == (2, cfg.no, 315)
    box_err = (pred[:, :4] - ref_pred[:, :4]).abs().max().item()
    rest_err = (pred[:, 4:] - ref_pred[:, 4:]).abs().max().item()
    print(f"{arch} {task}: box {box_err:.2e}px rest {rest_err:.2e}")
    assert box_err < 5e-4 and rest_err < 2e-5
    if task == "seg":
        assert tuple(got[1].shape) == (2, 32, 24, 40) and (got[1] - ref[1]).abs().max().item() < 2e-5


@pytest.mark.parametrize("arch", ["v8", "11"])
def test_oracle_on_a_square(arch):
    """imgsz = 64: the segment oracle keeps detections with non-zero mask logits; the OBB oracle's forward gives one
    (2, no, A) tensor in the dtype asked for"""
    from mtgv import spec

    cfg = spec.yolo11_config(imgsz=64) if arch == "11" else spec.DetectorConfig(imgsz=64)
    sd = spec.random_detector_state(cfg, 3, cls_bias=-0.9)
    frames = np.random.default_rng(5).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    dets, pred, protos = D.detect(sd, cfg, frames)
    assert sum(len(d["keep_idx"]) for d in dets) > 4
    for d in dets:
        assert (d["mask_logits"] != 0).any()
    ocfg = spec.yolo11_config(imgsz=64, task="obb") if arch == "11" else spec.DetectorConfig(imgsz=64, task="obb")
    osd = spec.random_detector_state(ocfg, 3, cls_bias=-0.9)
    for dtype in (torch.float32, torch.float64):
        opred = D.forward(osd, ocfg, frames, dtype=dtype)
        assert isinstance(opred, torch.Tensor) and opred.dtype == dtype and tuple(opred.shape) == (2, ocfg.no, ocfg.num_anchors)


def test_rect_shapes_and_letterbox():
    """96 x 160: 315 anchors, prototypes (n, 32, 24, 40); the expected rectangular letterbox of the geometry table's frames"""
    from mtgv import spec

    cfg = spec.DetectorConfig(input_hw=(96, 160))
    sd = spec.random_detector_state(cfg, 3, cls_bias=-0.9)
    frames = np.random.default_rng(1000 * 96 + 160).integers(0, 256, (3, 96, 160, 3), dtype=np.uint8)
    pred, protos = D.forward(sd, cfg, frames)
    assert tuple(pred.shape) == (3, 39, 315) and tuple(protos.shape) == (3, 32, 24, 40)
    # anchors: x runs over the grid's width first; box centres stay near their anchors for this random head
    a, s = D.make_anchors(cfg)
    assert a[0, :20].tolist() == [i + 0.5 for i in range(20)] and a[1, 20] == 1.5 and s[0, 240] == 16 and s[0, 300] == 32
    for hw, r, nhw, top, left, out in GEOMETRY:
        frame = np.random.default_rng(hw[0] * 7 + hw[1]).integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
        img, geo = resize_ref.letterbox_rect(frame)
        assert img.shape == (out[0], out[1], 3)
        inner = np.zeros(img.shape[:2], bool)
        inner[top : top + nhw[0], left : left + nhw[1]] = True
        assert (img[~inner] == 114).all()
        if nhw == hw:
            np.testing.assert_array_equal(img[inner].reshape(hw[0], hw[1], 3), frame)
