"""CPU: the OBB family's key tables, the restatement the GPU tests compare against (oracle/obb_ref.py: ProbIoU, the
not-greedy rotated NMS rule, this project's card-orientation rule) and the export mirror of the OBB head.  The arithmetic
is ultralytics 8.3.x's as recalled - unpinned."""
import numpy as np
import pytest
import torch

from mtgv import spec
from oracle import obb_ref as R


def _cfg(arch, **kw):
    return spec.yolo11_config(task="obb", **kw) if arch == "11" else spec.DetectorConfig(task="obb", **kw)


@pytest.mark.parametrize("arch", ["v8", "11"])
def test_obb_key_tables(arch):
    cfg = _cfg(arch)
    assert cfg.no == 4 + cfg.nc + 1 and cfg.head_index == (23 if arch == "11" else 22)
    want = spec.detector_param_shapes(cfg)
    h = f"model.{cfg.head_index}"
    assert not any("proto" in k for k in want)
    for l, ch in enumerate((64, 128, 256)):
        assert want[f"{h}.cv4.{l}.0.conv.weight"] == (16, ch, 3, 3)
        assert want[f"{h}.cv4.{l}.1.conv.weight"] == (16, 16, 3, 3)
        assert want[f"{h}.cv4.{l}.2.weight"] == (1, 16, 1, 1) and want[f"{h}.cv4.{l}.2.bias"] == (1,)
    # everything but cv4 and proto is the segment family's table
    seg = spec.detector_param_shapes(spec.yolo11_config() if arch == "11" else spec.DetectorConfig())
    assert {k: v for k, v in want.items() if ".cv4." not in k} == {k: v for k, v in seg.items() if ".cv4." not in k and ".proto." not in k}
    sd = spec.random_detector_state(cfg, 5)
    assert list(sd) == list(want) and all(sd[k].shape == tuple(s) for k, s in want.items())
    back = spec.detector_config_for_state(sd)
    assert (back.task, back.arch, back.nc) == ("obb", cfg.arch, cfg.nc)
    assert spec.detector_config_for_state(spec.random_detector_state(spec.DetectorConfig(nc=2), 1)).task == "seg"
    with pytest.raises(KeyError):
        spec.DetectorConfig(task="pose")


def _boxes(rng, m):
    return np.stack([rng.uniform(0, 640, m), rng.uniform(0, 640, m), rng.uniform(8, 300, m), rng.uniform(8, 300, m), rng.uniform(-np.pi / 4, 3 * np.pi / 4, m)],
                    1).astype(np.float32)


def test_probiou_restatement_sanity():
    rng = np.random.default_rng(0)
    a = _boxes(rng, 500)
    b = a.copy()
    b[:, :2] += rng.uniform(-30, 30, (500, 2)).astype(np.float32)
    b[:, 2:4] *= rng.uniform(0.7, 1.3, (500, 2)).astype(np.float32)
    b[:, 4] += rng.uniform(-0.3, 0.3, 500).astype(np.float32)
    for dt, tol in ((np.float64, 1e-6), (np.float32, 2e-5)):  # the float32 restatement: a few 1e-6 of rounding on either side
        p = R.probiou(a, b, dt)
        assert np.abs(p - R.probiou(b, a, dt)).max() < tol  # symmetric
        sw = b[:, [0, 1, 3, 2, 4]].astype(np.float64)
        sw[:, 4] += np.pi / 2
        if dt is np.float64:  # (the angle shift itself is rounded when the inputs are float32)
            assert np.abs(p - R.probiou(a.astype(np.float64), sw, dt)).max() < 1e-6  # (w, h, t) -> (h, w, t + pi/2)
            tp = b.astype(np.float64)
            tp[:, 4] += np.pi
            assert np.abs(p - R.probiou(a.astype(np.float64), tp, dt)).max() < 1e-6  # t -> t + pi
        assert (R.probiou(a, a, dt) > 0.99).all()  # identical boxes
        far = a.copy()
        far[:, 0] += 10 * np.maximum(a[:, 2], a[:, 3])
        assert (R.probiou(a, far, dt) < 1e-3).all()  # ten widths apart
        assert ((p > -1e-6) & (p < 1)).all()


def _pred_of(boxes, scores, cls, nc=3, na=None):
    """pred (4 + nc + 1, na) with the given boxes on the first anchors, the rest below every threshold"""
    m = len(boxes)
    na = na or m
    pred = np.zeros((4 + nc + 1, na), np.float32)
    pred[2:4] = 10.0
    pred[:4, :m] = boxes[:, :4].T
    pred[4 + nc, :m] = boxes[:, 4]
    pred[4 + np.asarray(cls), np.arange(m)] = scores
    return pred


def test_rule_is_not_the_greedy_sweep():
    """A > B > C by score; A suppresses B, B overlaps C, A does not overlap C: the rule drops C, a greedy sweep keeps it"""
    base = np.array([100, 100, 60, 120, 0.3], np.float32)
    boxes = np.stack([base, base + np.float32([10, 0, 0, 0, 0]), base + np.float32([20, 0, 0, 0, 0])])
    p = R.probiou(boxes[[0, 1, 0]], boxes[[1, 2, 2]])
    assert p[0] > 0.75 and p[1] > 0.75 and p[2] < 0.65
    pred = _pred_of(boxes, [0.9, 0.8, 0.7], [0, 0, 0], na=7)
    out = R.nms_rotated_single(pred, 3, 0.25, 0.7)
    assert out["keep_idx"].tolist() == [0]
    assert R.nms_greedy_single(pred, 3, 0.25, 0.7).tolist() == [0, 2]
    np.testing.assert_array_equal(out["rboxes"], boxes[:1])
    assert out["conf"].tolist() == [np.float32(0.9)] and out["cls"].tolist() == [0]
    # class-aware: the same three boxes in three classes all stay; max_det truncates in score order
    pred = _pred_of(boxes, [0.9, 0.8, 0.7], [0, 1, 2], na=7)
    assert R.nms_rotated_single(pred, 3, 0.25, 0.7)["keep_idx"].tolist() == [0, 1, 2]
    assert R.nms_rotated_single(pred, 3, 0.25, 0.7, max_det=2)["keep_idx"].tolist() == [0, 1]
    # ties: anchor ascending
    pred = _pred_of(boxes[[0, 2]], [0.8, 0.8], [0, 0], na=7)
    assert R.nms_rotated_single(pred, 3, 0.25, 0.7)["keep_idx"].tolist() == [0, 1]


PAD = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)


def _cards(dets, k=1, **kw):
    """dets: list of (x, y, w, h, theta, cls) of one frame, score-descending"""
    d = np.asarray(dets, np.float32).reshape(-1, 6)
    md = max(len(d), 1) + 2
    rb = np.zeros((1, md, 5), np.float32)
    cl = np.zeros((1, md), np.int32)
    rb[0, : len(d)] = d[:, :5]
    cl[0, : len(d)] = d[:, 5].astype(np.int32)
    conf = np.zeros((1, md), np.float32)
    conf[0, : len(d)] = np.linspace(0.9, 0.5, len(d))
    return R.obb_cards(np.array([len(d)], np.int32), rb, conf, cl, PAD, k, **kw)


def _q(tl, tr, br, bl):
    return np.array([tl, tr, br, bl], np.float32)


def test_card_rule_hand_made_frames():
    H = np.float32(np.pi / 2)
    up = _q([70, 40], [130, 40], [130, 160], [70, 160])  # card 60 x 120 centred (100, 100), upright
    # upright, nothing to orient it: assumed upright
    q, sel, fidx, st = _cards([(100, 100, 60, 120, 0, 0)])
    np.testing.assert_allclose(q[0], up, atol=1e-4)
    assert st.tolist() == [1] and fidx.tolist() == [0]
    np.testing.assert_allclose(sel[0], [70, 40, 130, 160], atol=1e-4)
    # theta = pi (rotated 180 degrees) and unoriented: still read upright
    np.testing.assert_allclose(_cards([(100, 100, 60, 120, np.pi, 0)])[0][0], up, atol=1e-4)
    # given as w > h with theta = pi/2: the same card
    q, _, _, st = _cards([(100, 100, 120, 60, H, 0)])
    np.testing.assert_allclose(q[0], up, atol=1e-4)
    assert st.tolist() == [1]
    # lying on its side (long axis horizontal), unoriented: "up" is the end with negative x
    side = _q([40, 130], [40, 70], [160, 70], [160, 130])
    for det in ((100, 100, 120, 60, 0, 0), (100, 100, 60, 120, H, 0)):
        q, _, _, st = _cards([det])
        np.testing.assert_allclose(q[0], side, atol=1e-4)
        assert st.tolist() == [1]
    # a top box in the lower half: the card is upside down (rotated 180 degrees), oriented
    down = _q([130, 160], [70, 160], [70, 40], [130, 40])
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (100, 140, 50, 30, 0, 1)])
    np.testing.assert_allclose(q[0], down, atol=1e-4)
    assert st.tolist() == [2]
    # a top box in the upper half: upright, oriented; the bottom box is not consulted
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (100, 60, 50, 30, 0, 1), (100, 70, 50, 30, 0, 2)])
    np.testing.assert_allclose(q[0], up, atol=1e-4)
    assert st.tolist() == [2]
    # a bottom box only, in the upper half: upside down
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (100, 60, 50, 30, 0, 2)])
    np.testing.assert_allclose(q[0], down, atol=1e-4)
    assert st.tolist() == [2]
    # on its side with the top box at the right end: top edge is the right side
    right = _q([160, 70], [160, 130], [40, 130], [40, 70])
    q, _, _, st = _cards([(100, 100, 120, 60, 0, 0), (150, 100, 20, 50, 0, 1)])
    np.testing.assert_allclose(q[0], right, atol=1e-4)
    assert st.tolist() == [2]
    # a top box whose centre lies outside the card is ignored (here: beside it), and so is one of an unused class
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (140, 140, 50, 30, 0, 1)])
    np.testing.assert_allclose(q[0], up, atol=1e-4)
    assert st.tolist() == [1]
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (100, 140, 50, 30, 0, 1)], top_cls=-1, bottom_cls=-1)
    np.testing.assert_allclose(q[0], up, atol=1e-4)
    assert st.tolist() == [1]
    # of two top boxes inside, the higher-scoring (earlier) one decides
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (100, 140, 50, 30, 0, 1), (100, 60, 50, 30, 0, 1)])
    np.testing.assert_allclose(q[0], down, atol=1e-4)
    # a top box exactly on the short axis decides nothing: the bottom box does
    q, _, _, st = _cards([(100, 100, 60, 120, 0, 0), (110, 100, 50, 30, 0, 1), (100, 150, 50, 30, 0, 2)])
    np.testing.assert_allclose(q[0], up, atol=1e-4)
    assert st.tolist() == [2]
    # a rotated card (30 degrees), top box toward its upper end: corners are centre +- U h/2 +- R w/2
    th = np.float32(np.pi / 6)
    u = np.array([-np.sin(th), np.cos(th)])
    U = -u  # the end with negative y
    Rv = np.array([-U[1], U[0]])
    c = np.array([300.0, 200.0])
    want = np.stack([c + U * 60 - Rv * 30, c + U * 60 + Rv * 30, c - U * 60 + Rv * 30, c - U * 60 - Rv * 30])
    top = c + U * 40
    q, sel, _, st = _cards([(300, 200, 60, 120, th, 0), (top[0], top[1], 40, 20, th, 1)])
    np.testing.assert_allclose(q[0], want, atol=1e-3)
    np.testing.assert_allclose(sel[0], [want[:, 0].min(), want[:, 1].min(), want[:, 0].max(), want[:, 1].max()], atol=1e-3)
    assert st.tolist() == [2]
    # slots: the k-th card-class detection in score order, pads beyond
    q, sel, fidx, st = _cards([(100, 100, 60, 120, 0, 1), (400, 100, 60, 120, 0, 0)], k=2)
    np.testing.assert_allclose(q[0], up + np.float32([300, 0]), atol=1e-4)
    np.testing.assert_array_equal(q[1], _q([5, 6], [7, 6], [7, 8], [5, 8]))
    np.testing.assert_array_equal(sel[1], PAD[1])
    assert st.tolist() == [1, 0] and fidx.tolist() == [0, 0]


@pytest.mark.parametrize("arch", ["v8", "11"])
def test_obb_export_mirror(arch, tmp_path):
    from mtgv.export_detector import DetectorModule, export_torchscript, to_torch_module
    from oracle import detector_ref as D

    cfg = _cfg(arch, imgsz=64)
    want = spec.detector_param_shapes(cfg)
    have = [(k, tuple(v.shape)) for k, v in DetectorModule(cfg).state_dict().items() if not k.endswith("num_batches_tracked")]
    assert have == [(k, tuple(s)) for k, s in want.items()]
    sd = spec.random_detector_state(cfg, 3)
    frames = np.random.default_rng(4).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    ref = D.forward(sd, cfg, frames)
    assert tuple(ref.shape) == (2, cfg.no, cfg.num_anchors)
    ang = ref[:, -1].numpy()
    assert (ang >= -np.pi / 4 - 1e-6).all() and (ang < 3 * np.pi / 4 + 1e-6).all() and ang.std() > 1e-3
    x = D.preprocess(frames)
    with torch.no_grad():
        pred = to_torch_module(cfg, sd)(x)
    assert isinstance(pred, torch.Tensor)
    np.testing.assert_allclose(pred.numpy(), ref.numpy(), atol=1e-5)
    p = str(tmp_path / "obb.pt")
    export_torchscript(cfg, sd, p)
    with torch.no_grad():
        tp = torch.jit.load(p)(x)
    np.testing.assert_allclose(tp.numpy(), ref.numpy(), atol=1e-5)
