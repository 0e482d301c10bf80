"""GPU: mtgv_mask_contours / mtgv_mask_contours_logits (csrc/contours.hip) against the host specification
`mtgv.adapters._mask_segments` - the same points in the same order, exactly - on the cases of tests/contours_common.py
(tests/test_contours_cpu.py proves the algorithm on the CPU first), the caps, determinism, and the adapter."""
import numpy as np
import pytest
import torch

import contours_common as cc

pytestmark = pytest.mark.gpu

SENT = -7777  # what every output buffer holds before a call
GUARD = 256   # int32 words behind the point buffer that must keep the sentinel
ADAPTER_DETS = 4  # detections of the random-weight frame that the adapter tests trace


def _call(src: torch.Tensor, dims, h, w, strategy, max_points, logits=False):
    """one library call on buffers filled with the sentinel -> (points (n, max_points, 2), guard, n_points, n_blobs, status)"""
    from mtgv import native

    L = native.lib()
    n = src.shape[0]
    buf = torch.full((n * max_points * 2 + GUARD,), SENT, dtype=torch.int32, device="cuda")
    counts = torch.full((3, n), SENT, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.mtgv_mask_contours_workspace_bytes(n, h, w, max_points))
    ws = torch.zeros((ws_bytes + 3) // 4, dtype=torch.int32, device="cuda")
    fn = L.mtgv_mask_contours_logits if logits else L.mtgv_mask_contours
    native.check(fn(native.ptr(src), n, *dims, cc.STRATEGIES[strategy], max_points, native.ptr(buf), native.ptr(counts[0]),
                    native.ptr(counts[1]), native.ptr(counts[2]), native.ptr(ws), ws_bytes, native.stream()))
    torch.cuda.synchronize()
    b, c = buf.cpu().numpy(), counts.cpu().numpy()
    return b[: n * max_points * 2].reshape(n, max_points, 2), b[n * max_points * 2 :], c[0], c[1], c[2]


def run_masks(masks, strategy="all", max_points=cc.MAX_POINTS):
    m = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint8)).cuda()
    return _call(m, m.shape[1:], m.shape[1], m.shape[2], strategy, max_points)


def run_logits(logits: torch.Tensor, scale=4, strategy="all", max_points=cc.MAX_POINTS):
    _, mh, mw = logits.shape
    return _call(logits.contiguous(), (mh, mw, scale), mh * scale, mw * scale, strategy, max_points, logits=True)


_HOST = {}


def host(name, mask, strategy):
    """the host reference, computed once per (case, strategy)"""
    key = (name, strategy)
    if key not in _HOST:
        _HOST[key] = cc.host_contours(mask, strategy)
    return _HOST[key]


def check_mask(res, i, want, blobs, name):
    pts, guard, n_pts, n_blobs, status = res
    assert status[i] == 0 and n_blobs[i] == blobs and n_pts[i] == len(want), (name, status[i], n_blobs[i], blobs, n_pts[i], len(want))
    assert np.array_equal(pts[i, : n_pts[i]], want), (name, pts[i, : n_pts[i]].tolist(), want.tolist())
    assert (pts[i, n_pts[i] :] == SENT).all() and (guard == SENT).all(), name


@pytest.mark.parametrize("strategy", ["all", "largest"])
def test_mask_form_equals_the_host(strategy):
    for name, m in cc.cases():
        want, blobs = host(name, m, strategy)
        check_mask(run_masks(m[None], strategy), 0, want, blobs, name)


@pytest.mark.parametrize("strategy", ["all", "largest"])
def test_batches(strategy):
    for name, masks in cc.batches():
        res = run_masks(masks, strategy)
        for i, m in enumerate(masks):
            want, blobs = host(f"{name} / {i}", m, strategy)
            check_mask(res, i, want, blobs, f"{name} / {i}")


def _smooth(rng, mh, mw, cell):
    """random logits that vary smoothly: a coarse normal field, bilinearly enlarged"""
    coarse = torch.from_numpy(rng.standard_normal((1, 1, -(-mh // cell) + 1, -(-mw // cell) + 1)).astype(np.float32))
    return torch.nn.functional.interpolate(coarse, size=(mh, mw), mode="bilinear", align_corners=True)[0, 0]


def _logit_batches():
    rng = np.random.default_rng(17)
    small = torch.stack([_smooth(rng, 6, 10, c) for c in (2, 3, 5, 2)])
    card = torch.from_numpy(np.where(cc.card_mask(), 3.0, -3.0).astype(np.float32))[None, None]
    card = torch.nn.functional.avg_pool2d(card, 4)[0, 0]  # x4 bilinear interpolation crosses zero on the card's boundary
    big = torch.stack([card + 1.5 * _smooth(rng, 160, 160, 20), card, 0.5 * _smooth(rng, 160, 160, 40) - 0.2])
    return [("6x10", small), ("160x160", big)]


@pytest.mark.parametrize("strategy", ["all", "largest"])
def test_logits_form_equals_binarize_plus_mask_form(strategy):
    from mtgv.detector import binarize_masks

    for name, logits in _logit_batches():
        logits = logits.cuda().contiguous()
        masks = binarize_masks(logits, 4).cpu().numpy()
        assert masks.any(axis=(1, 2)).sum() >= 2, name
        from_logits = run_logits(logits, 4, strategy)
        from_masks = run_masks(masks, strategy)
        for i, m in enumerate(masks):
            want, blobs = host(f"logits {name} / {i}", m, strategy)
            check_mask(from_logits, i, want, blobs, f"logits {name} / {i}")
            check_mask(from_masks, i, want, blobs, f"masks of {name} / {i}")
        for a, b in zip(from_logits, from_masks):
            assert np.array_equal(a, b), name


def test_point_cap():
    """more points than max_points: status 1, the first max_points points written, nothing behind them, the batch's other
    masks untouched by it"""
    u = np.zeros(cc.RANDOM_SHAPE, np.uint8)
    u[5:17, 40:52] = cc.u_shape("up")
    u[20:32, 3:15] = cc.u_shape("left")
    masks = np.stack([u, cc.random_mask(0.3, 0), np.ones(cc.RANDOM_SHAPE, np.uint8), np.zeros(cc.RANDOM_SHAPE, np.uint8)])
    pts, guard, n_pts, n_blobs, status = res = run_masks(masks, "all", max_points=64)
    wants = [host(f"cap / {i}", m, "all") for i, m in enumerate(masks)]
    assert len(wants[1][0]) > 64 and status[1] == 1 and n_pts[1] == 64 and n_blobs[1] == wants[1][1]
    assert np.array_equal(pts[1], wants[1][0][:64])
    assert (guard == SENT).all()
    over = [i for i, (w, _) in enumerate(wants) if len(w) > 64]
    assert over == [1]
    for i in (0, 2, 3):
        check_mask(res, i, wants[i][0], wants[i][1], f"cap / {i}")


def test_blob_cap():
    grid = cc.stride2_grid()
    assert int(grid.sum()) > cc.MAX_BLOBS
    masks = np.stack([grid, np.pad(np.ones((10, 10), np.uint8), 28)])
    pts, guard, n_pts, n_blobs, status = res = run_masks(masks)
    assert status[0] == 1 and n_pts[0] == 0 and n_blobs[0] == int(grid.sum())
    assert (pts[0] == SENT).all() and (guard == SENT).all()
    check_mask(res, 1, *host("blob cap / square", masks[1], "all"), "blob cap / square")


def test_run_cap():
    """more row runs than the run table holds (a 140 x 140 checkerboard has 9800): status 1, nothing written"""
    board = (np.add.outer(np.arange(140), np.arange(140)) % 2 == 0).astype(np.uint8)
    assert board.sum() > cc.MAX_RUNS
    pts, guard, n_pts, n_blobs, status = run_masks(board[None])
    assert status[0] == 1 and n_pts[0] == 0 and (pts == SENT).all() and (guard == SENT).all()


def test_determinism():
    masks = np.stack([cc.random_mask(d, 1) for d in cc.RANDOM_DENSITIES])
    first, second = run_masks(masks), run_masks(masks)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    for i in range(len(masks)):
        one = run_masks(masks[i : i + 1])
        assert one[0][0].tobytes() == first[0][i].tobytes()
        assert (one[2][0], one[3][0], one[4][0]) == (first[2][i], first[3][i], first[4][i])


def test_wrappers():
    from mtgv.crop import mask_contours, mask_contours_from_logits

    m = np.stack([cc.u_shape("down"), cc.u_shape("left")])
    pts, n_pts, n_blobs, status = mask_contours(torch.from_numpy(m).cuda(), "largest", 64)
    assert pts.shape == (2, 64, 2) and pts.dtype == torch.int32 and pts.is_cuda and status.tolist() == [0, 0] and n_blobs.tolist() == [1, 1]
    for i in range(2):
        assert np.array_equal(pts[i, : int(n_pts[i])].cpu().numpy(), host(f"wrapper / {i}", m[i], "largest")[0])
    logits = torch.from_numpy(np.where(np.kron(cc.u_shape("up"), np.ones((2, 2))), 2.0, -2.0).astype(np.float32))[None].cuda()
    out = mask_contours_from_logits(logits, 4)
    assert out[0].shape == (1, cc.MAX_POINTS, 2) and int(out[3][0]) == 0 and int(out[2][0]) == 1 and int(out[1][0]) >= 8
    with pytest.raises(ValueError):
        mask_contours(torch.from_numpy(m).cuda(), "longest")


# ---- the adapter ----
@pytest.fixture(scope="module")
def segmenter_case():
    """the detector, frame and host-traced result the adapter tests share (the frame of tests/test_gpu_adapters.py).  The
    random-weight masks are speckle of hundreds of blobs each, seconds of Python tracing for the whole frame: the adapter
    sees the frame's ADAPTER_DETS most confident detections."""
    import dataclasses

    from mtgv import spec
    from mtgv.adapters import CardSegmenter
    from mtgv.detector import Detector

    cfg = spec.DetectorConfig()
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=1)
    real_detect = det.detect

    def detect(*args, **kw):
        d = real_detect(*args, **kw)
        return dataclasses.replace(d, **{f.name: getattr(d, f.name)[:ADAPTER_DETS] for f in dataclasses.fields(d)})

    det.detect = detect
    frame = np.random.default_rng(8).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    return det, frame, CardSegmenter(detector=det, contours="trace_host")(frame)


def _same_segments(got, want):
    assert len(got) == len(want) and len(want) > 0
    for g, w in zip(got, want):
        assert g.conf == w.conf and g.label == w.label
        assert g.points.dtype == w.points.dtype == np.float32 and g.points.shape == w.points.shape
        assert g.points.tobytes() == w.points.tobytes()


def test_adapter_trace_equals_trace_host(segmenter_case):
    from mtgv.adapters import CardSegmenter

    det, frame, want = segmenter_case
    seg = CardSegmenter(detector=det)
    assert seg.contours == "trace"
    _same_segments(seg(frame), want)


def test_adapter_falls_back_per_mask_over_the_cap(segmenter_case, monkeypatch):
    from mtgv.adapters import CardSegmenter

    det, frame, want = segmenter_case
    sizes = sorted(len(s.points) for s in want)
    cap = max(1, sizes[len(sizes) // 2])  # about half of the masks are over it
    monkeypatch.setattr(CardSegmenter, "TRACE_MAX_POINTS", cap)
    _same_segments(CardSegmenter(detector=det, contours="trace")(frame), want)


def test_adapter_on_card_shaped_masks(monkeypatch):
    """two card-shaped detections (the masks of tests/test_gpu_adapters.py's outline test): no fallback, same points"""
    import mtgv.adapters as A
    from mtgv import spec
    from mtgv.detector import Detections, Detector

    cfg = spec.DetectorConfig()
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=1)
    masks = np.stack([cc.card_mask(), cc.card_mask(640, 640, (420.0, 200.0), (60.0, 90.0), -50.0, 15.0)])
    big = torch.from_numpy(np.where(masks, 4.0, -4.0).astype(np.float32))[:, None]
    logits = torch.nn.functional.avg_pool2d(big, 4)[:, 0].cuda().contiguous()
    fake = Detections(torch.tensor([[0.0, 0.0, 640.0, 640.0]] * 2, device="cuda"), torch.tensor([0.9, 0.8], device="cuda"),
                      torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), logits)
    monkeypatch.setattr(det, "detect", lambda *a, **k: fake)
    monkeypatch.setattr(A, "_mask_segments", None)  # the device path must not trace on the host
    frame = np.zeros((480, 640, 3), np.uint8)
    got = A.CardSegmenter(detector=det, contours="trace")(frame)
    monkeypatch.undo()
    monkeypatch.setattr(det, "detect", lambda *a, **k: fake)
    _same_segments(got, A.CardSegmenter(detector=det, contours="trace_host")(frame))
    assert all(len(s.points) > 100 for s in got)
