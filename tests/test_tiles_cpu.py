"""CPU-only: the host side of tiled detection - tile_grid's geometry, the merge rule as mtgv.tiles.merge_tiles_host states it
on the designed cases of tiles_common, the two new ABI entries and their caps (refused without a device), and the
refusals of the pipelines."""
import itertools
import math
import types

import numpy as np
import pytest
import torch

import tiles_common as tc
from mtgv.tiles import TiledFrames, merge_tiles_host, tile_grid

SIZES = [(64, 64), (97, 131), (300, 500), (1080, 1920)]
WINDOWS = [(128, 160), (640, 640)]
OVERLAPS = [0, 32, 127]


@pytest.mark.parametrize("size,window,overlap", list(itertools.product(SIZES, WINDOWS, OVERLAPS)))
def test_tile_grid_covers_the_frame(size, window, overlap):
    (h, w), (wh, ww) = size, window
    g = tile_grid(h, w, window, overlap)
    assert g.dtype == np.int32 and g.shape[1] == 4
    ny = max(1, math.ceil((h - overlap) / (wh - overlap)))
    nx = max(1, math.ceil((w - overlap) / (ww - overlap)))
    assert len(g) == ny * nx
    assert [tuple(r[:2]) for r in g] == sorted(tuple(r[:2]) for r in g), "not in raster order"
    cover = np.zeros((h, w), np.int32)
    for y0, x0, th, tw in g:
        assert y0 >= 0 and x0 >= 0 and y0 + th <= h and x0 + tw <= w, "a window leaves its frame"
        assert (th, tw) == (min(wh, h), min(ww, w))
        cover[y0 : y0 + th, x0 : x0 + tw] += 1
    assert cover.min() >= 1, "a pixel is in no window"
    assert g[-1][0] + g[-1][2] == h and g[-1][1] + g[-1][3] == w, "the last window is not flush"
    if h <= wh:
        assert set(g[:, 0]) == {0} and set(g[:, 2]) == {h}
    if w <= ww:
        assert set(g[:, 1]) == {0} and set(g[:, 3]) == {w}
    full = tile_grid(h, w, window, overlap, with_full=True)
    assert np.array_equal(full[:-1], g) and full[-1].tolist() == [0, 0, h, w]


def test_tile_grid_refuses_a_bad_overlap():
    for overlap in (-1, 128, 200):
        with pytest.raises(AssertionError, match="overlap"):
            tile_grid(300, 500, (128, 160), overlap)


def _axis_ok(size, origins, extent, edge, starts, max_len):
    """ok[i, e]: some window of the axis holds the interval [starts[i], starts[i] + e] with no inner side within `edge` of it
    (the cut rule's comparisons, in float32); intervals that leave the axis count as held"""
    a = np.asarray(starts, np.float32)[:, None, None]
    b = a + np.arange(max_len + 1, dtype=np.float32)[None, :, None]
    o = np.array(origins, np.int64)[None, None, :]
    lo_ok = np.where(o > 0, ~(a < o.astype(np.float32) + np.float32(edge)), a >= o)
    hi_ok = np.where(o + extent < size, ~(b > (o + extent).astype(np.float32) - np.float32(edge)), b <= o + extent)
    return (lo_ok & hi_ok).any(axis=2) | (b[:, :, 0] > size)


@pytest.mark.parametrize("size,window,overlap", [(s, w, o) for s, w, o in itertools.product(SIZES, WINDOWS, [32, 127])])
def test_some_window_sees_every_small_box_whole(size, window, overlap):
    """every axis-aligned box of extent <= overlap - 2 * edge lies in some window whose inner sides are at least `edge` away
    from it (the cut rule then keeps it there): every position at 97 x 131, every seventh elsewhere, every extent.  The
    windows are the product of the two axes' intervals, so the property is checked per axis."""
    (h, w), edge = size, 2.0
    g = tile_grid(h, w, window, overlap)
    step = 1 if size == (97, 131) else 7
    ext = int(overlap - 2 * edge)
    for n, origins, extent in ((h, sorted(set(g[:, 0])), int(g[0, 2])), (w, sorted(set(g[:, 1])), int(g[0, 3]))):
        starts = np.arange(0, n + 1, step)
        ok = _axis_ok(n, origins, extent, edge, starts, ext)
        assert ok.shape == (len(starts), ext + 1) and ok.all(), f"an interval at {starts[np.argwhere(~ok)[0][0]]} of an axis of {n} is whole in no window"
        # two pixels longer (one still fits between integer positions): where the first two windows overlap by no more than
        # `overlap`, some interval is whole in no window - the bound is the rule's, not slack in this check
        if len(origins) > 1 and origins[1] - origins[0] == extent - overlap:
            assert not _axis_ok(n, origins, extent, edge, np.arange(0, n + 1), ext + 2).all()


# ---------------------------------------------------------------------------
# the merge rule on the designed cases
# ---------------------------------------------------------------------------
CASES = tc.designed()


def _slots(out, f, k):
    n = int(out["n_sel"][f])
    return n, out["src_slot"][f * k : f * k + n].tolist(), out["sel_conf"][f * k : f * k + n].tolist()


def _check_pads(c, out):
    k = c["k"]
    for f, (h, w) in enumerate(c["hw"]):
        for s in range(int(out["n_sel"][f]), k):
            o = f * k + s
            pb = c["pad_frac"][s] * np.array([w, h, w, h], np.float32)
            assert out["src_slot"][o] == -1 and out["sel_conf"][o] == 0
            assert np.array_equal(out["sel_boxes_src"][o], pb)
            assert np.array_equal(out["quads_src"][o], [[pb[0], pb[1]], [pb[2], pb[1]], [pb[2], pb[3]], [pb[0], pb[3]]])
    assert out["frame_idx"].tolist() == np.repeat(np.arange(len(c["hw"])), k).tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_pads_and_shapes(name):
    c = CASES[name]
    out = tc.host(c)
    F, k = len(c["hw"]), c["k"]
    assert {n: out[n].shape for n in tc.OUTPUTS} == {"sel_boxes_src": (F * k, 4), "quads_src": (F * k, 4, 2), "frame_idx": (F * k,),
                                                     "sel_conf": (F * k,), "src_slot": (F * k,), "n_sel": (F,)}
    _check_pads(c, out)


def test_overlap_of_two_and_of_four_windows_gives_one_hit():
    n, slots, conf = _slots(tc.host(CASES["overlap_two"]), 0, 4)
    assert (n, slots) == (1, [1 * 4 + 0]) and conf == [np.float32(0.9)]
    c = CASES["corner_four"]
    out = tc.host(c)
    n, slots, conf = _slots(out, 0, 4)
    assert (n, slots) == (1, [4 * 4 + 0]) and conf == [np.float32(0.95)]
    assert out["sel_boxes_src"][0].tolist() == [135, 100, 150, 120]
    assert out["quads_src"][0].tolist() == [[136, 101], [149, 101], [149, 119], [136, 119]]  # the quad, not the box's corners


def test_equal_confidence_the_lower_tile_wins():
    assert _slots(tc.host(CASES["equal_conf"]), 0, 4)[:2] == (1, [0])


def test_cut_rule_inner_side_frame_side_and_strictness():
    out = tc.host(CASES["inner_and_frame_side"])
    assert _slots(out, 0, 4)[:2] == (1, [0]) and out["sel_boxes_src"][0].tolist() == [0, 10, 20, 40]
    out = tc.host(CASES["exactly_edge"])
    assert _slots(out, 0, 4)[:2] == (1, [4]) and out["sel_boxes_src"][0].tolist() == [130, 10, 286, 40]
    # a quarter pixel closer to either inner side: dropped
    for box in ((129.75, 10, 286, 40), (130, 10, 286.25, 40)):
        assert int(tc.host(tc.case(tc.tables([tc.BIG]), [(1, box, 0.9)], 4, 4))["n_sel"][0]) == 0


def test_threshold_is_strict():
    n, slots, _ = _slots(tc.host(CASES["ios_equal"]), 0, 8)
    assert (n, slots) == (3, [0, 1, 2])


@pytest.mark.parametrize("name,winner", [("fragment_low", 12 * 4), ("fragment_high", 0)])
def test_fragment_and_whole_card_give_one_hit(name, winner):
    """The whole card (full-frame window) and a fragment of it that survived the cut rule (tile 0): intersection over the
    smaller area is 1, so one of the two goes - under IoU (0.42) both would stay.  The greedy pass runs in confidence order,
    so the one that stays is the more confident of the two."""
    assert _slots(tc.host(CASES[name]), 0, 4)[:2] == (1, [winner])
    c = dict(CASES[name], ios=2.4)  # the IoU-like outcome for contrast: with nothing suppressed both are reported
    assert int(tc.host(c)["n_sel"][0]) == 2


def test_more_than_k_none_and_n_det_over_kt():
    n, slots, conf = _slots(tc.host(CASES["more_than_k"]), 0, 8)
    assert n == 8 and slots == list(range(8)) and conf == sorted(conf, reverse=True) and min(conf) > 0.45
    out = tc.host(CASES["none"])
    assert int(out["n_sel"][0]) == 0 and (out["src_slot"] == -1).all()
    c = CASES["n_det_over_kt"]
    assert int(c["n_det"][0]) == 6 and _slots(tc.host(c), 0, 8)[:2] == (4, [0, 1, 2, 3])


def test_full_window_with_a_ratio_and_two_frames():
    c = CASES["full_ratio"]
    assert c["ratio"][0] == 0.32 and c["geo"][0].tolist() == [96, 160, 16, 0]
    out = tc.host(c)
    assert int(out["n_sel"][0]) == 2
    np.testing.assert_allclose(out["sel_boxes_src"][:2], [[100, 50, 220, 200], [300, 20, 360, 110]], atol=1e-3)
    # the quads were drawn in by one input pixel: 1 / 0.32 camera pixels
    np.testing.assert_allclose(out["quads_src"][0], [[103.125, 53.125], [216.875, 53.125], [216.875, 196.875], [103.125, 196.875]], atol=1e-3)
    c = CASES["two_frames"]
    assert np.diff(c["tile_start"]).tolist() == [6, 1]
    out = tc.host(c)
    assert _slots(out, 0, 4)[:2] == (3, [0, 1 * 4, 5 * 4]) and _slots(out, 1, 4)[:2] == (2, [6 * 4, 6 * 4 + 1])
    np.testing.assert_allclose(out["sel_boxes_src"][4:6], [[10, 10, 50, 70], [60, 10, 100, 70]], atol=1e-3)
    # a tile_start range beyond max_tiles_per_frame: that frame has no candidates, the other is unchanged
    cut = tc.host(dict(c, max_tiles_per_frame=2))
    assert cut["n_sel"].tolist() == [0, 2] and np.array_equal(cut["src_slot"][4:], out["src_slot"][4:])


def test_random_and_cap_cases_are_what_they_claim():
    c = tc.cap_case()
    assert np.diff(c["tile_start"]).tolist() == [16] and (c["n_det"] == 64).all()
    out = tc.host(c)
    assert int(out["n_sel"][0]) == 64 and len(set(out["src_slot"].tolist())) == 64
    conf = out["sel_conf"].tolist()
    assert conf == sorted(conf, reverse=True)
    ties = [i for i in range(63) if conf[i] == conf[i + 1]]
    assert ties and all(out["src_slot"][i] < out["src_slot"][i + 1] for i in ties)  # tile ascending, then j
    r = tc.random_case(3, 8, 8, True)
    n_tiles = np.diff(r["tile_start"])
    assert n_tiles.min() >= 1 and n_tiles.max() <= 16 and int(r["n_det"].max()) > 1
    out = tc.host(r)
    assert 0 < int(out["n_sel"].sum()) < int(np.minimum(r["n_det"], 8).sum()), "nothing was merged away"


# ---------------------------------------------------------------------------
# ABI and refusals
# ---------------------------------------------------------------------------
def test_abi_entries_and_caps_without_a_device():
    from mtgv import native

    L = native.lib()
    assert L.mtgv_version() >= 117
    assert len(native.SIGNATURES["mtgv_letterbox_tiles_u8"][1]) == 12 and len(native.SIGNATURES["mtgv_tiles_merge"][1]) == 25

    def merge(max_tiles, kt, k, max_det=300, frames=1):
        return L.mtgv_tiles_merge(None, None, None, None, max_tiles, max_det, kt, None, None, None, None, None, frames, max_tiles, None, k, 2.0, 0.5,
                                  None, None, None, None, None, None, None)

    assert merge(41, 25, 8) == 1
    msg = L.mtgv_last_error().decode()
    assert "1025 candidates" in msg and "41 tiles" in msg and "25 cards per tile" in msg and "1024" in msg
    assert merge(4, 8, 65) == 1 and "65 cards per frame" in L.mtgv_last_error().decode()
    assert merge(1, 9, 8, max_det=8) == 1 and "9 cards per tile" in L.mtgv_last_error().decode()
    assert merge(1, 8, 8, frames=65536) == 1 and "65536 frames" in L.mtgv_last_error().decode()
    assert merge(16, 64, 64) == 1 and "null" in L.mtgv_last_error().decode()  # inside every cap: the arguments are looked at next
    assert L.mtgv_letterbox_tiles_u8(None, None, None, 1, None, None, 65536, None, 128, 160, 114, None) == 1
    assert "65536 tiles" in L.mtgv_last_error().decode()
    with pytest.raises(AssertionError, match="k=65"):
        merge_tiles_host(np.zeros((0,)), np.zeros((0, 8, 4)), np.zeros((0, 8)), None, np.zeros((0, 5)), np.zeros((0, 4)), np.zeros((0,)), [0, 0], [(8, 8)], tc.pad_frac(65), 4, 65)


def _fake_pipeline(quad_source):
    from mtgv.pipeline import Pipeline

    cfg = types.SimpleNamespace(task="obb" if quad_source == "obb" else "seg", input_hw=None, imgsz=640, in_h=640, in_w=640)
    det = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), max_batch=4)
    enc = types.SimpleNamespace(cfg=types.SimpleNamespace(image_hw=(192, 128), z_size=8), max_batch=64)
    return Pipeline(det, enc, types.SimpleNamespace(), 8, quad_source=quad_source)


def _fake_tiles():
    z = torch.zeros((1,), dtype=torch.int32)
    return TiledFrames(torch.zeros((3,), dtype=torch.uint8), z.long(), z, z, z, z, z.double(), torch.zeros((1, 8, 8, 3), dtype=torch.uint8))


def test_refusals_say_so():
    pipe = _fake_pipeline("obb")
    with pytest.raises(NotImplementedError, match="obb.*rotated overlap rule"):
        pipe.run(_fake_tiles())
    pipe = _fake_pipeline("box")
    assert pipe.Kt == 8 and pipe.tile_merge == {"edge": 2.0, "ios": 0.5}
    with pytest.raises(NotImplementedError, match="Pipeline.run_many does not take TiledFrames"):
        pipe.run_many([_fake_tiles()])
    from mtgv.track import TrackedPipeline

    tp = TrackedPipeline.__new__(TrackedPipeline)  # (a DeviceTracker needs a GPU; the refusal comes before it is used)
    tp.pipeline, tp.embed_budget = pipe, 4
    with pytest.raises(NotImplementedError, match="TrackedPipeline.run_many does not take TiledFrames"):
        tp.run_many([(_fake_tiles(), [0], 0.0)])
