"""CPU-only: the rotated tile merge as mtgv.tiles states it in numpy - the pair function quad_inter_host on analytic cases and
against float64, merge_tiles_obb_host on the designed cases of tiles_obb_common and, on random frames, against a float64
evaluation of the same rule; the two ABI entries and their caps (refused without a device); the pipeline's switch."""
import numpy as np
import pytest

import tiles_common as tc
import tiles_obb_common as oc
from mtgv.tiles import merge_tiles_host, merge_tiles_obb_host, quad_bounds, quad_inter_host

CASES = oc.designed()


# ---------------------------------------------------------------------------
# the pair function
# ---------------------------------------------------------------------------
def test_quad_inter_analytic_cases_are_exact():
    """integer coordinates: float32 is exact, so is the comparison"""
    pairs = oc.analytic_pairs()
    assert len(pairs) == len(oc.ANALYTIC) * 32
    inter, area_a, area_b = quad_inter_host(np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs]))
    bad = [(p[0], float(g), float(p[3])) for p, g in zip(pairs, inter) if g != p[3]]
    assert not bad, bad[:8]
    for (name, a, b, _), ga, gb in zip(pairs, area_a, area_b):
        assert ga == abs(oc.area2_f64(a)) / 2 and gb == abs(oc.area2_f64(b)) / 2, name


def test_quad_inter_against_float64():
    """3000 card-like pairs anywhere in 3840 x 2160 against plain polygon clipping in Python floats: the largest difference
    measured is 2.1e-3 px^2 (bound 0.01: four orders of magnitude below ios * min(area) of a card); on axis-aligned quads it
    is iw * ih of merge_tiles_host's rule 5 within the same bound (measured 2.4e-3); the areas differ by 2.2e-3 at most."""
    a, b = oc.card_pairs(3000)
    inter, area_a, area_b = quad_inter_host(a, b)
    want = np.array([oc.inter_f64(x, y) for x, y in zip(a, b)])
    err = float(np.abs(inter.astype(np.float64) - want).max())
    err_area = max(float(np.abs(area_a - [abs(oc.area2_f64(x)) / 2 for x in a]).max()), float(np.abs(area_b - [abs(oc.area2_f64(x)) / 2 for x in b]).max()))
    print(f"quad_inter_host vs float64: inter {err:.2e} px^2, area {err_area:.2e} px^2, {np.mean(want > 0):.2f} of the pairs intersect")
    assert np.mean(want > 0) > 0.9 and err < 0.01 and err_area < 0.01
    # axis-aligned: the boxes of the same pairs
    ba, bb = quad_bounds(a), quad_bounds(b)

    def corners(x):
        return np.stack([x[:, [0, 1]], x[:, [2, 1]], x[:, [2, 3]], x[:, [0, 3]]], 1)

    inter, _, _ = quad_inter_host(corners(ba), corners(bb))
    iw = np.maximum(0, np.minimum(ba[:, 2], bb[:, 2]) - np.maximum(ba[:, 0], bb[:, 0]))
    ih = np.maximum(0, np.minimum(ba[:, 3], bb[:, 3]) - np.maximum(ba[:, 1], bb[:, 1]))
    err = float(np.abs(inter - iw * ih).max())
    print(f"axis-aligned vs iw * ih: {err:.2e} px^2")
    assert (iw * ih > 0).mean() > 0.9 and err < 0.01


# ---------------------------------------------------------------------------
# the merge rule on the designed cases
# ---------------------------------------------------------------------------
def _slots(out, f, k):
    n = int(out["n_sel"][f])
    s = slice(f * k, f * k + n)
    return n, out["src_slot"][s].tolist(), out["state"][s].tolist(), out["oriented_by"][s].tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_pads_and_shapes(name):
    c = CASES[name]
    out = oc.host(c)
    F, k = len(c["hw"]), c["k"]
    assert set(out) == set(oc.OUTPUTS)
    assert {n: out[n].shape for n in oc.OUTPUTS} == {"sel_boxes_src": (F * k, 4), "quads_src": (F * k, 4, 2), "frame_idx": (F * k,), "sel_conf": (F * k,),
                                                     "src_slot": (F * k,), "n_sel": (F,), "state": (F * k,), "oriented_by": (F * k,)}
    assert out["frame_idx"].tolist() == np.repeat(np.arange(F), k).tolist()
    for f, (h, w) in enumerate(c["hw"]):
        n = int(out["n_sel"][f])
        for s in range(k):
            o = f * k + s
            if s < n:
                assert out["src_slot"][o] >= 0 and out["state"][o] in (1, 2) and np.array_equal(out["sel_boxes_src"][o], quad_bounds(out["quads_src"][o])[0])
                continue
            pb = c["pad_frac"][s] * np.array([w, h, w, h], np.float32)
            assert out["src_slot"][o] == -1 and out["sel_conf"][o] == 0 and out["state"][o] == 0 and out["oriented_by"][o] == -1
            assert np.array_equal(out["sel_boxes_src"][o], pb)
            assert np.array_equal(out["quads_src"][o], [[pb[0], pb[1]], [pb[2], pb[1]], [pb[2], pb[3]], [pb[0], pb[3]]])


def test_side_by_side_at_45_degrees_both_survive():
    c = CASES["side_by_side_45"]
    out = oc.host(c)
    assert _slots(out, 0, 4)[:2] == (2, [0, 1])
    assert out["quads_src"][0].tolist() == oc.STRIP_A.tolist() and out["quads_src"][1].tolist() == oc.STRIP_B.tolist()
    # the case is what it claims: on the bounding boxes the axis-aligned rule keeps one of the two
    boxes = np.zeros((1, 8, 4), np.float32)
    boxes[0, :2] = out["sel_boxes_src"][:2]
    assert boxes[0, :2].tolist() == [[10, 30, 77, 97], [20, 40, 87, 107]]
    flat = merge_tiles_host(c["n_det"], boxes, c["conf"], None, c["tiles"], c["geo"], c["ratio"], c["tile_start"], c["hw"], c["pad_frac"], 4, 4)
    assert int(flat["n_sel"][0]) == 1
    assert quad_inter_host(oc.STRIP_A[None], oc.STRIP_B[None])[0][0] == 0


def test_overlap_of_two_and_of_four_windows_gives_one_hit():
    out = oc.host(CASES["overlap_two"])
    assert _slots(out, 0, 4) == (1, [1 * 4], [1], [-1]) and out["sel_conf"][0] == np.float32(0.9)
    assert out["sel_boxes_src"][0].tolist() == [134, 20, 148, 34]
    out = oc.host(CASES["corner_four"])
    assert _slots(out, 0, 4) == (1, [4 * 4], [2], [-1]) and out["sel_conf"][0] == np.float32(0.95)
    assert out["quads_src"][0].tolist() == [[140, 102], [148, 110], [142, 116], [134, 108]]


def test_equal_confidence_the_lower_tile_wins():
    assert _slots(oc.host(CASES["equal_conf"]), 0, 4)[:2] == (1, [0])


@pytest.mark.parametrize("name,winner", [("fragment_low", 12 * 4), ("fragment_high", 0)])
def test_fragment_and_whole_card_give_one_hit(name, winner):
    assert _slots(oc.host(CASES[name]), 0, 4)[:2] == (1, [winner])
    assert int(oc.host(dict(CASES[name], ios=2.4))["n_sel"][0]) == 2  # with nothing suppressed both are reported


def test_cut_rule_inner_side_frame_side_and_strictness():
    out = oc.host(CASES["inner_and_frame_side"])
    assert _slots(out, 0, 4)[:2] == (1, [0]) and out["sel_boxes_src"][0].tolist() == [0, 10, 20, 40]
    out = oc.host(CASES["exactly_edge"])
    assert _slots(out, 0, 4)[:2] == (1, [4]) and out["sel_boxes_src"][0].tolist() == [130, 10, 286, 40]
    # a quarter pixel closer to either inner side: dropped
    assert int(oc.host(CASES["edge_left_strict"])["n_sel"][0]) == 0 and int(oc.host(CASES["edge_right_strict"])["n_sel"][0]) == 0


def test_threshold_is_strict():
    c = CASES["ios_equal"]
    inter, area_a, area_b = quad_inter_host(c["quads"][[0, 2]], c["quads"][[1, 3]])
    assert inter.tolist() == [2048, 2064] and area_a.tolist() == [4096, 4096] and area_b.tolist() == [4096, 4096]
    assert _slots(oc.host(c), 0, 8)[:2] == (3, [0, 1, 2])


def test_orientation_transfer():
    up, down = oc.UP.tolist(), oc.DOWN.tolist()
    out = oc.host(CASES["orient_flip"])  # upside down relative to the oriented duplicate: rolled by two
    assert _slots(out, 0, 4) == (1, [0], [2], [1 * 4]) and out["quads_src"][0].tolist() == down
    assert out["sel_boxes_src"][0].tolist() == [20, 10, 60, 70]
    out = oc.host(CASES["orient_agree"])
    assert _slots(out, 0, 4) == (1, [0], [2], [1 * 4]) and out["quads_src"][0].tolist() == up
    out = oc.host(CASES["orient_two_donors"])  # the earlier of the two in the order (tile 2, 0.8) decides
    assert _slots(out, 0, 4) == (1, [0], [2], [2 * 4]) and out["quads_src"][0].tolist() == down
    out = oc.host(CASES["orient_kept_oriented"])
    assert _slots(out, 0, 4) == (1, [0], [2], [-1]) and out["quads_src"][0].tolist() == up
    out = oc.host(CASES["orient_perpendicular"])  # d == 0: nothing to learn
    assert _slots(out, 0, 4) == (1, [0], [1], [-1]) and out["quads_src"][0].tolist() == up
    out = oc.host(CASES["orient_behind_unoriented"])  # the donor is the first *oriented* one that was dropped
    assert _slots(out, 0, 4) == (1, [0], [2], [2 * 4]) and out["quads_src"][0].tolist() == down and out["sel_conf"][0] == np.float32(0.9)


def test_markers_counts_and_states_are_not_trusted():
    c = CASES["markers_only"]
    assert c["state"][4] == 1 and c["cls"][1, :2].tolist() == [oc.TOP, oc.BOTTOM]
    assert _slots(oc.host(c), 0, 4)[:2] == (1, [0])
    c = CASES["n_det_over_max_det"]  # 99 detections claimed of max_det 8: the scan stops at 8, kt = 4 slots
    assert int(c["n_det"][0]) == 99 and _slots(oc.host(c), 0, 8)[:2] == (4, [0, 1, 2, 3])
    c = CASES["n_det_negative"]
    assert int(c["n_det"][1]) == -3 and c["state"][4] == 1 and _slots(oc.host(c), 0, 4)[:2] == (1, [0])
    c = CASES["state_three"]
    assert c["state"][:2].tolist() == [1, 3] and _slots(oc.host(c), 0, 4)[:2] == (1, [0])


def test_more_than_k_none_and_two_frames():
    out = oc.host(CASES["more_than_k"])
    n, slots, states, _ = _slots(out, 0, 8)
    conf = out["sel_conf"].tolist()
    assert n == 8 and slots == list(range(8)) and conf == sorted(conf, reverse=True) and min(conf) > 0.45 and set(states) == {1, 2}
    out = oc.host(CASES["none"])
    assert int(out["n_sel"][0]) == 0 and (out["src_slot"] == -1).all() and (out["state"] == 0).all()
    c = CASES["two_frames"]
    assert np.diff(c["tile_start"]).tolist() == [7, 1] and c["ratio"][6] == 0.4 and c["ratio"][7] == 1.28
    assert c["cls"][6, :2].tolist() == [oc.TOP, oc.CARD] and c["cls"][7, :4].tolist() == [oc.BOTTOM, oc.CARD, oc.TOP, oc.CARD]  # card j is not detection j
    out = oc.host(c)
    # frame 0: the square of tile 0 is oriented by its duplicate in the full window; `small` is kept from tile 1
    assert _slots(out, 0, 4) == (2, [0, 1 * 4], [2, 2], [6 * 4, -1]) and _slots(out, 1, 4) == (2, [7 * 4, 7 * 4 + 1], [1, 2], [-1, -1])
    assert out["sel_conf"][:2].tolist() == [np.float32(0.9), np.float32(0.7)] and out["sel_conf"][4:6].tolist() == [np.float32(0.5), np.float32(0.4)]
    np.testing.assert_allclose(out["quads_src"][4], oc.rq(40, 50, 30, 50, 0.7), atol=1e-3)
    # a tile_start range beyond max_tiles_per_frame: that frame has no candidates, the other is unchanged
    cut = oc.host(dict(c, max_tiles_per_frame=2))
    assert cut["n_sel"].tolist() == [0, 2] and np.array_equal(cut["src_slot"][4:], out["src_slot"][4:])
    assert [oc.host(g)["n_sel"].tolist() for g in oc.garbage_tile_start_cases()] == [[2, 0], [0, 2], [0, 0], [0, 0]]


def test_cap_and_nan_cases_are_what_they_claim():
    c = oc.cap_case()
    assert np.diff(c["tile_start"]).tolist() == [16] and (c["n_det"] == 64).all() and (c["state"] > 0).all()
    out = oc.host(c)
    assert int(out["n_sel"][0]) == 64 and len(set(out["src_slot"].tolist())) == 64
    conf = out["sel_conf"].tolist()
    assert conf == sorted(conf, reverse=True)
    ties = [i for i in range(63) if conf[i] == conf[i + 1]]
    assert ties and all(out["src_slot"][i] < out["src_slot"][i + 1] for i in ties)  # tile ascending, then j
    c = oc.nan_case()
    assert np.isnan(c["quads"]).sum() == 1 and np.isinf(c["quads"]).sum() == 1
    out = oc.host(c)
    assert int(out["n_sel"][0]) == 3 and np.isnan(out["quads_src"]).sum() == 1 and np.isinf(out["quads_src"]).sum() == 0  # (the mapping clips an inf)


# ---------------------------------------------------------------------------
# random frames against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed,kt,k", oc.RANDOM)
def test_random_frames_against_float64(seed, kt, k):
    """first the margins of every decision taken, in float64 - |inter - ios * min(area)| > 1 px^2, every bound more than 0.01 px
    from a cut line, distinct confidences (the seeds of tiles_obb_common.RANDOM are chosen so) - then the float32 rule's kept
    sets, order, states and donors are the float64 ones"""
    c = oc.random_case(seed, kt, k)
    want, (m_inter, m_cut, m_conf) = oc.merge_f64(c)
    print(f"seed {seed}: margins inter {m_inter:.3g} px^2, cut {m_cut:.3g} px, conf {m_conf:.3g}; kept {[len(x) for x in want]}")
    assert m_inter > 1 and m_cut > 0.01 and m_conf > 0
    out = oc.host(c)
    n_cand = int(((c["state"] == 1) | (c["state"] == 2)).sum())
    assert 0 < int(out["n_sel"].sum()) < n_cand, "nothing was merged away"
    for f, kept in enumerate(want):
        n, slots, states, by = _slots(out, f, k)
        assert (n, slots, states, by) == (len(kept), [x[0] for x in kept], [x[1] for x in kept], [x[2] for x in kept]), f
    if k >= 8:
        assert (out["oriented_by"] >= 0).any(), "no orientation was carried over"


# ---------------------------------------------------------------------------
# ABI and the pipeline's switch
# ---------------------------------------------------------------------------
def test_abi_entries_and_caps_without_a_device():
    from mtgv import native

    L = native.lib()
    assert L.mtgv_version() >= 119
    assert len(native.SIGNATURES["mtgv_tiles_merge_obb"][1]) == 29 and len(native.SIGNATURES["mtgv_op_quad_inter"][1]) == 7

    def merge(max_tiles, kt, k, max_det=300, frames=1):
        return L.mtgv_tiles_merge_obb(None, None, None, None, None, max_tiles, max_det, kt, None, None, None, None, None, frames, max_tiles, None, k,
                                      2.0, 0.5, 0, None, None, None, None, None, None, None, None, None)

    assert merge(41, 25, 8) == 1
    msg = L.mtgv_last_error().decode()
    assert "1025 candidates" in msg and "41 tiles" in msg and "25 cards per tile" in msg and "1024" in msg
    assert merge(4, 8, 65) == 1 and "65 cards per frame" in L.mtgv_last_error().decode()
    assert merge(1, 9, 8, max_det=8) == 1 and "9 cards per tile" in L.mtgv_last_error().decode()
    assert merge(1, 8, 8, frames=65536) == 1 and "65536 frames" in L.mtgv_last_error().decode()
    assert merge(16, 64, 64) == 1 and "null" in L.mtgv_last_error().decode()  # inside every cap: the arguments are looked at next
    assert L.mtgv_op_quad_inter(None, None, -1, None, None, None, None) == 1 and "m=-1" in L.mtgv_last_error().decode()
    assert L.mtgv_op_quad_inter(None, None, 4, None, None, None, None) == 1 and "null" in L.mtgv_last_error().decode()
    with pytest.raises(AssertionError, match="k=65"):
        merge_tiles_obb_host(np.zeros((0,)), np.zeros((0, 8)), np.zeros((0, 8)), np.zeros((0, 4, 2)), np.zeros((0,)), np.zeros((0, 5)), np.zeros((0, 4)),
                             np.zeros((0,)), [0, 0], [(8, 8)], tc.pad_frac(65), 4, 65)


def _fake_pipeline(quad_source, **kw):
    import types

    import torch

    from mtgv.pipeline import Pipeline

    cfg = types.SimpleNamespace(task="obb" if quad_source == "obb" else "seg", input_hw=None, imgsz=640, in_h=640, in_w=640)
    det = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), max_batch=4)
    enc = types.SimpleNamespace(cfg=types.SimpleNamespace(image_hw=(192, 128), z_size=8), max_batch=64)
    return Pipeline(det, enc, types.SimpleNamespace(), 8, quad_source=quad_source, **kw)


def test_pipeline_switch():
    pipe = _fake_pipeline("obb", tile_merge={"rule": "rotated"})
    assert pipe.tile_merge == {"edge": 2.0, "ios": 0.5, "rule": "rotated"}
    assert _fake_pipeline("obb", tile_merge={"rule": "rotated", "ios": 0.3}).tile_merge["ios"] == 0.3
    for source in ("box", "mask"):
        with pytest.raises(AssertionError, match=f'rotated.*{source}'):
            _fake_pipeline(source, tile_merge={"rule": "rotated"})
    with pytest.raises(AssertionError, match="probiou"):
        _fake_pipeline("obb", tile_merge={"rule": "probiou"})
    with pytest.raises(AssertionError, match="iou"):
        _fake_pipeline("obb", tile_merge={"iou": 0.5})
    assert _fake_pipeline("obb").tile_merge == {"edge": 2.0, "ios": 0.5} and _fake_pipeline("box").tile_merge == {"edge": 2.0, "ios": 0.5}
    with pytest.raises(NotImplementedError, match=r'tile_merge=\{"rule": "rotated"\}'):  # the refusal says how to turn the path on
        import torch

        from mtgv.tiles import TiledFrames

        z = torch.zeros((1,), dtype=torch.int32)
        _fake_pipeline("obb").run(TiledFrames(torch.zeros((3,), dtype=torch.uint8), z.long(), z, z, z, z, z.double(), torch.zeros((1, 8, 8, 3), dtype=torch.uint8)))
