"""Tiled detection on the GPU: the cut (mtgv_letterbox_tiles_u8) against the ragged letterbox of each window's contiguous copy,
the merge (mtgv_tiles_merge) against mtgv.tiles.merge_tiles_host, and their callers Pipeline.run(TiledFrames) and
TrackedPipeline.run(TiledFrames).

Every comparison is exact (bytes, or float32 bit patterns): the kernels restate single operations of their host rules."""
import functools

import numpy as np
import pytest
import torch

import source_frames_common as sc
import tiles_common as tc

pytestmark = pytest.mark.gpu

IN_HW = (128, 160)
ENC_HW = (192, 128)
K = 8
CLS_BIAS = -2.2  # the random-weight detector then finds between 1 and K cards in the two ONE_TILE frames; every test asserts what it needs
ONE_TILE_SEEDS = (21, 27)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# 1. the cut
# ---------------------------------------------------------------------------
CUT_SHAPES = [(97, 131), (300, 500), (64, 64)]
MARK, GUARD = 0xA5, 4096


def _ragged_dev(frames, pad=1003):
    """the frames back to back in the middle of a larger tensor, at an odd address"""
    buf, offsets, hw = sc.ragged(frames)
    big = torch.full((buf.size + 2 * pad,), 0x3C, dtype=torch.uint8, device="cuda")
    big[pad : pad + buf.size] = _cuda(buf)
    return big[pad : pad + buf.size], offsets, hw


def _guarded(nt):
    big = torch.full((2 * GUARD + nt * IN_HW[0] * IN_HW[1] * 3,), MARK, dtype=torch.uint8, device="cuda")
    return big, big[GUARD:-GUARD].view(nt, IN_HW[0], IN_HW[1], 3)


def _reference_cut(frames, tiles):
    """mtgv_letterbox_ragged_u8 on a contiguous copy of every window (torch slicing), one launch for all of them"""
    from mtgv.pipeline import SourceFrames

    wins = [_cuda(frames[f])[y0 : y0 + wh, x0 : x0 + ww].contiguous() for f, y0, x0, wh, ww in tiles]
    sizes = np.array([w.numel() for w in wins], np.int64)
    sf = SourceFrames.from_ragged(torch.cat([w.view(-1) for w in wins]), np.concatenate([[0], np.cumsum(sizes)[:-1]]), [w.shape[:2] for w in wins],
                                  input_hw=IN_HW)
    return wins, sf


@pytest.mark.parametrize("window,overlap", [(IN_HW, 33), ((200, 250), 33)])
def test_cut_equals_the_ragged_letterbox_of_each_window(window, overlap):
    from mtgv.tiles import TiledFrames, cut_tiles

    frames = [sc.noise_frame(h, w, 100 * h + w) for h, w in CUT_SHAPES]
    buf, offsets, hw = _ragged_dev(frames)
    assert buf.data_ptr() % 2 == 1 and [int(o) % 2 for o in offsets[1:]] == [1, 1]
    tf = TiledFrames.from_ragged(buf, offsets, hw, window_hw=window, overlap=overlap, with_full=False, input_hw=IN_HW)
    tiles = tf.tiles_h.tolist()
    nt = len(tiles)
    assert np.diff(tf.tile_start_h).tolist() == ([1, 12, 1] if window == IN_HW else [1, 6, 1])
    assert any(t[2] % 2 == 1 for t in tiles), "no window starts at an odd column"
    assert any(t[0] == 1 and t[1] + t[3] == 300 and t[2] + t[4] == 500 for t in tiles), "no flush last window"
    assert tiles[-1] == [2, 0, 0, 64, 64]  # the frame smaller than the window: one clipped window
    wins, ref = _reference_cut(frames, tiles)
    assert torch.equal(tf.geo, ref.geo) and torch.equal(tf.ratio, ref.ratio)
    assert torch.equal(tf.frames, ref.frames)
    big, dst = _guarded(nt)
    cut_tiles(tf.buf, tf.offsets, tf.hw, tf.tiles, tf.geo, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst, ref.frames) and (big[:GUARD] == MARK).all() and (big[-GUARD:] == MARK).all()
    if window == IN_HW:  # the 12 whole windows are at scale 1: the slice itself (the two clipped ones are scaled up to fit)
        whole = [t for t in range(nt) if tuple(wins[t].shape[:2]) == IN_HW]
        assert len(whole) == 12
        for t in whole:
            assert tf.geo[t].cpu().tolist() == [128, 160, 0, 0] and float(tf.ratio[t]) == 1.0 and torch.equal(dst[t], wins[t])
        # and a scale-1 window that does not fill the input: the slice inside (nh, nw), 114 outside
        part = np.array([[1, 13, 251, 100, 131]], np.int32)
        geo = np.array([[100, 131, 14, 14]], np.int32)
        big1, one = _guarded(1)
        cut_tiles(tf.buf, tf.offsets, tf.hw, _cuda(part), _cuda(geo), one)
        inner = torch.zeros(IN_HW, dtype=torch.bool, device="cuda")
        inner[14:114, 14:145] = True
        assert torch.equal(one[0][inner].view(100, 131, 3), _cuda(frames[1])[13:113, 251:382]) and (one[0][~inner] == 114).all()
        assert (big1[:GUARD] == MARK).all() and (big1[-GUARD:] == MARK).all()
    else:
        assert float(tf.ratio[1]) == 0.64  # (200, 250) into (128, 160): a real resample


def test_cut_does_not_trust_its_tables():
    """a frame index of -1 and beyond nf, an empty window and one that starts at the frame's end: all pad; a window that
    leaves its frame is clamped into it; nothing outside dst is written"""
    from mtgv.detector import fit_geometry
    from mtgv.tiles import cut_tiles

    frames = [sc.noise_frame(h, w, 100 * h + w) for h, w in CUT_SHAPES]
    buf, offsets, hw = _ragged_dev(frames)
    tiles = np.array([[-1, 0, 0, 128, 160], [3, 0, 0, 64, 64], [1, 10, 10, 0, 50], [1, 300, 0, 128, 160], [1, 250, 450, 128, 160],
                      [0, -5, -7, 60, 70], [1, 0, 339, 128, 160]], np.int32)
    clamped = {4: (1, 250, 450, 50, 50), 5: (0, 0, 0, 60, 70), 6: (1, 0, 339, 128, 160)}
    geo = np.tile(np.array([[128, 160, 0, 0]], np.int32), (len(tiles), 1))
    for t, (_, _, _, wh, ww) in clamped.items():
        geo[t] = fit_geometry(wh, ww, *IN_HW)[1:]
    big, dst = _guarded(len(tiles))
    cut_tiles(buf, _cuda(offsets), _cuda(hw.astype(np.int32)), _cuda(tiles), _cuda(geo), dst)
    torch.cuda.synchronize()
    assert (big[:GUARD] == MARK).all() and (big[-GUARD:] == MARK).all()
    for t in range(4):
        assert (dst[t] == 114).all(), t
    _, ref = _reference_cut(frames, list(clamped.values()))
    for i, t in enumerate(clamped):
        assert torch.equal(dst[t], ref.frames[i]), t


# ---------------------------------------------------------------------------
# 2. the merge
# ---------------------------------------------------------------------------
def _tiled(c):
    """a TiledFrames of a case's tables (the merge reads no pixel)"""
    from mtgv.tiles import TiledFrames

    F = len(c["hw"])
    return TiledFrames(torch.zeros((4,), dtype=torch.uint8, device="cuda"), torch.zeros((F,), dtype=torch.int64, device="cuda"), _cuda(c["hw"]),
                       _cuda(c["tiles"]), _cuda(c["tile_start"]), _cuda(c["geo"]), _cuda(c["ratio"]), None, c["tiles"], c["tile_start"], c["hw"])


def _check_merge(c, name):
    from mtgv.tiles import merge_tiles

    want = tc.host(c)
    tf = _tiled(c)
    args = (tf, _cuda(c["n_det"]), _cuda(c["boxes"]), _cuda(c["conf"]), None if c["quads"] is None else _cuda(c["quads"]), c["kt"], _cuda(c["pad_frac"]),
            c["k"], c["edge"], c["ios"], c["max_tiles_per_frame"])
    got, again = merge_tiles(*args), merge_tiles(*args)
    torch.cuda.synchronize()
    for n in tc.OUTPUTS:
        g, a, w = got[n].cpu().numpy(), again[n].cpu().numpy(), want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, (name, n)
        if w.dtype == np.float32:
            g, a, w = sc.bits(g), sc.bits(a), sc.bits(w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{name}: {n} differs from merge_tiles_host at {bad[:4].tolist()}: {got[n].cpu().numpy()[tuple(bad[0])]} != {want[n][tuple(bad[0])]}"
        assert np.array_equal(g, a), f"{name}: {n} differs between two launches"
    return want


def test_merge_designed_cases():
    for name, c in sorted(tc.designed().items()):
        _check_merge(c, name)


@pytest.mark.parametrize("kt", [1, 8, 64])
def test_merge_random_frames(kt):
    """8 frames per launch, 72 in all: every K, with and without quads"""
    n_sel = 0
    for i, k in enumerate((1, 8, 64)):
        want = _check_merge(tc.random_case(100 * kt + k, kt, k, quads=bool((i + kt) % 2)), f"random kt={kt} k={k}")
        n_sel += int(want["n_sel"].sum())
    assert n_sel > 0


def test_merge_at_the_cap_and_beyond_max_tiles():
    want = _check_merge(tc.cap_case(), "cap")
    assert int(want["n_sel"][0]) == 64
    c = dict(tc.designed()["two_frames"], max_tiles_per_frame=2)  # frame 0 has 6 tiles
    assert _check_merge(c, "beyond max_tiles")["n_sel"].tolist() == [0, 2]


# ---------------------------------------------------------------------------
# 3. - 5. the pipelines
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parts(max_batch=32):
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher

    cfg = spec.DetectorConfig(input_hw=IN_HW)
    det = Detector(cfg, spec.random_detector_state(cfg, 3, cls_bias=CLS_BIAS), max_batch=max_batch)
    ecfg = spec.EncoderConfig("ae", ENC_HW, 3, 48, (1, 1, 1, 1), (8, 16, 32, 64), "pool+linear", True)
    enc = Encoder(ecfg, spec.random_encoder_state(ecfg, 1), max_batch=2 * K)
    m = Matcher(48, capacity=64)
    m.add(np.random.default_rng(1).standard_normal((64, 48)).astype(np.float32))
    return det, enc, m


def _pipe(quad_source, max_batch=32, **kw):
    from mtgv.pipeline import Pipeline

    det, enc, m = _parts(max_batch)
    return Pipeline(det, enc, m, K, 1, quad_source=quad_source, **kw)


@pytest.mark.parametrize("quad_source", ["box", "mask"])
def test_one_tile_is_the_untiled_path(quad_source):
    """frames of the input's own size, one window each, no cut rule (edge 0) and no suppression (ios 1: an intersection never
    exceeds the smaller area): every detected slot equals Pipeline.run(SourceFrames).  `boxes` are compared against the untiled
    boxes clipped to the frame - the mapping's clip, the identity on a box that lies inside the frame."""
    from mtgv.pipeline import SourceFrames
    from mtgv.tiles import TiledFrames

    frames = _cuda(np.stack([tc.blocks_frame(*IN_HW, seed) for seed in ONE_TILE_SEEDS]))
    pipe = _pipe(quad_source, tile_merge=dict(edge=0.0, ios=1.0))
    tf = TiledFrames.from_frames(frames, input_hw=IN_HW)
    assert tf.tiles_h.tolist() == [[0, 0, 0, 128, 160], [1, 0, 0, 128, 160]] and torch.equal(tf.frames, frames)
    out = pipe.run(tf)
    ref = pipe.run(SourceFrames.from_frames(frames, input_hw=IN_HW))
    torch.cuda.synchronize()
    n_tile = out["det"]["n_det"].cpu().tolist()
    print("n_det per tile", n_tile, "untiled", ref["n_det"].cpu().tolist())
    assert all(1 <= n <= K for n in n_tile), f"{n_tile} detections per tile: the test wants between 1 and {K}"
    assert out["n_det"].cpu().tolist() == n_tile and ref["n_det"].cpu().tolist() == n_tile
    assert tuple(out["boxes"].shape) == (2, K, 4) and tuple(out["quads_src"].shape) == (2, K, 4, 2) and tuple(out["tile_slot"].shape) == (2, K)
    hi = torch.tensor([IN_HW[1], IN_HW[0], IN_HW[1], IN_HW[0]], dtype=torch.float32, device="cuda")
    for f, n in enumerate(n_tile):
        assert out["tile_slot"][f].cpu().tolist() == [f * K + j for j in range(n)] + [-1] * (K - n)
        assert torch.equal(out["boxes"][f, :n], torch.minimum(torch.maximum(ref["boxes"][f, :n], torch.zeros_like(hi)), hi))
        for name in ("quads_src", "crops", "z", "ids"):
            a, b = (o[name].reshape(2, K, -1) for o in (out, ref))
            assert torch.equal(a[f, :n], b[f, :n]), (name, f)
    assert (out["crops"].float().std(dim=(1, 2, 3)) > 1).all()


TILED_SHAPES = [(300, 420), (256, 320)]


@pytest.mark.parametrize("quad_source,max_batch", [("mask", 32), ("box", 4)])
def test_tiled_step_equals_its_parts(quad_source, max_batch):
    """27 tiles of two frames (16 + 1 and 9 + 1 with the full windows): the step equals Detector.forward on the tiles (in the
    detector's chunks: 4 at a time in the second case), merge_tiles_host and the de-warp with the identity geometry"""
    from mtgv.crop import mask_quads_from_logits, select_cards, warp_quads_src
    from mtgv.tiles import TiledFrames

    frames = [tc.blocks_frame(h, w, 7 * h + w, n_blocks=10) for h, w in TILED_SHAPES]
    buf, offsets, hw = sc.ragged(frames)
    pipe = _pipe(quad_source, max_batch)
    det = pipe.detector
    tf = TiledFrames.from_ragged(_cuda(buf), offsets, hw, window_hw=IN_HW, overlap=48, with_full=True, input_hw=IN_HW)
    assert np.diff(tf.tile_start_h).tolist() == [17, 10] and det.max_batch == max_batch
    out = pipe.run(tf)
    parts = [det.forward(tf.frames[i : i + max_batch], mask_rows=K if quad_source == "mask" else 0) for i in range(0, 27, max_batch)]
    d = {k: (None if v is None else torch.cat([p[k] for p in parts])) for k, v in parts[0].items()}
    torch.cuda.synchronize()
    for k, v in d.items():
        assert (out["det"][k] is None) if v is None else torch.equal(out["det"][k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    quads = None
    if quad_source == "mask":
        sel, _, _ = select_cards(d["n_det"], d["boxes"], pipe._pad_tile, K, want_quads=False)
        quads = mask_quads_from_logits(d["mask_logits"].view(27 * K, *d["mask_logits"].shape[-2:]), sel)[0].cpu().numpy()
    want = tc.merge_tiles_host(d["n_det"].cpu().numpy(), d["boxes"].cpu().numpy(), d["conf"].cpu().numpy(), quads, tf.tiles_h, tf.geo.cpu().numpy(),
                               tf.ratio.cpu().numpy(), tf.tile_start_h, tf.hw_h, tc.pad_frac(K), K, K, 2.0, 0.5)
    print("n_det per tile", d["n_det"].cpu().tolist(), "n_sel", want["n_sel"].tolist())
    n_cand = int(np.minimum(d["n_det"].cpu().numpy(), K).sum())
    assert 0 < int(want["n_sel"].sum()) < n_cand, "the merge had nothing to drop"
    assert np.array_equal(sc.bits(out["boxes"].cpu().numpy().reshape(2 * K, 4)), sc.bits(want["sel_boxes_src"]))
    assert np.array_equal(sc.bits(out["quads_src"].cpu().numpy().reshape(2 * K, 4, 2)), sc.bits(want["quads_src"]))
    assert np.array_equal(out["tile_slot"].cpu().numpy().reshape(-1), want["src_slot"]) and np.array_equal(out["n_det"].cpu().numpy(), want["n_sel"])
    crops, qs = warp_quads_src(tf.sources(), _cuda(want["quads_src"]), _cuda(want["frame_idx"]), ENC_HW, 0.05)
    assert torch.equal(qs, _cuda(want["quads_src"]))  # the identity geometry leaves camera pixels as they are
    assert torch.equal(out["crops"], crops)
    ids, scores = pipe.matcher.match(pipe.encoder.encode(crops), 1)
    assert torch.equal(out["ids"], ids.view(2, K, 1)) and torch.equal(out["scores"].view(torch.int32), scores.view(2, K, 1).view(torch.int32))


def test_tracked_pipeline_tiled_frames():
    """two cameras of different frame sizes over three steps: track_ids, the due sets, the matches and the tracker's state are
    those of a second DeviceTracker fed the step's quads_src and n_det directly"""
    from mtgv.track import DeviceTracker, TrackedPipeline
    from mtgv.tiles import TiledFrames

    pipe = _pipe("mask")
    TOP = 3
    policy = dict(initialization_delay=1)
    tp = TrackedPipeline(pipe, streams=2, top_k=TOP, max_tracks=64, **policy)
    other = DeviceTracker(2, K, 48, TOP, 64, **policy)
    frames = [tc.blocks_frame(h, w, 7 * h + w, n_blocks=10) for h, w in TILED_SHAPES]
    buf, offsets, hw = sc.ragged(frames)
    n_due_total = 0
    for step in range(3):
        tf = TiledFrames.from_ragged(_cuda(buf), offsets, hw, window_hw=IN_HW, overlap=48, with_full=True, input_hw=IN_HW)
        now = [10.0 + 0.6 * step, 10.01 + 0.6 * step]
        out = tp.run(tf, [1, 0], now)
        assert torch.equal(out["quads"], out["quads_src"]) and tuple(out["n_det"].shape) == (2,) and tuple(out["tile_slot"].shape) == (2, K)
        tid, due_idx, n_due_dev = other.update(out["quads_src"], [1, 0], now, n_det=out["n_det"])
        n_due = int(n_due_dev.item())
        assert n_due == out["n_due"] and torch.equal(tid, out["track_ids"]) and torch.equal(due_idx, out["due_idx"])
        if n_due:
            q = other.commit(pipe.encoder.encode(other.gather(out["crops"])[:n_due]))
            ids, scores = other.store(*pipe.matcher.match(q, TOP))
        else:
            ids, scores = other.store()
        assert torch.equal(ids, out["ids"]) and torch.equal(scores.view(torch.int32), out["scores"].view(torch.int32))
        n_due_total += n_due
    assert n_due_total > 0 and int(out["track_ids"].max()) > 0, "no track became due: the run checked nothing"
    for s in range(2):
        a, b = tp.tracker.state(s), other.state(s)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), (s, k)
    assert float(out["quads"][..., 0].max()) > IN_HW[1]  # camera pixels, not the network's
