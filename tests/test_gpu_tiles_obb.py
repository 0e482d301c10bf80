"""Tiled detection for OBB detectors on the GPU: the rotated merge (mtgv_tiles_merge_obb) against
mtgv.tiles.merge_tiles_obb_host, its pair function (mtgv_op_quad_inter) against quad_inter_host, and their callers
Pipeline.run(TiledFrames) and TrackedPipeline.run(TiledFrames) of an OBB pipeline with tile_merge={"rule": "rotated"}.

Every comparison is exact (bytes, or float32 bit patterns): the kernels restate single operations of their host rules."""
import functools

import numpy as np
import pytest
import torch

import source_frames_common as sc
import tiles_common as tc
import tiles_obb_common as oc

pytestmark = pytest.mark.gpu

MARK, GUARD = 0x5A, 1024


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tiled(c):
    """a TiledFrames of a case's tables (the merge reads no pixel)"""
    from mtgv.tiles import TiledFrames

    F = len(c["hw"])
    return TiledFrames(torch.zeros((4,), dtype=torch.uint8, device="cuda"), torch.zeros((F,), dtype=torch.int64, device="cuda"), _cuda(c["hw"]),
                       _cuda(c["tiles"]), _cuda(c["tile_start"]), _cuda(c["geo"]), _cuda(c["ratio"]), None, c["tiles"], c["tile_start"], c["hw"])


# ---------------------------------------------------------------------------
# 1. the merge kernel, through the ABI into guarded buffers
# ---------------------------------------------------------------------------
def _launch(c):
    """mtgv_tiles_merge_obb into outputs that lie between guard bytes -> (outputs as numpy, the guards are untouched)"""
    from mtgv import native

    F, k, kt = len(c["hw"]), c["k"], c["kt"]
    shapes = {"sel_boxes_src": ((F * k, 4), torch.float32), "quads_src": ((F * k, 4, 2), torch.float32), "frame_idx": ((F * k,), torch.int32),
              "sel_conf": ((F * k,), torch.float32), "src_slot": ((F * k,), torch.int32), "n_sel": ((F,), torch.int32), "state": ((F * k,), torch.int32),
              "oriented_by": ((F * k,), torch.int32)}
    raw, out = {}, {}
    for n, (shape, dt) in shapes.items():
        raw[n] = torch.full((2 * GUARD + int(np.prod(shape)) * 4,), MARK, dtype=torch.uint8, device="cuda")
        out[n] = raw[n][GUARD:-GUARD].view(dt).view(shape)
    tf = _tiled(c)
    dev = [_cuda(c[n]) for n in ("n_det", "conf", "cls", "quads", "state")] + [_cuda(c["pad_frac"])]
    mt = tf.max_tiles_per_frame if c["max_tiles_per_frame"] is None else int(c["max_tiles_per_frame"])
    native.check(native.lib().mtgv_tiles_merge_obb(
        *(native.ptr(t) for t in dev[:5]), c["tiles"].shape[0], c["conf"].shape[1], kt, native.ptr(tf.tiles), native.ptr(tf.geo), native.ptr(tf.ratio),
        native.ptr(tf.tile_start), native.ptr(tf.hw), F, mt, native.ptr(dev[5]), k, float(c["edge"]), float(c["ios"]), int(c["card_cls"]),
        *(native.ptr(out[n]) for n in oc.OUTPUTS), native.stream()))
    torch.cuda.synchronize()
    clean = all(bool((r[:GUARD] == MARK).all()) and bool((r[-GUARD:] == MARK).all()) for r in raw.values())
    return {n: out[n].cpu().numpy() for n in oc.OUTPUTS}, clean


def _check_merge(c, name, want=None):
    want = oc.host(c) if want is None else want
    got, clean = _launch(c)
    again, _ = _launch(c)
    assert clean, f"{name}: a guard byte around an output was written"
    for n in oc.OUTPUTS:
        g, a, w = got[n], again[n], want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, (name, n)
        if w.dtype == np.float32:
            g, a, w = sc.bits(g), sc.bits(a), sc.bits(w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{name}: {n} differs from merge_tiles_obb_host at {bad[:4].tolist()}: {got[n][tuple(bad[0])]} != {want[n][tuple(bad[0])]}"
        assert np.array_equal(g, a), f"{name}: {n} differs between two launches"
    return want


def test_merge_designed_cases():
    for name, c in sorted(oc.designed().items()):
        _check_merge(c, name)


@pytest.mark.parametrize("seed,kt,k", oc.RANDOM)
def test_merge_random_frames(seed, kt, k):
    want = _check_merge(oc.random_case(seed, kt, k), f"random seed={seed} kt={kt} k={k}")
    assert int(want["n_sel"].sum()) > 0


def test_merge_at_the_cap():
    want = _check_merge(oc.cap_case(), "cap")
    assert int(want["n_sel"][0]) == 64 and set(want["state"].tolist()) == {1, 2}


def test_merge_nan_inf_and_garbage_tile_start():
    want = _check_merge(oc.nan_case(), "nan")
    assert np.isnan(want["quads_src"]).any()
    n_sel = [_check_merge(c, f"tile_start {c['tile_start'].tolist()}")["n_sel"].tolist() for c in oc.garbage_tile_start_cases()]
    assert n_sel == [[2, 0], [0, 2], [0, 0], [0, 0]]  # ([0, 8, 8]: 8 tiles exceed max_tiles_per_frame = 7)
    c = dict(oc.designed()["two_frames"], max_tiles_per_frame=2)
    assert _check_merge(c, "beyond max_tiles")["n_sel"].tolist() == [0, 2]


def test_merge_tiles_obb_wrapper():
    """the Python entry writes the same as the ABI call"""
    from mtgv.tiles import merge_tiles_obb

    c = oc.designed()["two_frames"]
    want = oc.host(c)
    got = merge_tiles_obb(_tiled(c), *(_cuda(c[n]) for n in ("n_det", "conf", "cls", "quads", "state")), c["kt"], _cuda(c["pad_frac"]), c["k"], c["edge"],
                          c["ios"], c["card_cls"])
    assert set(got) == set(oc.OUTPUTS)
    for n in oc.OUTPUTS:
        assert np.array_equal(got[n].cpu().numpy().view(np.int32), want[n].view(np.int32)), n


def test_quad_inter_equals_the_host_rule():
    """4096 pairs: the card-like generator of the CPU test and every analytic case"""
    from mtgv.tiles import quad_inter, quad_inter_host

    ana = oc.analytic_pairs()
    a, b = oc.card_pairs(4096 - len(ana), seed=1)
    a, b = np.concatenate([a, np.stack([p[1] for p in ana])]), np.concatenate([b, np.stack([p[2] for p in ana])])
    assert a.shape == (4096, 4, 2)
    want = quad_inter_host(a, b)
    got = quad_inter(_cuda(a), _cuda(b))
    torch.cuda.synchronize()
    for n, g, w in zip(("inter", "area_a", "area_b"), got, want):
        bad = np.argwhere(sc.bits(g.cpu().numpy()) != sc.bits(w))
        assert bad.size == 0, f"{n} differs at {bad[:4].tolist()}: {g.cpu().numpy()[bad[0][0]]} != {w[bad[0][0]]}"
    assert np.array_equal(got[0].cpu().numpy()[-len(ana):], np.array([p[3] for p in ana], np.float32))


# ---------------------------------------------------------------------------
# 2. the pipelines: YOLO11n-obb at 640 x 640, the AE-nano encoder, a 1000-row bank
# ---------------------------------------------------------------------------
ENC_HW = (192, 128)
K = 8
DET_SEED = 3
TILED_SHAPES = [(700, 900), (720, 880)]


@functools.lru_cache(maxsize=None)
def _parts():
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher

    cfg = spec.yolo11_config(task="obb")
    det = Detector(cfg, spec.random_detector_state(cfg, DET_SEED, cls_bias=-0.9), max_batch=4)
    ecfg = spec.encoder_config("cnvnxt2ae_nano", ENC_HW, "conv+linear")
    enc = Encoder(ecfg, spec.random_encoder_state(ecfg, 1), max_batch=2 * K)
    m = Matcher(ecfg.z_size, capacity=1000)
    m.add(np.random.default_rng(1).standard_normal((1000, ecfg.z_size)).astype(np.float32))
    return det, enc, m


def _pipe(**tile_merge):
    from mtgv.pipeline import Pipeline

    det, enc, m = _parts()
    return Pipeline(det, enc, m, K, 1, quad_source="obb", tile_merge=tile_merge or None)


def _tiled_batch():
    from mtgv.tiles import TiledFrames

    frames = [tc.blocks_frame(h, w, 7 * h + w, n_blocks=10) for h, w in TILED_SHAPES]
    buf, offsets, hw = sc.ragged(frames)
    tf = TiledFrames.from_ragged(_cuda(buf), offsets, hw, window_hw=(640, 640), overlap=128, with_full=True)
    assert np.diff(tf.tile_start_h).tolist() == [5, 5]
    return frames, tf


def test_the_refusal_stays_without_the_switch():
    _, tf = _tiled_batch()
    with pytest.raises(NotImplementedError, match="obb.*rotated overlap rule"):
        _pipe().run(tf)


def test_one_tile_is_the_untiled_path():
    """a 640 x 640 frame as a single window, no cut rule (edge 0) and no suppression (ios 2: an intersection never exceeds the
    smaller area): every card slot equals Pipeline.run(SourceFrames) of the frame - quads_src, card_state, crops and ids.  The
    detector's own count (det.n_det, every class) is the untiled n_det; the step's n_det is the number of cards, which the
    untiled path reports as card_state > 0."""
    from mtgv.pipeline import SourceFrames
    from mtgv.tiles import TiledFrames

    frames = _cuda(tc.blocks_frame(640, 640, 21, n_blocks=10)[None])
    pipe = _pipe(rule="rotated", edge=0.0, ios=2.0)
    tf = TiledFrames.from_frames(frames)
    assert tf.tiles_h.tolist() == [[0, 0, 0, 640, 640]] and torch.equal(tf.frames, frames)
    out = pipe.run(tf)
    ref = pipe.run(SourceFrames.from_frames(frames))
    torch.cuda.synchronize()
    n = int(out["n_det"][0])
    print("cards", n, "detections", ref["n_det"].cpu().tolist(), "states", ref["card_state"].cpu().tolist())
    assert 1 <= n <= K, f"{n} cards: the test wants between 1 and {K}"
    assert torch.equal(out["det"]["n_det"], ref["n_det"]) and n == int((ref["card_state"] > 0).sum())
    assert tuple(out["quads_src"].shape) == (1, K, 4, 2) and tuple(out["card_state"].shape) == (1, K) and tuple(out["tile_slot"].shape) == (1, K)
    assert out["tile_slot"][0].cpu().tolist() == list(range(n)) + [-1] * (K - n)
    assert torch.equal(out["quads"], out["quads_src"])
    for name in ("quads_src", "card_state", "crops", "z", "ids"):
        a, b = (o[name].reshape(1, K, -1) for o in (out, ref))
        assert torch.equal(a[0, :n], b[0, :n]), name
    assert (out["card_state"][0, n:] == 0).all() and (out["crops"][:n].float().std(dim=(1, 2, 3)) > 1).all()


def test_tiled_step_equals_its_parts():
    """10 tiles of two frames (4 + the full window each), forward in chunks of 4: the step equals Detector.forward on the
    tiles, obb_cards per tile, merge_tiles_obb_host, the oracle's de-warp of those quads from the source frames, the encoder and
    the matcher - bit for bit"""
    from mtgv.crop import obb_cards
    from oracle import warp_ref

    frames, tf = _tiled_batch()
    pipe = _pipe(rule="rotated")
    det = pipe.detector
    out = pipe.run(tf)
    parts = [det.forward(tf.frames[i : i + 4]) for i in range(0, 10, 4)]
    d = {k: (None if v is None else torch.cat([p[k] for p in parts])) for k, v in parts[0].items()}
    torch.cuda.synchronize()
    for k, v in d.items():
        assert (out["det"][k] is None) if v is None else torch.equal(out["det"][k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    quads, _, _, state = obb_cards(d["n_det"], d["rboxes"], d["conf"], d["cls"], pipe._pad_tile, K, 0, 1, 2)
    want = oc.merge_tiles_obb_host(d["n_det"].cpu().numpy(), d["conf"].cpu().numpy(), d["cls"].cpu().numpy(), quads.cpu().numpy(), state.cpu().numpy(),
                                   tf.tiles_h, tf.geo.cpu().numpy(), tf.ratio.cpu().numpy(), tf.tile_start_h, tf.hw_h, tc.pad_frac(K), K, K, 2.0, 0.5, 0)
    n_cand = int((state > 0).sum())
    print("n_det per tile", d["n_det"].cpu().tolist(), "card slots", n_cand, "n_sel", want["n_sel"].tolist(), "state", want["state"].tolist(),
          "oriented_by", want["oriented_by"].tolist())
    assert int(want["n_sel"].sum()) > 0
    assert np.array_equal(sc.bits(out["boxes"].cpu().numpy().reshape(2 * K, 4)), sc.bits(want["sel_boxes_src"]))
    assert np.array_equal(sc.bits(out["quads_src"].cpu().numpy().reshape(2 * K, 4, 2)), sc.bits(want["quads_src"]))
    assert torch.equal(out["quads"], out["quads_src"])
    assert np.array_equal(out["tile_slot"].cpu().numpy().reshape(-1), want["src_slot"]) and np.array_equal(out["n_det"].cpu().numpy(), want["n_sel"])
    assert np.array_equal(out["card_state"].cpu().numpy().reshape(-1), want["state"])
    oracle = np.stack([warp_ref.warp_quad(frames[int(want["frame_idx"][q])], want["quads_src"][q], ENC_HW, 0.05) for q in range(2 * K)])
    np.testing.assert_array_equal(out["crops"].cpu().numpy(), oracle)
    z = pipe.encoder.encode(_cuda(oracle))
    ids, scores = pipe.matcher.match(z, 1)
    assert torch.equal(out["z"], z) and torch.equal(out["ids"], ids.view(2, K, 1))
    assert torch.equal(out["scores"].view(torch.int32), scores.view(2, K, 1).view(torch.int32))


def test_tracked_pipeline_tiled_frames():
    """two steps of the same batch: the ids the first step gave are the second step's, and the tracker saw quads_src with
    card_state - a second DeviceTracker fed them directly gives the same ids, due sets and state"""
    from mtgv.track import DeviceTracker, TrackedPipeline

    pipe = _pipe(rule="rotated")
    policy = dict(initialization_delay=0)
    tp = TrackedPipeline(pipe, streams=2, top_k=1, max_tracks=64, **policy)
    other = DeviceTracker(2, K, pipe.encoder.cfg.z_size, 1, 64, **policy)
    _, tf = _tiled_batch()
    ids = []
    for step in range(2):
        now = [10.0 + 0.6 * step, 10.01 + 0.6 * step]
        out = tp.run(tf, [1, 0], now)
        assert torch.equal(out["quads"], out["quads_src"]) and tuple(out["card_state"].shape) == (2, K) and tuple(out["n_det"].shape) == (2,)
        assert out["n_det"].cpu().tolist() == (out["card_state"] > 0).sum(1).cpu().tolist()
        tid, due_idx, n_due = other.update(out["quads_src"], [1, 0], now, state=out["card_state"])
        assert int(n_due.item()) == out["n_due"] and torch.equal(tid, out["track_ids"]) and torch.equal(due_idx, out["due_idx"])
        if out["n_due"]:
            other.store(*pipe.matcher.match(other.commit(pipe.encoder.encode(other.gather(out["crops"])[: out["n_due"]])), 1))
        else:
            other.store()
        ids.append(out["track_ids"].cpu().numpy())
    card = out["card_state"].cpu().numpy() > 0
    assert card.any() and (ids[0][card] > 0).all() and np.array_equal(ids[0], ids[1]), (ids[0].tolist(), ids[1].tolist())
    assert (ids[1][~card] == 0).all()
    for s in range(2):
        a, b = tp.tracker.state(s), other.state(s)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), (s, k)
