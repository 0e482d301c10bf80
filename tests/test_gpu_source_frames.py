"""Cards cropped from the camera's frames in the batched paths (`SourceFrames`): the ragged letterbox
(mtgv_letterbox_ragged_u8), the de-warp from source frames (mtgv_warp_quads_src) against oracle/warp_ref.py, and their
callers - Pipeline.run / run_many, TrackedPipeline.run, JpegDecoder.decode_sources, JpegFrames(keep_source=True).

Every comparison is exact (bytes, or float32 bit patterns): the kernels restate single operations of the oracles."""
import functools
import io

import numpy as np
import pytest
import torch

import source_frames_common as sc
import track_common as tc
from oracle import resize_ref, warp_ref

pytestmark = pytest.mark.gpu

# the small detector's input, built as tests/test_gpu_rect.py builds its SMALL handles: DetectorConfig(input_hw=(96, 160)) with
# the default imgsz (both sides of input_hw must lie in [32, imgsz], so an imgsz of 96 cannot hold a 160-wide input)
IN_HW = (96, 160)
ENC_HW = (192, 128)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _source_frames(frames, input_hw, surround=None, pad=1003):
    """SourceFrames of a list of numpy frames.  surround: the ragged buffer is a slice in the middle of a larger tensor whose
    other bytes have that value (an odd `pad` in front: the buffer itself starts at an odd address)"""
    from mtgv.pipeline import SourceFrames

    buf, offsets, hw = sc.ragged(frames)
    if surround is None:
        dev = _cuda(buf)
    else:
        big = torch.full((buf.size + 2 * pad,), surround, dtype=torch.uint8, device="cuda")
        big[pad : pad + buf.size] = _cuda(buf)
        dev = big[pad : pad + buf.size]
    return SourceFrames.from_ragged(dev, offsets, hw, input_hw=input_hw)


# ---------------------------------------------------------------------------
# a. the ragged letterbox
# ---------------------------------------------------------------------------
LB_SHAPES = [(37, 53), (96, 128), (96, 64), (20, 30), (241, 321)]


@pytest.mark.parametrize("dst_hw", [(96, 128), (128, 128)])
def test_letterbox_ragged(dst_hw):
    """one launch for five frames of different sizes (an exact fit, a portrait, an upscaled one; every offset behind the first
    is odd) equals mtgv_letterbox_rect_u8 frame by frame and the oracle's letterbox / letterbox_rect, every byte"""
    from mtgv import native as nv
    from mtgv.detector import fit_geometry, rect_geometry

    oh, ow = dst_hw
    frames = [sc.noise_frame(h, w, 100 * h + w) for h, w in LB_SHAPES]
    sf = _source_frames(frames, dst_hw)
    assert [int(o) % 2 for o in sf.offsets.cpu()[1:]] == [1, 1, 1, 1]
    got = sf.frames.cpu().numpy()
    assert got.shape == (len(frames), oh, ow, 3)
    n_oracle = 0
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        r, nh, nw, top, left = fit_geometry(h, w, oh, ow)
        assert sf.geo[i].cpu().tolist() == [nh, nw, top, left] and float(sf.ratio[i]) == r
        one = torch.full((1, oh, ow, 3), 7, dtype=torch.uint8, device="cuda")
        nv.check(nv.lib().mtgv_letterbox_rect_u8(nv.ptr(_cuda(f)), 1, h, w, nv.ptr(one), oh, ow, nh, nw, top, left, 114, nv.stream()))
        np.testing.assert_array_equal(got[i], one[0].cpu().numpy(), err_msg=f"frame {i} {h}x{w} against the per-frame launch")
        if oh == ow:
            np.testing.assert_array_equal(got[i], resize_ref.letterbox(f, oh), err_msg=f"frame {i} against the oracle")
            n_oracle += 1
        elif rect_geometry(h, w, ow, 32)[5:] == (oh, ow):  # (oh, ow) is this frame shape's own LetterBox(auto=True) rectangle
            np.testing.assert_array_equal(got[i], resize_ref.letterbox_rect(f, ow, 32)[0], err_msg=f"frame {i} against the oracle")
            n_oracle += 1
        if (nh, nw) == (h, w):
            np.testing.assert_array_equal(got[i, top : top + nh, left : left + nw], f)
    assert n_oracle >= 4
    # another pad value, into a caller's tensor
    from mtgv.pipeline import SourceFrames

    out = torch.full((len(frames), oh, ow, 3), 9, dtype=torch.uint8, device="cuda")
    sf2 = SourceFrames.from_ragged(sf.buf, sf.offsets, sf.hw, input_hw=dst_hw, pad_value=0, out=out)
    assert sf2.frames.data_ptr() == out.data_ptr()
    got2 = out.cpu().numpy()
    for i, (nh, nw, top, left) in enumerate(sf.geo.cpu().tolist()):
        inner = np.zeros((oh, ow), bool)
        inner[top : top + nh, left : left + nw] = True
        assert np.array_equal(got2[i][inner], got[i][inner]) and (got2[i][~inner] == 0).all() and (got[i][~inner] == 114).all()
    with pytest.raises(AssertionError, match="outside a buffer"):
        SourceFrames.from_ragged(sf.buf[:-1], sf.offsets, sf.hw, input_hw=dst_hw)


# ---------------------------------------------------------------------------
# b. the de-warp from source frames against the oracle
# ---------------------------------------------------------------------------
WARP_SHAPES = [(37, 53), (241, 321), (64, 96)]
WARP_IN = (128, 192)  # the (64, 96) frame's ratio is exactly 2 with no pad: a corner can sit exactly on its last pixel


def _warp_case():
    frames = [sc.noise_frame(h, w, 7 * h + w) for h, w in WARP_SHAPES]
    from mtgv.detector import fit_geometry

    def det(f, pts):  # source pixels of frame f -> the detector input's (float64, rounded to float32 by the array)
        r, _, _, top, left = fit_geometry(*WARP_SHAPES[f], *WARP_IN)
        return [[x * r + left, y * r + top] for x, y in pts]

    quads = np.array([
        det(1, [(60.3, 40.2), (200.7, 52.1), (190.2, 180.9), (50.5, 170.4)]),  # interior
        [[-30, -30], [100, -20], [95, 90], [-25, 85]],                         # over the left and the top border of frame 0: clipped, its first pixel is a tap
        det(1, [(250, 150), (400, 160), (390, 300), (240, 290)]),              # over the right and the bottom border
        det(2, [(-20, -10), (30, -8), (28, 30), (-18, 28)]),                   # over the left and the top border of the last frame
        det(2, [(40, 20), (90, 18), (95, 63), (38, 60)]),                      # a corner exactly on the last frame's last pixel
        det(2, [(10, 10)] * 4),                                                # degenerate: all corners equal, a singular system
    ], np.float32)
    fidx = np.array([1, 0, 1, 2, 2, 2], np.int32)
    return frames, quads, fidx


@pytest.mark.parametrize("out_hw", [(16, 12), ENC_HW])
def test_warp_from_sources_against_the_oracle(out_hw):
    """six quads over three frames whose second and third offsets are no multiples of 4: quads_src is the restatement bit for
    bit, every crop is the oracle's warp of its own source frame byte for byte, and the bytes around the buffer (0x00 or
    0xff) change nothing: no byte outside a frame is used"""
    from mtgv.crop import warp_quads_src

    frames, quads, fidx = _warp_case()
    want_src = sc.map_quads(quads, fidx, WARP_SHAPES, WARP_IN)
    assert want_src[4, 2].tolist() == [95.0, 63.0]
    outs = []
    for surround in (0x00, 0xFF):
        sf = _source_frames(frames, WARP_IN, surround)
        assert sf.buf.data_ptr() % 2 == 1 and int(sf.offsets[1]) % 4 != 0 and int(sf.offsets[2]) % 4 != 0
        crops, quads_src = warp_quads_src(sf, _cuda(quads), _cuda(fidx), out_hw, 0.05)
        torch.cuda.synchronize()
        outs.append((crops.cpu().numpy(), quads_src.cpu().numpy()))
    (c0, q0), (c1, q1) = outs
    assert np.array_equal(sc.bits(q0), sc.bits(want_src)) and np.array_equal(sc.bits(q1), sc.bits(want_src))
    np.testing.assert_array_equal(c0, c1, err_msg="the bytes around the ragged buffer reached a crop")
    for q in range(len(quads)):
        ref = warp_ref.warp_quad(frames[fidx[q]], want_src[q], out_hw, 0.05)
        np.testing.assert_array_equal(c0[q], ref, err_msg=f"quad {q}")
    # the degenerate quad: a singular system, all coefficients 0 - every pixel is the frame's pixel (0, 0), as mtgv_warp_quads gives
    assert (c0[5] == frames[2][0, 0]).all()
    assert all(c0[q].std() > 1 for q in range(5))
    # the clips were taken: corners on the frames' borders, (w, h) of frame 1 among them (taps beyond it are border 0)
    assert want_src[1, 0].tolist() == [0.0, 0.0] and want_src[3, 0].tolist() == [0.0, 0.0] and want_src[2, 2].tolist() == [321.0, 241.0]


def test_warp_from_sources_unknown_frame_is_zeros():
    """a frame index outside [0, nf): a crop of zeros and corners 0, nothing read"""
    from mtgv.crop import warp_quads_src

    frames, quads, fidx = _warp_case()
    sf = _source_frames(frames, WARP_IN)
    bad = np.array([1, 3, -1, 2, 2, 2], np.int32)
    crops, quads_src = warp_quads_src(sf, _cuda(quads), _cuda(bad), (16, 12), 0.05)
    good, good_src = warp_quads_src(sf, _cuda(quads), _cuda(fidx), (16, 12), 0.05)
    assert (crops[1] == 0).all() and (crops[2] == 0).all() and (quads_src[1] == 0).all() and (quads_src[2] == 0).all()
    for q in (0, 3, 4, 5):
        assert torch.equal(crops[q], good[q]) and torch.equal(quads_src[q], good_src[q])


# ---------------------------------------------------------------------------
# c. frames of one size: mtgv_warp_quads on the same tensor
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("out_hw", [(16, 13), ENC_HW])  # width 13: one pixel per thread
def test_one_size_equals_warp_quads(out_hw):
    from mtgv.crop import warp_quads, warp_quads_src
    from mtgv.pipeline import SourceFrames

    frames = _cuda(np.stack([sc.noise_frame(48, 64, 40 + i) for i in range(4)]))
    sf = SourceFrames.from_frames(frames, input_hw=(96, 160))
    assert sf.buf.data_ptr() == frames.data_ptr() and sf.offsets.cpu().tolist() == [i * 48 * 64 * 3 for i in range(4)]
    assert tuple(sf.frames.shape) == (4, 96, 160, 3)
    rng = np.random.default_rng(3)
    base = np.array([[30, 10], [120, 14], [116, 80], [26, 76]], np.float32)
    quads = (base[None] + rng.uniform(-28, 28, (10, 4, 2))).astype(np.float32)
    fidx = (np.arange(10) % 4).astype(np.int32)
    crops, quads_src = warp_quads_src(sf, _cuda(quads), _cuda(fidx), out_hw, 0.05)
    assert np.array_equal(sc.bits(quads_src.cpu().numpy()), sc.bits(sc.map_quads(quads, fidx, [(48, 64)] * 4, (96, 160))))
    assert torch.equal(crops, warp_quads(frames, quads_src, _cuda(fidx), out_hw, 0.05))
    assert (crops.float().std(dim=(1, 2, 3)) > 1).all()
    # frames of the detector's own size are its input: no copy, no launch
    same = SourceFrames.from_frames(frames, input_hw=(48, 64))
    assert same.frames.data_ptr() == frames.data_ptr() and same.geo.cpu().tolist() == [[48, 64, 0, 0]] * 4


# ---------------------------------------------------------------------------
# d. Pipeline.run(SourceFrames)
# ---------------------------------------------------------------------------
F, K = 3, 4
PIPE_SHAPES = [(192, 320), (96, 160), (270, 480)]


def _pattern():
    """a textured (96, 160) pattern: noise with a few flat cards on it"""
    p = sc.noise_frame(96, 160, 5)
    p[20:70, 30:62] = (200, 60, 40)
    p[30:80, 100:130] = (30, 180, 90)
    return p


@functools.lru_cache(maxsize=None)
def _frames():
    """frame 0 is the exact 2 x nearest upsample of the pattern: its letterbox into (96, 160) is the pattern itself"""
    up = np.ascontiguousarray(_pattern().repeat(2, axis=0).repeat(2, axis=1))
    return [up, sc.noise_frame(96, 160, 11), sc.noise_frame(270, 480, 12)]


@functools.lru_cache(maxsize=None)
def _parts(task, cls_bias=-0.9):
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher

    cfg = spec.DetectorConfig(task=task, input_hw=IN_HW)
    det = Detector(cfg, spec.random_detector_state(cfg, 3, cls_bias=cls_bias), max_batch=F)
    ecfg = spec.EncoderConfig("ae", ENC_HW, 3, 48, (1, 1, 1, 1), (8, 16, 32, 64), "pool+linear", True)
    enc = Encoder(ecfg, spec.random_encoder_state(ecfg, 1), max_batch=F * K)
    m = Matcher(48, capacity=64)
    m.add(np.random.default_rng(1).standard_normal((64, 48)).astype(np.float32))
    return det, enc, m


def _pipe(quad_source, thumbs=None, cls_bias=-0.9):
    from mtgv.pipeline import Pipeline

    det, enc, m = _parts("obb" if quad_source == "obb" else "seg", cls_bias)
    return Pipeline(det, enc, m, K, 1, quad_source=quad_source, thumbnail_quality=thumbs)


def _det_quads(pipe, out):
    """the (F * K, 4, 2) quads in the detector input's pixels that a run handed to the de-warp"""
    from mtgv.crop import boxes_to_quads, mask_quads_from_logits

    if pipe.quad_source == "obb":
        return out["quads"].reshape(F * K, 4, 2)
    if pipe.quad_source == "box":
        return boxes_to_quads(out["boxes"].reshape(F * K, 4))
    ml = out["det"]["mask_logits"]
    return mask_quads_from_logits(ml.reshape(F * K, *ml.shape[-2:]), out["boxes"].reshape(F * K, 4))[0]


@pytest.mark.parametrize("quad_source", ["box", "mask", "obb"])
def test_pipeline_run_source_frames(quad_source):
    pytest.importorskip("PIL")
    from PIL import Image

    from mtgv.jpeg import split_files

    frames = _frames()
    pipe = _pipe(quad_source, thumbs=50)
    sf = _source_frames(frames, IN_HW)
    np.testing.assert_array_equal(sf.frames[0].cpu().numpy(), _pattern())
    out = pipe.run(sf)
    ref = pipe.run(sf.frames)
    torch.cuda.synchronize()
    assert "quads_src" not in ref and "quads_src" not in ref["det"]
    assert (set(out), set(out["det"])) == tc.output_keys(quad_source, sources=True, thumbs=True)
    assert (set(ref), set(ref["det"])) == tc.output_keys(quad_source, thumbs=True)
    assert int(out["n_det"].min()) >= K, "the detector found fewer than K detections: the slots would be pad boxes"
    for k, v in ref["det"].items():  # the detections are those of the frames: bit for bit
        assert (out["det"][k] is None) if v is None else torch.equal(out["det"][k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    assert torch.equal(out["boxes"], ref["boxes"])  # boxes stay pixels of the detector's input
    quads = _det_quads(pipe, out).cpu().numpy()
    fidx = np.repeat(np.arange(F), K)
    want_src = sc.map_quads(quads, fidx, PIPE_SHAPES, IN_HW)
    got_src = out["quads_src"].cpu().numpy()
    assert got_src.shape == (F, K, 4, 2) and np.array_equal(sc.bits(got_src.reshape(F * K, 4, 2)), sc.bits(want_src))
    oracle = np.stack([warp_ref.warp_quad(frames[fidx[q]], want_src[q], ENC_HW, 0.05) for q in range(F * K)])
    np.testing.assert_array_equal(out["crops"].cpu().numpy(), oracle)
    assert not torch.equal(out["crops"][:K], ref["crops"][:K])  # (frame 0 at twice the input's resolution: other pixels)
    z = pipe.encoder.encode(_cuda(oracle))
    ids, _ = pipe.matcher.match(z, 1)
    assert torch.equal(out["ids"], ids.view(F, K, 1))
    files = split_files(out["thumbs"], out["thumb_offsets"])
    assert len(files) == F * K
    for j, data in enumerate(files):  # what the encoder's own test expects: Pillow's bytes for the crop
        b = io.BytesIO()
        Image.fromarray(oracle[j]).save(b, "JPEG", quality=50, subsampling=2)
        assert data == b.getvalue(), j


def test_source_crop_is_closer_to_the_camera_frame():
    """The property with no threshold.  Frame 0 is the 2 x nearest upsample of a textured pattern, so the detector's input is
    the pattern itself and both runs crop the same card quads (a detector that finds nothing: the pad boxes, which lie inside
    the frame).  Measured against the oracle's crop of the frame the camera delivered - what the reference computes - the
    crop from the source has a strictly lower mean absolute error than the crop from the letterboxed copy."""
    frames = _frames()
    pipe = _pipe("box", cls_bias=-12.0)
    sf = _source_frames(frames, IN_HW)
    out = pipe.run(sf)
    ref = pipe.run(sf.frames)
    torch.cuda.synchronize()
    assert (out["n_det"] == 0).all()
    boxes = out["boxes"][0].cpu().numpy()
    assert boxes[:, 0].min() >= 0 and boxes[:, 1].min() >= 0 and boxes[:, 2].max() <= IN_HW[1] and boxes[:, 3].max() <= IN_HW[0]
    qs = out["quads_src"][0].cpu().numpy()
    for k in range(K):
        truth = warp_ref.warp_quad(frames[0], qs[k], ENC_HW, 0.05).astype(np.float64)
        e_src = np.abs(out["crops"][k].cpu().numpy() - truth).mean()
        e_box = np.abs(ref["crops"][k].cpu().numpy() - truth).mean()
        print(f"card {k}: mean |crop - oracle| from the source {e_src:.3f}, from the letterboxed copy {e_box:.3f}")
        assert e_src < e_box


# ---------------------------------------------------------------------------
# e. TrackedPipeline.run(SourceFrames)
# ---------------------------------------------------------------------------
def test_tracked_pipeline_source_frames():
    """two cameras of different frame sizes over three steps: the tracker sees camera pixels - track_ids, n_due and ids are
    those of a second DeviceTracker fed quads_src directly"""
    from mtgv.track import DeviceTracker, TrackedPipeline

    pipe = _pipe("mask")
    TOP = 3
    policy = dict(initialization_delay=1)
    tp = TrackedPipeline(pipe, streams=2, top_k=TOP, max_tracks=64, **policy)
    other = DeviceTracker(2, K, 48, TOP, 64, **policy)
    frames = [_frames()[0], _frames()[2]]
    shapes = [f.shape[:2] for f in frames]
    n_due_total = 0
    for step in range(3):
        sf = _source_frames(frames, IN_HW)
        now = [10.0 + 0.6 * step, 10.01 + 0.6 * step]
        out = tp.run(sf, [1, 0], now)
        assert (set(out), set(out["det"])) == tc.output_keys("mask", tracked=True, sources=True)
        quads = _det_quads_2(pipe, out)
        want_src = sc.map_quads(quads, np.repeat(np.arange(2), K), shapes, IN_HW)
        assert np.array_equal(sc.bits(out["quads"].cpu().numpy().reshape(2 * K, 4, 2)), sc.bits(want_src))  # camera pixels
        assert torch.equal(out["quads"], out["quads_src"])
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
    # the larger camera's quads leave the detector input's range: camera pixels, not the network's
    assert float(out["quads"][1, ..., 0].max()) > IN_HW[1]


def _det_quads_2(pipe, out):
    from mtgv.crop import mask_quads_from_logits

    ml = out["det"]["mask_logits"]
    n = ml.shape[0] * ml.shape[1]
    return mask_quads_from_logits(ml.reshape(n, *ml.shape[-2:]), out["boxes"].reshape(n, 4))[0].cpu().numpy()


# ---------------------------------------------------------------------------
# f. JPEG
# ---------------------------------------------------------------------------
def _jpeg(h, w, seed):
    from PIL import Image

    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255 // (w - 1)), (y * 255 // (h - 1)), (x * 3 + y * 5 + seed * 40) % 256], -1).astype(np.uint8)
    a[h // 4 : h // 2, w // 3 : w // 2] = np.random.default_rng(seed).integers(0, 256, (h // 2 - h // 4, w // 2 - w // 3, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=85, subsampling=2)
    return b.getvalue()


def test_decode_sources():
    """frames equal decode_frames' and buf equals decode's, every byte: square, and a rectangle one file fits exactly"""
    pytest.importorskip("PIL")
    from mtgv.jpeg import JpegDecoder

    dec = JpegDecoder(4, 1 << 20, 1 << 20)
    datas = [_jpeg(48, 64, 1), _jpeg(75, 100, 2)]
    buf, offsets, hw, _ = dec.decode(datas)
    for kw in (dict(size=128), dict(input_hw=(48, 64)), dict(input_hw=IN_HW)):
        sf = dec.decode_sources(datas, **kw)
        assert torch.equal(sf.frames, dec.decode_frames(datas, **kw)), kw
        assert torch.equal(sf.buf, buf) and torch.equal(sf.offsets, offsets) and torch.equal(sf.hw, hw)
    assert sf.hw.cpu().tolist() == [[48, 64], [75, 100]] and int(dec.last_status.abs().sum()) == 0
    empty = dec.decode_sources([], input_hw=IN_HW)
    assert tuple(empty.frames.shape) == (0, 96, 160, 3) and empty.buf.numel() == 0


@pytest.mark.parametrize("overlap", ["off", "on"])
def test_jpeg_frames_keep_source(overlap, monkeypatch):
    """three leases over a ring of two: run_many equals run on each batch's decode_sources (buffers are reused), a lease's
    tensor() is still the frames"""
    pytest.importorskip("PIL")
    from mtgv.jpeg import JpegDecoder, JpegFrames

    monkeypatch.setenv("MTGV_OVERLAP", overlap)
    pipe = _pipe("box")
    batches = [[_jpeg(48, 64, 3 * b), _jpeg(75, 100, 3 * b + 1), _jpeg(48, 64, 3 * b + 2)] for b in range(3)]
    dec = JpegDecoder(4, 1 << 20, 1 << 20)
    want = []
    for b in batches:
        o = pipe.run(dec.decode_sources(b, input_hw=IN_HW))
        want.append({k: o[k].clone() for k in ("ids", "crops", "boxes", "quads_src")})
    src = JpegFrames(batches, "cuda", input_hw=IN_HW, depth=2, keep_source=True)
    assert len(src.src_bufs) == 2 and src.src_bufs[0].numel() == 2 * 48 * 64 * 3 + 75 * 100 * 3
    got = pipe.run_many(src.leases(3))
    torch.cuda.synchronize()
    assert len(got) == 3
    for i, (w, o) in enumerate(zip(want, got)):
        for k in w:
            assert torch.equal(w[k], o[k]), (i, k)
    assert not torch.equal(got[0]["crops"], got[2]["crops"])  # (batch 2 reused batch 0's buffers)
    # the frames a lease hands out are the letterboxed ones, and without keep_source nothing changes
    lease = next(iter(JpegFrames(batches[:1], "cuda", input_hw=IN_HW, depth=2, keep_source=True).leases(1)))
    assert torch.equal(lease.tensor(), dec.decode_frames(batches[0], input_hw=IN_HW)) and lease.sources().frames.data_ptr() == lease.tensor().data_ptr()
    plain = next(iter(JpegFrames(batches[:1], "cuda", input_hw=IN_HW, depth=2).leases(1)))
    assert not hasattr(plain, "sources") and torch.equal(plain.tensor(), lease.tensor())
