"""GPU JPEG encode (csrc/jpeg_enc.hip, mtgv.jpeg.JpegEncoder): byte-identical to Pillow (libjpeg-turbo defaults) over
sizes x qualities x 4:2:0 / 4:4:4, batch independence, no write past the files, limits checked before any launch, a
round trip through the GPU decoder, Pipeline thumbnails (run, run_many, MTGV_OVERLAP=on) and TrackerCtx."""
import io

import numpy as np
import pytest
import torch

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (33, 17), (192, 128), (128, 192), (480, 640), (488, 680)]
QUALITIES = [1, 10, 50, 75, 95, 100]


def _img(h, w, seed):
    """gradients, flat regions (long zero runs: EOB / ZRL) and noise (large AC categories)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.empty((h, w, 3), np.uint8)
    a[..., 0] = (x * 255 // max(w - 1, 1)).astype(np.uint8)
    a[..., 1] = (y * 255 // max(h - 1, 1)).astype(np.uint8)
    a[..., 2] = ((x * 3 + y * 5) % 256).astype(np.uint8)
    a[h // 3 : 2 * h // 3, : w // 2] = rng.integers(0, 256, 3, dtype=np.uint8)  # flat
    a[: h // 2, w // 2 :] = rng.integers(0, 256, (h // 2, w - w // 2, 3), dtype=np.uint8)  # noise
    return a


def _pil(a, q=50, sampling=420):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=q, subsampling=2 if sampling == 420 else 0)
    return b.getvalue()


_ENC = {}


def _enc():
    from mtgv.jpeg import JpegEncoder

    if "e" not in _ENC:
        _ENC["e"] = JpegEncoder(8, 8 * 496 * 688)
    return _ENC["e"]


@pytest.mark.parametrize("sampling", [420, 444])
@pytest.mark.parametrize("q", QUALITIES)
def test_bytes_equal_pillow(q, sampling):
    enc = _enc()
    for h, w in SIZES:
        imgs = np.stack([_img(h, w, 100 * h + w + k) for k in range(3)])
        files = enc.encode(torch.from_numpy(imgs).cuda(), q, sampling)
        for k in range(3):
            want = _pil(imgs[k], q, sampling)
            assert files[k] == want, (h, w, q, sampling, k, len(files[k]), len(want))


def test_noise_q100_444_largest_within_bound():
    from mtgv.jpeg import jpeg_encode_bound

    enc = _enc()
    for h, w in [(8, 8), (17, 33), (192, 128), (488, 680)]:
        a = np.random.default_rng(h * w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        files = enc.encode(torch.from_numpy(a).cuda(), 100, 444)
        for k in range(2):
            assert files[k] == _pil(a[k], 100, 444), (h, w, k)
            assert len(files[k]) <= jpeg_encode_bound(h, w, 444)


def test_all_ff_stuffing():
    """flat and striped images at the extremes (0 / 255) at quality 100: stuffing and 1-bit padding of the last byte"""
    enc = _enc()
    for v in (0, 255, 128):
        for s in (420, 444):
            a = np.full((3, 24, 40, 3), v, np.uint8)
            a[1, ::2] = 255 - v
            files = enc.encode(torch.from_numpy(a).cuda(), 100, s)
            for k in range(3):
                assert files[k] == _pil(a[k], 100, s), (v, s, k)


def test_batch_independence():
    enc = _enc()
    imgs = torch.from_numpy(np.stack([_img(192, 128, 7 + k) for k in range(8)])).cuda()
    many = enc.encode(imgs, 50, 420)
    for k in range(8):
        assert enc.encode(imgs[k : k + 1], 50, 420)[0] == many[k], k


def test_no_writes_past_output_and_limits():
    from mtgv.jpeg import JpegEncoder, jpeg_encode_bound

    enc = JpegEncoder(4, 4 * 192 * 128)
    imgs = torch.from_numpy(np.stack([_img(192, 128, k) for k in range(4)])).cuda()
    cap = 4 * jpeg_encode_bound(192, 128, 420)
    guard = 0xA5
    for q in (50, 100):
        out = torch.full((cap + 4096,), guard, dtype=torch.uint8, device="cuda")
        buf, offs = enc.encode_device(imgs, q, 420, out=out)
        torch.cuda.synchronize()
        off = offs.cpu().numpy()
        assert off[0] == 0 and (np.diff(off) > 0).all()
        tail = out[int(off[-1]) :].cpu().numpy()
        assert (tail == guard).all(), q
        data = out[: int(off[-1])].cpu().numpy().tobytes()
        for k in range(4):
            assert data[off[k] : off[k + 1]] == _pil(imgs[k].cpu().numpy(), q, 420), (q, k)
    # refused before any launch: the guard bytes stay untouched
    out = torch.full((cap - 1,), guard, dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError, match="jpeg: output capacity"):
        enc.encode_device(imgs, 50, 420, out=out)
    with pytest.raises(AssertionError, match="jpeg: 5 images"):
        enc.encode_device(torch.cat([imgs, imgs[:1]]), 50, 420)
    with pytest.raises(AssertionError, match="jpeg: batch needs"):
        enc.encode_device(torch.zeros((2, 400, 192, 3), dtype=torch.uint8, device="cuda"), 50, 420)
    with pytest.raises(AssertionError, match="jpeg: quality"):
        enc.encode_device(imgs, 0, 420)
    with pytest.raises(AssertionError, match="jpeg: sampling"):
        enc.encode_device(imgs, 50, 422)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == guard).all()
    # the handle still works after the refusals
    assert enc.encode(imgs[:1], 50, 420)[0] == _pil(imgs[0].cpu().numpy(), 50, 420)


def test_round_trip_gpu_decoder():
    from mtgv.jpeg import JpegDecoder

    enc = _enc()
    files = []
    for h, w in [(7, 9), (17, 33), (192, 128), (480, 640)]:
        for s in (420, 444):
            imgs = torch.from_numpy(np.stack([_img(h, w, h + w + s)])).cuda()
            files += enc.encode(imgs, 75, s)
    dec = JpegDecoder(len(files), sum(len(f) for f in files), len(files) * 496 * 688)
    buf, offs, hw, status = dec.decode(files)
    assert (status.cpu() == 0).all()
    for f, im in zip(files, JpegDecoder.images(buf, offs, hw)):
        want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        assert np.array_equal(im.cpu().numpy(), want)


def _pipeline(thumbs, F, K):
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline

    det_cfg = spec.DetectorConfig()
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=2000)
    m.add(np.random.default_rng(2).standard_normal((2000, 768)).astype(np.float32))
    det = Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F)
    enc = Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K)
    return (Pipeline(det, enc, m, K, 1, quad_source="mask"),
            Pipeline(det, enc, m, K, 1, quad_source="mask", thumbnail_quality=thumbs))


@pytest.mark.parametrize("overlap", ["off", "on"])
def test_pipeline_thumbnails(overlap, monkeypatch):
    from mtgv.jpeg import split_files

    monkeypatch.setenv("MTGV_OVERLAP", overlap)
    F, K = 4, 4
    plain, thumbed = _pipeline(50, F, K)
    assert plain._jpeg is None
    g = torch.Generator(device="cuda").manual_seed(21)
    batches = [torch.randint(0, 256, (F, 640, 640, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(3)]
    ref = plain.run_many(batches)
    got = thumbed.run_many(batches)
    single = thumbed.run(batches[0])
    torch.cuda.synchronize()
    assert "thumbs" not in ref[0]
    for r, o in zip(ref + ref[:1], got + [single]):
        for k in ("ids", "scores", "boxes", "crops", "z"):
            assert torch.equal(r[k].cpu(), o[k].cpu()), k
        assert o["thumb_offsets"].shape == (F * K + 1,) and o["thumb_offsets"].dtype == torch.int64
        files = split_files(o["thumbs"], o["thumb_offsets"])
        crops = o["crops"].cpu().numpy()
        assert len(files) == F * K
        for j in range(F * K):
            assert files[j] == _pil(crops[j], 50, 420), j


def test_tracker_ctx_gpu_thumbnails():
    """TrackerCtx(jpeg_encoder=...) gives the same to_dict() lists as the Pillow default on the same frames"""
    from mtgv import spec
    from mtgv.adapters import CardSegmenter, CoreMlEncoder, QdrantPoint, VectorStoreQdrant
    from mtgv.detector import Detector
    from mtgv.jpeg import JpegEncoder
    from mtgv.tracker import TrackerCtx

    cfg = spec.DetectorConfig()
    seg = CardSegmenter(detector=Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=1))
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    enc = CoreMlEncoder(state_dict=spec.random_encoder_state(enc_cfg, 1), max_batch=16)
    rng = np.random.default_rng(5)
    db = VectorStoreQdrant(capacity=256)
    db.save_points(QdrantPoint(id=f"id-{i}", vector=v.tolist(), payload={"n": i}) for i, v in enumerate(rng.standard_normal((200, 768)).astype(np.float32)))
    frames = [np.random.default_rng(8 + k).integers(0, 256, (480, 640, 3), dtype=np.uint8) for k in range(2)]
    frames = [frames[0]] * 3 + [frames[1]] * 2
    now = [10.0]
    a = TrackerCtx(0.5, 0.1, segmenter=seg, encoder=enc.model, vecs=db, clock=lambda: now[0])
    b = TrackerCtx(0.5, 0.1, segmenter=seg, encoder=enc.model, vecs=db, clock=lambda: now[0], jpeg_encoder=JpegEncoder(64, 64 * 192 * 128))
    seen = 0
    for f in frames:
        da = [o.to_dict() for o in a.update(f)]
        db_ = [o.to_dict() for o in b.update(f)]
        now[0] += 0.2
        assert da == db_
        seen += len(da)
        assert all(d["img"] for d in db_)
    assert seen > 0
