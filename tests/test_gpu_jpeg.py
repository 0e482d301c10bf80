"""GPU JPEG decode (csrc/jpeg.hip, mtgv.jpeg): bit-exact against Pillow (libjpeg-turbo: islow IDCT, fancy upsampling,
fixed-point YCbCr -> RGB) over sizes x qualities x samplings x Huffman tables x restart intervals, ragged batches,
letterboxed frames, a corrupt stream among good ones, the bank's make_cropped and Pipeline.run_many over JpegFrames."""
import io
import random

import numpy as np
import pytest
import torch

PIL = pytest.importorskip("PIL")
from PIL import Image, features  # noqa: E402

pytestmark = pytest.mark.gpu
TURBO = features.version("libjpeg_turbo")

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (480, 640), (488, 680), (1080, 1920)]
QUALITIES = [10, 50, 75, 95, 100]
SAMPLINGS = [0, 1, 2, "L"]  # 4:4:4, 4:2:2, 4:2:0, greyscale


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


def _jpeg(a, q, sub, optimize=False, **kw):
    b = io.BytesIO()
    im = Image.fromarray(a)
    if sub == "L":
        im.convert("L").save(b, "JPEG", quality=q, optimize=optimize, **kw)
    else:
        im.save(b, "JPEG", quality=q, subsampling=sub, optimize=optimize, **kw)
    return b.getvalue()


def _pil(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


_DEC = {}


def _decoder(n=512, nbytes=64 << 20, pix=64 << 20):
    key = (n, nbytes, pix)
    if key not in _DEC:
        from mtgv.jpeg import JpegDecoder

        _DEC[key] = JpegDecoder(n, nbytes, pix)
    return _DEC[key]


def _decode_list(datas):
    dec = _decoder()
    out = []
    # batches within the decoder's limits
    from mtgv.jpeg import _padded_pixels, jpeg_info

    cur, nb, pix = [], 0, 0
    batches = []
    for d in datas:
        p = _padded_pixels(jpeg_info(d))
        if cur and (len(cur) == dec.max_images or nb + len(d) > dec.max_bytes or pix + p > dec.max_pixels):
            batches.append(cur)
            cur, nb, pix = [], 0, 0
        cur.append(d)
        nb += len(d)
        pix += p
    batches.append(cur)
    for b in batches:
        buf, offs, hw, status = dec.decode(b, check=False)
        out += [(t.cpu().numpy(), int(st)) for t, st in zip(dec.images(buf, offs, hw), status.cpu())]
    return out


def _cases(restart=None):
    cases = []
    for si, (h, w) in enumerate(SIZES):
        a = _img(h, w, si)
        for q in QUALITIES:
            for sub in SAMPLINGS:
                for opt in (False, True):
                    kw = {} if restart is None else dict(restart_marker_blocks=restart)
                    cases.append(((h, w, q, sub, opt, restart), _jpeg(a, q, sub, opt, **kw)))
    return cases


def _check(cases):
    got = _decode_list([d for _, d in cases])
    bad = []
    for (key, d), (g, st) in zip(cases, got):
        ref = _pil(d)
        if st != 0 or g.shape != ref.shape or not np.array_equal(g, ref):
            n = int((g != ref).sum()) if g.shape == ref.shape else -1
            bad.append((key, st, n))
    assert not bad, f"{len(bad)} of {len(cases)} differ from Pillow (libjpeg-turbo {TURBO}): {bad[:12]}"


def test_bit_exact_vs_pillow():
    _check(_cases())


@pytest.mark.parametrize("restart", [1, 4, 64])
def test_bit_exact_restart_markers(restart):
    _check(_cases(restart))


def test_ragged_mixed_batch():
    cases = _cases() + _cases(4)
    cases = [c for c in cases if c[0][0] * c[0][1] <= 488 * 680]  # the largest frames are covered above
    random.Random(5).shuffle(cases)
    cases = cases[:400]
    datas = [d for _, d in cases]
    dec = _decoder()
    buf, offs, hw, status = dec.decode(datas)
    assert (status.cpu() == 0).all()
    imgs = dec.images(buf, offs, hw)
    singles = [dec.images(*dec.decode([d])[:3])[0].cpu() for d in datas[:40]]
    for i, (d, g) in enumerate(zip(datas, imgs)):
        assert np.array_equal(g.cpu().numpy(), _pil(d)), (i, cases[i][0], TURBO)
    for g, s in zip(imgs, singles):
        assert torch.equal(g.cpu(), s)


@pytest.mark.parametrize("hw", [(480, 640), (640, 480), (720, 1280)])
def test_decode_frames_letterbox(hw):
    from mtgv.detector import letterbox, letterbox_device

    h, w = hw
    datas = [_jpeg(_img(h, w, s), 80, 2) for s in range(3)]
    dec = _decoder()
    out = dec.decode_frames(datas).cpu().numpy()
    for i, d in enumerate(datas):
        ref = _pil(d)
        lb, _, _ = letterbox_device(torch.from_numpy(ref).cuda())
        assert np.array_equal(out[i], lb[0].cpu().numpy()), (i, hw, TURBO)
        if (h, w) in ((480, 640), (640, 480)):
            assert np.array_equal(out[i], letterbox(ref)[0])


def _corrupt(d, seed):
    """XOR 0x55 into 48 bytes in the middle of the entropy-coded data, never creating or breaking a marker"""
    sos = d.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(d[sos + 2 : sos + 4], "big")
    end = d.rindex(b"\xff\xd9")
    b = bytearray(d)
    rng = np.random.default_rng(seed)
    mid = start + (end - start) // 3
    done = 0
    for p in range(mid, end - 2):
        if done == 48:
            break
        if b[p] in (0xFF, 0xAA) or b[p - 1] == 0xFF or (b[p] ^ 0x55) in (0xFF,):
            continue
        if rng.random() < 0.5:
            b[p] ^= 0x55
            done += 1
    return bytes(b)


def test_corrupt_stream_is_isolated():
    datas = [_jpeg(_img(h, w, i), q, sub) for i, ((h, w), q, sub) in enumerate([((480, 640), 80, 2), ((488, 680), 95, 0), ((17, 33), 50, 1),
                                                                                ((480, 640), 75, "L"), ((256, 256), 90, 2)])]
    datas.append(_jpeg(_img(480, 640, 9), 75, 2, restart_marker_blocks=4))
    bad_idx = [1, 5]
    for j in bad_idx:
        datas[j] = _corrupt(datas[j], j)
    from mtgv.jpeg import jpeg_info

    infos = [jpeg_info(d) for d in datas]
    G = 256
    sizes = [f.h * f.w * 3 for f in infos]
    offs, pos = [], G
    for s in sizes:
        offs.append(pos)
        pos += s + G
    dst = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    dec = _decoder()
    status = dec._launch(datas, dst, np.array(offs, np.int64), np.array([f.w * 3 for f in infos], np.int64))
    st = status.cpu().numpy()
    host = dst.cpu().numpy()
    assert st.tolist() == [1 if i in bad_idx else 0 for i in range(len(datas))], (st, TURBO)
    guard = np.ones(pos, bool)
    for o, s in zip(offs, sizes):
        guard[o : o + s] = False
    assert (host[guard] == 0xA5).all(), "bytes outside the output slots changed"
    for i, (d, f, o) in enumerate(zip(datas, infos, offs)):
        if i not in bad_idx:
            assert np.array_equal(host[o : o + f.h * f.w * 3].reshape(f.h, f.w, 3), _pil(d)), i
    with pytest.raises(RuntimeError, match=r"\[1, 5\]"):
        dec.decode(datas)


def test_make_cropped_jpeg_matches_arrays():
    from mtgv.bank import make_cropped, make_cropped_jpeg

    datas = [_jpeg(_img(680, 488, 100 + i), [75, 90, 95][i % 3], [2, 0, 1][i % 3]) for i in range(256)]
    out = make_cropped_jpeg(datas, (192, 128))
    ref = make_cropped([_pil(d) for d in datas], (192, 128))
    assert torch.equal(out, ref), TURBO


def test_unsupported_raises_before_launch():
    from mtgv.jpeg import JpegDecoder

    dec = _decoder()
    b = io.BytesIO()
    Image.fromarray(_img(32, 32, 0)).save(b, "JPEG", progressive=True)
    with pytest.raises(AssertionError, match="progressive"):
        dec.decode([_jpeg(_img(8, 8, 0), 80, 2), b.getvalue()])
    with pytest.raises(AssertionError, match="at most"):
        JpegDecoder(1, 1 << 10, 1 << 10).decode([_jpeg(_img(64, 64, 0), 80, 2)] * 2)


def test_pipeline_run_many_jpeg_frames():
    from mtgv import spec
    from mtgv.detector import Detector, letterbox
    from mtgv.encoder import Encoder
    from mtgv.jpeg import JpegFrames
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline

    F, K = 32, 4
    det_cfg = spec.DetectorConfig()
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=2000)
    m.add(np.random.default_rng(2).standard_normal((2000, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F),
                    Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1, quad_source="mask")
    datas = [_jpeg(_img(480, 640, 40 + i), 80, 2) for i in range(F)]
    ref_frames = torch.from_numpy(np.stack([letterbox(_pil(d))[0] for d in datas])).cuda()
    src = JpegFrames([datas], "cuda")
    leases = list(src.leases(1))
    outs = pipe.run_many(iter(leases))
    ref = pipe.run_many([ref_frames])
    torch.cuda.synchronize()
    assert (leases[0].status.cpu() == 0).all()
    for k in ("ids", "scores", "boxes", "crops"):
        assert torch.equal(outs[0][k].cpu(), ref[0][k].cpu()), k
