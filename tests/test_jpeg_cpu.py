"""CPU-only: the host JPEG probe (mtgv_jpeg_info / mtgv.jpeg.jpeg_info) on Pillow-encoded files - geometry, sampling,
restart interval, unsupported features, malformed input (ERR_INVALID with a message, no crash)."""
import io

import numpy as np
import pytest

PIL = pytest.importorskip("PIL")
from PIL import Image, features  # noqa: E402

TURBO = features.version("libjpeg_turbo")


def _img(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 7) % 256], -1).astype(np.uint8)
    a[: h // 2, w // 2 :] = rng.integers(0, 256, (h // 2, w - w // 2, 3), dtype=np.uint8)
    return a


def _jpeg(a, mode="RGB", **kw):
    b = io.BytesIO()
    Image.fromarray(a).convert(mode).save(b, "JPEG", **kw)
    return b.getvalue()


@pytest.mark.parametrize(
    "kw,mode,sampling,ri",
    [
        (dict(subsampling=0), "RGB", 444, 0),
        (dict(subsampling=1), "RGB", 422, 0),
        (dict(subsampling=2), "RGB", 420, 0),
        (dict(), "L", 400, 0),
        (dict(subsampling=2, optimize=True), "RGB", 420, 0),
        (dict(subsampling=0, restart_marker_blocks=3), "RGB", 444, 3),
        (dict(subsampling=2, restart_marker_rows=2), "RGB", 420, 2 * 4),  # 4 MCUs of 16 px per row at w = 57
        (dict(restart_marker_blocks=5), "L", 400, 5),
    ],
)
def test_info_geometry(kw, mode, sampling, ri):
    from mtgv.jpeg import jpeg_info

    d = _jpeg(_img(37, 57), mode, quality=80, **kw)
    f = jpeg_info(d)
    assert (f.h, f.w) == (37, 57), (f, TURBO)
    assert f.components == (1 if mode == "L" else 3)
    assert f.sampling == sampling and f.restart_interval == ri and f.supported, (f, TURBO)


def test_info_unsupported():
    from mtgv.jpeg import jpeg_info

    a = _img(24, 40)
    f = jpeg_info(_jpeg(a, progressive=True))
    assert not f.supported and "progressive" in f.reason and (f.h, f.w) == (24, 40), f
    f = jpeg_info(_jpeg(a, "CMYK"))
    assert not f.supported and f.components == 4 and "CMYK" in f.reason, f


def _check_invalid(data, what):
    from mtgv import native

    L = native.lib()
    info = (native.c_i32 * 6)()
    import ctypes

    buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    rc = L.mtgv_jpeg_info(buf, len(data), info)
    msg = L.mtgv_last_error().decode()
    assert rc == 1 and msg.startswith("jpeg:"), (what, rc, msg, TURBO)
    return msg


def test_info_malformed():
    from mtgv import native
    from mtgv.jpeg import jpeg_info

    d = _jpeg(_img(32, 48), quality=90)
    assert "no SOI" in _check_invalid(b"\x00" + d[1:], "no SOI")
    assert "empty" in _check_invalid(b"", "empty")
    for cut in (3, 20, len(d) // 2, len(d) - 1):
        _check_invalid(d[:cut], f"truncated at {cut}")
    # no SOS: headers, then EOI
    sos = d.index(b"\xff\xda")
    assert "SOS" in _check_invalid(d[:sos] + b"\xff\xd9", "no SOS")
    # a DHT claiming 17 * 16 = 272 codes
    dht = d.index(b"\xff\xc4")
    bad = bytearray(d)
    bad[dht + 5 : dht + 21] = bytes([17] * 16)
    assert "256" in _check_invalid(bytes(bad), "DHT > 256 codes")
    # Python surface: AssertionError (status 1) with the message
    with pytest.raises(AssertionError, match="jpeg:"):
        jpeg_info(d[:20])
    with pytest.raises(AssertionError, match="empty"):
        jpeg_info(b"")
    assert native.lib().mtgv_jpeg_info(None, 0, None) == 1


def test_decoder_needs_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mtgv.jpeg import JpegDecoder

    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        JpegDecoder(1, 1 << 16, 1 << 16)
