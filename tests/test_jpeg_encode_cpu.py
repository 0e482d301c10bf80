"""CPU-only: the host side of the GPU JPEG encoder (mtgv.jpeg.jpeg_header / jpeg_encode_bound): the header equals
Pillow's file through the end of SOS byte for byte, parses as the decoder expects, invalid arguments are refused
with a `jpeg:` message, and the encoder refuses to run without a GPU."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

SIZES = [(1, 1), (7, 9), (17, 33), (192, 128), (128, 192), (480, 640)]
QUALITIES = [1, 5, 10, 25, 50, 75, 90, 100]


def _sos_end(d: bytes) -> int:
    q = 2
    while True:
        m, n = d[q + 1], d[q + 2] << 8 | d[q + 3]
        q += 2 + n
        if m == 0xDA:
            return q


@pytest.mark.parametrize("sampling", [420, 444])
@pytest.mark.parametrize("q", QUALITIES)
def test_header_equals_pillow(q, sampling):
    Image = pytest.importorskip("PIL.Image")
    from mtgv.jpeg import jpeg_header

    for h, w in SIZES:
        b = io.BytesIO()
        Image.fromarray(np.full((h, w, 3), 77, np.uint8)).save(b, "JPEG", quality=q, subsampling=2 if sampling == 420 else 0)
        ref = b.getvalue()
        assert jpeg_header(h, w, q, sampling) == ref[: _sos_end(ref)], (h, w, q, sampling)


@pytest.mark.parametrize("sampling", [420, 444])
def test_header_parses(sampling):
    from mtgv import native
    from mtgv.jpeg import jpeg_header

    for h, w in SIZES + [(65535, 65535)]:
        d = jpeg_header(h, w, 50, sampling) + b"\x00\xff\xd9"  # + one byte of entropy-coded data and EOI
        info = (C.c_int32 * 6)()
        native.check(native.lib().mtgv_jpeg_info(C.create_string_buffer(d, len(d)), len(d), info))
        assert list(info) == [h, w, 3, sampling, 0, 1], (h, w, list(info))


def test_header_quality_1_is_baseline():
    """force_baseline: every table entry fits 8 bits (255 at quality 1)"""
    from mtgv.jpeg import jpeg_header

    d = jpeg_header(8, 8, 1, 420)
    assert d[20:25] == b"\xff\xdb\x00\x43\x00" and d[89:94] == b"\xff\xdb\x00\x43\x01"  # 8-bit tables 0 and 1
    assert d[25:89] == bytes([255] * 64) and d[94:158] == bytes([255] * 64)


def test_bound():
    from mtgv.jpeg import jpeg_encode_bound, jpeg_header

    # 623 header + 2 x (blocks x 1660 bits) + EOI: 4:2:0 has 6 blocks per 16 x 16 MCU, 4:4:4 3 per 8 x 8
    assert jpeg_encode_bound(192, 128, 420) == 623 + 2 * (12 * 8 * 6 * 1660 // 8) + 2
    assert jpeg_encode_bound(1, 1, 444) == 623 + 2 * -(-3 * 1660 // 8) + 2
    assert jpeg_encode_bound(17, 17, 420) == jpeg_encode_bound(32, 32, 420)
    assert len(jpeg_header(1, 1)) == 623


def _rejects(fn, *args):
    from mtgv import native

    rc = fn(*args)
    assert rc == 1, (args, rc)
    assert native.lib().mtgv_last_error().startswith(b"jpeg:"), native.lib().mtgv_last_error()


def test_host_functions_reject_bad_arguments():
    from mtgv import native

    L = native.lib()
    n = C.c_int64(0)
    buf = (C.c_uint8 * 1024)()
    for h, w, s in [(0, 8, 420), (8, 0, 420), (65536, 8, 420), (8, 65536, 444), (8, 8, 422), (8, 8, 400), (8, 8, 0)]:
        _rejects(L.mtgv_jpeg_encode_bound, h, w, s, C.byref(n))
        _rejects(L.mtgv_jpeg_encode_header, h, w, 50, s, buf, 1024, C.byref(n))
    for q in (0, -1, 101, 1000):
        _rejects(L.mtgv_jpeg_encode_header, 8, 8, q, 420, buf, 1024, C.byref(n))
    _rejects(L.mtgv_jpeg_encode_header, 8, 8, 50, 420, buf, 622, C.byref(n))
    assert L.mtgv_jpeg_encode_header(8, 8, 50, 420, buf, 623, C.byref(n)) == 0 and n.value == 623
    from mtgv.jpeg import jpeg_encode_bound, jpeg_header

    with pytest.raises(AssertionError, match="jpeg: quality"):
        jpeg_header(8, 8, 0)
    with pytest.raises(AssertionError, match="jpeg: sampling"):
        jpeg_encode_bound(8, 8, 422)


def test_encoder_requires_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mtgv.jpeg import JpegEncoder

    with pytest.raises(RuntimeError, match="no HIP device"):
        JpegEncoder(4, 4 * 192 * 128)
