"""CPU-only: the host probe for progressive files (mtgv_jpeg_info_ex / mtgv.jpeg.jpeg_info(d, progressive=True)) on
Pillow-encoded files - geometry, scan counts, the default probe's refusal, an incomplete progression, an illegal scan
script, and every truncation at a marker boundary (ERR_INVALID with a message, no crash)."""
import ctypes
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


def _markers(d):
    """offsets of every marker segment of the file (SOI first, EOI last); entropy-coded data is stepped over"""
    out, p = [0], 2
    while p < len(d):
        assert d[p] == 0xFF, p
        m = d[p + 1]
        out.append(p)
        if m == 0xD9:
            break
        p += 2 + ((d[p + 2] << 8) | d[p + 3])
        if m == 0xDA:
            while not (d[p] == 0xFF and d[p + 1] != 0 and not 0xD0 <= d[p + 1] <= 0xD7):
                p += 1
    return out


@pytest.mark.parametrize(
    "kw,mode,sampling,ri,scans",
    [
        (dict(subsampling=0), "RGB", 444, 0, 10),
        (dict(subsampling=1), "RGB", 422, 0, 10),
        (dict(subsampling=2), "RGB", 420, 0, 10),
        (dict(), "L", 400, 0, 6),
        (dict(subsampling=0, restart_marker_blocks=3), "RGB", 444, 3, 10),
        (dict(subsampling=2, restart_marker_rows=2), "RGB", 420, 2 * 4, 10),  # 4 MCUs of 16 px per row at w = 57
        (dict(restart_marker_blocks=5), "L", 400, 5, 6),
    ],
)
def test_info_progressive(kw, mode, sampling, ri, scans):
    from mtgv import native
    from mtgv.jpeg import jpeg_info

    assert native.lib().mtgv_version() >= 106
    d = _jpeg(_img(37, 57), mode, quality=80, progressive=True, **kw)
    f = jpeg_info(d, progressive=True)
    assert f.supported and f.progressive and f.reason == "", (f, TURBO)
    assert (f.h, f.w) == (37, 57) and f.components == (1 if mode == "L" else 3), (f, TURBO)
    assert f.sampling == sampling and f.restart_interval == ri and f.scans == scans, (f, TURBO)
    g = jpeg_info(d)  # the default probe is unchanged
    assert not g.supported and "progressive" in g.reason and not g.progressive and g.scans == 1, g
    # a baseline file through the progressive probe: what the default probe says
    b = _jpeg(_img(37, 57), mode, quality=80, **kw)
    assert jpeg_info(b, progressive=True) == jpeg_info(b) and jpeg_info(b).supported and not jpeg_info(b).progressive


def test_info_incomplete_progression():
    from mtgv.jpeg import jpeg_info

    d = _jpeg(_img(24, 40), quality=80, progressive=True)
    sos = [p for p in _markers(d) if d[p + 1] == 0xDA]
    assert len(sos) == 10
    last = sos[-1]  # Y 1-63 refinement 1 -> 0: without it luma AC stays at Al 1
    f = jpeg_info(d[:last] + b"\xff\xd9", progressive=True)
    assert not f.supported and f.progressive and f.scans == 9, f
    assert "incomplete progression" in f.reason and "component 0" in f.reason and "Al 1" in f.reason, f


def test_info_illegal_script():
    from mtgv.jpeg import jpeg_info

    d = _jpeg(_img(24, 40), quality=80, progressive=True)
    sos = [p for p in _markers(d) if d[p + 1] == 0xDA]
    # scan 5 is the first luma refinement, Ah 2 Al 1 (the last byte of its SOS segment): claim Ah 3 Al 2 instead
    p = sos[5] + 2 + ((d[sos[5] + 2] << 8) | d[sos[5] + 3]) - 1
    assert d[p] == 0x21, hex(d[p])
    for ahal in (0x32, 0x20, 0x01):  # wrong Ah; Al != Ah - 1; a second first scan
        bad = bytearray(d)
        bad[p] = ahal
        with pytest.raises(AssertionError, match=r"jpeg: SOS of scan 5: illegal"):
            jpeg_info(bytes(bad), progressive=True)
    # an AC scan with Ss = 0
    bad = bytearray(d)
    bad[p - 2] = 0
    with pytest.raises(AssertionError, match=r"jpeg: SOS of scan 5: illegal spectral selection"):
        jpeg_info(bytes(bad), progressive=True)


def test_info_truncated_at_every_marker():
    from mtgv import native

    L = native.lib()
    for mode, kw in (("RGB", dict(subsampling=2)), ("L", dict(restart_marker_blocks=2))):
        d = _jpeg(_img(24, 40), mode, quality=80, progressive=True, **kw)
        cuts = _markers(d)[1:]
        assert len(cuts) > 15
        for cut in cuts + [c + 1 for c in cuts] + [c + 3 for c in cuts if c + 3 < len(d)]:
            info = (native.c_i32 * 8)()
            buf = ctypes.create_string_buffer(d[:cut], cut)
            rc = L.mtgv_jpeg_info_ex(buf, cut, native.JPEG_PROGRESSIVE, info)
            msg = L.mtgv_last_error().decode()
            assert rc == 1 and msg.startswith("jpeg:"), (mode, cut, rc, msg, TURBO)
    assert L.mtgv_jpeg_info_ex(None, 0, native.JPEG_PROGRESSIVE, None) == 1
    info = (native.c_i32 * 8)()
    assert L.mtgv_jpeg_info_ex(ctypes.create_string_buffer(d, len(d)), len(d), 2, info) == 1 and b"flags" in L.mtgv_last_error()
