"""GPU decode of progressive JPEG files (csrc/jpeg_prog.hip, mtgv.jpeg with progressive=True): bit-exact against Pillow
(libjpeg-turbo) over the smallest shapes at which the scan walk can go wrong - sizes whose padded MCU grid is larger than
the scans' own block grids, every sampling, qualities with long EOB runs and with dense refinement, restart intervals - a
flat 1024 x 1024 image (one EOB run in the top category), ragged batches mixed with baseline files, a cut scan among good
files, and the bank-build helpers.  tests/golden/jpeg_progressive.npz holds a dozen of the small files with Pillow's RGB
output, so that the exactness check also runs where Pillow is absent or links another libjpeg; running this file as a
script writes it."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_progressive.npz")

SIZES = [(1, 1), (7, 9), (8, 24), (16, 24), (17, 33), (37, 57)]
QUALITIES = [10, 75, 100]
SAMPLINGS = [0, 1, 2, "L"]  # 4:4:4, 4:2:2, 4:2:0, greyscale


def _img(h, w, seed):
    """tests/test_gpu_jpeg.py::_img: gradients, flat regions (long zero runs: EOB runs) and noise (large categories)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.empty((h, w, 3), np.uint8)
    a[..., 0] = (x * 255 // max(w - 1, 1)).astype(np.uint8)
    a[..., 1] = (y * 255 // max(h - 1, 1)).astype(np.uint8)
    a[..., 2] = ((x * 3 + y * 5) % 256).astype(np.uint8)
    a[h // 3 : 2 * h // 3, : w // 2] = rng.integers(0, 256, 3, dtype=np.uint8)  # flat
    a[: h // 2, w // 2 :] = rng.integers(0, 256, (h // 2, w - w // 2, 3), dtype=np.uint8)  # noise
    return a


def _jpeg(a, q, sub, progressive=True, **kw):
    from PIL import Image

    b = io.BytesIO()
    im = Image.fromarray(a)
    if sub == "L":
        im.convert("L").save(b, "JPEG", quality=q, progressive=progressive, **kw)
    else:
        im.save(b, "JPEG", quality=q, subsampling=sub, progressive=progressive, **kw)
    return b.getvalue()


def _pil(d):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


_DEC = {}


def _decoder(progressive=True):
    if progressive not in _DEC:
        from mtgv.jpeg import JpegDecoder

        _DEC[progressive] = JpegDecoder(512, 16 << 20, 8 << 20, progressive=progressive, max_scans=5120 if progressive else None)
    return _DEC[progressive]


def _check(cases):
    """cases: (key, file); one batch through the progressive decoder, every image equal to Pillow's"""
    dec = _decoder()
    buf, offs, hw, status = dec.decode([d for _, d in cases], check=False)
    st = status.cpu().numpy()
    bad = []
    for (key, d), g, s in zip(cases, dec.images(buf, offs, hw), st):
        ref, g = _pil(d), g.cpu().numpy()
        if s != 0 or g.shape != ref.shape or not np.array_equal(g, ref):
            bad.append((key, int(s), int((g != ref).sum()) if g.shape == ref.shape else -1))
    assert not bad, f"{len(bad)} of {len(cases)} differ from Pillow: {bad[:12]}"


def _small_cases(**kw):
    return [((h, w, q, sub, tuple(kw.items())), _jpeg(_img(h, w, si), q, sub, **kw)) for si, (h, w) in enumerate(SIZES) for q in QUALITIES
            for sub in SAMPLINGS]


def _golden_cases():
    """a dozen small files: every sampling, the three qualities, both restart forms, the grids that differ from the MCU grid"""
    picks = [((8, 24), 75, 2, {}), ((16, 24), 10, 2, {}), ((17, 33), 100, 2, {}), ((37, 57), 75, 1, {}), ((37, 57), 10, 0, {}),
             ((37, 57), 100, "L", {}), ((7, 9), 75, 1, {}), ((1, 1), 75, 2, {}), ((37, 57), 75, 2, dict(restart_marker_blocks=2)),
             ((37, 57), 10, "L", dict(restart_marker_blocks=2)), ((17, 33), 75, 2, dict(restart_marker_rows=1)),
             ((16, 24), 100, 0, dict(restart_marker_rows=1))]
    return [_jpeg(_img(h, w, i), q, sub, **kw) for i, ((h, w), q, sub, kw) in enumerate(picks)]


def test_golden_files_bit_exact():
    """no Pillow needed: the committed files against the RGB that Pillow 12.2 / libjpeg-turbo gave for them"""
    z = np.load(GOLDEN)
    n = int(z["n"])
    assert n >= 12
    datas = [z[f"file{i}"].tobytes() for i in range(n)]
    from mtgv.jpeg import jpeg_info

    assert all(jpeg_info(d, progressive=True).progressive for d in datas)
    dec = _decoder()
    buf, offs, hw, status = dec.decode(datas)
    assert (status.cpu() == 0).all()
    for i, g in enumerate(dec.images(buf, offs, hw)):
        assert np.array_equal(g.cpu().numpy(), z[f"rgb{i}"]), i
    # one at a time: the same pixels
    for i in (0, 5, 8):
        g = dec.images(*dec.decode([datas[i]])[:3])[0]
        assert np.array_equal(g.cpu().numpy(), z[f"rgb{i}"]), i


def test_bit_exact_vs_pillow():
    pytest.importorskip("PIL")
    _check(_small_cases())


@pytest.mark.parametrize("kw", [dict(restart_marker_blocks=2), dict(restart_marker_rows=1)], ids=["blocks2", "rows1"])
def test_bit_exact_restart_markers(kw):
    pytest.importorskip("PIL")
    _check(_small_cases(**kw))


def test_flat_image_one_long_eob_run():
    """1024 x 1024 flat grey: 16384 all-zero luma blocks, one EOB run in the top category per scan; then one noisy corner"""
    pytest.importorskip("PIL")
    a = np.full((1024, 1024, 3), 128, np.uint8)
    b = a.copy()
    b[:64, :64] = np.random.default_rng(3).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    _check([(("flat", sub), _jpeg(a, 90, sub)) for sub in (2, "L")] + [(("corner", sub), _jpeg(b, 90, sub)) for sub in (2, "L")])


def test_ragged_mixed_batch():
    """baseline and progressive files of different sizes interleaved through one progressive handle; the baseline images
    bit-identical to what a default handle gives"""
    pytest.importorskip("PIL")
    cases = []
    for si, (h, w) in enumerate(SIZES + [(120, 200)]):
        for k, sub in enumerate(SAMPLINGS):
            prog = (si + k) % 2 == 0
            kw = dict(restart_marker_blocks=3) if (si + k) % 3 == 0 else {}
            cases.append(((h, w, sub, prog), _jpeg(_img(h, w, 10 + si), [75, 10, 100][k % 3], sub, progressive=prog, **kw), prog))
    datas = [d for _, d, _ in cases]
    dec = _decoder()
    buf, offs, hw, status = dec.decode(datas)
    assert (status.cpu() == 0).all()
    imgs = [g.cpu() for g in dec.images(buf, offs, hw)]
    for (key, d, _), g in zip(cases, imgs):
        assert np.array_equal(g.numpy(), _pil(d)), key
    base = [i for i, c in enumerate(cases) if not c[2]]
    plain = _decoder(False)
    b2, o2, hw2, _ = plain.decode([datas[i] for i in base])
    for i, g in zip(base, plain.images(b2, o2, hw2)):
        assert torch.equal(imgs[i], g.cpu()), cases[i][0]


def _cut_last_scan(d):
    """the last scan's entropy-coded data cut to half, EOI kept"""
    sos = d.rindex(b"\xff\xda")
    start = sos + 2 + int.from_bytes(d[sos + 2 : sos + 4], "big")
    end = d.rindex(b"\xff\xd9")
    cut = start + (end - start) // 2
    if d[cut - 1] == 0xFF:
        cut -= 1
    return d[:cut] + b"\xff\xd9"


def test_cut_scan_is_isolated():
    pytest.importorskip("PIL")
    from mtgv.jpeg import jpeg_info

    datas = [_jpeg(_img(120, 200, 1), 75, 2), _jpeg(_img(97, 131, 2), 90, 2), _jpeg(_img(64, 64, 3), 75, 0, progressive=False),
             _jpeg(_img(88, 40, 4), 90, "L"), _jpeg(_img(33, 65, 5), 50, 1)]
    bad_idx = [1, 3]
    for j in bad_idx:
        datas[j] = _cut_last_scan(datas[j])
    infos = [jpeg_info(d, progressive=True) for d in datas]
    assert all(f.supported for f in infos), infos
    G = 256  # canary bytes before, between and behind the output slots
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
    assert st.tolist() == [1 if i in bad_idx else 0 for i in range(len(datas))], st
    guard = np.ones(pos, bool)
    for o, s in zip(offs, sizes):
        guard[o : o + s] = False
    assert (host[guard] == 0xA5).all(), "bytes outside the output slots changed"
    for i, (d, f, o) in enumerate(zip(datas, infos, offs)):
        if i not in bad_idx:
            assert np.array_equal(host[o : o + f.h * f.w * 3].reshape(f.h, f.w, 3), _pil(d)), i
    with pytest.raises(RuntimeError, match=r"\[1, 3\]"):
        dec.decode(datas)


def test_refusals_before_launch():
    pytest.importorskip("PIL")
    from mtgv.jpeg import JpegDecoder

    d = _jpeg(_img(24, 40, 0), 75, 2)
    with pytest.raises(AssertionError, match="scans"):
        JpegDecoder(4, 1 << 16, 1 << 16, progressive=True, max_scans=19).decode([d, d])  # 20 scans
    sos = [i for i in range(len(d) - 1) if d[i] == 0xFF and d[i + 1] == 0xDA]
    with pytest.raises(AssertionError, match="incomplete progression"):
        _decoder().decode([d, d[: sos[-1]] + b"\xff\xd9"])


def test_make_cropped_jpeg_progressive_matches_arrays():
    pytest.importorskip("PIL")
    from mtgv.bank import make_cropped, make_cropped_jpeg

    datas = [_jpeg(_img(680, 488, 100 + i), [75, 90, 95][i % 3], [2, 0, 1][i % 3]) for i in range(64)]
    out = make_cropped_jpeg(datas, (192, 128))
    ref = make_cropped([_pil(d) for d in datas], (192, 128))
    assert torch.equal(out, ref)


def test_build_bank_jpeg_mixed():
    pytest.importorskip("PIL")
    from mtgv import spec
    from mtgv.adapters import VectorStoreQdrant
    from mtgv.bank import build_bank_jpeg
    from mtgv.encoder import Encoder

    cfg = spec.encoder_config("cnvnxt2ae_nano")
    enc = Encoder(cfg, spec.random_encoder_state(cfg, 1), max_batch=8)
    cards = [(f"00000000-0000-0000-0000-{i:012d}", _jpeg(_img(204, 146, i), 90, 2, progressive=i % 2 == 0)) for i in range(11)]
    store = VectorStoreQdrant(capacity=64)
    assert build_bank_jpeg(cards, enc, store, batch_size=4) == 11
    assert build_bank_jpeg(cards, enc, store, batch_size=4) == 0  # already present


if __name__ == "__main__":  # writes the golden file
    files = _golden_cases()
    arrays = {"n": np.int64(len(files))}
    for i, d in enumerate(files):
        arrays[f"file{i}"] = np.frombuffer(d, np.uint8)
        arrays[f"rgb{i}"] = _pil(d)
    np.savez_compressed(GOLDEN, **arrays)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
