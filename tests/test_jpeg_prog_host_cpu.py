"""CPU-only: the progressive JPEG path before any GPU run.  tests/host/jpeg_prog_host_check.cpp links the host side
(csrc/jpeg_host.cpp) and includes the scan decode the kernels run (csrc/jpeg_prog_decode.h), is built as a stand-alone
program with AddressSanitizer + UBSan and run over Pillow progressive files and their mutants.  For the intact files it
writes the assembled coefficients out; they must equal, block for block, the coefficients of the same image saved as
a baseline file at the same quality and sampling (libjpeg quantises identically in both modes), which a small baseline
Huffman decoder below reads.  No HIP, no Python extension, nothing preloaded: the program has its own main."""
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mtg-vision_amd", "csrc")
GXX_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _img(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 7) % 256], -1).astype(np.uint8)
    a[: h // 2, w // 2 :] = rng.integers(0, 256, (h // 2, w - w // 2, 3), dtype=np.uint8)
    return a


def baseline_coefficients(data: bytes) -> np.ndarray:
    """(blocks, 64) int16 of a baseline Huffman file: MCU order, natural order within the block, DC predictions undone"""
    pos, tables, comps, ri = 2, {}, [], 0
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        ln = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4 : pos + 2 + ln]
        pos += 2 + ln
        if m == 0xC4:
            o = 0
            while o < len(seg):
                bits = seg[o + 1 : o + 17]
                vals = seg[o + 17 : o + 17 + sum(bits)]
                code, k, lut = 0, 0, {}
                for l in range(1, 17):
                    for _ in range(bits[l - 1]):
                        lut[(l, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                tables[seg[o]] = lut
                o += 17 + len(vals)
        elif m in (0xC0, 0xC1):
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [[seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, 0, 0] for c in range(seg[5])]
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            assert seg[0] == len(comps)
            for j in range(seg[0]):
                comps[j][3], comps[j][4] = seg[2 + 2 * j] >> 4, seg[2 + 2 * j] & 15
            break
    if len(comps) == 1:
        comps[0][1] = comps[0][2] = 1
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    nmcu = -(-w // (8 * hm)) * -(-h // (8 * vm))
    # the bit string of every restart segment, stuffing removed
    segs, cur, i = [], bytearray(), pos
    while True:
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif data[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= data[i + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            segs.append(bytes(cur))
            break
    out = []
    per = ri if ri else nmcu
    assert len(segs) == -(-nmcu // per), (len(segs), nmcu, per)
    for si, sg in enumerate(segs):
        bits = "".join(f"{b:08b}" for b in sg)
        p, pred = 0, [0] * len(comps)

        def sym(lut):
            nonlocal p
            code = 0
            for l in range(1, 17):
                code = (code << 1) | int(bits[p + l - 1])
                if (l, code) in lut:
                    p += l
                    return lut[(l, code)]
            raise AssertionError("bad code")

        def value(s):
            nonlocal p
            if s == 0:
                return 0
            v = int(bits[p : p + s], 2)
            p += s
            return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

        for _ in range(min(per, nmcu - si * per)):
            for ci, (_, ch, cv, td, ta) in enumerate(comps):
                for _ in range(ch * cv):
                    blk = [0] * 64
                    pred[ci] += value(sym(tables[td]))
                    blk[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs = sym(tables[0x10 | ta])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        blk[ZIGZAG[k]] = value(s)
                        k += 1
                    out.append(blk)
    return np.array(out, np.int16)


CASES = [  # name, (h, w), mode, save arguments
    ("m_444_q80.jpg", (37, 57), "RGB", dict(quality=80, subsampling=0)),
    ("m_420_q75_rst.jpg", (37, 57), "RGB", dict(quality=75, subsampling=2, restart_marker_blocks=2)),
    ("m_grey_q80.jpg", (37, 57), "L", dict(quality=80)),
    ("422_q10.jpg", (37, 57), "RGB", dict(quality=10, subsampling=1)),
    ("420_q100.jpg", (37, 57), "RGB", dict(quality=100, subsampling=2)),
    ("420_q10_16x24.jpg", (16, 24), "RGB", dict(quality=10, subsampling=2)),
    ("420_q75_8x24.jpg", (8, 24), "RGB", dict(quality=75, subsampling=2)),
    ("422_q75_7x9_rows.jpg", (7, 9), "RGB", dict(quality=75, subsampling=1, restart_marker_rows=1)),
    ("444_1x1.jpg", (1, 1), "RGB", dict(quality=75, subsampling=0)),
    ("grey_q10_rst.jpg", (17, 33), "L", dict(quality=10, restart_marker_blocks=2)),
    ("420_q90_flat.jpg", (64, 96), "RGB", dict(quality=90, subsampling=2)),
]


def test_progressive_host_code_under_sanitizers(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: sanitizer runs belong on the CPU machine")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    Image = pytest.importorskip("PIL.Image")

    def encode(a, mode, **kw):
        b = io.BytesIO()
        Image.fromarray(a).convert(mode).save(b, "JPEG", **kw)
        return b.getvalue()

    files, want = [], {}
    for k, (name, (h, w), mode, kw) in enumerate(CASES):
        a = _img(h, w, k) if "flat" not in name else np.full((h, w, 3), 97, np.uint8)
        (tmp_path / name).write_bytes(encode(a, mode, progressive=True, **kw))
        files.append(str(tmp_path / name))
        want[name] = baseline_coefficients(encode(a, mode, **kw))
    (tmp_path / "baseline_420.jpg").write_bytes(encode(_img(37, 57), "RGB", quality=80, subsampling=2))
    files.insert(2, str(tmp_path / "baseline_420.jpg"))  # between progressive files in the mixed batch

    exe = str(tmp_path / "jpeg_prog_host_check")
    srcs = [os.path.join(ROOT, "tests", "host", "jpeg_prog_host_check.cpp"), os.path.join(CSRC, "jpeg_host.cpp")]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs]
    ccs = [subprocess.Popen([gxx, *GXX_FLAGS, "-Wall", "-I", CSRC, "-c", s, "-o", o], stderr=subprocess.PIPE, text=True)
           for s, o in zip(srcs, objs)]  # the two translation units side by side
    for cc in ccs:
        err = cc.communicate()[1]
        assert cc.returncode == 0 and err == "", err[-4000:]
    ld = subprocess.run([gxx, *GXX_FLAGS, *objs, "-o", exe], capture_output=True, text=True)
    assert ld.returncode == 0, ld.stderr[-4000:]
    out = tmp_path / "coef"
    out.mkdir()
    r = subprocess.run([exe, str(out), *files], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    m = re.search(r"progressive (\d+) other (\d+) unsupported (\d+) invalid (\d+) \(plans (\d+), refused (\d+), images decoded (\d+), status 1 (\d+)\)",
                  r.stdout)
    assert m is not None, r.stdout
    assert all(int(x) > 0 for x in m.groups()), r.stdout
    for name, ref in want.items():
        got = np.fromfile(out / (name + ".coef"), np.int16).reshape(-1, 64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        bad = np.nonzero((got != ref).any(1))[0]
        assert bad.size == 0, (name, bad[:8].tolist(), got[bad[0]].tolist(), ref[bad[0]].tolist())
