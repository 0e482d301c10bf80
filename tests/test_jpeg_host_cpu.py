"""CPU-only: the JPEG codecs' host side (csrc/jpeg_host.cpp: marker walk, decode plan, staging image, encoder header)
built as a stand-alone program with AddressSanitizer + UBSan (tests/host/jpeg_host_check.cpp) and run over Pillow files
and their mutants.  No HIP, no Python extension, nothing preloaded: the program has its own main."""
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


def _img(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 7) % 256], -1).astype(np.uint8)
    a[: h // 2, w // 2 :] = rng.integers(0, 256, (h // 2, w - w // 2, 3), dtype=np.uint8)
    return a


def test_host_code_under_sanitizers(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: sanitizer runs belong on the CPU machine")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    Image = pytest.importorskip("PIL.Image")

    def save(name, a, mode="RGB", **kw):
        b = io.BytesIO()
        Image.fromarray(a).convert(mode).save(b, "JPEG", **kw)
        p = tmp_path / name
        p.write_bytes(b.getvalue())
        return str(p)

    small = _img(37, 57)
    files = [
        save("444.jpg", small, quality=80, subsampling=0),
        save("420_restart.jpg", small, quality=80, subsampling=2, restart_marker_blocks=3),
        save("grey.jpg", small, "L", quality=80),
        save("422_optimised.jpg", small, quality=80, subsampling=1, optimize=True),
        save("progressive.jpg", small, quality=80, progressive=True),
        save("420_640x480.jpg", _img(480, 640, 1), quality=80, subsampling=2),
    ]
    exe = str(tmp_path / "jpeg_host_check")
    srcs = [os.path.join(ROOT, "tests", "host", "jpeg_host_check.cpp"), os.path.join(CSRC, "jpeg_host.cpp")]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs]
    ccs = [subprocess.Popen([gxx, *GXX_FLAGS, "-Wall", "-I", CSRC, "-c", s, "-o", o], stderr=subprocess.PIPE, text=True)
           for s, o in zip(srcs, objs)]  # the two translation units side by side
    for cc in ccs:
        err = cc.communicate()[1]
        assert cc.returncode == 0 and err == "", err[-4000:]
    ld = subprocess.run([gxx, *GXX_FLAGS, *objs, "-o", exe], capture_output=True, text=True)
    assert ld.returncode == 0, ld.stderr[-4000:]
    r = subprocess.run([exe, *files], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    m = re.search(r"supported (\d+) unsupported (\d+) invalid (\d+)", r.stdout)
    assert m is not None, r.stdout
    assert all(int(x) > 0 for x in m.groups()), r.stdout
