"""CPU-only: the host composition that folds Proto's ConvTranspose2d(k2, s2, bias) into the 3x3 conv behind it
(mtgv_op_proto_fold_compose, detector.h).

  - the composed weights We [4][o][dy][dx][c] and the nine-class bias table against an fp64 composition written here
    from the formula: per element |got - ref| <= 2^-24 |ref|, one rounding to f32;
  - the fold as a function: four 2x2 phase convs over the zero-padded low-resolution map with the fp64 composition,
    against conv_transpose2d -> conv2d(padding=1) in fp64 at 1e-12 relative, on grids where borders coincide (1x1: all
    four in one pixel; 1x4: top and bottom), an odd grid and two images."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from mtgv import native

    if not os.path.exists(native.LIB_PATH):
        subprocess.run([sys.executable, os.path.join(ROOT, "mtg-vision_amd", "build.py")], check=True)
    return native.lib()


def taps(a, d):
    """S(a, d): the (t, k) of phase a that read low-resolution offset d"""
    out = []
    for t in range(3):
        r = a + t - 1
        if r // 2 - (a - 1) == d:  # floor division
            out.append((t, r % 2))  # non-negative modulus
    return out


def test_tap_sets():
    assert taps(0, 0) == [(0, 1)] and taps(0, 1) == [(1, 0), (2, 1)]
    assert taps(1, 0) == [(0, 0), (1, 1)] and taps(1, 1) == [(2, 0)]


def compose64(wt, bt, w2, b2):
    """fp64: wt (c, m, 2, 2), bt (m), w2 [o][3][3][m], b2 [o] -> We [4][o][2][2][c], bias9 [9][o]"""
    wt, bt, w2, b2 = (np.asarray(x, dtype=np.float64) for x in (wt, bt, w2, b2))
    c, o = wt.shape[0], w2.shape[0]
    we = np.zeros((4, o, 2, 2, c))
    for a in range(2):
        for b in range(2):
            for dy in range(2):
                for dx in range(2):
                    for ty, kh in taps(a, dy):
                        for tx, kw in taps(b, dx):
                            we[2 * a + b, :, dy, dx, :] += w2[:, ty, tx, :] @ wt[:, :, kh, kw].T
    bias9 = np.zeros((9, o))
    inside = {0: (1, 2), 1: (0, 1, 2), 2: (0, 1)}  # class -> cv2 taps whose upsampled pixel exists
    for rc in range(3):
        for cc in range(3):
            bias9[3 * rc + cc] = b2 + sum(w2[:, ty, tx, :] @ bt for ty in inside[rc] for tx in inside[cc])
    return we, bias9


def params(rng, c):
    wt = (rng.standard_normal((c, c, 2, 2)) / np.sqrt(c)).astype(np.float32)
    bt = rng.standard_normal(c).astype(np.float32)
    w2 = (rng.standard_normal((c, 3, 3, c)) / np.sqrt(9 * c)).astype(np.float32)
    b2 = rng.standard_normal(c).astype(np.float32)
    return wt, bt, w2, b2


def compose_native(lib, wt, bt, w2, b2):
    from mtgv import native as nv

    c, mid, o = wt.shape[0], wt.shape[1], w2.shape[0]
    we = np.full((4, o, 2, 2, c), np.nan, dtype=np.float32)
    b9 = np.full((9, o), np.nan, dtype=np.float32)
    arrs = [np.ascontiguousarray(x) for x in (wt, bt, w2, b2)]
    nv.check(lib.mtgv_op_proto_fold_compose(*[x.ctypes.data_as(C.c_void_p) for x in arrs], c, mid, o, we.ctypes.data_as(C.c_void_p),
                                            b9.ctypes.data_as(C.c_void_p)))
    return we, b9


@pytest.mark.parametrize("c", [8, 64])
def test_composition_is_one_rounding_of_fp64(lib, c):
    rng = np.random.default_rng(100 + c)
    p = params(rng, c)
    we, b9 = compose_native(lib, *p)
    we64, b964 = compose64(*p)
    for name, got, ref in (("We", we, we64), ("bias9", b9, b964)):
        assert np.isfinite(got).all()
        excess = np.abs(got.astype(np.float64) - ref) - 2.0**-24 * np.abs(ref)
        print(f"proto fold compose c={c} {name}: max |got - ref| / |ref| = {np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)):.3g}")
        assert (excess <= 0).all(), (name, float(excess.max()))


def apply_fold64(x, we, bias9):
    """x (n, h, w, c) fp64 -> (n, 2h, 2w, o): out(2i + a, 2j + b) = sum We[a, b][o][dy][dx][c] x[i + a - 1 + dy][j + b - 1 + dx][c] + bias"""
    n, h, w, c = x.shape
    o = we.shape[1]
    xp = np.zeros((n, h + 2, w + 2, c))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((n, 2 * h, 2 * w, o))
    for a in range(2):
        for b in range(2):
            acc = np.zeros((n, h, w, o))
            for dy in range(2):
                for dx in range(2):
                    acc += xp[:, a + dy : a + dy + h, b + dx : b + dx + w] @ we[2 * a + b, :, dy, dx, :].T
            out[:, a::2, b::2] = acc
    cls = lambda k, size: np.where(k == 0, 0, np.where(k == size - 1, 2, 1))
    rc, cc = cls(np.arange(2 * h), 2 * h), cls(np.arange(2 * w), 2 * w)
    return out + bias9[3 * rc[:, None] + cc[None, :]][None]


def unfolded64(x, wt, bt, w2, b2):
    """conv_transpose2d -> conv2d(padding=1) in fp64, NHWC in and out"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    y = F.conv_transpose2d(t(x).permute(0, 3, 1, 2), t(wt), t(bt), stride=2)
    y = F.conv2d(y, t(w2).permute(0, 3, 1, 2), t(b2), padding=1)
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("c", [8, 64])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 1, 4), (1, 5, 7), (2, 5, 7)])
def test_fold_is_the_same_function(c, n, h, w):
    rng = np.random.default_rng(200 + c)
    p = params(rng, c)
    x = rng.standard_normal((n, h, w, c))
    got = apply_fold64(x, *compose64(*p))
    ref = unfolded64(x, *p)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"proto fold function c={c} {(n, h, w)}: max relative difference {err:.3g}")
    assert err < 1e-12


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7)])
def test_phase_launches_as_described(lib, n, h, w):
    """the library's f32 composition applied the way Detector::proto describes its four launches - a 2x2 / stride-1 conv
    over the low-resolution map with (1 - a) rows of padding above and (1 - b) columns left, taps in (dy, dx, c) order,
    row (i, j) written to pixel (2i + a, 2j + b), bias by the border class of that pixel - against the layers in fp64.
    Bound: the composition's one f32 rounding per weight, 2^-24, over K = 4 c products of O(1) terms plus the bias,
    taken as 1e-5 of the output's scale."""
    c = 64
    rng = np.random.default_rng(300)
    p = params(rng, c)
    we, b9 = compose_native(lib, *p)
    x = rng.standard_normal((n, h, w, c))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    out = torch.zeros(n, c, 2 * h, 2 * w, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            wq = torch.from_numpy(we[2 * a + b].astype(np.float64)).permute(0, 3, 1, 2)  # [o][dy][dx][c] -> (o, c, dy, dx)
            out[:, :, a::2, b::2] = F.conv2d(F.pad(xt, (1 - b, b, 1 - a, a)), wq)
    cls = lambda k, size: np.where(k == 0, 0, np.where(k == size - 1, 2, 1))
    table = b9.astype(np.float64)[3 * cls(np.arange(2 * h), 2 * h)[:, None] + cls(np.arange(2 * w), 2 * w)[None, :]]
    got = out.permute(0, 2, 3, 1).numpy() + table[None]
    ref = unfolded64(x, *p)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"proto fold launches {(n, h, w)}: max relative difference {err:.3g}")
    assert err < 1e-5
