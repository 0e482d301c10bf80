"""Shared by test_c2f_tail_cpu.py and test_gpu_c2f_tail_direct.py: the cases of the fused C2f tail's direct test
(mtgv_op_c2f_tail, c2f_tail_kernel.h), their seeded draws and the fp64 reference of the operation, with the mistakes a
kernel of this kind is likely to make as switches of that reference.  No GPU needed here.

  t     = SiLU(W1 (*) y_last + b1)             3x3 / stride 1 / pad 1, ch -> ch
  y_new = [y_last +] SiLU(W2 (*) t + b2)       3x3 / stride 1 / pad 1, ch -> ch  (t padded with zeros)
  out   = SiLU(W3 . [cat slices | y_new] + b3) 1x1, (2 + nb) ch -> 2 ch

The reference is torch conv2d in fp64 on NCHW from the values the kernel reads - the unpacked SP8 image of the input
and the exact f32 weights - with nothing rounded in between.

Draws as in test_gpu_sp8_conv.py: input N(0,1), weights N(0,1) / sqrt(K), biases N(0,1); but the first two and the last
two rows of every image are scaled by 8, so that a halo read that crosses into the neighbouring image of a batch moves
the border outputs far past the tolerance."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import sp8_util as sp

Case = namedtuple("Case", "n h w ch nb shortcut cat_ct cat_co out_ct out_co")

# The smallest shapes c2f_tail_ok admits (tiles of 8 x 32 pixels at ch 16, 8 x 16 at ch 32; H, W >= 80)
CASES = [
    Case(1, 80, 96, 16, 1, True, 32, 0, 32, 0),     # minimum size; 30 tiles (ragged over the 8 XCDs); cat has no room for y_new
    Case(2, 88, 96, 16, 1, False, 64, 8, 48, 8),    # a combination no network runs; views with offsets; an image boundary
    Case(1, 80, 128, 16, 1, True, 48, 0, 32, 0),    # 40 tiles (a multiple of 8); tiles inside, not only on borders
    Case(1, 80, 80, 32, 1, False, 64, 0, 64, 0),    # minimum size; 50 tiles; no room for y_new
    Case(2, 80, 96, 32, 1, True, 104, 8, 80, 16),   # scale s's C2f-2 combination; offsets
    Case(1, 88, 80, 32, 2, True, 128, 0, 64, 0),    # rectangular, H not a multiple of 16
    Case(3, 80, 80, 32, 2, False, 136, 8, 72, 8),   # a combination no network runs; three images
]

# Bound of max |fused launch - fp64| on CASES: twice the largest error of the three-launch composition (gemm_sp_kernel,
# not the code under test) against the same reference on these cases, rounded up to one significant digit; the measured
# values are in the docstring of test_gpu_c2f_tail_direct.py (largest 1.04e-5).
TOL = 3e-5

SCALED_ROWS, ROW_SCALE = 2, 8.0
MUTATIONS = ("t_not_zeroed", "shortcut_flipped", "w1_w2_exchanged", "slices_reversed", "cross_image_halo")


def applies(mutation, case):
    """whether the mistake can show at this case at all: the slices in front of y_last can only be out of order where there
    are two of them, and only a batch has a neighbouring image"""
    if mutation == "slices_reversed":
        return case.nb == 2
    if mutation == "cross_image_halo":
        return case.n > 1
    return True


Draw = namedtuple("Draw", "x w1 b1 w2 b2 w3 b3")


def weights(rng, cout, k, cin):
    """[cout][k][k][cin] and bias (test_gpu_sp8_conv.py's draw)"""
    return (rng.standard_normal((cout, k, k, cin)) / np.sqrt(k * k * cin)).astype(np.float32), rng.standard_normal(cout).astype(np.float32)


def draw(case, seed):
    """x: the (1 + nb) ch channels of cat the launch reads as f32 rows [n h w][(1 + nb) ch]; w1, w2 [ch][3][3][ch], w3
    [2 ch][(2 + nb) ch]"""
    n, h, w, ch, nb = case.n, case.h, case.w, case.ch, case.nb
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, (1 + nb) * ch)).astype(np.float32)
    x[:, :SCALED_ROWS] *= np.float32(ROW_SCALE)
    x[:, h - SCALED_ROWS :] *= np.float32(ROW_SCALE)
    w1, b1 = weights(rng, ch, 3, ch)
    w2, b2 = weights(rng, ch, 3, ch)
    w3, b3 = weights(rng, 2 * ch, 1, (2 + nb) * ch)
    return Draw(x.reshape(n * h * w, -1), w1, b1, w2, b2, np.ascontiguousarray(w3.reshape(2 * ch, -1)), b3)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def reference(case, d, mutation=None):
    """fp64 rows [n h w][2 ch] of the tail on the SP8 image of d.x; `mutation` one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    n, h, w, ch, nb = case.n, case.h, case.w, case.ch, case.nb
    xv = sp.unpack(sp.pack(d.x)).reshape(n, h, w, -1)
    if mutation == "cross_image_halo":  # the images one below the other as one map: no zero rows between them
        xv, n, h = xv.reshape(1, n * h, w, -1), 1, n * h
    cat = _d(xv).permute(0, 3, 1, 2)
    slices = [cat[:, i * ch : (i + 1) * ch] for i in range(1 + nb)]
    y_last = slices[nb]
    w1, b1, w2, b2 = (_d(a) for a in (d.w1, d.b1, d.w2, d.b2))
    if mutation == "w1_w2_exchanged":
        w1, b1, w2, b2 = w2, b2, w1, b1
    w1, w2 = w1.permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2)
    if mutation == "t_not_zeroed":  # t where the first conv's zero-padded input gives it, one pixel beyond the frame too
        t = F.silu(F.conv2d(y_last, w1, b1, padding=2))
        y_new = F.silu(F.conv2d(t, w2, b2, padding=0))
    else:
        t = F.silu(F.conv2d(y_last, w1, b1, padding=1))
        y_new = F.silu(F.conv2d(t, w2, b2, padding=1))
    if case.shortcut != (mutation == "shortcut_flipped"):
        y_new = y_last + y_new
    front = slices[:nb][::-1] if mutation == "slices_reversed" else slices[:nb]
    full = torch.cat(front + [y_last, y_new], 1)
    out = F.silu(F.conv2d(full, _d(d.w3)[:, :, None, None], _d(d.b3)))
    return out.permute(0, 2, 3, 1).reshape(-1, 2 * ch).numpy()


def seed_of(index):
    return 7100 + index


@functools.lru_cache(maxsize=None)
def drawn(index):
    """(draw, fp64 reference) of CASES[index], computed once and shared: read-only for every user"""
    d = draw(CASES[index], seed_of(index))
    return d, reference(CASES[index], d)


def flops(case):
    """algorithmic FLOPs of the three layers"""
    m = case.n * case.h * case.w
    return 2.0 * m * (2 * 9 * case.ch**2 + 2 * case.ch * (2 + case.nb) * case.ch)
