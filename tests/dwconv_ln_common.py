"""Shared by test_dwconv_ln_cpu.py and test_gpu_dwconv_ln_direct.py: the cases of dwconv7_ln's direct test
(mtgv_op_dwconv7_ln; dwconv7_ln_kernel.h, dwconv7_ln_stream_kernel.h, dwconv7_ln_image_kernel.h), their seeded draws and
the fp64 reference of the operation, with the mistakes a kernel of this kind is likely to make as switches of that
reference.  No GPU needed here.

  y   = W (*) x + b                                   depthwise 7x7 / stride 1 / pad 3 (correlation, zero padding)
  out = (y - mean_C y) / sqrt(var_C y + eps) ln_w + ln_b   per pixel over the C channels, biased variance

The reference is torch conv2d (groups = C) and the LayerNorm in fp64 from the exact f32 inputs, nothing rounded in between.

Draw: x N(0, 1) with the outermost three rows and three columns of every image scaled by 8 - a halo read that crosses
into the neighbouring image or the neighbouring row (in the streaming and whole-image forms a row's masked columns address
the adjacent row in LDS) then moves border outputs far past the tolerance; taps N(0, 1) / 7; conv bias 200 + N(0, 1) per
channel, an offset common to all channels that the LayerNorm has to cancel (why the kernels take the variance in two
passes); ln_w 1 + 0.3 N(0, 1), ln_b 0.3 N(0, 1).  Channel 0's bias carries 5 sqrt(C) more: one channel far from its
pixel's mean.  Dividing by C - 1 moves an output by |z| / 2C, and without such a channel (|z| up to 5) that mistake moved
the reference by 3.0e-3 at C = 1024 - 100 x the tolerance that draw had, no more.  Offset and outlier are the pair,
of 28 measured, at which every mistake but the one-pass variance stays past 100 TOL on every case and the one-pass
variance is past 2 TOL on every case (separation() has the measurements)."""
import functools
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ROWS, STREAM, IMAGE = 0, 1, 2
EPS = 1e-6

# env: the launcher's switches the case runs under; form: {kind, TW, TH, WL} mtgv_op_dwconv7_ln_form must report
Case = namedtuple("Case", "n h w c env form eps", defaults=(EPS,))

_ROWS0 = (("MTGV_DW_ROWS", "0"),)
_IMAGE1 = (("MTGV_DW_IMAGE", "1"),)

# The smallest shapes that still reach each of the 16 instantiations the dispatcher can reach (8 forms x 2 output formats)
CASES = [
    Case(2, 7, 6, 16, (), (ROWS, 4, 3, 1)),        # c4n = 4 < P = 12: the reduction loop runs 3 rounds; ragged last rows (7 = 2 x 3 + 1) and last strip
    Case(3, 4, 9, 40, (), (ROWS, 4, 3, 1)),        # c4n = 10: 250 of 256 threads hold a strip
    Case(1, 3, 4, 20, (), (ROWS, 4, 3, 1)),        # C % 8 != 0: f32 only, SP8 is refused
    Case(2, 5, 4, 280, (), (ROWS, 4, 3, 1)),       # the largest C whose tap table fits 64 KB (test_dwconv_ln_cpu.py checks it)
    Case(2, 4, 11, 288, (), (ROWS, 8, 3, 0)),      # the first SP8-capable C past that limit; ragged strip
    Case(2, 7, 5, 320, (), (ROWS, 4, 3, 0)),       # AE-nano width
    Case(1, 3, 8, 1024, (), (ROWS, 8, 3, 0)),      # c4n = 256, S = 1: the widest dwconv7_ln_supported admits
    Case(1, 1, 1, 8, (), (ROWS, 2, 1, 0)),         # W < 4 takes the single-row form on the default path
    Case(2, 5, 2, 16, (), (ROWS, 2, 1, 0)),
    Case(2, 3, 3, 24, (), (ROWS, 2, 1, 0)),
    Case(2, 7, 6, 32, _ROWS0, (ROWS, 4, 1, 0)),    # MTGV_DW_ROWS=0: single-row form at strip widths 4 and 8
    Case(2, 7, 11, 96, _ROWS0, (ROWS, 8, 1, 0)),
    Case(128, 1, 32, 96, (), (STREAM, 4, 3, 0)),   # every halo row outside the image
    Case(128, 14, 32, 96, (), (STREAM, 4, 3, 0)),  # the 12-slot ring wraps (5 steps); ragged last step (2 rows)
    Case(129, 13, 16, 192, (), (STREAM, 4, 3, 0)),  # ring wraps; last step one row
    Case(3, 12, 8, 384, _IMAGE1, (IMAGE, 8, 6, 0)),  # MTGV_DW_IMAGE=1: both instantiations at a small batch
    Case(3, 6, 4, 768, _IMAGE1, (IMAGE, 4, 6, 0)),
    Case(128, 12, 8, 384, (), (IMAGE, 8, 6, 0)),   # the launcher's own rule
    Case(2, 7, 6, 16, (), (ROWS, 4, 3, 1), 0.5),   # eps of the order of the variance: where eps sits becomes visible
]
BATCH_CASES = (0, 15)  # batch independence: one row-group case and one whole-image case

# shapes the fused launch refuses: (what, (n, h, w, c), out_fmt); mtgv_op_dwconv7_ln answers each with status 1 and launches nothing
REFUSALS = [
    ("W = 6, C = 12", (2, 4, 6, 12), 0),  # c4n = 3 lanes cannot cover a 4-pixel strip (the block runs the unfused pair there)
    ("C % 4 != 0", (1, 3, 4, 18), 0),
    ("C = 1028", (1, 3, 8, 1028), 0),     # c4n = 257 > 256 threads
    ("SP8 at C = 20", (1, 3, 4, 20), 1),
]

# Bound of max |fused launch - fp64| on CASES: twice the largest error of mtgv_op_dwconv7 followed by mtgv_op_layernorm
# (dwconv7_kernel and ln_rows_kernel, not the code under test) against the same reference on these cases, rounded up to one
# significant digit.  The factor 2: the fused kernels may contract or associate the same f32 arithmetic differently and
# have no other reason to be further from fp64.  The measured values are in the docstring of test_gpu_dwconv_ln_direct.py:
# the largest is 4.54e-5 (128 x 14 x 32 x 96), twice that 9.08e-5.
TOL = 1e-4

BORDER, BORDER_SCALE, BIAS_OFFSET, OUTLIER = 3, 8.0, 200.0, 5.0
MUTATIONS = ("taps_transposed", "kernel_flipped", "hpad_adjacent_row", "vpad_neighbour_image", "bias_dropped", "var_unbiased",
             "eps_outside_sqrt", "eps_dropped", "one_pass_f32")


def applies(mutation, case):
    """whether the mistake can show at this case at all"""
    n, h, w = case.n, case.h, case.w
    if mutation in ("taps_transposed", "kernel_flipped"):
        return h * w > 1  # a 1 x 1 image sees the centre tap alone
    if mutation == "hpad_adjacent_row":
        return n * h > 1  # the pixels before and after a row: the adjacent row's, at the first and last row the neighbouring image's
    if mutation == "vpad_neighbour_image":
        return n > 1
    if mutation in ("eps_outside_sqrt", "eps_dropped"):
        # the bias draw alone gives every pixel a variance of order 1 or more: eps = 1e-6 changes sqrt(var + eps) by 5e-7
        # relative wherever it sits, below f32 resolution.  Only the eps = 0.5 case can tell.
        return case.eps > 1e-3
    return True


def separation(mutation):
    """how far a mistake must move the fp64 reference on every case it applies to (test_dwconv_ln_cpu.py): 100 TOL, but
    2 TOL for one_pass_f32 - past that a kernel which matches the mistaken reference to TOL, as one making this mistake and
    no other would, is more than TOL from the right one and fails the GPU test.

    Why not 100 TOL: E[y^2] - mean^2 in f32 and the two-pass form the kernels use (hence TOL) both lose more as the bias
    offset grows, the one-pass form faster - but a larger TOL takes var_unbiased (at most |z| / 2C, C up to 1024) and
    eps_dropped (eps = 0.5 against the outlier's variance) under 100 TOL first.  Measured, per (offset, outlier sqrt(C)
    multiple): TOL by the rule above from the separate kernels on the GPU; then over the 19 cases the smallest
    var_unbiased / TOL, eps_dropped / TOL, the smallest one_pass_f32 / TOL and the number of cases where it passes 100 TOL:
      (30, 3)    TOL 3e-5   var 306   eps 1670   one-pass 0.4    0 cases     (100, 3)   TOL 7e-5   var 131   eps 717   0.8   1
      (200, 5)   TOL 1e-4   var 120   eps 289    one-pass 2.1    2 cases     (300, 3)   TOL 3e-4   var 31    -         6.9   3
      (300, 10)  TOL 9e-5   var 162   eps 100    one-pass 1.2    5           (400, 9)   TOL 1e-4   var 143   eps 109   1.8   6
      (400, 10)  TOL 1e-4   var 146   eps 90     one-pass 3.6    6           (450, 9)   TOL 1e-4   var 143   eps 109   1.8   8
      (700, 10)  TOL 2e-4   var 73    eps 45     one-pass 1.0    6           (1000, 3)  TOL 6e-4   var 15    -         5.1   10
      (1000, 10) TOL 2e-4   var 73    -          one-pass 0.9    10          (1000, 30) TOL 7e-5   var 226   eps 16    2.6   6
    and 16 more between them: none brings the one-pass variance past 100 TOL on more than 10 of the 19 cases, and none on
    more than 8 while the other mistakes keep their 100 TOL; the small cases (1 x 1 x 1 x 8: 0.0 .. 5.5 TOL across the
    settings) sum too few channels.  (200, 5) is the one that keeps every other mistake past 100 TOL with room and the
    one-pass variance past 2 TOL on all 19 cases (2.1 .. 386 TOL)."""
    return (2 if mutation == "one_pass_f32" else 100) * TOL


Draw = namedtuple("Draw", "x w49 bias ln_w ln_b")


def draw(case, seed):
    """x [n][h][w][c], w49 [49 (kh 7 + kw)][c], bias, ln_w, ln_b [c]; all f32"""
    n, h, w, c = case.n, case.h, case.w, case.c
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    scale = np.ones((h, w), np.float32)
    scale[:BORDER] = scale[h - BORDER :] = BORDER_SCALE
    scale[:, :BORDER] = scale[:, max(w - BORDER, 0) :] = BORDER_SCALE
    x *= scale[None, :, :, None]
    w49 = (rng.standard_normal((49, c)) / 7.0).astype(np.float32)
    bias = BIAS_OFFSET + rng.standard_normal(c)
    bias[0] += OUTLIER * np.sqrt(c)
    bias = bias.astype(np.float32)
    ln_w = (1.0 + 0.3 * rng.standard_normal(c)).astype(np.float32)
    ln_b = (0.3 * rng.standard_normal(c)).astype(np.float32)
    return Draw(x, w49, bias, ln_w, ln_b)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _padded(x, mutation):
    """(n, h, w, c) fp64 -> the (n, c, h + 6, w + 6) map the 49 taps read: zeros around every image, or what a kernel that
    forgets one of the two masks reads there"""
    n, h, w, c = x.shape
    if mutation == "hpad_adjacent_row":  # no column mask: the three pixels before and after a row in memory
        flat = torch.cat([x.new_zeros(3, c), x.reshape(n * h * w, c), x.new_zeros(3, c)])
        rows = flat.unfold(0, w + 6, w)  # [n h][c][w + 6]
        return F.pad(rows.reshape(n, h, c, w + 6).permute(0, 2, 1, 3), (0, 0, 3, 3))
    xp = F.pad(x.permute(0, 3, 1, 2), (3, 3, 0, 0))  # columns
    if mutation == "vpad_neighbour_image":  # no row mask: the images one below the other as one map
        tall = F.pad(xp.permute(1, 0, 2, 3).reshape(c, n * h, w + 6), (0, 0, 3, 3))
        return tall.unfold(1, h + 6, h).permute(1, 0, 3, 2)  # [n][c][h + 6][w + 6]
    return F.pad(xp, (0, 0, 3, 3))


def reference(case, d, mutation=None, images=None):
    """fp64 [n][h][w][c] of the operation; `mutation` one of MUTATIONS; `images`: of the first so many images only"""
    assert mutation is None or (mutation in MUTATIONS and applies(mutation, case)), mutation
    c, eps = case.c, float(case.eps)
    x = _d(d.x if images is None else d.x[:images])
    k = _d(d.w49).reshape(7, 7, c)
    if mutation == "taps_transposed":
        k = k.permute(1, 0, 2)
    if mutation == "kernel_flipped":
        k = k.flip(0, 1)
    bias = None if mutation == "bias_dropped" else _d(d.bias)
    if mutation in ("hpad_adjacent_row", "vpad_neighbour_image"):
        y = F.conv2d(_padded(x, mutation), k.permute(2, 0, 1)[:, None], bias, groups=c)
    else:
        y = F.conv2d(x.permute(0, 3, 1, 2), k.permute(2, 0, 1)[:, None], bias, padding=3, groups=c)
    y = y.permute(0, 2, 3, 1)  # NHWC
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).sum(-1, keepdim=True) / (c - 1 if mutation == "var_unbiased" else c)
    if mutation == "one_pass_f32":  # sum and sum of squares over the channels in one pass, in f32, channel after channel
        y32 = y.numpy().astype(np.float32)
        m32 = np.cumsum(y32, -1, dtype=np.float32)[..., -1:] / np.float32(c)
        v32 = np.cumsum(y32 * y32, -1, dtype=np.float32)[..., -1:] / np.float32(c) - m32 * m32
        var = _d(np.maximum(v32, np.float32(0)))
    if mutation == "eps_outside_sqrt":
        rstd = 1.0 / (var.sqrt() + eps)
    elif mutation == "eps_dropped":
        rstd = 1.0 / var.sqrt()
    else:
        rstd = 1.0 / (var + eps).sqrt()
    return ((y - mean) * rstd * _d(d.ln_w) + _d(d.ln_b)).numpy()


def seed_of(index):
    return 11300 + index


@functools.lru_cache(maxsize=None)
def drawn(index):
    """(draw, fp64 reference) of CASES[index], computed once and shared: read-only for every user"""
    d = draw(CASES[index], seed_of(index))
    ref = reference(CASES[index], d)
    for a in (*d, ref):
        a.setflags(write=False)
    return d, ref


class Switches:
    """the launcher's two switches set as a case states them (unset where it does not name one) for the calls inside,
    then put back; the library reads them per call"""

    NAMES = ("MTGV_DW_ROWS", "MTGV_DW_IMAGE")

    def __init__(self, env, **over):
        self.kv = {**{k: None for k in self.NAMES}, **dict(env), **over}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def form_of(n, h, w, c):
    """(status, (kind, TW, TH, WL)) by mtgv_op_dwconv7_ln_form under the switches in force; needs no GPU"""
    import ctypes as C

    from mtgv import native

    f = (C.c_int32 * 4)(-1, -1, -1, -1)
    rc = native.lib().mtgv_op_dwconv7_ln_form(n, h, w, c, f)
    return rc, tuple(f)
