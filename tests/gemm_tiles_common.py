"""Shared by test_gemm_tiles_cpu.py and test_gpu_gemm_tiles.py: the cases of the direct test of the convert-on-load
implicit-GEMM kernel (gemm_kernel.h: gemm_f32.hip, gemm_f16x3.hip) under every tile it is built for, their seeded draws,
their fp64 references and the shape arithmetic that says which of the kernel's paths a case reaches.  No GPU needed here.

The kernel's block tile is BM = 128 rows by BN = 32 tn columns, K staged BK at a time; built for TILES.  Per block it
takes the fast loader (dense, whole tile inside the problem, K % BK == 0) or the predicated one, and the interior epilogue
(whole tile inside, rows map 1:1, no crop) or the edge one.  A case therefore has to offer, under every tile, a tile wholly
inside the problem AND a ragged last row and column tile; tile_facts() computes that from the shape and the CPU test holds
every case to what its `expect` says.

Routing.  With MTGV_GEMM_PREC=f16x3 gemm_launch hands every launch gemm_sp_plan accepts to the LDS-DMA split kernel.  The
cases here must stay on the convert-on-load kernel in both precisions: sp_refusals() restates gemm_sp_plan's refusals for
f32 inputs as arithmetic on the launch and every case needs at least one.

Draws (seeded): input N(0,1), weights N(0,1) / sqrt(K), bias N(0,1), residual N(0,1), GRN multipliers U(0.5, 1.5), GRN
shift N(0,1).  Bound: 3e-5 absolute against fp64, the bound test_conv_random_geometry and test_linear_random_shapes hold
this kernel to at the same scaling; dense K <= 316 and conv K <= 512, what those tests cover.

One case differs from the plan it was written to: the 1x1 conv reading channels [16, 40) of 48 and writing channels
[8, 176) of 192 is a dense launch to gemm_launch (is_conv() is false for 1x1 / stride 1 / pad 0) with K = 24, every stride
a multiple of 8 and 4, 168 columns and 297 rows - gemm_sp_plan accepts it in f16x3.  It writes into 194 floats per pixel
here (ldo % 4 != 0), which keeps both slices and stays on this kernel."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

TILES = [(1, 1, 16), (1, 2, 16), (1, 3, 16), (1, 4, 16), (1, 5, 16), (1, 1, 32)]  # gemm_kernel.h: kGemmTiles, as (1, tn, bk)
UNBUILT = [(1, 2, 32), (2, 2, 16)]  # well-formed for MTGV_GEMM_TILE but not in kGemmTiles (tm is always 1): refused when the launch is planned
BM = 128
TOL = 3e-5
GRN_RTOL = 1e-5
NONE, GELU, MISH, SILU, SIGMOID = 0, 1, 2, 3, 4  # common.h: Act
ACTS = {NONE: lambda x: x, GELU: F.gelu, MISH: F.mish, SILU: F.silu, SIGMOID: torch.sigmoid}
ALL_TN = frozenset({1, 2, 3, 4, 5})


def _t64(a):
    """a (read-only) numpy array as a float64 torch tensor: a copy"""
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))  # a case's draw does not depend on the other cases


def tile_id(t):
    return "%d,%d,%d" % t


# ---- shape arithmetic ----
def tile_facts(M, N, K, tile):
    """what a launch of M x N x K offers the kernel under `tile`"""
    tm, tn, bk = tile
    bm, bn = BM * tm, 32 * tn
    return {
        "interior": M // bm >= 1 and N // bn >= 1,  # a row tile and a column tile wholly inside: one block takes the fast paths
        "ragged_m": M % bm != 0,
        "ragged_n": N % bn != 0,
        "k_tail": K % bk != 0,
        "tiles": (-(-M // bm)) * (-(-N // bn)),
    }


def is_conv(kh, kw, stride, pad):
    """gemm_f32.h is_conv(): A is gathered through a window"""
    return not (kh == 1 and kw == 1 and stride == 1 and pad == 0)


def sp_refusals(L):
    """gemm_sp_plan's reasons to decline a launch with f32 input rows (a_fmt 0), by name; empty: it would take it.
    L: dict(M, N, K, conv, remap, batch, c_total, c_off, ldo, o_off, ldr or None)"""
    why = []
    if L["batch"] != 1:
        why.append("batch > 1")
    if L["conv"]:
        why.append("f32-input conv")
    if L["remap"]:
        why.append("remap from f32 input")
    if L["K"] % 8 != 0:
        why.append("K % 8 != 0")
    if L["ldo"] % 4 != 0:
        why.append("ldo % 4 != 0")
    if L["N"] < 64 or L["M"] < 128:
        why.append("M < 128 or N < 64 from f32 rows")
    return why


# ---- dense cases: mtgv_op_linear / mtgv_op_linear_ex ----
# expect: interior / ragged_n = the set of tn (at either BK) for which it holds; ragged_m; k_tail = (at BK 16, at BK 32)
Dense = namedtuple("Dense", "name M N K act res hw scale shift grn interior ragged_m ragged_n k_tail")


def _dense(name, M, N, K, act=NONE, res=False, hw=0, scale=False, shift=False, grn=False, interior=ALL_TN, ragged_m=True,
           ragged_n=ALL_TN, k_tail=(False, False)):
    return Dense(name, M, N, K, act, res, hw, scale, shift, grn, frozenset(interior), ragged_m, frozenset(ragged_n), k_tail)


_ACT_NAME = {NONE: "none", GELU: "gelu", MISH: "mish", SILU: "silu", SIGMOID: "sigmoid"}
DENSE = (
    # fast loader + interior epilogue, one case per activation instance (sigmoid: the run-time switch), with and without
    # the interior residual prefetch
    [_dense(f"fast-{_ACT_NAME[a]}{'-res' if r else ''}", 293, 331, 96, act=a, res=r) for a in (NONE, GELU, MISH, SILU, SIGMOID) for r in (False, True)]
    + [
        _dense("ktail-4-both", 293, 331, 100, k_tail=(True, True)),
        _dense("ktail-bk32-only", 293, 331, 112, k_tail=(False, True)),
        _dense("whole-cols", 293, 320, 100, ragged_n={3, 4}, k_tail=(True, True)),
        _dense("tiny-1x8x4", 1, 8, 4, interior=(), k_tail=(True, True)),
        _dense("tiny-130x63x64", 130, 63, 64, interior={1}),
    ]
    # GRN prologue: per-image multipliers on A; hw = 1 fills the multiplier tile to nseg_max = 128 images
    + [_dense(f"apro-hw{hw}{'-res' if r else ''}", M, 331, 100, res=r, hw=hw, scale=True, k_tail=(True, True)) for hw, M in ((1, 293), (24, 288), (130, 260)) for r in (False, True)]
    + [_dense("apro-hw24-shift", 288, 331, 100, hw=24, scale=True, shift=True, k_tail=(True, True))]
    # GRN partial sums behind mish: a tile inside one image (the one_image shortcut), many images per tile, an image over two tiles
    + [_dense(f"grn-hw{hw}", M, 331, 96, act=MISH, hw=hw, grn=True, ragged_m=M % BM != 0) for hw, M in ((256, 768), (24, 288), (130, 260))]
)
DENSE_BY_NAME = {c.name: c for c in DENSE}
UNBUILT_CASE = "fast-none"


def dense_launch(c):
    return dict(M=c.M, N=c.N, K=c.K, conv=False, remap=False, batch=1, c_total=c.K, c_off=0, ldo=c.N, o_off=0, ldr=c.N if c.res else None)


@functools.lru_cache(maxsize=None)
def dense_draw(name):
    c = DENSE_BY_NAME[name]
    rng = _rng(name)
    d = {
        "a": rng.standard_normal((c.M, c.K)).astype(np.float32),
        "w": (rng.standard_normal((c.N, c.K)) / np.sqrt(c.K)).astype(np.float32),
        "b": rng.standard_normal(c.N).astype(np.float32),
        "r": rng.standard_normal((c.M, c.N)).astype(np.float32) if c.res else None,
        "sc": (rng.random((c.M // c.hw, c.K)) + 0.5).astype(np.float32) if c.scale else None,
        "sh": rng.standard_normal(c.K).astype(np.float32) if c.shift else None,
    }
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def dense_ref(name):
    """(out fp64 [M][N], per-image sum(act(...)^2) fp64 [M / hw][N] or None); the sums are of the value before the residual"""
    c, d = DENSE_BY_NAME[name], dense_draw(name)
    a = _t64(d["a"])
    if c.scale:
        a = a * _t64(d["sc"]).repeat_interleave(c.hw, 0)
    if c.shift:
        a = a + _t64(d["sh"])
    y = ACTS[c.act](F.linear(a, _t64(d["w"]), _t64(d["b"])))
    sums = (y * y).view(c.M // c.hw, c.hw, c.N).sum(1).numpy() if c.grn else None
    if c.res:
        y = y + _t64(d["r"])
    return y.numpy(), sums


# ---- conv cases: mtgv_op_conv2d_ex, f32 input ----
# n images of h x w, channels [x_co, x_co + cin) of x_ct in; channels [out_co, out_co + cout) of out_ct out; res = (ct, co) or
# None; os > 1: output row (img, y, x) goes to pixel (img, y os + oy, x os + ox) of the os-times larger grid
Conv = namedtuple("Conv", "name n h w cin cout k stride pad act x_ct x_co out_ct out_co res os oy ox k_tail")


def _conv(name, h, w, cin, k, stride, pad, act, k_tail, cout=168, x=None, out=None, res=None, os_=1, oy=0, ox=0):
    x_ct, x_co = x or (cin, 0)
    out_ct, out_co = out or (cout, 0)
    return Conv(name, 3, h, w, cin, cout, k, stride, pad, act, x_ct, x_co, out_ct, out_co, res, os_, oy, ox, k_tail)


CONV = [
    _conv("3x3s1-cin12-silu", 11, 9, 12, 3, 1, 1, SILU, (True, True)),      # K 108
    _conv("3x3s1-cin16-none", 11, 9, 16, 3, 1, 1, NONE, (False, True)),     # K 144
    _conv("3x3s1-cin32-mish", 11, 9, 32, 3, 1, 1, MISH, (False, False)),    # K 288, the run-time activation instance
    _conv("3x3s2-cin12-silu", 21, 17, 12, 3, 2, 1, SILU, (True, True)),     # odd map, the last tap row and column in the padding
    _conv("2x2s2-cin20-none", 22, 18, 20, 2, 2, 0, NONE, (False, True)),    # downsample, K 80
    _conv("4x4s4-cin4-none", 44, 36, 4, 4, 4, 0, NONE, (False, False)),     # stem, K 64
    _conv("1x1-slices-silu", 11, 9, 24, 1, 1, 0, SILU, (True, True), x=(48, 16), out=(194, 8)),  # (the docstring's last paragraph)
    _conv("3x3s1-res-slice-silu", 11, 9, 12, 3, 1, 1, SILU, (True, True), out=(192, 8), res=(200, 24)),
    _conv("3x3s1-scatter-os2-silu", 11, 9, 16, 3, 1, 1, SILU, (False, True), os_=2, oy=1, ox=0),
]
CONV_BY_NAME = {c.name: c for c in CONV}


def conv_out_hw(c):
    return (c.h + 2 * c.pad - c.k) // c.stride + 1, (c.w + 2 * c.pad - c.k) // c.stride + 1


def conv_launch(c):
    oh, ow = conv_out_hw(c)
    return dict(M=c.n * oh * ow, N=c.cout, K=c.k * c.k * c.cin, conv=is_conv(c.k, c.k, c.stride, c.pad), remap=c.os > 1, batch=1,
                c_total=c.x_ct, c_off=c.x_co, ldo=c.out_ct, o_off=c.out_co, ldr=c.res[0] if c.res else None)


@functools.lru_cache(maxsize=None)
def conv_draw(name):
    c = CONV_BY_NAME[name]
    oh, ow = conv_out_hw(c)
    rng = _rng(name)
    K = c.k * c.k * c.cin
    d = {
        "x": rng.standard_normal((c.n * c.h * c.w, c.cin)).astype(np.float32),
        "w": (rng.standard_normal((c.cout, c.k, c.k, c.cin)) / np.sqrt(K)).astype(np.float32),
        "b": rng.standard_normal(c.cout).astype(np.float32),
        "r": rng.standard_normal((c.n * oh * ow, c.cout)).astype(np.float32) if c.res else None,
    }
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def conv_ref(name):
    """fp64 rows [n oh ow][cout] in the conv's own row order (the scatter is the test's to undo)"""
    c, d = CONV_BY_NAME[name], conv_draw(name)
    x = _t64(d["x"]).view(c.n, c.h, c.w, c.cin).permute(0, 3, 1, 2)
    y = F.conv2d(x, _t64(d["w"]).permute(0, 3, 1, 2), _t64(d["b"]), stride=c.stride, padding=c.pad)
    y = ACTS[c.act](y).permute(0, 2, 3, 1).reshape(-1, c.cout)
    if c.res:
        y = y + _t64(d["r"])
    return y.numpy()


def scatter_rows(c):
    """index of the output pixel (in the os-times larger grid) that conv row m is written to"""
    oh, ow = conv_out_hw(c)
    img, y, x = np.meshgrid(np.arange(c.n), np.arange(oh), np.arange(ow), indexing="ij")
    return ((img * oh * c.os + y * c.os + c.oy) * (ow * c.os) + x * c.os + c.ox).reshape(-1)


# ---- mask cases: mtgv_op_mask_logits ----
Mask = namedtuple("Mask", "name n nm mh mw max_det mask_rows n_det in_h in_w")
MASK = [
    Mask("rows200", 3, 32, 12, 20, 300, 200, (0, 5, 250), 48, 80),
    Mask("rows16", 3, 32, 12, 20, 300, 16, (0, 5, 250), 48, 80),
]
MASK_BY_NAME = {c.name: c for c in MASK}
FORM_AUTO, FORM_PIXELS, FORM_GEMM = 0, 1, 2


def mask_launch(c):
    npx = c.mh * c.mw
    return dict(M=c.mask_rows, N=npx, K=c.nm, conv=False, remap=False, batch=c.n, c_total=c.nm, c_off=0, ldo=npx, o_off=0, ldr=None)


def placed_boxes(c):
    """xyxy boxes in input pixels whose edges, times crop_scale = mw / in_w (a power of two here: the products are exact),
    land where the comparisons decide"""
    s = c.in_w // c.mw
    assert c.in_w == s * c.mw and c.in_h == s * c.mh and s & (s - 1) == 0
    return np.array(
        [
            [2 * s, 1 * s, 10 * s, 6 * s],                          # edges on integer pixels: 2 <= x < 10, 1 <= y < 6
            [2.5 * s, 1.5 * s, 7.5 * s, 5.5 * s],                   # on half-integers: 3 <= x <= 7, 2 <= y <= 5
            [0, 0, c.in_w, c.in_h],                                 # the whole map
            [c.in_w + s, c.in_h + s, c.in_w + 9 * s, c.in_h + 5 * s],  # wholly outside
            [10 * s, 1 * s, 2 * s, 6 * s],                          # x2 < x1: nothing
            [(c.mw - 1) * s, (c.mh - 1) * s, c.in_w, c.in_h],       # the last pixel alone
            [-3 * s, -2 * s, 1 * s, 1 * s],                         # over the corner: pixel (0, 0) alone
        ],
        dtype=np.float32,
    )


@functools.lru_cache(maxsize=None)
def mask_draw(name):
    c = MASK_BY_NAME[name]
    rng = _rng(name)
    boxes = np.empty((c.n, c.max_det, 4), dtype=np.float32)
    xy1 = rng.random((c.n, c.max_det, 2)) * [c.in_w, c.in_h] - 4
    boxes[..., :2] = xy1
    boxes[..., 2:] = xy1 + rng.random((c.n, c.max_det, 2)) * [c.in_w * 0.6, c.in_h * 0.6]
    p = placed_boxes(c)
    for z in range(c.n):  # every frame's first rows in another order, so that a frame of 5 detections has placed boxes too
        boxes[z, : len(p)] = np.roll(p, z, axis=0)
    d = {
        "coef": rng.standard_normal((c.n, c.max_det, c.nm)).astype(np.float32),
        "protos": (rng.standard_normal((c.n, c.mh * c.mw, c.nm)) / np.sqrt(c.nm)).astype(np.float32),
        "boxes": boxes,
        "n_det": np.array(c.n_det, dtype=np.int32),
        "crop_scale": np.float32(c.mw / c.in_w),
    }
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def crop_inside(boxes, crop_scale, mh, mw):
    """[rows][mh * mw] bool: the kernel's rule - float32(box) * float32(crop_scale) rounded to f32, compared in f32 with the
    pixel's integer coordinates, low edges inclusive and high edges exclusive"""
    b = boxes.astype(np.float32) * np.float32(crop_scale)
    assert b.dtype == np.float32
    px = np.arange(mw, dtype=np.float32)[None, None, :]
    py = np.arange(mh, dtype=np.float32)[None, :, None]
    inside = (px >= b[:, 0, None, None]) & (px < b[:, 2, None, None]) & (py >= b[:, 1, None, None]) & (py < b[:, 3, None, None])
    return inside.reshape(len(boxes), mh * mw)


def mask_reference(coef, protos, n_det, boxes, crop_scale, mask_rows, mh, mw):
    """(logits fp64 [n][mask_rows][mh mw], inside bool of the same shape): fp64 dot products inside the box of kept rows, 0 elsewhere"""
    n = coef.shape[0]
    out = np.zeros((n, mask_rows, mh * mw), dtype=np.float64)
    ins = np.zeros((n, mask_rows, mh * mw), dtype=bool)
    for z in range(n):
        mc = min(int(n_det[z]), mask_rows)
        ins[z, :mc] = crop_inside(boxes[z, :mc], crop_scale, mh, mw)
        out[z, :mc] = (coef[z, :mc].astype(np.float64) @ protos[z].astype(np.float64).T) * ins[z, :mc]
    return out, ins


@functools.lru_cache(maxsize=None)
def mask_ref(name):
    c, d = MASK_BY_NAME[name], mask_draw(name)
    return mask_reference(d["coef"], d["protos"], d["n_det"], d["boxes"], d["crop_scale"], c.mask_rows, c.mh, c.mw)
