"""The detector's SP8 conv paths of the LDS-DMA split GEMM, one launch at a time against fp64 (mtgv_op_conv2d_ex):
the nine-tap gather, the staged input window with both ring depths and the 16-k tile, dense SP8 rows with channel
slices, the SP8-out / SP8-residual epilogues, the chained 1x1 and the whole-ConvTranspose scatter - at map widths and
channel counts the 640 x 640 forward never runs - and the claim that results do not depend on the tile configuration.

Every case
  - draws input N(0,1), weights N(0,1) / sqrt(K), bias N(0,1) from a seeded generator;
  - places the input inside a larger allocation in which every byte that is not one of the conv's input channels is an
    fp16 NaN (the pixel's other channels, and w + 2 pixels before the first and after the last image);
  - prefills the output allocation (8 pixels of margin either side) with a NaN byte pattern, then requires every
    word outside channels [co, co + cout) to be unchanged and every value inside to be finite;
  - compares with torch conv2d / conv_transpose2d in fp64 on the CPU from the unpacked SP8 input values and the exact
    f32 weights (activation and residual in fp64, a chained pair as two fp64 layers with nothing rounded in between)
    at 3e-5 absolute, the bound test_conv_random_geometry holds this kernel family to at the same input scaling
    (K <= 3 x 3 x 96 here);
  - asserts the {tile configuration, A mode, epilogue id, ring depth} the library reports for the launch, so that no
    case passes by running another kernel than the one it names.
Each case prints its measured maximum error (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sp8_util as sp

pytestmark = pytest.mark.gpu

TOL = 3e-5
ACTS = {0: lambda x: x, 2: F.mish, 3: F.silu, 4: torch.sigmoid}
NONE, MISH, SILU, SIGMOID = 0, 2, 3, 4
F32, SP8 = 0, 1
# gemm_sp_cfg.h: SpAMode, SpEpi, the tile table (kSpTile) and the ring depths
A_SP8, A_CONV, A_WINDOW = 0, 2, 5
EPI_ARGS, EPI_F32, EPI_SP8_OUT, EPI_RES_SP8, EPI_CHAIN = -1, 0, 1, 4, 32
TILE_BN = {0: 128, 1: 192, 2: 96, 3: 64, 4: 32, 5: 192}  # 128-row tiles in 32-k stages: what MTGV_SP_CFG can force
CFG_96, CFG_64, CFG_32, CFG_OS_NQ, CFG_WIN16 = 2, 3, 4, 3, 6
RING, DEEP_RING = 2, 4
CANARY = 0x7FC17FC1  # a NaN as f32 and as either fp16 half
MARGIN = 8           # output pixels of canary before and after the tensor


@pytest.fixture(autouse=True)
def _f16x3():
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision("f16x3")
    yield
    native.set_gemm_precision(before)


class Buf:
    """px pixels x ct floats (f32 or SP8) with `guard` more pixels on either side; channels [co, co + c) are the tensor"""

    def __init__(self, px, ct, co, c, fmt, guard, canary=False):
        assert ct % 8 == 0 and co % 8 == 0 and c % 8 == 0 and co + c <= ct
        self.px, self.ct, self.co, self.c, self.fmt, self.guard = px, ct, co, c, fmt, guard
        self.host = np.empty((px + 2 * guard, ct), dtype=np.float32)
        if canary:
            self.host.view(np.uint32)[:] = CANARY
        else:
            self.host.reshape(-1, 8)[:] = sp.nan_sp8()
        self.dev = None

    def set(self, values):
        """writes the tensor; returns the values a kernel reads from it, in fp64"""
        assert values.shape == (self.px, self.c)
        img = sp.pack(values) if self.fmt == SP8 else values.astype(np.float32)
        self.host[self.guard : self.guard + self.px, self.co : self.co + self.c] = img
        return sp.unpack(img) if self.fmt == SP8 else img.astype(np.float64)

    def upload(self):
        self.dev = torch.from_numpy(self.host).cuda()
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.guard * self.ct * 4

    def read(self):
        """(values fp64, words uint32) of the tensor, after checking that nothing else changed and all of it was written"""
        got = self.dev.cpu().numpy()
        inside = np.ascontiguousarray(got[self.guard : self.guard + self.px, self.co : self.co + self.c])
        rest = got.view(np.uint32).copy()
        rest[self.guard : self.guard + self.px, self.co : self.co + self.c] = CANARY
        assert (rest == CANARY).all(), "bytes outside the output channels changed"
        vals = sp.unpack(inside) if self.fmt == SP8 else inside.astype(np.float64)
        assert np.isfinite(vals).all(), "output channels not finite (unwritten or poisoned by the guard band)"
        return vals, inside.view(np.uint32)


def sp8_input(rng, n, h, w, c, ct=None, co=0):
    b = Buf(n * h * w, ct or c, co, c, SP8, guard=w + 2)
    vals = b.set(rng.standard_normal((n * h * w, c)).astype(np.float32))
    return b.upload(), vals


def output(px, c, fmt, ct=None, co=0):
    return Buf(px, ct or c, co, c, fmt, guard=MARGIN, canary=True).upload()


def weights(rng, cout, k, cin):
    """[cout][kh][kw][cin] and bias"""
    return (rng.standard_normal((cout, k, k, cin)) / np.sqrt(k * k * cin)).astype(np.float32), rng.standard_normal(cout).astype(np.float32)


def conv_ex(x, n, h, w, wt, bias, stride, pad, act, out=None, res=None, os_=1, oy=0, ox=0, os_nq=0, w2=None, bias2=None, act2=NONE, out2=None):
    """one mtgv_op_conv2d_ex launch; returns the reported path"""
    from mtgv import native as nv

    keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in (wt, bias, w2, bias2)]
    d = nv.ConvEx()
    d.x, d.n, d.h, d.w, d.x_ct, d.x_co, d.cin, d.x_fmt = x.ptr, n, h, w, x.ct, x.co, x.c, x.fmt
    d.wt, d.bias = keep[0].data_ptr(), keep[1].data_ptr()
    d.cout, d.kh, d.kw, d.stride, d.pad, d.act = wt.shape[0], wt.shape[1], wt.shape[2], stride, pad, act
    assert wt.shape[3] == x.c
    if out is not None:
        d.out, d.out_ct, d.out_co, d.out_fmt = out.ptr, out.ct, out.co, out.fmt
    if res is not None:
        d.res, d.res_ct, d.res_co, d.res_fmt = res.ptr, res.ct, res.co, res.fmt
    d.os, d.oy, d.ox, d.os_nq = os_, oy, ox, os_nq
    if w2 is not None:
        d.w2, d.bias2, d.cout2, d.act2 = keep[2].data_ptr(), keep[3].data_ptr(), w2.shape[0], act2
        d.out2, d.out2_ct, d.out2_co, d.out2_fmt = out2.ptr, out2.ct, out2.co, out2.fmt
    path = (C.c_int32 * 4)(-9, -9, -9, -9)
    nv.check(nv.lib().mtgv_op_conv2d_ex(C.byref(d), path, nv.stream()))
    torch.cuda.synchronize()
    return tuple(path)


def ref_conv(xv, n, h, w, wt, bias, stride, pad, act, res=None):
    """fp64 NHWC conv + activation (+ residual) as rows [n oh ow][cout]"""
    x = torch.from_numpy(xv.reshape(n, h, w, -1)).permute(0, 3, 1, 2)
    y = F.conv2d(x, torch.from_numpy(wt).double().permute(0, 3, 1, 2), torch.from_numpy(bias).double(), stride=stride, padding=pad)
    y = ACTS[act](y).permute(0, 2, 3, 1).reshape(-1, wt.shape[0]).numpy()
    return y if res is None else y + res


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


class ConvCase:
    """one conv launch with everything it needs kept, so that it can run again (under another tile configuration)"""

    def __init__(self, seed, shape, k, stride, act, out_fmt, x_view=(None, 0), out_view=(None, 0), res_view=None):
        n, h, w, cin, cout = shape
        rng = np.random.default_rng(seed)
        self.shape, self.k, self.stride, self.pad, self.act = shape, k, stride, k // 2, act
        self.x, xv = sp8_input(rng, n, h, w, cin, *x_view)
        self.wt, self.bias = weights(rng, cout, k, cin)
        self.oh, self.ow = out_hw(h, w, k, stride, self.pad)
        self.out_args = (n * self.oh * self.ow, cout, out_fmt, *out_view)
        self.res, rv = None, None
        if res_view is not None:  # SP8 residual rows
            self.res = Buf(n * self.oh * self.ow, res_view[0], res_view[1], cout, SP8, guard=MARGIN)
            rv = self.res.set(rng.standard_normal((n * self.oh * self.ow, cout)).astype(np.float32))
            self.res.upload()
        self.ref = ref_conv(xv, n, h, w, self.wt, self.bias, stride, self.pad, act, rv)

    def run(self):
        """(path, max |error| against fp64, output words)"""
        n, h, w, _, _ = self.shape
        out = output(*self.out_args)
        path = conv_ex(self.x, n, h, w, self.wt, self.bias, self.stride, self.pad, self.act, out, self.res)
        vals, words = out.read()
        return path, float(np.abs(vals - self.ref).max()), words

    def check(self, want_path, label):
        path, err, words = self.run()
        print(f"sp8conv {label} {self.shape} act={self.act}: path={path} max_err={err:.3g}")
        assert path == want_path, (label, self.shape, path)
        assert err < TOL, (label, self.shape, err)
        return words


def epi_of(out_fmt, res=False):
    return (EPI_SP8_OUT if out_fmt == SP8 else EPI_F32) | (EPI_RES_SP8 if res else 0)


# ---- tap gather: 3x3 stride 2 pad 1 ----
GATHER = [
    ((2, 9, 7, 8, 40), {}),  # odd sizes, K = 72 (a K tail in 32-k stages, 8-channel taps), 40 rows and 40 columns: ragged both ways
    ((3, 16, 16, 24, 64), {}),
    ((2, 6, 10, 64, 16), {"x_view": (96, 16), "out_view": (48, 24)}),  # channels 16.. of 96 in, 24.. of 48 out
]


@pytest.mark.parametrize("shape,views", GATHER)
@pytest.mark.parametrize("act,out_fmt", [(SILU, SP8), (NONE, F32), (SIGMOID, F32)])
def test_tap_gather(shape, views, act, out_fmt):
    ConvCase(1, shape, 3, 2, act, out_fmt, **views).check((CFG_32, A_CONV, epi_of(out_fmt), RING), "gather")


def test_tap_gather_sp8_residual_at_channel_offset():
    c = ConvCase(2, (3, 16, 16, 24, 64), 3, 2, SILU, SP8, out_view=(96, 8), res_view=(128, 40))
    c.check((CFG_32, A_CONV, epi_of(SP8, True), RING), "gather+res")


# ---- dense SP8 rows (1x1) ----
@pytest.mark.parametrize("out_fmt", [F32, SP8])
def test_dense_1x1_channel_slice(out_fmt):
    """K = 16 of a 48-float pixel: half a 32-k stage, the rest of the stage must come from the zero page, not the NaN
    neighbours"""
    ConvCase(3, (2, 5, 7, 16, 24), 1, 1, NONE, out_fmt, x_view=(48, 32)).check((CFG_32, A_SP8, epi_of(out_fmt), RING), "dense")


def test_dense_1x1_sp8_residual():
    c = ConvCase(4, (1, 20, 20, 128, 64), 1, 1, SILU, SP8, res_view=(64, 0))
    c.check((CFG_32, A_SP8, epi_of(SP8, True), RING), "dense+res")


# ---- window conv: 3x3 stride 1 pad 1, Cin % 32 == 0 ----
WINDOW = [
    (5, 5, 7, 32, 32),     # 35-pixel images: one 128-pixel tile spans four of them
    (2, 1, 9, 32, 64),     # one-row maps: every dy != 0 tap is padding
    (2, 9, 1, 32, 32),     # one-column maps: every dx != 0 tap is padding, the window's rows are single pixels
    (1, 3, 130, 64, 48),   # a row wider than a tile
]


@pytest.mark.parametrize("shape", WINDOW)
def test_window(shape):
    ConvCase(5, shape, 3, 1, SILU, SP8).check((CFG_32, A_WINDOW, EPI_SP8_OUT, DEEP_RING), "window")
    ConvCase(6, shape, 3, 1, NONE, F32).check((CFG_32, A_WINDOW, EPI_F32, DEEP_RING), "window")


def test_window_sp8_residual():
    c = ConvCase(7, (3, 20, 20, 96, 96), 3, 1, SILU, SP8, res_view=(96, 0))
    c.check((CFG_32, A_WINDOW, epi_of(SP8, True), DEEP_RING), "window+res")


def test_window_two_deep_ring_by_tile_count():
    """600 tiles: more than one round (kSpRoundTiles = 512), so the two-deep ring"""
    ConvCase(8, (3, 160, 160, 32, 32), 3, 1, SILU, SP8).check((CFG_32, A_WINDOW, EPI_SP8_OUT, RING), "window 600 tiles")


# Widths on both sides of each threshold (gemm_sp_cfg.h, two blocks per CU = 80 KB each):
#   128 x 32 tile, 128-byte pixels: window = ceil8(128 + 2 w + 2) x 128 B, weight ring 4 KB per stage.
#     deep ring:  window + 16 KB <= 80 KB  <=>  w <= 191;   fits:  window + 8 KB <= 80 KB  <=>  w <= 223
#   16-k tile, 64-byte pixels: window = ceil16(128 + 2 w + 2) x 64 B, weight ring 2 KB per stage.
#     deep ring:  window + 8 KB <= 80 KB  <=>  w <= 511;    fits:  window + 4 KB <= 80 KB  <=>  w <= 543
# (beyond "fits" a 16-channel conv falls back to the tap gather on the 128 x 32 tile)
THRESHOLDS = [
    (32, 191, (CFG_32, A_WINDOW, EPI_SP8_OUT, DEEP_RING)),
    (32, 192, (CFG_32, A_WINDOW, EPI_SP8_OUT, RING)),
    (32, 223, (CFG_32, A_WINDOW, EPI_SP8_OUT, RING)),
    (32, 224, (CFG_32, A_CONV, EPI_SP8_OUT, RING)),
    (16, 511, (CFG_WIN16, A_WINDOW, EPI_SP8_OUT, DEEP_RING)),
    (16, 512, (CFG_WIN16, A_WINDOW, EPI_SP8_OUT, RING)),
    (16, 543, (CFG_WIN16, A_WINDOW, EPI_SP8_OUT, RING)),
    (16, 544, (CFG_32, A_CONV, EPI_SP8_OUT, RING)),
]


@pytest.mark.parametrize("c,w,want", THRESHOLDS)
def test_window_width_thresholds(c, w, want):
    ConvCase(9, (2, 2, w, c, c), 3, 1, SILU, SP8).check(want, "threshold")


# ---- the 16-k window tile ----
@pytest.mark.parametrize("shape", [(4, 6, 6, 16, 16), (2, 40, 40, 48, 32)])
def test_win16(shape):
    ConvCase(10, shape, 3, 1, SILU, SP8).check((CFG_WIN16, A_WINDOW, EPI_SP8_OUT, DEEP_RING), "win16")
    ConvCase(11, shape, 3, 1, NONE, F32).check((CFG_WIN16, A_WINDOW, EPI_F32, DEEP_RING), "win16")


def test_win16_not_taken_beyond_one_column_tile():
    """N = 40 > 32: the tap gather on the 128 x 32 tile, with 16-channel taps"""
    ConvCase(12, (2, 12, 12, 16, 40), 3, 1, SILU, SP8).check((CFG_32, A_CONV, EPI_SP8_OUT, RING), "win16 off")


def test_win16_two_deep_ring_by_tile_count():
    ConvCase(13, (3, 160, 160, 16, 16), 3, 1, SILU, SP8).check((CFG_WIN16, A_WINDOW, EPI_SP8_OUT, RING), "win16 600 tiles")


# ---- chained 1x1 ----
CHAIN_SIZES = [(32, 32), (64, 32), (64, 64), (96, 32), (96, 64), (96, 96)]
CHAIN_CFG = {32: CFG_32, 64: CFG_64, 96: CFG_96}


@pytest.mark.parametrize("n,h,w", [(2, 9, 7), (1, 20, 20)])
@pytest.mark.parametrize("stride,amode", [(2, A_CONV), (1, A_WINDOW)])
def test_chained_1x1(n, h, w, stride, amode):
    """3x3 + SiLU, then a 1x1, as one launch: bit-identical to two launches with an SP8 intermediate, and within
    tolerance of two fp64 layers"""
    cin = 32
    rng = np.random.default_rng(14)
    x, xv = sp8_input(rng, n, h, w, cin)
    oh, ow = out_hw(h, w, 3, stride, 1)
    px = n * oh * ow
    worst = 0.0
    for cout, cout2 in CHAIN_SIZES:
        w1, b1 = weights(rng, cout, 3, cin)
        w2, b2 = weights(rng, cout2, 1, cout)
        mid_ref = ref_conv(xv, n, h, w, w1, b1, stride, 1, SILU)
        mid = output(px, cout, SP8)
        p1 = conv_ex(x, n, h, w, w1, b1, stride, 1, SILU, mid)
        assert p1[1] == amode and p1[2] == EPI_SP8_OUT, p1
        mid.read()
        for act2 in (SILU, NONE):
            ref = ref_conv(mid_ref, n, oh, ow, w2, b2, 1, 0, act2)
            for fmt2 in (SP8, F32):
                view = (cout2 + 24, 16)  # the second output at channels 16.. of a wider pixel
                two = output(px, cout2, fmt2, *view)
                p2 = conv_ex(mid, n, oh, ow, w2, b2, 1, 0, act2, two)
                assert p2[1] == A_SP8, p2
                one = output(px, cout2, fmt2, *view)
                path = conv_ex(x, n, h, w, w1, b1, stride, 1, SILU, None, w2=w2.reshape(cout2, cout), bias2=b2, act2=act2, out2=one)
                assert path == (CHAIN_CFG[cout], amode, EPI_CHAIN, DEEP_RING if amode == A_WINDOW else RING), (cout, cout2, path)
                v1, bits1 = one.read()
                _, bits2 = two.read()
                assert (bits1 == bits2).all(), (cout, cout2, act2, fmt2)
                err = float(np.abs(v1 - ref).max())
                worst = max(worst, err)
                assert err < TOL, (cout, cout2, act2, fmt2, err)
    print(f"sp8conv chain {(n, h, w)} stride={stride}: max_err={worst:.3g}")


def test_chain_refused_is_an_error():
    """a pair the kernel cannot chain (no SiLU between the layers) is status 1, not two launches"""
    rng = np.random.default_rng(15)
    x, _ = sp8_input(rng, 1, 4, 4, 32)
    w1, b1 = weights(rng, 32, 3, 32)
    w2, b2 = weights(rng, 32, 1, 32)
    out2 = output(16, 32, SP8)
    with pytest.raises(AssertionError, match="chain"):
        conv_ex(x, 1, 4, 4, w1, b1, 1, 1, NONE, None, w2=w2.reshape(32, 32), bias2=b2, act2=NONE, out2=out2)


# ---- ConvTranspose2d(k = 2, s = 2) as a scattered 1x1 ----
class UpCase:
    def __init__(self, seed, n, h, w, cin, nq, out_fmt):
        rng = np.random.default_rng(seed)
        self.n, self.h, self.w, self.nq, self.out_fmt = n, h, w, nq, out_fmt
        self.x, xv = sp8_input(rng, n, h, w, cin)
        wt = (rng.standard_normal((cin, nq, 2, 2)) / np.sqrt(cin)).astype(np.float32)  # ConvTranspose2d layout
        b = rng.standard_normal(nq).astype(np.float32)
        # rows ordered (kh, kw, cout), the bias repeated per group
        self.w_all = np.ascontiguousarray(wt.transpose(2, 3, 1, 0).reshape(4 * nq, 1, 1, cin))
        self.b_all = np.tile(b, 4)
        self.b = b
        xt = torch.from_numpy(xv.reshape(n, h, w, cin)).permute(0, 3, 1, 2)
        y = F.conv_transpose2d(xt, torch.from_numpy(wt).double(), torch.from_numpy(b).double(), stride=2)
        self.ref = y.permute(0, 2, 3, 1).reshape(-1, nq).numpy()

    def out(self):
        return output(self.n * 4 * self.h * self.w, self.nq, self.out_fmt, self.nq + 8, 8)

    def one_launch(self):
        o = self.out()
        path = conv_ex(self.x, self.n, self.h, self.w, self.w_all, self.b_all, 1, 0, NONE, o, os_=2, os_nq=self.nq)
        return (path, *o.read())

    def four_launches(self):
        o = self.out()
        for q in range(4):
            wq = self.w_all[q * self.nq : (q + 1) * self.nq]
            path = conv_ex(self.x, self.n, self.h, self.w, wq, self.b, 1, 0, NONE, o, os_=2, oy=q >> 1, ox=q & 1)
            assert path[1:] == (A_SP8, EPI_ARGS, RING), path
        return o.read()


@pytest.mark.parametrize("n,h,w,cin", [(2, 5, 7, 32), (1, 20, 20, 64)])
@pytest.mark.parametrize("nq", [64, 32, 8])
@pytest.mark.parametrize("out_fmt", [SP8, F32])
def test_conv_transpose_scatter(n, h, w, cin, nq, out_fmt):
    c = UpCase(16, n, h, w, cin, nq, out_fmt)
    path, vals, bits = c.one_launch()
    assert path == (CFG_OS_NQ if nq == 64 else CFG_32, A_SP8, EPI_ARGS, RING), path
    err = float(np.abs(vals - c.ref).max())
    print(f"sp8conv up {(n, h, w, cin)} nq={nq}: path={path} max_err={err:.3g}")
    assert err < TOL
    _, bits4 = c.four_launches()
    assert (bits == bits4).all()


# ---- results do not depend on the tile configuration ----
class forced_cfg:
    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        os.environ["MTGV_SP_CFG"] = str(self.cfg)

    def __exit__(self, *exc):
        os.environ.pop("MTGV_SP_CFG", None)


def _conv_under_every_tile(case, label):
    """a ConvCase under MTGV_SP_CFG = 0..5: the forced tile runs; bit-identical to the unforced launch while the A mode
    stays, within tolerance of fp64 always"""
    path0, err0, bits0 = case.run()
    assert err0 < TOL
    moved = 0
    for cfg in range(6):
        with forced_cfg(cfg):
            path, err, bits = case.run()
        print(f"sp8conv tiles {label} cfg={cfg}: path={path} max_err={err:.3g}")
        assert path[0] == cfg and path[2] == path0[2], (label, cfg, path)
        assert err < TOL, (label, cfg, err)
        if path[1] == path0[1]:
            assert (bits == bits0).all(), (label, cfg)
        else:  # a wider tile's weight ring leaves no room for the window: window <-> gather, another summation order
            assert {path[1], path0[1]} == {A_WINDOW, A_CONV}, (label, cfg, path)
            moved += 1
    return moved


def test_tile_independence_tap_gather():
    assert _conv_under_every_tile(ConvCase(17, (2, 9, 7, 8, 40), 3, 2, SILU, SP8), "gather") == 0


def test_tile_independence_dense():
    assert _conv_under_every_tile(ConvCase(18, (1, 20, 20, 128, 64), 1, 1, SILU, SP8, res_view=(64, 0)), "dense") == 0


def test_tile_independence_window():
    assert _conv_under_every_tile(ConvCase(19, (5, 5, 7, 32, 32), 3, 1, SILU, SP8), "window") == 0
    # w = 130: the window fits beside the rings of the 96-, 64- and 32-column tiles only (w <= 127 at 128, <= 63 at 192 columns)
    assert _conv_under_every_tile(ConvCase(20, (1, 3, 130, 64, 48), 3, 1, SILU, SP8), "window wide") == 3


def test_tile_independence_conv_transpose():
    c = UpCase(21, 1, 20, 20, 64, 64, SP8)
    path0, vals0, bits0 = c.one_launch()
    assert path0[0] == CFG_OS_NQ
    for cfg in range(6):
        with forced_cfg(cfg):
            path, vals, bits = c.one_launch()
        assert path == (cfg, A_SP8, EPI_ARGS, RING), path
        assert (bits == bits0).all(), cfg
        assert np.abs(vals - c.ref).max() < TOL


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _linear_ex(tmp_path, a, w, b, r, act, hw, sc, want_grn):
    """one mtgv_op_linear_ex launch under the launch profiler: (out, per-image sums of the GRN partials or None, columns
    of the LDS-DMA tile that ran)"""
    from mtgv import native as nv

    L = nv.lib()
    (m, k), n = a.shape, w.shape[0]
    out = torch.full((m, n), float("nan"), device="cuda")
    A, W, B, R, SC = _dev(a), _dev(w), _dev(b), _dev(r) if r is not None else None, _dev(sc) if sc is not None else None
    part = torch.zeros(int(L.mtgv_op_linear_ex_part_floats(m, n, k, act, hw)) + 4, device="cuda") if want_grn else None
    csv = str(tmp_path / "gemm.csv")
    nv.check(L.mtgv_profile_gemm(1))
    try:
        nv.check(L.mtgv_op_linear_ex(nv.ptr(A), nv.ptr(W), nv.ptr(B), nv.ptr(R), nv.ptr(out), m, n, k, act, hw, nv.ptr(SC), None, nv.ptr(part), nv.stream()))
        torch.cuda.synchronize()
        nv.check(L.mtgv_profile_gemm_dump(csv.encode()))
    finally:
        nv.check(L.mtgv_profile_gemm(0))
    rows = [ln.split(",") for ln in open(csv).read().split()[1:]]
    assert len(rows) == 1 and rows[0][17] == "1", rows  # one launch, on the LDS-DMA kernel
    # its LDS fill: per tile the 128 x K A panel, the bn x K B panel and, with multipliers, 1 KB per 32-k stage
    fill = float(rows[0][18])
    bn = [c for c in sorted(set(TILE_BN.values())) if fill == -(-m // 128) * -(-n // c) * ((128 + c) * k * 4 + (k // 32 * 1024 if sc is not None else 0))]
    assert len(bn) == 1, (fill, bn)
    sums = None
    if want_grn:
        ur, sm = C.c_int32(0), C.c_int32(0)
        nv.check(L.mtgv_op_last_grn_layout(C.byref(ur), C.byref(sm)))
        unit, segmax = ur.value, sm.value
        assert segmax == (unit - 1) // hw + 2
        units = -(-m // unit)
        p = part[: units * segmax * n].cpu().double().view(units, segmax, n)
        sums = torch.zeros(m // hw, n, dtype=torch.float64)
        for t in range(units):
            first, last = (t * unit) // hw, (min((t + 1) * unit, m) - 1) // hw
            for s in range(last - first + 1):
                sums[first + s] += p[t, s]
    return out.cpu(), sums, bn[0]


LINEAR = [
    ("plain f32 rows", 49, 37, 96, 392, NONE, False, True, False),
    ("per-image multipliers + residual", 24, 50, 64, 72, NONE, True, True, False),
    ("mish + GRN partials", 130, 6, 320, 96, MISH, False, False, True),
]


@pytest.mark.parametrize("label,hw,nimg,n,k,act,scaled,resid,grn", LINEAR)
def test_tile_independence_linear_ex(tmp_path, label, hw, nimg, n, k, act, scaled, resid, grn):
    rng = np.random.default_rng(22)
    m = hw * nimg
    a = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    r = rng.standard_normal((m, n)).astype(np.float32) if resid else None
    sc = (rng.random((nimg, k)) + 0.5).astype(np.float32) if scaled else None
    a2 = torch.from_numpy(a).double() * (torch.from_numpy(sc).double().repeat_interleave(hw, 0) if scaled else 1.0)
    ref = ACTS[act](F.linear(a2, torch.from_numpy(w).double(), torch.from_numpy(b).double()))
    if resid:
        ref = ref + torch.from_numpy(r).double()
    out0, _, _ = _linear_ex(tmp_path, a, w, b, r, act, hw, sc, grn)
    assert (out0.double() - ref).abs().max().item() < 5e-5  # the bound of test_linear_ex_scaled_a_with_residual_pwconv2_shapes
    for cfg in range(6):
        with forced_cfg(cfg):
            out, sums, bn = _linear_ex(tmp_path, a, w, b, r, act, hw, sc, grn)
        assert bn == TILE_BN[cfg], (label, cfg, bn)
        assert torch.equal(out.view(torch.int32), out0.view(torch.int32)), (label, cfg)
        if grn:  # the partials' unit is a wave's rows, 64 or 32 by tile: the per-image sums are what the consumer reads
            o = out.double()
            want = (o * o).view(nimg, hw, n).sum(1)
            assert ((sums - want).abs() / (want.abs() + 1e-3)).max().item() < 1e-5, (label, cfg)
