"""mtgv_op_area_attn (YOLO12's area attention and its depthwise 7x7 positional encoding: detector_v12.hip) against a float64
torch evaluation.  The detector's ABlocks run the same function; the whole network is tests/test_gpu_yolo12.py's."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo12_ref as R

pytestmark = pytest.mark.gpu

# (n, h, w, heads, area): 6 tokens per area; 15 (1.5 rows of the map); 400 (two query tiles of 256, the second ragged; 25 key
# groups of 16); 400 in one area; 300 (a ragged last key group) with 8 heads; 6 tokens in all
SHAPES = [(1, 4, 6, 2, 4), (3, 6, 10, 2, 4), (2, 40, 40, 2, 4), (2, 20, 20, 4, 1), (2, 30, 40, 8, 4), (1, 2, 3, 4, 1)]
QK_SCALE = 1.8  # logits q.k / sqrt(32) up to about 19: peaked softmaxes


def _sid(s):
    return "n%d-%dx%d-h%d-a%d" % s


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """qkv (n, h * w, heads * 96) float32 with q and k scaled, pe weights [49][c] and bias [c]"""
    n, h, w, heads, area = shape
    rng = np.random.default_rng(list(shape))
    qkv = rng.standard_normal((n, h * w, heads, 96)).astype(np.float32)
    qkv[..., :64] *= QK_SCALE
    c = heads * 32
    w49 = (rng.standard_normal((49, c)) / 7).astype(np.float32)
    bias = (0.1 * rng.standard_normal(c)).astype(np.float32)
    return qkv.reshape(n, h * w, heads * 96), w49, bias


def _torch_eval(shape, qkv, w49, bias, pe, dtype):
    """the expression in torch at `dtype`: (n, h * w, c)"""
    n, h, w, heads, area = shape
    c = heads * 32
    x = torch.from_numpy(qkv).to(dtype).transpose(1, 2).reshape(n, heads * 96, h, w)
    y, v = R.area_attention(x, heads, area)
    if pe:
        wt = torch.from_numpy(w49).to(dtype).T.reshape(c, 1, 7, 7)
        y = y + F.conv2d(v, wt, torch.from_numpy(bias).to(dtype), padding=3, groups=c)
    return y.flatten(2).transpose(1, 2).double().numpy()


@functools.lru_cache(maxsize=None)
def _reference(shape, pe):
    """(float64 result, error of the float32 torch evaluation against it): computed once"""
    qkv, w49, bias = _inputs(shape)
    r64 = _torch_eval(shape, qkv, w49, bias, pe, torch.float64)
    r32 = _torch_eval(shape, qkv, w49, bias, pe, torch.float32)
    return r64, float(np.abs(r32 - r64).max())


def _run(shape, qkv, pe):
    from mtgv.detector import area_attn

    n, h, w, heads, area = shape
    _, w49, bias = _inputs(shape)
    args = (torch.from_numpy(w49).cuda(), torch.from_numpy(bias).cuda()) if pe else ()
    out = area_attn(torch.from_numpy(qkv).cuda(), h, w, heads, area, *args)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("pe", [False, True], ids=["attn", "attn+pe"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_against_float64(shape, pe):
    """the kernel is allowed 4 x the error of the same expression in float32 torch on the same inputs (another summation
    order, the hardware exponential)"""
    qkv, _, _ = _inputs(shape)
    r64, err32 = _reference(shape, pe)
    got = _run(shape, qkv, pe)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"{_sid(shape)} pe {pe}: kernel {err:.2e}, float32 torch {err32:.2e} (max |ref| {np.abs(r64).max():.2f})")
    assert got.shape == r64.shape and np.isfinite(got).all()
    assert err <= 4 * err32


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[4] > 1], ids=_sid)
def test_areas_are_isolated(shape):
    """overwriting area 0's q / k / v rows leaves the attention output of areas 1..3 bit-identical, and changes area 0's"""
    n, h, w, heads, area = shape
    qkv, _, _ = _inputs(shape)
    na = h * w // area
    other = qkv.copy()
    other[:, :na] = np.random.default_rng(11).standard_normal(other[:, :na].shape).astype(np.float32)
    a, b = _run(shape, qkv, False), _run(shape, other, False)
    assert np.array_equal(a[:, na:].view(np.int32), b[:, na:].view(np.int32))
    assert (a[:, :na] != b[:, :na]).any(axis=2).all()


def test_bad_arguments_launch_nothing():
    from mtgv import native as nv

    qkv = torch.zeros((1, 25, 2 * 96), device="cuda")
    out = torch.full((1, 25, 64), float("nan"), device="cuda")
    L = nv.lib()
    for h, w, heads, area in ((5, 5, 2, 4), (5, 5, 0, 1), (5, 5, 2, 0), (5, 5, 2, -1)):
        rc = L.mtgv_op_area_attn(nv.ptr(qkv), None, None, 1, h, w, heads, area, nv.ptr(out), nv.stream())
        assert rc == 1 and "area_attn" in L.mtgv_last_error().decode(), (h, w, heads, area, rc)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert L.mtgv_op_area_attn(nv.ptr(qkv), None, None, 1, 5, 5, 2, 5, nv.ptr(out), nv.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
