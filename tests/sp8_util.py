"""Host-side SP8 (mtg-vision_amd/csrc/sp8.h): the split operand format of the LDS-DMA GEMM, for tests.

A row of K f32 values (K % 8 == 0, the last axis) is K / 8 chunks of 32 bytes: the 8 fp16 hi halves, then the 8 fp16 lo
halves; hi = fp16(x), lo = fp16(x - f32(hi)), both round-to-nearest-even.  Same bytes per element as f32, so an SP8
tensor is carried as a float32 array of the same shape whose bits are the fp16 pairs."""
import numpy as np


def pack(x):
    """f32 values (..., K) -> their SP8 byte image as a float32 array of the same shape"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.shape[-1] % 8 == 0, x.shape
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    c = x.reshape(x.shape[:-1] + (x.shape[-1] // 8, 8))
    out = np.empty(c.shape[:-1] + (16,), dtype=np.float16)
    out[..., :8] = hi.reshape(c.shape)
    out[..., 8:] = lo.reshape(c.shape)
    return out.view(np.float32).reshape(x.shape)


def unpack(b):
    """SP8 byte image (float32-typed, (..., K)) -> float64(hi) + float64(lo)"""
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert b.shape[-1] % 8 == 0, b.shape
    h = b.view(np.float16).reshape(b.shape[:-1] + (b.shape[-1] // 8, 16))
    return (h[..., :8].astype(np.float64) + h[..., 8:].astype(np.float64)).reshape(b.shape)


def nan_sp8():
    """one chunk (8 float32-typed words) whose 16 halves are all fp16 NaN"""
    return np.full(16, 0x7E00, dtype=np.uint16).view(np.float32).copy()
