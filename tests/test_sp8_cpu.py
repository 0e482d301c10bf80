"""CPU-only: the host-side SP8 helpers (tests/sp8_util.py) against the format sp8.h defines - round-trip error bounds,
byte layout, and pack(unpack(.)) as the identity."""
import numpy as np

import sp8_util as sp


def test_round_trip_within_sp8_bounds():
    """sp8.h: x = hi + lo + O(2^-22 |x|) while lo is a normal fp16 (|x| >= 2^-3), 2^-25 absolute below"""
    x = np.random.default_rng(0).standard_normal((1 << 17, 8)).astype(np.float32)  # 2^20 samples
    err = np.abs(sp.unpack(sp.pack(x)) - x.astype(np.float64))
    big = np.abs(x) >= 2.0**-3
    assert big.any() and (~big).any()
    assert (err[big] / np.abs(x[big].astype(np.float64))).max() <= 2.0**-22
    assert err[~big].max() <= 2.0**-25
    # values fp16 holds exactly (and zero) survive exactly
    e = np.array([0.0, 1.0, -2.5, 2.0**-14, 65504.0, -0.0, 0.333251953125, 1024.0], dtype=np.float32)
    assert (sp.unpack(sp.pack(e)) == e).all()


def test_byte_layout():
    """chunk c of a pixel: hi halves at bytes [32c, 32c + 16), lo halves at [32c + 16, 32c + 32); shape and pitch kept"""
    x = np.random.default_rng(1).standard_normal((3, 5, 24)).astype(np.float32)
    p = sp.pack(x)
    assert p.dtype == np.float32 and p.shape == x.shape
    raw = p.view(np.uint8).reshape(3, 5, 24 * 4)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    for c in range(3):
        assert (raw[..., 32 * c : 32 * c + 16] == np.ascontiguousarray(hi[..., 8 * c : 8 * c + 8]).view(np.uint8)).all()
        assert (raw[..., 32 * c + 16 : 32 * c + 32] == np.ascontiguousarray(lo[..., 8 * c : 8 * c + 8]).view(np.uint8)).all()
    # a channel slice at a multiple of 8 is the pack of the slice
    assert (p[..., 8:24].view(np.uint32) == sp.pack(x[..., 8:24]).view(np.uint32)).all()


def test_pack_of_unpack_is_identity():
    """hi + lo is an f32 value that SP8 holds exactly: packing it again loses nothing, so the GPU tests' inputs
    (unpacked SP8 values) are exact in both formats.  The identity is one of values: where lo rounded up to half an ulp
    of an odd hi, re-splitting the sum picks the even neighbour as hi and -half an ulp as lo - other bytes, same sum."""
    x = np.random.default_rng(2).standard_normal((1 << 16, 16)).astype(np.float32) * np.float32(3.0)
    p = sp.pack(x)
    u = sp.unpack(p)
    assert u.dtype == np.float64
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    p2 = sp.pack(u.astype(np.float32))
    assert (sp.unpack(p2) == u).all()
    same = (p2.view(np.uint32) == p.view(np.uint32)).reshape(-1, 8).all(axis=1)  # per chunk
    assert same.mean() > 0.99
    assert (sp.pack(sp.unpack(p2).astype(np.float32)).view(np.uint32) == p2.view(np.uint32)).all()  # and then a fixed point


def test_nan_chunk():
    n = sp.nan_sp8()
    assert n.dtype == np.float32 and n.shape == (8,)
    assert np.isnan(n.view(np.float16)).all() and np.isnan(sp.unpack(n)).all()
