"""CPU-only: the ABI of the source-frame path (mtgv_letterbox_ragged_u8, mtgv_warp_quads_src), the quad mapping against
`mtgv.adapters.to_frame_points` (ultralytics' scale_coords + clip_coords, what CardSegmenter applies on the host), and the
geometry tables of `SourceFrames`."""
import ctypes
import os

import numpy as np
import pytest

import source_frames_common as sc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mtgv.h")
NEW = ("mtgv_letterbox_ragged_u8", "mtgv_warp_quads_src")
FRAME_SHAPES = [(480, 640), (720, 1280), (1080, 1920), (37, 53), (96, 64)]
INPUTS = [(640, 640), (384, 640), (96, 160)]  # a square and two rectangles


def test_abi_declares_and_binds_the_entries():
    from mtgv import native

    names = sc.declared(HEADER)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/mtgv.h"
        assert n in native.SIGNATURES, f"{n} is not bound in native.py"
    assert sorted(native.SIGNATURES) == names
    L = native.lib()
    raw = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(raw, n) for n in NEW)
    assert L.mtgv_version() >= 111
    assert len(native.SIGNATURES["mtgv_letterbox_ragged_u8"][1]) == 10 and len(native.SIGNATURES["mtgv_warp_quads_src"][1]) == 17


def test_entries_refuse_bad_arguments_without_a_gpu():
    from mtgv import native

    L = native.lib()
    z = native.c_vp(0)
    assert L.mtgv_letterbox_ragged_u8(z, z, z, z, 0, z, 96, 128, 114, z) == 0  # no frames: nothing to do
    assert L.mtgv_letterbox_ragged_u8(z, z, z, z, 2, z, 96, 128, 114, z) == 1 and b"null" in L.mtgv_last_error()
    assert L.mtgv_letterbox_ragged_u8(z, z, z, z, 2, z, 0, 128, 114, z) == 1
    assert L.mtgv_letterbox_ragged_u8(z, z, z, z, 2, z, 96, 128, 256, z) == 1
    assert L.mtgv_warp_quads_src(z, z, z, z, z, 1, z, z, 1, 16, 12, 0.05, z, z, z, 0, z) == 1 and b"null" in L.mtgv_last_error()
    with pytest.raises(AssertionError):
        native.check(L.mtgv_warp_quads_src(z, z, z, z, z, 1, z, z, 1, 16, 12, 0.05, z, z, z, 0, z))


def _probe_quads(h, w, in_hw, seed):
    """corners in the detector's input: random ones, some in the pad and beyond the input, and the corners of the image
    rectangle and of the input themselves"""
    from mtgv.detector import fit_geometry

    _, nh, nw, top, left = fit_geometry(h, w, *in_hw)
    rng = np.random.default_rng(seed)
    q = rng.uniform(-40.0, max(in_hw) + 40.0, (30, 4, 2)).astype(np.float32)
    q[0] = [[left, top], [left + nw, top], [left + nw, top + nh], [left, top + nh]]
    q[1] = [[0, 0], [in_hw[1], 0], [in_hw[1], in_hw[0]], [0, in_hw[0]]]
    q[2] = q[0] + np.float32(0.5)
    q[3] = np.trunc(q[3])  # integer corners, as the mask quads are
    return q


@pytest.mark.parametrize("in_hw", INPUTS)
@pytest.mark.parametrize("hw", FRAME_SHAPES)
def test_mapping_equals_to_frame(hw, in_hw):
    from mtgv.adapters import to_frame_points
    from mtgv.detector import fit_geometry

    h, w = hw
    ratio, _, _, top, left = fit_geometry(h, w, *in_hw)
    quads = _probe_quads(h, w, in_hw, 1000 * h + w)
    want = to_frame_points(quads, ratio, left, top, h, w).astype(np.float32)
    got = sc.map_quads(quads, np.zeros(len(quads), np.int64), [hw], in_hw)
    assert np.array_equal(sc.bits(got), sc.bits(want))
    assert got[..., 0].min() == 0 and got[..., 0].max() == w and got[..., 1].min() == 0 and got[..., 1].max() == h  # both clips were taken
    # the image rectangle's corners come back as the frame's: a tight bound, one pixel of the coarser grid
    assert np.abs(got[0] - np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float32)).max() <= max(1.0, 1.0 / ratio)


def test_mapping_picks_each_quads_own_frame():
    hw = [(37, 53), (241, 321), (64, 96)]
    quads = np.tile(np.array([[10, 12], [100, 14], [98, 90], [8, 88]], np.float32), (3, 1, 1))
    got = sc.map_quads(quads, [2, 0, 1], hw, (128, 192))
    for q, f in enumerate([2, 0, 1]):
        np.testing.assert_array_equal(got[q], sc.map_quads(quads[:1], [0], [hw[f]], (128, 192))[0])
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("in_hw", INPUTS)
def test_source_frames_geometry_is_fit_geometry(in_hw):
    from mtgv.detector import fit_geometry, letterbox_geometry
    from mtgv.pipeline import SourceFrames

    geo, ratio = SourceFrames.geometry(FRAME_SHAPES, in_hw)
    assert geo.dtype == np.int32 and geo.shape == (len(FRAME_SHAPES), 4) and ratio.dtype == np.float64 and ratio.shape == (len(FRAME_SHAPES),)
    for i, (h, w) in enumerate(FRAME_SHAPES):
        r, nh, nw, top, left = fit_geometry(h, w, *in_hw)
        assert geo[i].tolist() == [nh, nw, top, left] and ratio[i] == r
        if in_hw[0] == in_hw[1]:
            assert (r, nh, nw, top, left) == letterbox_geometry(h, w, in_hw[0])
    g0, r0 = SourceFrames.geometry(np.zeros((0, 2), np.int64), in_hw)
    assert g0.shape == (0, 4) and r0.shape == (0,)


def test_ragged_layout_offsets():
    frames = [sc.noise_frame(h, w, h) for h, w in [(37, 53), (241, 321), (64, 96)]]
    buf, offsets, hw = sc.ragged(frames)
    assert offsets.tolist() == [0, 5883, 5883 + 232083] and offsets[1] % 4 != 0 and offsets[2] % 4 != 0
    assert buf.size == offsets[2] + 64 * 96 * 3
    for f, o, (h, w) in zip(frames, offsets, hw):
        np.testing.assert_array_equal(buf[o : o + h * w * 3].reshape(h, w, 3), f)


def test_source_frames_needs_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mtgv.pipeline import SourceFrames

    with pytest.raises((RuntimeError, AssertionError)):
        SourceFrames.from_ragged(torch.zeros(12, dtype=torch.uint8), [0], [(2, 2)], size=64)
