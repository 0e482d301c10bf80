"""CPU: the contour kernel's algorithm (restated in tests/contours_common.py) equals the host specification
`mtgv.adapters._mask_segments` on every case, the cases stay inside the kernel's caps, and the C ABI of
mtgv_mask_contours refuses bad arguments before it touches a device.  The GPU side is tests/test_gpu_contours.py."""
import os
import re

import numpy as np
import pytest

import contours_common as cc
from conftest import ROOT


@pytest.fixture(scope="module")
def all_cases():
    return cc.cases()


@pytest.mark.parametrize("strategy", ["all", "largest"])
def test_restatement_equals_host(all_cases, strategy):
    for name, m in all_cases:
        want, blobs = cc.host_contours(m, strategy)
        got = cc.device_contours(m, strategy)
        assert got["status"] == 0, name
        assert got["n_blobs"] == blobs, name
        assert got["n_points"] == len(want) and np.array_equal(got["points"], want), (name, got["points"].tolist(), want.tolist())


def test_inverted_v_is_cut_short_like_the_host():
    """the stopping rule (cur == start from any direction) leaves the left arm unvisited: the host's answer, pinned"""
    m = np.zeros((3, 5), np.uint8)
    for y, x in [(0, 2), (1, 1), (2, 0), (1, 3), (2, 4)]:
        m[y, x] = 1
    assert cc.host_contours(m)[0].tolist() == [[2, 0], [4, 2]]
    assert cc.device_contours(m)["points"].tolist() == [[2, 0], [4, 2]]


def test_dense_traces_of_random_masks(all_cases):
    """every blob's dense chain, not only what CHAIN_APPROX_SIMPLE keeps of it"""
    from scipy import ndimage

    from mtgv.adapters import _trace_blob

    seen = 0
    for name, m in all_cases:
        if not name.startswith("random"):
            continue
        lab, n = ndimage.label(np.pad(m != 0, 1), structure=np.ones((3, 3), int))
        dense = cc.device_contours(m)["dense"]
        assert len(dense) == n, name
        for i in range(n):
            assert np.array_equal(dense[i], _trace_blob(lab == i + 1)), (name, i)
        seen += n
    assert seen > 300


def test_cases_stay_inside_the_caps(all_cases):
    """no case may pass because a cap cut it short"""
    for name, m in all_cases:
        r = cc.device_contours(m, "all")
        assert r["n_points"] <= cc.MAX_POINTS and r["n_runs"] <= cc.MAX_RUNS and r["n_blobs"] <= cc.MAX_BLOBS, name
    big = [r for r in (cc.device_contours(m) for name, m in all_cases if name.startswith("card")) if r["n_points"] > 500]
    assert len(big) == 2  # the card masks are the reference's size of problem (hundreds of points each)


def test_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "mtg-vision_amd", "csrc", "contours.hip")).read()
    assert int(re.search(r"CT_MAX_RUNS = (\d+);", src).group(1)) == cc.MAX_RUNS
    assert int(re.search(r"CT_MAX_BLOBS = (\d+);", src).group(1)) == cc.MAX_BLOBS


def test_overflow_cases_of_the_restatement():
    r = cc.device_contours(cc.random_mask(0.3, 0), "all", max_points=64)
    want = cc.host_contours(cc.random_mask(0.3, 0))[0]
    assert len(want) > 64 and r["status"] == 1 and r["n_points"] == 64 and np.array_equal(r["points"], want[:64])
    g = cc.device_contours(cc.stride2_grid())
    assert g["n_blobs"] == 33 * 33 > cc.MAX_BLOBS and g["status"] == 1 and g["n_points"] == 0


# ---- the C ABI, no device ----
@pytest.fixture(scope="module")
def lib():
    from mtgv import native

    return native.lib()


def test_version_and_symbols(lib):
    assert lib.mtgv_version() >= 107
    for name in ("mtgv_mask_contours_workspace_bytes", "mtgv_mask_contours", "mtgv_mask_contours_logits"):
        assert hasattr(lib, name), name


def _mask_call(lib, n=1, h=8, w=8, strategy=0, max_points=16, ws=None):
    ws = lib.mtgv_mask_contours_workspace_bytes(max(n, 1), max(h, 1), max(w, 1), max(max_points, 1)) if ws is None else ws
    return lib.mtgv_mask_contours(None, n, h, w, strategy, max_points, None, None, None, None, None, ws, None)


def _logits_call(lib, n=1, mh=2, mw=2, scale=4, strategy=0, max_points=16, ws=None):
    ws = lib.mtgv_mask_contours_workspace_bytes(max(n, 1), 8, 8, max(max_points, 1)) if ws is None else ws
    return lib.mtgv_mask_contours_logits(None, n, mh, mw, scale, strategy, max_points, None, None, None, None, None, ws, None)


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(max_points=0), dict(strategy=2), dict(strategy=-1),
                                dict(h=4096, w=4096), dict(ws=0)])
def test_argument_errors_without_a_device(lib, kw):
    assert _mask_call(lib, **kw) == 1
    assert lib.mtgv_last_error().startswith(b"mask_contours:"), lib.mtgv_last_error()
    kl = {{"h": "mh", "w": "mw"}.get(k, k): v for k, v in kw.items()}
    assert _logits_call(lib, **kl) == 1
    assert lib.mtgv_last_error().startswith(b"mask_contours:"), lib.mtgv_last_error()


def test_scale_and_null_errors_without_a_device(lib):
    for scale in (0, -4):
        assert _logits_call(lib, scale=scale) == 1 and lib.mtgv_last_error().startswith(b"mask_contours:")
    # everything valid but the pointers: still refused before any device call
    assert _mask_call(lib) == 1 and b"mask_contours: null" in lib.mtgv_last_error()
    assert _logits_call(lib) == 1 and b"mask_contours: null" in lib.mtgv_last_error()
    # 640 x 640 fits, the next LDS-sized step does not
    assert b"null" in (_mask_call(lib, h=640, w=640) and lib.mtgv_last_error())
    assert b"LDS" in (_mask_call(lib, h=1280, w=1280) and lib.mtgv_last_error())


def test_workspace_bytes_monotone(lib):
    f = lib.mtgv_mask_contours_workspace_bytes
    base = (2, 64, 64, 128)
    assert f(*base) > 0
    for k in range(4):
        vals = [f(*[b * s if i == k else b for i, b in enumerate(base)]) for s in (1, 2, 3, 5, 8)]
        assert all(a <= b for a, b in zip(vals, vals[1:])), (k, vals)
    assert f(4, 64, 64, 128) > f(2, 64, 64, 128)


def test_wrappers_are_exported():
    from mtgv import crop
    from mtgv.adapters import CardSegmenter

    assert callable(crop.mask_contours) and callable(crop.mask_contours_from_logits)
    assert crop.CONTOUR_STRATEGIES == cc.STRATEGIES
    assert CardSegmenter.TRACE_MAX_POINTS == cc.MAX_POINTS
