"""Whole-image form of dwconv7_ln (deep stages: 12 x 8 x 384, 6 x 4 x 768) against the single-row form (the row-group
kernel at one output row per thread, MTGV_DW_ROWS=0), bit for bit.  The forms share their arithmetic, so this says nothing
about a mistake they all make: the absolute reference is tests/test_gpu_dwconv_ln_direct.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Env:
    """set / unset process environment variables for one launch (the launcher reads them per call) and put them back"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# forms by the launcher's switches: the single-row form, whatever the launcher picks by itself (whole image from 128
# images at the two deep shapes, else row groups), the whole-image form at any batch size where its rule admits the shape
FORMS = {
    "single_row": dict(MTGV_DW_ROWS="0", MTGV_DW_IMAGE=None),
    "default": dict(MTGV_DW_ROWS=None, MTGV_DW_IMAGE=None),
    "image": dict(MTGV_DW_ROWS="1", MTGV_DW_IMAGE="1"),
    "no_image": dict(MTGV_DW_ROWS="1", MTGV_DW_IMAGE="0"),
}

SHAPES = [
    (256, 12, 8, 384, False),
    (256, 6, 4, 768, False),
    (130, 12, 8, 384, False),
    (3, 6, 4, 768, False),
    (256, 12, 8, 384, True),   # exact zeros and negative zeros in the input: skipping the padded taps must not change a bit
    (3, 6, 4, 768, True),
    (130, 12, 8, 320, False),  # AE-nano deep shape: 320 threads or 640 do not fill the SIMDs alike, stays on the row groups
    (130, 6, 8, 384, False),   # just outside the rule (height): must take the old path and still agree
]


@pytest.mark.parametrize("prec", ["f16x3", "f32"])  # the normalised tensor is written as SP8 words / as f32
@pytest.mark.parametrize("n,h,w,c,zeros", SHAPES)
def test_dwconv_ln_image_form_is_bit_identical(n, h, w, c, zeros, prec):
    """dwconv7_ln's output (the block's normalised tensor in the workspace, raw 32-bit words: SP8 in the f16x3 GEMM
    mode, f32 in the f32 mode) and the block's output are the same bits from the single-row form, the launcher's own
    choice, the whole-image form forced at any batch size, and the launcher with that form switched off."""
    from mtgv import native as nv

    rng = np.random.default_rng(c + n)
    f = lambda *sh: _dev(rng.standard_normal(sh).astype(np.float32))  # noqa: E731
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    if zeros:
        m = rng.integers(0, 4, x.shape)
        x[m == 0] = 0.0
        x[m == 1] = -0.0
    X = _dev(x)
    s = lambda t: t * 0.3  # noqa: E731
    args = [s(f(49, c)), s(f(c)), 1 + s(f(c)), s(f(c)), s(f(4 * c, c)), s(f(4 * c)), s(f(1, 1, 1, 4 * c)), s(f(1, 1, 1, 4 * c)), s(f(c, 4 * c)), s(f(c))]
    nws = int(nv.lib().mtgv_op_block_workspace_floats(n, h, w, c))
    t = n * h * w * c  # the workspace starts with two tensors of the block's size; dwconv7_ln writes the second
    before = nv.get_gemm_precision()
    res = {}
    try:
        nv.set_gemm_precision(prec)
        for name, env in FORMS.items():
            with _Env(**env):
                ws = torch.full((nws,), float("nan"), device="cuda")
                out = torch.full((n, h, w, c), float("nan"), device="cuda")
                nv.check(nv.lib().mtgv_op_block(nv.ptr(X), nv.ptr(out), n, h, w, c, 2, *[nv.ptr(a) for a in args], nv.ptr(ws), nv.stream()))
                torch.cuda.synchronize()
            res[name] = (ws[t:2 * t].view(torch.int32).clone(), out)
    finally:
        nv.set_gemm_precision(before)
    ref_t2, ref_out = res["single_row"]
    assert torch.isfinite(ref_out).all()
    for name in ("default", "image", "no_image"):
        t2, out = res[name]
        assert torch.equal(t2, ref_t2), f"{name}: normalised tensor differs from the single-row form's"
        assert torch.equal(out.view(torch.int32), ref_out.view(torch.int32)), f"{name}: block output differs"


def test_dwconv_ln_output_formats_differ():
    """the two GEMM modes of the test above do exercise the two output formats of dwconv7_ln"""
    from mtgv import native as nv

    n, h, w, c = 3, 6, 4, 768
    rng = np.random.default_rng(1)
    f = lambda *sh: _dev(rng.standard_normal(sh).astype(np.float32) * 0.3)  # noqa: E731
    X = f(n, h, w, c)
    args = [f(49, c), f(c), 1 + f(c), f(c), f(4 * c, c), f(4 * c), f(1, 1, 1, 4 * c), f(1, 1, 1, 4 * c), f(c, 4 * c), f(c)]
    nws = int(nv.lib().mtgv_op_block_workspace_floats(n, h, w, c))
    t = n * h * w * c
    before = nv.get_gemm_precision()
    words = {}
    try:
        for prec in ("f16x3", "f32"):
            nv.set_gemm_precision(prec)
            with _Env(MTGV_DW_ROWS="1", MTGV_DW_IMAGE="1"):
                ws = torch.zeros(nws, device="cuda")
                out = torch.empty((n, h, w, c), device="cuda")
                nv.check(nv.lib().mtgv_op_block(nv.ptr(X), nv.ptr(out), n, h, w, c, 2, *[nv.ptr(a) for a in args], nv.ptr(ws), nv.stream()))
                torch.cuda.synchronize()
            words[prec] = ws[t:2 * t].clone()
    finally:
        nv.set_gemm_precision(before)
    assert not torch.equal(words["f16x3"].view(torch.int32), words["f32"].view(torch.int32))
    # SP8: chunks of 8 channels as [8 fp16 hi][8 fp16 lo], hi + lo = the f32 value to 2^-22 relative (2^-25 absolute floor)
    sp = words["f16x3"].view(torch.float16).view(-1, 2, 8).float()
    val = (sp[:, 0] + sp[:, 1]).reshape(-1)
    ref = words["f32"]
    assert ((val - ref).abs() <= ref.abs() * 2.0 ** -21 + 2.0 ** -24).all()
