"""dwconv7_ln (dwconv7_ln_rows_kernel<TW, TH, SP8, WL>, dwconv7_ln_stream_kernel, dwconv7_ln_image_kernel) as a single op,
mtgv_op_dwconv7_ln, against fp64 - at the smallest shapes that reach each of the forms the dispatcher can pick, in both
output formats (the table: dwconv_ln_common.CASES; draws and reference: dwconv_ln_common.py).

Every case
  - must run the form the table names (the entry point reports what it launched);
  - places x and out in one allocation, each between regions of NaNs wider than three rows and three pixels, out itself
    NaN before the call: every word outside out must come back unchanged, every value of out finite;
  - f32 output: max |out - fp64| <= TOL; SP8 output: |unpack(out) - fp64| <= TOL + 2^-21 |ref| + 2^-24, the format's own
    bound (sp8.h) on top;
  - run again under MTGV_DW_ROWS=0 (the single-row form: the row-group kernel at TH = 1) gives the same bits in both
    formats - on the operation's own output;
  - two cases (a row-group one, a whole-image one): image 0 run alone gives the bits it has in the batch.

TOL (dwconv_ln_common.TOL) comes from mtgv_op_dwconv7 followed by mtgv_op_layernorm - separate kernels, not the code under
test - against the same fp64 reference on the same cases: twice the largest of those errors, rounded up to one
significant digit.  max |out - fp64| (pytest -s prints them; the separate kernels write f32):
  case                                      form {kind, TW, TH, WL}   separate kernels   fused f32   fused SP8
  (2, 7, 6, 16)                             {0, 4, 3, 1}              1.53e-05           1.5e-05     1.5e-05
  (3, 4, 9, 40)                             {0, 4, 3, 1}              1.51e-05           1.85e-05    1.85e-05
  (1, 3, 4, 20)                             {0, 4, 3, 1}              1.47e-05           1.47e-05    -
  (2, 5, 4, 280)                            {0, 4, 3, 1}              1.7e-05            2.42e-05    2.42e-05
  (2, 4, 11, 288)                           {0, 8, 3, 0}              1.54e-05           2.75e-05    2.76e-05
  (2, 7, 5, 320)                            {0, 4, 3, 0}              1.73e-05           2.77e-05    2.77e-05
  (1, 3, 8, 1024)                           {0, 8, 3, 0}              1.51e-05           4.41e-05    4.41e-05
  (1, 1, 1, 8)                              {0, 2, 1, 0}              2.47e-06           2.47e-06    2.47e-06
  (2, 5, 2, 16)                             {0, 2, 1, 0}              9.54e-06           9.54e-06    9.56e-06
  (2, 3, 3, 24)                             {0, 2, 1, 0}              1.28e-05           1.17e-05    1.17e-05
  (2, 7, 6, 32) MTGV_DW_ROWS=0              {0, 4, 1, 0}              1.34e-05           1.39e-05    1.39e-05
  (2, 7, 11, 96) MTGV_DW_ROWS=0             {0, 8, 1, 0}              1.95e-05           2.19e-05    2.19e-05
  (128, 1, 32, 96)                          {1, 4, 3, 0}              1.88e-05           2.23e-05    2.23e-05
  (128, 14, 32, 96)                         {1, 4, 3, 0}              4.54e-05           4.54e-05    4.54e-05
  (129, 13, 16, 192)                        {1, 4, 3, 0}              4.34e-05           4.5e-05     4.49e-05
  (3, 12, 8, 384) MTGV_DW_IMAGE=1           {2, 8, 6, 0}              2.33e-05           3.26e-05    3.26e-05
  (3, 6, 4, 768) MTGV_DW_IMAGE=1            {2, 4, 6, 0}              1.88e-05           3.4e-05     3.4e-05
  (128, 12, 8, 384)                         {2, 8, 6, 0}              2.5e-05            3.65e-05    3.66e-05
  (2, 7, 6, 16) eps=0.5                     {0, 4, 3, 1}              1.31e-05           1.39e-05    1.39e-05
Largest of the separate kernels 4.54e-5, twice that 9.08e-5: TOL = 1e-4.  The fused forms stay within 4.54e-5; at
C = 1024 the row-group kernel, which adds a pixel's 256 quad sums in one chain, is 2.9 x the separate kernels' error there.

A second test holds the entry point to its refusals: status 1, nothing launched and an untouched output for every shape
or format dwconv7_ln_supported does not admit, and for null pointers - it never runs the unfused pair instead."""
import ctypes as C

import numpy as np
import pytest
import torch

import dwconv_ln_common as cc
import sp8_util as sp
from dwconv_ln_common import CASES, REFUSALS, TOL, Switches

pytestmark = pytest.mark.gpu

F32, SP8 = 0, 1
NAN_WORD = np.float32(np.nan).view(np.uint32)


def _dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared draws are read-only)


class Arena:
    """[guard | x | guard | out | guard] in one allocation, everything but x NaN; the guards are whole KB and at least
    three rows and four pixels long, so a halo read without its mask lands in NaNs, not in another tensor"""

    def __init__(self, x):
        n, h, w, c = x.shape
        self.shape, self.t = x.shape, x.size
        self.g = -(-((3 * w + 4) * c) // 256) * 256
        self.host = np.full(3 * self.g + 2 * self.t, np.nan, np.float32)
        self.x0, self.o0 = self.g, 2 * self.g + self.t
        self.host[self.x0 : self.x0 + self.t] = x.reshape(-1)
        self.dev = torch.from_numpy(self.host).cuda()

    def ptr(self, off):
        return C.c_void_p(self.dev.data_ptr() + 4 * off)

    def read(self):
        """(out as words [n h w][c], nothing else changed?)"""
        got = self.dev.cpu().numpy().view(np.uint32)
        out = got[self.o0 : self.o0 + self.t].reshape(-1, self.shape[3]).copy()
        rest = got.copy()
        rest[self.o0 : self.o0 + self.t] = NAN_WORD
        return out, bool((rest == self.host.view(np.uint32)).all())


def fused(case, x, dw, fmt, **over):
    """one mtgv_op_dwconv7_ln call on x under the case's switches (and `over`): (status, form, out words, rest unchanged?)"""
    from mtgv import native as nv

    n, h, w, c = x.shape
    a = Arena(x)
    form = (C.c_int32 * 4)(-1, -1, -1, -1)
    with Switches(case.env, **over):
        rc = nv.lib().mtgv_op_dwconv7_ln(a.ptr(a.x0), *[nv.ptr(t) for t in dw], a.ptr(a.o0), n, h, w, c, case.eps, fmt, form, nv.stream())
    if rc not in (0, 1):  # a failed launch: the device context is gone, nothing after it in this process means anything
        pytest.exit(f"mtgv_op_dwconv7_ln: status {rc}, {nv.lib().mtgv_last_error().decode()}", returncode=3)
    torch.cuda.synchronize()
    return (rc, tuple(form)) + a.read()


def pair(case, d, dw):
    """mtgv_op_dwconv7 then mtgv_op_layernorm, the separate kernels: out as float64 [n h w][c]"""
    from mtgv import native as nv

    n, h, w, c = d.x.shape
    X, tmp, out = _dev(d.x), torch.full(d.x.shape, float("nan"), device="cuda"), torch.full(d.x.shape, float("nan"), device="cuda")
    nv.check(nv.lib().mtgv_op_dwconv7(nv.ptr(X), nv.ptr(dw[0]), nv.ptr(dw[1]), nv.ptr(tmp), n, h, w, c, nv.stream()))
    nv.check(nv.lib().mtgv_op_layernorm(nv.ptr(tmp), nv.ptr(dw[2]), nv.ptr(dw[3]), nv.ptr(out), n * h * w, c, case.eps, nv.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64).reshape(-1, c)


def values(words, fmt):
    return sp.unpack(words.view(np.float32)) if fmt == SP8 else words.view(np.float32).astype(np.float64)


def label(case):
    env = " ".join(f"{k}={v}" for k, v in case.env)
    return f"({case.n}, {case.h}, {case.w}, {case.c})" + (f" {env}" if env else "") + (f" eps={case.eps}" if case.eps != cc.EPS else "")


@pytest.mark.parametrize("index", range(len(CASES)))
def test_dwconv_ln_direct(index):
    case = CASES[index]
    d, ref = cc.drawn(index)
    ref = ref.reshape(-1, case.c)
    dw = [_dev(a) for a in (d.w49, d.bias, d.ln_w, d.ln_b)]
    err_pair = float(np.abs(pair(case, d, dw) - ref).max())
    for fmt in (F32, SP8) if case.c % 8 == 0 else (F32,):
        rc, form, words, rest_same = fused(case, d.x, dw, fmt)
        vals = values(words, fmt)
        err = np.abs(vals - ref)
        print(f"dwconv7_ln {index} {label(case)} fmt {fmt}: status {rc}, form {form}, max_err fused={np.nanmax(err):.3g} "
              f"separate kernels={err_pair:.3g}")
        # 1. the form
        assert rc == 0 and form == case.form, (index, fmt, rc, form)
        # 2. writes: all of out, nothing else
        assert rest_same, "words outside out changed"
        assert np.isfinite(vals).all(), "out not finite (unwritten, or poisoned by a NaN neighbour)"
        # 3. against fp64
        bound = TOL + (2.0**-21 * np.abs(ref) + 2.0**-24 if fmt == SP8 else 0.0)
        assert (err <= bound).all(), (index, fmt, float(err.max()))
        # 4. the single-row form gives the same bits
        rc0, form0, words0, rest0_same = fused(case, d.x, dw, fmt, MTGV_DW_ROWS="0")
        assert rc0 == 0 and form0[0] == cc.ROWS and form0[2] == 1 and rest0_same, (index, fmt, rc0, form0)
        assert (words0 == words).all(), (index, fmt, int((words0 != words).sum()))
        # 5. batch independence
        if index in cc.BATCH_CASES:
            rc1, form1, words1, rest1_same = fused(case, d.x[:1], dw, fmt)
            assert rc1 == 0 and form1 == case.form and rest1_same, (index, fmt, rc1, form1)
            assert (words1 == words[: case.h * case.w]).all(), (index, fmt)


NULLS = ["x", "w49", "bias", "ln_w", "ln_b", "out", "form"]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS] + [f"null {k}" for k in NULLS])
def test_refusals(what):
    """what the fused launch does not take is status 1 with nothing written - never mtgv_op_dwconv7 + mtgv_op_layernorm"""
    from mtgv import native as nv

    (n, h, w, c), fmt = next((r[1], r[2]) for r in REFUSALS if r[0] == what) if not what.startswith("null") else ((2, 7, 6, 16), F32)
    rng = np.random.default_rng(11390)
    a = Arena(rng.standard_normal((n, h, w, c)).astype(np.float32))
    dw = [_dev(rng.standard_normal(s).astype(np.float32)) for s in ((49, c), c, c, c)]
    form = (C.c_int32 * 4)(-1, -1, -1, -1)
    args = dict(x=a.ptr(a.x0), w49=nv.ptr(dw[0]), bias=nv.ptr(dw[1]), ln_w=nv.ptr(dw[2]), ln_b=nv.ptr(dw[3]), out=a.ptr(a.o0), form=form)
    if what.startswith("null"):
        args[what[5:]] = None
    with Switches(()):
        rc = nv.lib().mtgv_op_dwconv7_ln(*[args[k] for k in NULLS[:6]], n, h, w, c, 1e-6, fmt, args["form"], nv.stream())
    msg = nv.lib().mtgv_last_error().decode()
    torch.cuda.synchronize()
    words, rest_same = a.read()
    print(f"dwconv7_ln refusal, {what}: status {rc}, '{msg}'")
    assert rc == 1 and "dwconv7_ln" in msg, (what, rc, msg)
    assert (words == NAN_WORD).all() and rest_same, what
