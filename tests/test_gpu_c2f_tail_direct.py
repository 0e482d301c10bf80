"""The fused C2f tail kernels (c2f_tail_kernel.h: c2f_tail_kernel at ch = 16, c2f_tail32_kernel<1|2> at ch = 32) as a
single op, mtgv_op_c2f_tail, against fp64 - at the smallest maps c2f_tail_ok admits, every (ch, bottlenecks, shortcut)
combination it admits, batches, and channel views with offsets and spare channels (the table: c2f_tail_common.CASES).

Every case (draws and reference: c2f_tail_common.py; f16x3 mode)
  - places the input inside an allocation in which every byte that is not one of the (1 + nb) ch channels the launch reads
    is an fp16 NaN: the pixel's other channels - the slice where a network's cat would have room for y_new among them -
    and w + 2 pixels before the first and after the last image; the allocation must come back bit-unchanged;
  - prefills the output allocation (8 pixels of margin either side) with a NaN pattern, requires every word outside
    channels [out_co, out_co + cout) to be unchanged and every value inside to be finite;
  - requires status 0, exactly one launch in the launch profiler and the three layers' algorithmic FLOPs,
    2 M (2 * 9 ch^2 + cout (2 + nb) ch);
  - requires the output words to equal those of the three mtgv_op_conv2d_ex launches the kernel replaces (3x3 SiLU into
    SP8, 3x3 SiLU with the SP8 residual into the next slice of a private cat, 1x1 SiLU over the (2 + nb) ch channels),
    whose paths it prints;
  - holds max |out - fp64| to TOL and prints it (pytest -s);
  - for n > 1: each image run alone gives the bits of its rows in the batch.

TOL comes from the three-launch composition - gemm_sp_kernel, not the code under test - against the same fp64 reference
on the same seven cases: TOL = twice the largest of those errors, rounded up to one significant digit.
  case (n, H x W, ch, nb, shortcut)      three launches   fused launch
  (1, 80 x 96, 16, 1, yes)               7.52e-06         7.52e-06
  (2, 88 x 96, 16, 1, no)                6.71e-06         6.71e-06
  (1, 80 x 128, 16, 1, yes)              6.04e-06         6.04e-06
  (1, 80 x 80, 32, 1, no)                7.96e-06         7.96e-06
  (2, 80 x 96, 32, 1, yes)               1.04e-05         1.04e-05
  (1, 88 x 80, 32, 2, yes)               9.51e-06         9.51e-06
  (3, 80 x 80, 32, 2, no)                9.24e-06         9.24e-06
The fused launch's outputs are the three launches' bit for bit, so the columns agree.  Largest 1.04e-5, twice that
2.08e-5: TOL = 3e-5 (c2f_tail_common.TOL) - the bound test_gpu_sp8_conv.py holds a single layer to at unit input scale;
the three layers together, border rows scaled by 8 included, stay a third of it.

A second test holds the entry point to its refusals: status 1, an untouched output and no launch for every shape, view or
mode c2f_tail_ok does not admit - it never falls back to the three launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import c2f_tail_common as cc
import sp8_util as sp
from c2f_tail_common import CASES, TOL, Case
from test_gpu_sp8_conv import CANARY, SILU, SP8, Buf, conv_ex, output

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _f16x3():
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision("f16x3")
    yield
    native.set_gemm_precision(before)


class View:
    """channels [co, co + c) of a Buf, as conv_ex takes a tensor"""

    def __init__(self, buf, co, c):
        self.ptr, self.ct, self.co, self.c, self.fmt = buf.ptr, buf.ct, co, c, buf.fmt


def cat_buf(case, x, ct, co, room=0):
    """an SP8 cat of ct floats per pixel: the (1 + nb) ch channels of x from channel co on, then `room` channels that
    belong to the tensor but hold NaNs, NaNs everywhere else"""
    c_in = (1 + case.nb) * case.ch
    b = Buf(x.shape[0], ct, co, c_in + room, SP8, guard=case.w + 2)
    b.host[b.guard : b.guard + b.px, co : co + c_in] = sp.pack(x)
    return b.upload()


def words(t):
    return t.cpu().numpy().view(np.uint32)


def peek(buf):
    """(values fp64, words, nothing else changed?) of an output Buf, asserting nothing"""
    got = buf.dev.cpu().numpy()
    inside = np.ascontiguousarray(got[buf.guard : buf.guard + buf.px, buf.co : buf.co + buf.c])
    rest = got.view(np.uint32).copy()
    rest[buf.guard : buf.guard + buf.px, buf.co : buf.co + buf.c] = CANARY
    return sp.unpack(inside), inside.view(np.uint32), bool((rest == CANARY).all())


def device_weights(d):
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(d, k))).cuda() for k in ("w1", "b1", "w2", "b2", "w3", "b3")}


def descriptor(case, cat, out, dw, cout=None):
    from mtgv import native as nv

    t = nv.C2fTail()
    t.cat, t.cat_ct, t.cat_co = cat.ptr, case.cat_ct, case.cat_co
    t.n, t.h, t.w, t.ch, t.nb, t.shortcut = case.n, case.h, case.w, case.ch, case.nb, int(case.shortcut)
    t.w1, t.b1, t.w2, t.b2, t.w3, t.b3 = (dw[k].data_ptr() for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    t.cout = 2 * case.ch if cout is None else cout
    t.out, t.out_ct, t.out_co = out.ptr, case.out_ct, case.out_co
    return t


def call(t):
    """one mtgv_op_c2f_tail call under the launch profiler: (status, launches recorded, their algorithmic FLOPs)"""
    from mtgv import native as nv

    L = nv.lib()
    nv.check(L.mtgv_profile_gemm(1))
    try:
        rc = L.mtgv_op_c2f_tail(C.byref(t), nv.stream())
        if rc not in (0, 1):  # a failed launch: the device context is gone, nothing after it in this process means anything
            pytest.exit(f"mtgv_op_c2f_tail: status {rc}, {L.mtgv_last_error().decode()}", returncode=3)
        torch.cuda.synchronize()
        cnt, fl = C.c_int64(-1), C.c_double(-1)
        nv.check(L.mtgv_profile_gemm_read(None, C.byref(fl), C.byref(cnt)))
    finally:
        nv.check(L.mtgv_profile_gemm(0))
    return rc, cnt.value, fl.value


def fused(case, x, dw):
    """(status, launches, FLOPs, cat allocation unchanged?, output Buf)"""
    cat = cat_buf(case, x, case.cat_ct, case.cat_co)
    out = output(x.shape[0], 2 * case.ch, SP8, case.out_ct, case.out_co)
    rc, cnt, fl = call(descriptor(case, cat, out, dw))
    return rc, cnt, fl, bool((words(cat.dev) == cat.host.view(np.uint32)).all()), out


def three_launches(case, d):
    """the bottleneck's two convs and the block's 1x1 as mtgv_op_conv2d_ex launches on a private cat with room for y_new:
    (paths, output Buf)"""
    n, h, w, ch, nb = case.n, case.h, case.w, case.ch, case.nb
    co = case.cat_co
    cat = cat_buf(case, d.x, co + (2 + nb) * ch, co, room=ch)
    y_last, y_new = View(cat, co + nb * ch, ch), View(cat, co + (1 + nb) * ch, ch)
    tmp = output(n * h * w, ch, SP8)
    out = output(n * h * w, 2 * ch, SP8, case.out_ct, case.out_co)
    p1 = conv_ex(y_last, n, h, w, d.w1, d.b1, 1, 1, SILU, tmp)
    tmp.read()
    p2 = conv_ex(tmp, n, h, w, d.w2, d.b2, 1, 1, SILU, y_new, res=y_last if case.shortcut else None)
    p3 = conv_ex(View(cat, co, (2 + nb) * ch), n, h, w, d.w3.reshape(2 * ch, 1, 1, -1), d.b3, 1, 0, SILU, out)
    return (p1, p2, p3), out


def label(case):
    return f"({case.n}, {case.h} x {case.w}, {case.ch}, {case.nb}, {'yes' if case.shortcut else 'no'})"


@pytest.mark.parametrize("index", range(len(CASES)))
def test_c2f_tail_direct(index):
    case = CASES[index]
    d, ref = cc.drawn(index)
    dw = device_weights(d)
    rc, cnt, fl, cat_same, out = fused(case, d.x, dw)
    vals, bits, rest_same = peek(out)
    paths, out3 = three_launches(case, d)
    vals3, bits3, rest3_same = peek(out3)
    err, err3 = float(np.abs(vals - ref).max()), float(np.abs(vals3 - ref).max())
    print(f"c2f tail {index} {label(case)} cat {case.cat_ct}/{case.cat_co} out {case.out_ct}/{case.out_co}: status {rc}, {cnt} launch(es), "
          f"max_err fused={err:.3g} three launches={err3:.3g}, differing words {int((bits != bits3).sum())}, paths {paths}")
    # 1. one launch, the three layers' FLOPs
    assert rc == 0 and cnt == 1 and fl == cc.flops(case), (rc, cnt, fl, cc.flops(case))
    # 2. writes: only the output channels, all of them
    assert cat_same, "the launch changed cat's allocation"
    assert rest_same, "bytes outside the output channels changed"
    assert np.isfinite(vals).all(), "output channels not finite (unwritten or poisoned by a NaN neighbour)"
    # 3. bit identity with the launches it replaces
    assert rest3_same and np.isfinite(vals3).all()
    assert (bits == bits3).all(), (index, int((bits != bits3).sum()))
    # 4. against fp64
    assert err < TOL, (index, err)
    # 5. batch independence
    px = case.h * case.w
    for i in range(case.n if case.n > 1 else 0):
        rc1, _, _, _, out1 = fused(case._replace(n=1), d.x[i * px : (i + 1) * px], dw)
        _, bits1, rest1_same = peek(out1)
        assert rc1 == 0 and rest1_same
        assert (bits1 == bits[i * px : (i + 1) * px]).all(), (index, i)


OK16, OK32 = Case(1, 80, 96, 16, 1, True, 32, 0, 32, 0), Case(1, 80, 96, 32, 1, True, 64, 0, 64, 0)
REFUSALS = [
    ("H = 72", OK16._replace(h=72), {}),
    ("W = 80 at ch 16", OK16._replace(w=80), {}),
    ("W = 88 at ch 32", OK32._replace(w=88), {}),
    ("ch = 64", Case(1, 80, 96, 64, 1, True, 128, 0, 128, 0), {}),
    ("ch = 16 with nb = 2", OK16._replace(nb=2, cat_ct=48), {}),
    ("nb = 3", OK32._replace(nb=3, cat_ct=128), {}),
    ("cout != 2 ch", OK16, {"cout": 24}),
    ("cat_co = 4", OK16._replace(cat_ct=40), {"cat_co": 4}),
    ("cat_ct too narrow for 1 + nb slices", OK32._replace(nb=2, cat_ct=96), {"cat_ct": 88}),
    ("a null bias", OK32, {"b2": None}),
    ("f32 GEMM mode", OK16, {"mode": "f32"}),
]


@pytest.mark.parametrize("what,case,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, case, over):
    """what c2f_tail_ok does not admit is status 1 with nothing launched and nothing written - never the three launches.
    The buffers are those of the case as the table states it; `over` then changes the descriptor alone."""
    from mtgv import native as nv

    d = cc.draw(case, 7200)
    dw = device_weights(d)
    cat = cat_buf(case, d.x, case.cat_ct, case.cat_co)
    out = output(d.x.shape[0], 2 * case.ch, SP8, case.out_ct, case.out_co)
    t = descriptor(case, cat, out, dw, cout=over.get("cout"))
    for k in ("cat_co", "cat_ct"):
        if k in over:
            setattr(t, k, over[k])
    if "b2" in over:
        t.b2 = None
    nv.set_gemm_precision(over.get("mode", "f16x3"))  # (the fixture restores the mode)
    rc, cnt, _ = call(t)
    msg = nv.lib().mtgv_last_error().decode()
    print(f"c2f tail refusal, {what}: status {rc}, {cnt} launches, '{msg}'")
    assert rc == 1 and cnt == 0, (what, rc, cnt)
    assert (words(out.dev) == CANARY).all(), what
    assert (words(cat.dev) == cat.host.view(np.uint32)).all(), what
    if what == "H = 72":
        assert "c2f_tail: no fused kernel" in msg and "72 x 96" in msg, msg
