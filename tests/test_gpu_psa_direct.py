"""YOLO11's two own kernels (detector_v11.hip) as single ops against fp64: attn_kernel<32, 64, 16>, the C2PSA attention core
(mtgv_op_psa_attn), and the four instantiations of dwconv3_kernel<IN_SP8, OUT_SP8>, the depthwise 3x3 (mtgv_op_dwconv3) -
the launches Detector::c2psa and Detector::head_cls_v11 make, at the smallest shapes that reach each edge of the kernels
(cases, draws, references and the mistakes they separate: psa_common.py; shown without a GPU by test_psa_cpu.py).

Until now both were reached only through whole networks with random weights (test_gpu_yolo11.py and the "11" arms of the
rect, scales, OBB and full-size tests).  The largest |logit| C2PSA sees in test_gpu_yolo11.py's fixture
(spec.random_detector_state(cfg, 3, cls_bias=-0.9), the seed-4 frames; from oracle/detector_ref on the CPU) is 0.284: per
query the logits span at most 0.18, the largest softmax weight is 0.00273 where a mean over the 400 keys has 0.00250 (q, k
and v have a standard deviation of 0.33).  Those tests exercise the softmax as a mean; a running maximum that is never
updated, a rescale that misses the sum or a scale of 1 / sqrt(64) move their predictions by far less than their 1e-4.

Bound, both ops: 4 x the largest error of the same expression in float32 torch on the CPU on the same inputs, both errors
against the fp64 reference (test_gpu_area_attn.py's rule; the kernel sums in another order and uses the hardware
exponential).  max |out - fp64| as measured (pytest -s prints them; the float32 torch error of the small cases depends on
the CPU it runs on - 4.7e-7 and 9.9e-7 have both been seen at N = 6 - the kernel's does not):
  attention                            attention only                         with positional encoding
  (n, h, w, heads)  draw  max |logit|  kernel    float32 torch  max |ref|     kernel    float32 torch  max |ref|
  (1, 2, 3, 2)      flat   7.9         9.12e-07  4.69e-07       2.46          9.34e-07  4.45e-07       4.21
                    ramp   9.3         1.74e-06  4.77e-07       2.33          1.74e-06  5.04e-07       4.37
  (2, 4, 4, 2)      flat  10.8         1.36e-06  1.46e-06       3.10          1.37e-06  1.48e-06       6.03
                    ramp  12.3         1.38e-06  2.50e-06       3.40          1.52e-06  2.55e-06       6.23
  (3, 3, 7, 1)      flat  11.7         2.03e-06  1.11e-06       2.91          2.02e-06  1.07e-06       5.02
                    ramp  13.7         1.61e-06  1.28e-06       3.37          1.66e-06  1.24e-06       5.40
  (2, 16, 16, 2)    flat  17.7         5.05e-06  3.24e-06       3.50          4.91e-06  3.11e-06       7.39
                    ramp  23.0         5.22e-06  3.54e-06       3.82          5.20e-06  3.59e-06       7.81
  (1, 1, 257, 2)    flat  14.8         2.67e-06  2.23e-06       3.10          2.72e-06  2.25e-06       4.18
                    ramp  22.2         2.43e-06  3.58e-06       3.62          2.45e-06  3.57e-06       5.14
  (2, 15, 20, 2)    flat  17.4         5.28e-06  2.90e-06       3.40          5.21e-06  2.76e-06       5.86
                    ramp  20.4         3.25e-06  4.00e-06       3.59          3.32e-06  3.95e-06       6.70
  (1, 20, 20, 4)    flat  17.7         3.51e-06  3.81e-06       3.52          3.48e-06  3.91e-06       5.71
                    ramp  23.3         4.33e-06  6.03e-06       3.78          4.31e-06  6.06e-06       6.63
The kernel is between 0.6 and 3.7 x the float32 torch error; the closest to the bound is (1, 2, 3, 2) ramp at 3.7 x, six
keys, where float32 torch is at its most exact (4.8e-7 is two ulp of the result).
  depthwise 3x3, f32 -> f32                   on the draw                            on its SP8 rounding
  case                                        kernel    float32 torch  max |ref|     kernel    float32 torch
  (1, 1, 1, 8)                                8.87e-08  8.87e-08        3.7          5.52e-08  5.52e-08
  (2, 1, 5, 16)                               7.90e-07  7.90e-07       14.5          6.83e-07  6.83e-07
  (2, 5, 1, 16)                               6.05e-07  6.05e-07       10.2          6.05e-07  6.05e-07
  (3, 4, 6, 24)                               2.55e-06  2.55e-06       21.5          2.61e-06  2.61e-06
  (2, 7, 9, 72)                               2.80e-06  2.80e-06       30.1          2.80e-06  2.80e-06
  (2, 6, 5, 128) pe form                      3.96e-06  3.96e-06       26.2          3.84e-06  3.84e-06
  (2, 5, 7, 40) class-branch form, SiLU       1.94e-06  1.94e-06       18.2          2.12e-06  2.12e-06
  (2, 3, 4, 32) SiLU + addend, groups of 16   2.17e-06  2.17e-06       31.0          2.02e-06  2.02e-06
  the same at x_co = out_co = 4               1.75e-06  1.75e-06
The two columns agree to every digit: the largest error sits on a border pixel (input times 8), where the kernel's chain
- bias, then nine fmas in tap order - evidently is float32 torch's, and a SiLU of a large positive value is the identity
in both.  That the figure is the kernel's own was checked with a mistaken copy of the kernels (the gather expression
replaced by c; the rescale of the online softmax removed): the three gather cases fail in every format pair, the
attention fails at every N > 16.  The SP8 instantiations are bit-identical to these runs.

Attention, besides: the output is NaN before the call and finite after it; images and heads are isolated (overwriting
image 0's or head 0's rows leaves every other output bit-identical and changes that one's); a batch gives the bits of its
images run one at a time; with the positional encoding the op equals its two launches composed by hand from
mtgv_op_psa_attn without pe and mtgv_op_dwconv3 with the detector's gather arguments, bit for bit.

Depthwise 3x3, per case and format pair: input and output placed by test_gpu_sp8_conv's Buf - every channel of the input pixel the
kernel must not read and w + 2 pixels either side of the images hold a pattern that is NaN as f32 and as fp16, the output
allocation a canary that must survive outside the output channels, every value inside finite.  The f32 -> f32 run is
held to fp64; the three SP8 instantiations to bit identity with it, since the kernel computes the same f32 value under
`fp contract(off)` and only the load and the store differ: SP8 out = sp8_util.pack of the f32 result, SP8 in = the f32
run on float32(unpack(pack(x))) (itself held to fp64 on those values).

Refusals: every condition dwconv3_launch and psa_attn_launch check is status 1 with a message naming the op and an
untouched NaN-prefilled output."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import psa_common as pc
import sp8_util as sp
from test_gpu_sp8_conv import F32, SP8, Buf

pytestmark = pytest.mark.gpu

NAN_WORD = np.float32(np.nan).view(np.uint32)


def _dev(a):
    return torch.tensor(np.asarray(a), device="cuda")  # (a copy: the shared draws are read-only)


def _status(rc, op):
    from mtgv import native as nv

    if rc not in (0, 1):  # a failed launch: the device context is gone, nothing after it in this process means anything
        pytest.exit(f"{op}: status {rc}, {nv.lib().mtgv_last_error().decode()}", returncode=3)
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
def attn(case, qkv, pe=None):
    """one mtgv_op_psa_attn call on qkv (any batch of the case's maps) into a NaN-filled output: float32 (n, N, heads * 64)"""
    from mtgv import native as nv

    _, h, w, heads = case
    n = qkv.shape[0]
    assert qkv.shape == (n, h * w, heads * 128)
    Q, out = _dev(qkv), torch.full((n, h * w, heads * pc.HD), float("nan"), device="cuda")
    W, B = (_dev(pe[0]), _dev(pe[1])) if pe is not None else (None, None)
    rc = _status(nv.lib().mtgv_op_psa_attn(nv.ptr(Q), nv.ptr(W), nv.ptr(B), n, h, w, heads, nv.ptr(out), nv.stream()), "mtgv_op_psa_attn")
    assert rc == 0, nv.lib().mtgv_last_error().decode()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def attn_only(case, kind):
    got = attn(case, pc.attn_draw(case, kind).qkv)
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("pe", [False, True], ids=["attn", "attn+pe"])
@pytest.mark.parametrize("kind", pc.ATTN_DRAWS)
@pytest.mark.parametrize("case", pc.ATTN_CASES, ids=pc.attn_id)
def test_attention_against_float64(case, kind, pe):
    d = pc.attn_draw(case, kind)
    ref, bound, err32 = pc.attn_expected(case, kind, pe)
    got = attn(case, d.qkv, (d.pe_w9, d.pe_bias)) if pe else attn_only(case, kind)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"psa_attn {pc.attn_id(case)} {kind} pe {int(pe)}: kernel {err:.2e}, float32 torch {err32:.2e}, bound {bound:.2e} "
          f"(max |ref| {np.abs(ref).max():.2f}, max |logit| {pc.max_logit(case, kind):.1f})")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= bound


@pytest.mark.parametrize("case", [c for c in pc.ATTN_CASES if c[0] > 1], ids=pc.attn_id)
def test_images_are_isolated(case):
    """overwriting image 0's q / k / v rows leaves the other images' outputs bit-identical, and changes image 0's"""
    qkv = pc.attn_draw(case, "ramp").qkv
    other = qkv.copy()
    other[0] = np.random.default_rng(11491).standard_normal(other[0].shape).astype(np.float32)
    a, b = attn_only(case, "ramp"), attn(case, other)
    assert np.array_equal(a[1:].view(np.uint32), b[1:].view(np.uint32))
    assert (a[0] != b[0]).any(axis=1).all()


@pytest.mark.parametrize("case", [c for c in pc.ATTN_CASES if c[3] > 1], ids=pc.attn_id)
def test_heads_are_isolated(case):
    """overwriting head 0's q / k / v channels leaves the other heads' outputs bit-identical, and changes head 0's"""
    n, h, w, heads = case
    qkv = pc.attn_draw(case, "ramp").qkv
    other = qkv.copy()
    other[..., :128] = np.random.default_rng(11492).standard_normal(other[..., :128].shape).astype(np.float32)
    a, b = attn_only(case, "ramp"), attn(case, other)
    assert np.array_equal(a[..., pc.HD :].view(np.uint32), b[..., pc.HD :].view(np.uint32))
    assert (a[..., : pc.HD] != b[..., : pc.HD]).any(axis=2).all()


@pytest.mark.parametrize("case", [c for c in pc.ATTN_CASES if c[0] > 1], ids=pc.attn_id)
def test_batch_equals_single_images(case):
    qkv = pc.attn_draw(case, "flat").qkv
    batch = attn_only(case, "flat")
    for i in range(case[0]):
        assert np.array_equal(attn(case, qkv[i : i + 1])[0].view(np.uint32), batch[i].view(np.uint32)), i


@pytest.mark.parametrize("case", [(1, 1, 257, 2), (2, 15, 20, 2), (1, 20, 20, 4)], ids=pc.attn_id)
def test_pe_equals_its_two_launches(case):
    """mtgv_op_psa_attn with pe = the attention-only call, then mtgv_op_dwconv3 with the arguments Detector::c2psa passes:
    input channel offset 64, g_size 64, g_stride 128, the attention as addend"""
    from mtgv.detector import dwconv3, psa_attn

    n, h, w, heads = case
    d = pc.attn_draw(case, "flat")
    Q, W, B = _dev(d.qkv), _dev(d.pe_w9), _dev(d.pe_bias)
    whole = psa_attn(Q, h, w, heads, W, B)
    att = psa_attn(Q, h, w, heads)
    assert np.array_equal(att.cpu().numpy().view(np.uint32), attn_only(case, "flat").view(np.uint32))
    composed = dwconv3(Q.view(n, h, w, heads * 128), W, B, x_co=64, g_size=64, g_stride=128, add=att.view(n, h, w, heads * 64))
    torch.cuda.synchronize()
    assert torch.equal(whole.view(torch.int32).view(n, h, w, -1), composed.view(torch.int32))
    assert not torch.equal(whole, att)


# ---------------------------------------------------------------------------
# depthwise 3x3
# ---------------------------------------------------------------------------
def dw_input_values(case, d, rounded):
    """the input pixel [n h w][x_ct] as f32: the draw in the channels the kernel reads, NaN in every other one.  rounded:
    every value replaced by float32(unpack(pack(value))), what an SP8 input of the same draw holds"""
    px = case.n * case.h * case.w
    vals = np.full((px, pc.x_ct_of(case)), np.nan, np.float32)
    idx = pc.cin(case)
    vals[:, idx] = d.full.reshape(px, -1)[:, idx]
    return sp.unpack(sp.pack(vals)).astype(np.float32) if rounded else vals


def dw_run(case, d, x_fmt, out_fmt, rounded=False):
    """one mtgv_op_dwconv3 launch: (values the kernel read [n h w][x_ct] fp64, output values fp64, output words)"""
    from mtgv import native as nv

    n, h, w, c = case[:4]
    px, x_ct, out_ct = n * h * w, pc.x_ct_of(case), pc.out_ct_of(case)
    x = Buf(px, x_ct, 0, x_ct, x_fmt, guard=w + 2, canary=True)  # (the canary is a NaN in both formats)
    read = x.set(dw_input_values(case, d, rounded))
    x.upload()
    out = Buf(px, out_ct, case.out_co, c, out_fmt, guard=8, canary=True).upload()
    keep = [_dev(d.w9), _dev(d.bias), _dev(d.add) if case.add else None]
    a = nv.Dwconv3()
    a.x, a.n, a.h, a.w, a.x_ct, a.x_co, a.x_fmt = x.ptr, n, h, w, x_ct, case.x_co, x_fmt
    a.c, a.g_size, a.g_stride = c, case.g_size, case.g_stride
    a.w9, a.bias, a.act = keep[0].data_ptr(), keep[1].data_ptr(), case.act
    if case.add:
        a.add, a.add_ld = keep[2].data_ptr(), c
    a.out, a.out_ct, a.out_co, a.out_fmt = out.ptr, out_ct, case.out_co, out_fmt
    rc = _status(nv.lib().mtgv_op_dwconv3(C.byref(a), nv.stream()), "mtgv_op_dwconv3")
    assert rc == 0, nv.lib().mtgv_last_error().decode()
    vals, words = out.read()  # nothing outside the output channels changed, everything inside written and finite
    return read, vals, words


@functools.lru_cache(maxsize=None)
def dw_f32(index, rounded):
    """the f32 -> f32 run of DW_CASES[index] on the draw (or on its SP8 rounding), held to fp64: (output f32 [n h w][c], error, bound)"""
    case, d = pc.DW_CASES[index], pc.dw_draw(index)
    read, vals, words = dw_run(case, d, F32, F32, rounded)
    ref, bound, err32 = pc.dw_expected_of(case, d, read.reshape(case.n, case.h, case.w, -1)) if rounded else pc.dw_expected(index)
    err = float(np.abs(vals - ref.reshape(vals.shape)).max())
    print(f"dwconv3 {pc.dw_id(case)} f32 -> f32{' on SP8-rounded input' if rounded else ''}: kernel {err:.2e}, float32 torch {err32:.2e}, "
          f"bound {bound:.2e} (max |ref| {np.abs(ref).max():.1f})")
    out = words.view(np.float32).copy()
    out.setflags(write=False)
    return out, err, bound


@pytest.mark.parametrize("x_fmt,out_fmt", pc.FORMAT_PAIRS, ids=["f32-f32", "f32-sp8", "sp8-f32", "sp8-sp8"])
@pytest.mark.parametrize("index", range(len(pc.DW_CASES)), ids=[pc.dw_id(c) for c in pc.DW_CASES])
def test_dwconv3_against_float64(index, x_fmt, out_fmt):
    case, d = pc.DW_CASES[index], pc.dw_draw(index)
    base, err, bound = dw_f32(index, rounded=x_fmt == SP8)
    assert err <= bound, (err, bound)
    if (x_fmt, out_fmt) == (F32, F32):
        return
    read, vals, words = dw_run(case, d, x_fmt, out_fmt)
    if x_fmt == SP8:  # the kernel read what the rounded f32 run was given
        idx = pc.cin(case)
        assert np.array_equal(read[:, idx], dw_input_values(case, d, True)[:, idx].astype(np.float64))
    want = sp.pack(base) if out_fmt == SP8 else base
    assert np.array_equal(words, want.view(np.uint32)), int((words != want.view(np.uint32)).sum())


def test_dwconv3_f32_views_at_multiples_of_four():
    """x_co = out_co = 4: the f32 instantiation's own alignment unit (an SP8 side needs 8), through mtgv.detector.dwconv3"""
    from mtgv.detector import dwconv3

    case = pc.DW_CASE_QUADS
    d = pc.dw_draw_of(case, pc.DW_QUADS_SEED)
    ref, bound, err32 = pc.dw_expected_of(case, d)
    n, h, w, c = case[:4]
    x = _dev(dw_input_values(case, d, False).reshape(n, h, w, -1))
    out = torch.full((n, h, w, case.out_ct), float("nan"), device="cuda")
    dwconv3(x, _dev(d.w9), _dev(d.bias), x_co=case.x_co, g_size=case.g_size, g_stride=case.g_stride, act=case.act, add=_dev(d.add), out=out,
            out_co=case.out_co)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    inside = got[..., case.out_co : case.out_co + c]
    err = float(np.abs(inside.astype(np.float64) - ref).max())
    print(f"dwconv3 {pc.dw_id(case)} at x_co = out_co = 4: kernel {err:.2e}, float32 torch {err32:.2e}, bound {bound:.2e}")
    assert np.isfinite(inside).all() and err <= bound
    rest = got.view(np.uint32).copy()
    rest[..., case.out_co : case.out_co + c] = NAN_WORD
    assert (rest == NAN_WORD).all()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("what", [r[0] for r in pc.ATTN_REFUSALS])
def test_attention_refusals(what):
    from mtgv import native as nv

    base = pc.ATTN_REFUSAL_BASE
    rng = np.random.default_rng(11493)
    n, h, w, heads = (base[k] for k in ("n", "h", "w", "heads"))
    t = dict(qkv=_dev(rng.standard_normal((n, h * w, heads * 128 + 4)).astype(np.float32)),  # (+ 4: room behind a moved pointer)
             pe_w9=_dev(rng.standard_normal((9, heads * 64 + 4)).astype(np.float32)), pe_bias=_dev(rng.standard_normal(heads * 64 + 4).astype(np.float32)),
             out=torch.full((n, h * w, heads * 64 + 4), float("nan"), device="cuda"))
    a = pc.refusal_args(base, dict(pc.ATTN_REFUSALS)[what], {k: v.data_ptr() for k, v in t.items()})
    L = nv.lib()
    rc = _status(L.mtgv_op_psa_attn(a["qkv"], a["pe_w9"], a["pe_bias"], a["n"], a["h"], a["w"], a["heads"], a["out"], nv.stream()), "mtgv_op_psa_attn")
    msg = L.mtgv_last_error().decode()
    print(f"psa_attn refusal, {what}: status {rc}, '{msg}'")
    assert rc == 1 and "psa_attn" in msg, (what, rc, msg)
    assert torch.isnan(t["out"]).all(), what


def test_attention_refusal_base_runs():
    from mtgv import native as nv

    base = pc.ATTN_REFUSAL_BASE
    n, h, w, heads = (base[k] for k in ("n", "h", "w", "heads"))
    qkv, out = torch.randn((n, h * w, heads * 128), device="cuda"), torch.full((n, h * w, heads * 64), float("nan"), device="cuda")
    W, B = torch.randn((9, heads * 64), device="cuda"), torch.randn(heads * 64, device="cuda")
    assert _status(nv.lib().mtgv_op_psa_attn(nv.ptr(qkv), nv.ptr(W), nv.ptr(B), n, h, w, heads, nv.ptr(out), nv.stream()), "mtgv_op_psa_attn") == 0
    assert torch.isfinite(out).all()


def _dw_refusal_call(change):
    """the base call of DW_REFUSALS with `change`: (status, message, the NaN-prefilled output [pixels][out_ct])"""
    from mtgv import native as nv

    base = pc.DW_REFUSAL_BASE
    rng = np.random.default_rng(11494)
    px = base["n"] * base["h"] * base["w"]
    sizes = dict(x=px * base["x_ct"], w9=9 * base["c"], bias=base["c"], add=px * base["add_ld"])
    t = {k: _dev(rng.standard_normal(v + 4).astype(np.float32)) for k, v in sizes.items()}  # (+ 4: room behind a moved pointer)
    t["out"] = torch.full((px * base["out_ct"] + 4,), float("nan"), device="cuda")
    a = pc.refusal_args(base, change, {k: v.data_ptr() for k, v in t.items()})
    d = nv.Dwconv3()
    for k, _ in nv.Dwconv3._fields_:
        setattr(d, k, a[k])
    rc = _status(nv.lib().mtgv_op_dwconv3(C.byref(d), nv.stream()), "mtgv_op_dwconv3")
    return rc, nv.lib().mtgv_last_error().decode(), t["out"]


@pytest.mark.parametrize("what", [r[0] for r in pc.DW_REFUSALS])
def test_dwconv3_refusals(what):
    rc, msg, out = _dw_refusal_call(dict(pc.DW_REFUSALS)[what])
    print(f"dwconv3 refusal, {what}: status {rc}, '{msg}'")
    assert rc == 1 and "dwconv3" in msg, (what, rc, msg)
    assert torch.isnan(out).all(), what


def test_dwconv3_refusal_base_runs():
    """the call every refusal is one change of is itself taken, and so is an f32 view at a multiple of 4"""
    for change in ({}, dict(x_co=4, out_co=4)):
        rc, msg, out = _dw_refusal_call(change)
        assert rc == 0, msg
        assert torch.isnan(out[-4:]).all()
        out = out[:-4].view(-1, pc.DW_REFUSAL_BASE["out_ct"])
        co = change.get("out_co", 0)
        assert torch.isfinite(out[:, co : co + 32]).all() and torch.isnan(out[:, co + 32 :]).all() and torch.isnan(out[:, :co]).all()
