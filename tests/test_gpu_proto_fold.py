"""Proto's ConvTranspose2d(k2, s2, bias) folded into the 3x3 conv behind it: four 2x2 phase convs over the low-resolution
map with cv3 chained (gemm_sp_kernel.h, EPI 96), through mtgv_op_proto_tail - the function Detector::proto runs behind cv1.

Single op, 64 -> 64 -> 64 -> 32 channels, inputs scaled as in test_gpu_sp8_conv.py (input N(0,1), weights N(0,1) / sqrt(K),
biases N(0,1)):
  - the SP8 input sits at channels 16.. of a wider pixel, every other byte of the allocation (w + 2 pixels either side
    included) an fp16 NaN; the f32 output at channels 16.. of a wider pixel in an allocation prefilled with a NaN
    pattern that must survive outside the output channels;
  - reference: the unfolded definition in fp64 (conv_transpose2d -> conv2d(padding=1) -> SiLU -> 1x1 -> SiLU) on the
    unpacked SP8 input values and the exact f32 weights;
  - bound: 3e-5 absolute, the one test_gpu_sp8_conv.py holds a chained launch to at this scaling, with the fold on and off;
  - fold off is bit-identical to the three mtgv_op_conv2d_ex launches it consists of.
Detector level (imgsz 64, batch 3, both families): prototypes within 1e-4 of the CPU oracle with MTGV_PROTO_FOLD on and
off, the raw head bit-identical between the two, the launch count says which form ran and the profiler's algorithmic
FLOPs are the same.
Each case prints its errors (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_sp8_conv import F32, NONE, SILU, SP8, TOL, Buf, conv_ex, output, weights

pytestmark = pytest.mark.gpu

CH, NM = 64, 32
CASES = [
    (1, 1, 1),    # all four borders in one low-resolution pixel
    (3, 5, 7),    # 105 rows: one ragged tile spanning the images
    (5, 9, 11),   # 495 rows: several tiles, a ragged tail, tiles that straddle images and rows
    (2, 80, 80),  # the 640 x 640 forward's grid
]


@pytest.fixture(autouse=True)
def _f16x3():
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision("f16x3")
    yield
    native.set_gemm_precision(before)


class TailCase:
    def __init__(self, n, h, w):
        rng = np.random.default_rng(1000 + n * 100 + h)
        self.n, self.h, self.w = n, h, w
        self.x = Buf(n * h * w, CH + 32, 16, CH, SP8, guard=w + 2)
        xv = self.x.set(rng.standard_normal((n * h * w, CH)).astype(np.float32))
        self.x.upload()
        self.wt = (rng.standard_normal((CH, CH, 2, 2)) / np.sqrt(CH)).astype(np.float32)  # ConvTranspose2d layout (in, out, kh, kw)
        self.bt = rng.standard_normal(CH).astype(np.float32)
        self.w2, self.b2 = weights(rng, CH, 3, CH)
        w3, self.b3 = weights(rng, NM, 1, CH)
        self.w3 = np.ascontiguousarray(w3.reshape(NM, CH))
        d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
        y = F.conv_transpose2d(d(xv.reshape(n, h, w, CH)).permute(0, 3, 1, 2), d(self.wt), d(self.bt), stride=2)
        y = F.silu(F.conv2d(y, d(self.w2).permute(0, 3, 1, 2), d(self.b2), padding=1))
        y = F.silu(F.conv2d(y, d(self.w3)[:, :, None, None], d(self.b3)))
        self.ref = y.permute(0, 2, 3, 1).reshape(-1, NM).numpy()

    def out(self):
        return output(self.n * 4 * self.h * self.w, NM, F32, NM + 24, 16)

    def tail(self, fold):
        """(folded?, values, words) of one mtgv_op_proto_tail call"""
        from mtgv import native as nv

        o = self.out()
        keep = [np.ascontiguousarray(a) for a in (self.wt, self.bt, self.w2, self.b2, self.w3, self.b3)]
        d = nv.ProtoTail()
        d.pr1, d.n, d.h, d.w, d.pr1_ct, d.pr1_co, d.c = self.x.ptr, self.n, self.h, self.w, self.x.ct, self.x.co, CH
        d.wt, d.bt, d.w2, d.b2, d.w3, d.b3 = (a.ctypes.data for a in keep)
        d.nm, d.protos, d.protos_ct, d.protos_co, d.fold = NM, o.ptr, o.ct, o.co, int(fold)
        ran = C.c_int32(-1)
        nv.check(nv.lib().mtgv_op_proto_tail(C.byref(d), C.byref(ran), nv.stream()))
        torch.cuda.synchronize()
        return (ran.value, *o.read())

    def three_launches(self):
        """ConvTranspose (one scattered launch), cv2, cv3 as mtgv_op_conv2d_ex launches with SP8 intermediates"""
        n, h, w = self.n, self.h, self.w
        px = n * 4 * h * w
        w_all = np.ascontiguousarray(self.wt.transpose(2, 3, 1, 0).reshape(4 * CH, 1, 1, CH))  # rows (kh, kw, cout)
        pr2, pr3, o = output(px, CH, SP8), output(px, CH, SP8), self.out()
        conv_ex(self.x, n, h, w, w_all, np.tile(self.bt, 4), 1, 0, NONE, pr2, os_=2, os_nq=CH)
        pr2.read()
        conv_ex(pr2, n, 2 * h, 2 * w, self.w2, self.b2, 1, 1, SILU, pr3)
        pr3.read()
        conv_ex(pr3, n, 2 * h, 2 * w, self.w3.reshape(NM, 1, 1, CH), self.b3, 1, 0, SILU, o)
        return o.read()


@pytest.mark.parametrize("n,h,w", CASES)
def test_proto_tail(n, h, w):
    c = TailCase(n, h, w)
    ran_on, v_on, _ = c.tail(True)
    ran_off, v_off, bits_off = c.tail(False)
    e_on, e_off = float(np.abs(v_on - c.ref).max()), float(np.abs(v_off - c.ref).max())
    print(f"proto tail {(n, h, w)}: max_err folded={e_on:.3g} unfolded={e_off:.3g}" + ("  (folded > unfolded)" if e_on > e_off else ""))
    assert (ran_on, ran_off) == (1, 0)
    assert e_on < TOL and e_off < TOL, (e_on, e_off)
    _, bits3 = c.three_launches()
    assert (bits_off == bits3).all()


def _launches(det, frames, n):
    """(pred, protos, GEMM launches, algorithmic FLOPs the launch profiler credits) of one forward"""
    from mtgv import native as nv

    L = nv.lib()
    nv.check(L.mtgv_profile_gemm(1))
    try:
        det.forward(frames, True, 0)
        torch.cuda.synchronize()
        cnt, fl = C.c_int64(0), C.c_double(0)
        nv.check(L.mtgv_profile_gemm_read(None, C.byref(fl), C.byref(cnt)))
    finally:
        nv.check(L.mtgv_profile_gemm(0))
    pred, protos = (t.clone() for t in det.raw_outputs(n))
    return pred, protos, cnt.value, fl.value


@pytest.mark.parametrize("arch", ["v8", "11"])
def test_detector_fold_on_and_off(arch):
    from mtgv import spec
    from mtgv.detector import Detector
    from oracle import detector_ref as D

    cfg = spec.yolo11_config(imgsz=64) if arch == "11" else spec.DetectorConfig(imgsz=64)
    sd = spec.random_detector_state(cfg, 5)
    frames = np.random.default_rng(6).integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)
    _, ref_protos = D.forward(sd, cfg, frames)
    ref_protos = np.asarray(ref_protos)
    det = Detector(cfg, sd, max_batch=4)
    dev = torch.from_numpy(frames).cuda()
    had = os.environ.pop("MTGV_PROTO_FOLD", None)
    try:
        pred_on, protos_on, n_on, fl_on = _launches(det, dev, 3)
        os.environ["MTGV_PROTO_FOLD"] = "0"
        pred_off, protos_off, n_off, fl_off = _launches(det, dev, 3)
    finally:
        os.environ.pop("MTGV_PROTO_FOLD", None)
        if had is not None:
            os.environ["MTGV_PROTO_FOLD"] = had
    e_on = float(np.abs(protos_on.cpu().numpy() - ref_protos).max())
    e_off = float(np.abs(protos_off.cpu().numpy() - ref_protos).max())
    print(f"detector {arch} imgsz 64: protos max_err folded={e_on:.3g} unfolded={e_off:.3g}; GEMM launches {n_on} / {n_off}")
    assert n_on - n_off == 2  # four phase launches instead of ConvTranspose + (cv2, cv3 chained)
    assert fl_on == fl_off  # ... credited with the algorithmic FLOPs of the layers they replace
    assert e_on < 1e-4 and e_off < 1e-4
    assert torch.equal(pred_on, pred_off)
    assert not torch.equal(protos_on, protos_off)  # another rounding, not the same launches twice
