"""MTGV_DET_HEAD_DIRECT (csrc/detector.hip): the segment head's class branch as one chained launch per level (its final
1x1 padded to a 32-column block of the head rows) and NMS straight from the head rows (the row form of nms_kernel,
csrc/nms.hip) instead of a decode pass over every anchor.  Neither changes a bit of any output, so =1 (the default) is
compared with =0 (the class 3x3 and 1x1 as two launches, decode_kernel, NMS on pred) in one process, in both schedules
of the forward's fork-join, at batch 3 and batch 1.

The detector is small (imgsz 224: maps 28 / 14 / 7, 1029 anchors).  It is built twice: at the default confidence
threshold, where random weights may leave a frame without detections, and at threshold 0, where every anchor is a
candidate and every frame must have detections - the comparison cannot pass on empty outputs there."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

IMGSZ, BATCH, MASK_ROWS = 224, 3, 8
KEYS = ("n_det", "boxes", "conf", "cls", "keep_idx", "mask_logits", "pred", "protos")


@pytest.fixture(scope="module", params=["v8", "11"])
def setup(request):
    from mtgv import spec
    from mtgv.detector import Detector

    dets = {}
    for name, conf in (("default", None), ("all", 0.0)):
        kw = {"imgsz": IMGSZ} if conf is None else {"imgsz": IMGSZ, "conf": conf}
        cfg = spec.yolo11_config(**kw) if request.param == "11" else spec.DetectorConfig(**kw)
        dets[name] = Detector(cfg, spec.random_detector_state(cfg, 7), max_batch=BATCH)
    frames = torch.randint(0, 256, (BATCH, IMGSZ, IMGSZ, 3), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda",
                           dtype=torch.uint8)
    return request.param, dets, frames


def _run(det, frames, direct, fork, mode="f16x3"):
    """one forward under the switch and schedule: its outputs, pred / protos of mtgv_detector_raw after it, and the
    launch profiler's count of GEMM launches"""
    from mtgv import native

    L = native.lib()
    before = native.get_gemm_precision()
    had = os.environ.get("MTGV_DET_HEAD_DIRECT")
    os.environ["MTGV_DET_HEAD_DIRECT"] = direct
    native.set_gemm_precision(mode)
    det.set_fork(fork)
    try:
        native.check(L.mtgv_profile_gemm(1))
        try:
            out = {k: v.clone() for k, v in det.forward(frames, True, MASK_ROWS).items()}
            torch.cuda.synchronize()
            ms, fl, nl = C.c_double(), C.c_double(), C.c_int64()
            native.check(L.mtgv_profile_gemm_read(C.byref(ms), C.byref(fl), C.byref(nl)))
        finally:
            native.check(L.mtgv_profile_gemm(0))
        out["launches"], out["flops"] = int(nl.value), float(fl.value)
        pred, protos = det.raw_outputs(frames.shape[0])
        out["pred"], out["protos"] = pred.clone(), protos.clone()
        torch.cuda.synchronize()
        return out
    finally:
        det.set_fork(-1)
        native.set_gemm_precision(before)
        if had is None:
            os.environ.pop("MTGV_DET_HEAD_DIRECT", None)
        else:
            os.environ["MTGV_DET_HEAD_DIRECT"] = had


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("thres", ["default", "all"])
@pytest.mark.parametrize("batch", [BATCH, 1])
def test_head_direct_is_bit_identical(setup, batch, thres):
    arch, dets, frames = setup
    det, fr = dets[thres], frames[:batch]
    for fork in (0, 1):
        base = _run(det, fr, "0", fork)
        got = _run(det, fr, "1", fork)
        print(f"{arch} batch {batch} {thres} fork {fork}: n_det {base['n_det'].tolist()} -> {got['n_det'].tolist()}, "
              f"GEMM launches {base['launches']} -> {got['launches']}")
        if thres == "all":
            # every anchor is a candidate: every frame has detections
            assert (base["pred"][:, 4:4 + det.cfg.nc].amax(1) > 0.0).all()
            assert (base["n_det"] > 0).all() and (got["n_det"] > 0).all()
        for k in KEYS:  # pred: mtgv_detector_raw after a direct forward decodes on demand
            assert torch.equal(_bits(got[k]), _bits(base[k])), (k, arch, batch, thres, fork)
        # YOLOv8: the class branch's 1x1 rides on its 3x3 at each of the three levels; YOLO11's class branch is untouched
        assert base["launches"] - got["launches"] == (3 if arch == "v8" else 0), (base["launches"], got["launches"])
        # and the launch profiler credits the same algorithmic FLOPs (the padded rows of the chained 1x1 are not counted)
        assert got["flops"] == base["flops"], (got["flops"], base["flops"])


def test_head_direct_f32_activations(setup):
    """f32 GEMM operands: nothing chains (the chain is an SP8 path), NMS still runs from the head rows"""
    arch, dets, frames = setup
    base = _run(dets["all"], frames, "0", 0, "f32")
    got = _run(dets["all"], frames, "1", 0, "f32")
    assert (got["n_det"] > 0).all() and got["launches"] == base["launches"]
    for k in KEYS:
        assert torch.equal(_bits(got[k]), _bits(base[k])), (k, arch)


def test_raw_after_decode_forward_then_direct_forward(setup):
    """pred of mtgv_detector_raw follows the last forward, whichever form it ran: a decode-path forward of other frames
    in between must not leave its pred behind"""
    arch, dets, frames = setup
    det = dets["all"]
    want = _run(det, frames, "0", 0)["pred"]
    other = _run(det, frames.flip(0), "0", 0)["pred"]
    assert not torch.equal(other, want)
    assert torch.equal(_bits(_run(det, frames, "1", 0)["pred"]), _bits(want))
