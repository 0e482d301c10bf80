"""SPPF's three chained 5x5 max pools at a map small enough to look at every case of the window: imgsz 224 gives a 7x7
map at stride 32, where every border clip of the 5x5 window (0, 1 or 2 rows / columns cut on either side) and exactly
one unclipped centre pixel occur.  On SP8 activations (f16x3) the pools run as one launch (sppf_pools_sp8_kernel) or,
with MTGV_SPPF_POOLS1=0, as three (maxpool5_sp8_kernel); both scan the window with the same sp8_max5x5
(csrc/detector_kernel.h).  On f32 activations rowops' maxpool5_kernel runs.

The test cannot tell which pool kernel ran: it sees the network's outputs only.  The equality of the two forms is what
guards the shared scan; the oracle bound (the project's 1e-4, boxes in pixels: imgsz * 1e-4) says that both are right."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMGSZ, BATCH = 224, 2


@pytest.fixture(scope="module", params=["v8", "11"])
def setup(request):
    from mtgv import spec
    from mtgv.detector import Detector
    from oracle import detector_ref as D

    cfg = spec.yolo11_config(imgsz=IMGSZ) if request.param == "11" else spec.DetectorConfig(imgsz=IMGSZ)
    sd = spec.random_detector_state(cfg, 7)
    frames = np.random.default_rng(8).integers(0, 256, (BATCH, IMGSZ, IMGSZ, 3), dtype=np.uint8)
    ref_pred, ref_protos = (np.asarray(a) for a in D.forward(sd, cfg, frames))
    return cfg, Detector(cfg, sd, max_batch=BATCH), torch.from_numpy(frames).cuda(), ref_pred, ref_protos


def _raw(det, frames, mode, pools1):
    """(pred, protos) of one forward in GEMM operand mode `mode`; pools1: None leaves MTGV_SPPF_POOLS1 unset"""
    from mtgv import native

    before = native.get_gemm_precision()
    had = os.environ.pop("MTGV_SPPF_POOLS1", None)
    native.set_gemm_precision(mode)
    try:
        if pools1 is not None:
            os.environ["MTGV_SPPF_POOLS1"] = pools1
        det.forward(frames, True, 0)
        return tuple(t.clone() for t in det.raw_outputs(BATCH))
    finally:
        native.set_gemm_precision(before)
        os.environ.pop("MTGV_SPPF_POOLS1", None)
        if had is not None:
            os.environ["MTGV_SPPF_POOLS1"] = had


def _check_oracle(cfg, pred, protos, ref_pred, ref_protos, what):
    pred, protos = pred.cpu().numpy(), protos.cpu().numpy()
    box_err = np.abs(pred[:, :4] - ref_pred[:, :4]).max()
    rest_err = np.abs(pred[:, 4:] - ref_pred[:, 4:]).max()
    proto_err = np.abs(protos - ref_protos).max()
    print(f"{what}: box {box_err:.2e}px cls/coef {rest_err:.2e} protos {proto_err:.2e}")
    assert box_err < cfg.imgsz * 1e-4 and rest_err < 1e-4 and proto_err < 1e-4, what


def test_sp8_pools_one_launch_equals_three(setup):
    cfg, det, frames, ref_pred, ref_protos = setup
    pred1, protos1 = _raw(det, frames, "f16x3", None)
    pred3, protos3 = _raw(det, frames, "f16x3", "0")
    assert torch.equal(pred1, pred3) and torch.equal(protos1, protos3)
    _check_oracle(cfg, pred1, protos1, ref_pred, ref_protos, f"{cfg.arch} f16x3 pools in one launch")
    _check_oracle(cfg, pred3, protos3, ref_pred, ref_protos, f"{cfg.arch} f16x3 pools in three launches")


def test_f32_pools(setup):
    cfg, det, frames, ref_pred, ref_protos = setup
    pred, protos = _raw(det, frames, "f32", None)
    _check_oracle(cfg, pred, protos, ref_pred, ref_protos, f"{cfg.arch} f32")
