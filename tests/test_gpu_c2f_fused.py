"""The fused C2f tail (c2f_tail_kernel.h: a block's last bottleneck and its closing 1x1 conv as one launch, the
bottleneck's intermediates in LDS) computes the bits of the three launches it replaces."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("pred", "protos", "n_det", "keep_idx", "boxes", "conf", "cls", "mask_logits")


# YOLOv8n-seg at 640: C2f-2 (160 x 160), C2f-4 and C2f-15 (80 x 80) each trade three launches for one
FUSED_BLOCKS = 3


def _run(det, frames, fuse, fork=None):
    """One forward under the switch; besides the outputs, the launch profiler's count and algorithmic FLOPs of it."""
    import ctypes as C

    from mtgv import native

    L = native.lib()
    saved = {k: os.environ.get(k) for k in ("MTGV_DET_C2F_FUSE", "MTGV_DET_FORK")}
    os.environ["MTGV_DET_C2F_FUSE"] = fuse
    if fork is not None:
        os.environ["MTGV_DET_FORK"] = fork
    try:
        n = frames.shape[0]
        native.check(L.mtgv_profile_gemm(1))
        try:
            out = {k: (v.clone() if v is not None else None) for k, v in det.forward(frames, True, 8).items()}
            torch.cuda.synchronize()
            ms, fl, nl = C.c_double(), C.c_double(), C.c_int64()
            native.check(L.mtgv_profile_gemm_read(C.byref(ms), C.byref(fl), C.byref(nl)))
        finally:
            native.check(L.mtgv_profile_gemm(0))
        out["launches"], out["flops"] = int(nl.value), float(fl.value)
        pred, protos = det.raw_outputs(n)
        out["pred"], out["protos"] = pred.clone(), protos.clone()
        torch.cuda.synchronize()
        return out
    finally:
        for k, v in saved.items():  # what the caller had set stays set
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("batch", [32, 3])
def test_c2f_fused_tail_is_bit_identical_to_its_three_launches(batch):
    """YOLOv8n-seg on random frames (every pixel of every frame border is non-zero, and so are the activations there: the
    tiles on all four borders zero the out-of-frame pixels of the first conv's output), MTGV_DET_C2F_FUSE=1 against =0 in
    one process, with the other switches at their defaults and with the serial schedule: every output, every bit."""
    from mtgv import spec
    from mtgv.detector import Detector

    cfg = spec.DetectorConfig()
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=32)
    g = torch.Generator(device="cuda").manual_seed(11 + batch)
    frames = torch.randint(0, 256, (batch, 640, 640, 3), generator=g, device="cuda", dtype=torch.uint8)
    for edge in (frames[:, 0], frames[:, -1], frames[:, :, 0], frames[:, :, -1]):
        assert (edge.float().sum(-1) > 0).float().mean().item() > 0.99
    for fork in (None, "0"):
        base = _run(det, frames, "0", fork)
        assert (base["n_det"] > 0).any()
        got = _run(det, frames, "1", fork)
        # the fused kernels really ran: one launch where there were three, in each of the three blocks, and the launch
        # profiler credits them with the same algorithmic FLOPs
        assert base["launches"] - got["launches"] == 2 * FUSED_BLOCKS, (base["launches"], got["launches"])
        assert got["flops"] == base["flops"], (got["flops"], base["flops"])
        for k in KEYS:
            assert torch.equal(got[k], base[k]), (k, fork, batch)


def test_c2f_fused_tail_batch1_equals_its_frame_of_batch32():
    from mtgv import spec
    from mtgv.detector import Detector

    cfg = spec.DetectorConfig()
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=32)
    g = torch.Generator(device="cuda").manual_seed(7)
    frames = torch.randint(0, 256, (32, 640, 640, 3), generator=g, device="cuda", dtype=torch.uint8)
    full = _run(det, frames, "1")
    assert _run(det, frames, "0")["launches"] - full["launches"] == 2 * FUSED_BLOCKS
    for i in (0, 17, 31):
        one = _run(det, frames[i : i + 1], "1")
        assert _run(det, frames[i : i + 1], "0")["launches"] - one["launches"] == 2 * FUSED_BLOCKS
        n = int(one["n_det"][0])
        assert n > 0 and n == int(full["n_det"][i])
        for k in ("pred", "protos"):
            assert torch.equal(one[k][0], full[k][i]), (k, i)
        for k in ("keep_idx", "boxes", "conf", "cls"):  # rows of the frame's detections (the rest is padding)
            assert torch.equal(one[k][0, :n], full[k][i, :n]), (k, i)
        assert torch.equal(one["mask_logits"][0, : min(n, 8)], full["mask_logits"][i, : min(n, 8)]), i
