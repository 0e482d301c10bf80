"""Detector scales s and m on the GPU (mtgv_detector_cfg.scale, spec.detector_scale_config) through the C ABI, against
oracle/detector_ref.py: forward parity, the stem kernels alone, NMS / masks / end to end, scale n unchanged, errors.

Cases and how they were chosen: tests/scales_common.py (tests/test_scales_cpu.py checks on the CPU that they leave the GPU
two thirds of its tolerance).  Shapes are small - 64 x 96 at batch 3 of 4 (P5 is 2 x 3, nothing is a multiple of a tile) and
160 x 224 (P3 = 560 rows, no multiple of the GEMM's 128-row tile) - because what changes with the scale is channel counts:
every layer width, the head's slices, the chained launches' predicates, the attention's head count."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest
import torch

import scales_common as S
import sp8_util
from oracle import detector_ref as D
from oracle import obb_ref

pytestmark = pytest.mark.gpu


def _with_mode(mode, fn):
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision(mode)
    try:
        return fn()
    finally:
        native.set_gemm_precision(before)


@functools.lru_cache(maxsize=None)
def _detector(arch, scale, task, hw, n, **kw):
    """the handle of a case, built with no argument beyond the state dict and the input rectangle: the scale comes from
    the weights (spec.detector_config_for_state)"""
    from mtgv import spec
    from mtgv.detector import Detector

    cfg, sd, _ = S.inputs(arch, scale, task, hw, n, **kw)
    found = spec.detector_config_for_state(sd, input_hw=hw, iou=cfg.iou)
    assert found == cfg
    return Detector(found, sd, max_batch=n + 1 if n == 3 else n)


# ---------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------
def _check_forward(case, mode):
    """raw outputs against the float64 oracle: class scores, coefficients / angle and prototypes within 1e-4 (the project's
    figure, BASELINE.json), box coordinates within max(in_h, in_w) * 1e-4 px"""
    cfg, _, frames = S.inputs(*case)
    _, ref_pred, ref_protos = S.reference(*case)
    det = _detector(*case)
    n = len(frames)

    def run():
        det.forward(torch.from_numpy(frames).cuda(), True, 0)
        return det.raw_outputs(n)

    pred, protos = _with_mode(mode, run)
    assert tuple(pred.shape) == (n, cfg.no, cfg.num_anchors)
    pred = pred.cpu().numpy().astype(np.float64)
    nc = cfg.nc
    box_err = np.abs(pred[:, :4] - ref_pred[:, :4]).max()
    cls_err = np.abs(pred[:, 4 : 4 + nc] - ref_pred[:, 4 : 4 + nc]).max()
    rest_err = np.abs(pred[:, 4 + nc :] - ref_pred[:, 4 + nc :]).max()
    if cfg.task == "obb":
        assert protos is None
        proto_err = 0.0
    else:
        assert tuple(protos.shape) == (n, cfg.nm, cfg.in_h // 4, cfg.in_w // 4)
        proto_err = np.abs(protos.cpu().numpy().astype(np.float64) - ref_protos).max()
    print(f"{S.case_id(case)} {mode}: box {box_err:.2e}px cls {cls_err:.2e} coef/angle {rest_err:.2e} protos {proto_err:.2e}")
    assert np.isfinite(pred).all()
    assert cls_err < 1e-4 and rest_err < 1e-4 and proto_err < 1e-4
    assert box_err < max(cfg.in_h, cfg.in_w) * 1e-4


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("case", S.FORWARD_CASES, ids=S.case_id)
def test_forward_small(case, mode):
    _check_forward(case, mode)


@pytest.mark.parametrize("case", S.MID_CASES, ids=S.case_id)
def test_forward_mid(case):
    _check_forward(case, "f16x3")


def test_flops_grow_with_the_scale():
    """mtgv_detector_flops counts the scale's own layers.  ultralytics' published GFLOPs at 640 x 640 [external - recalled]:
    yolov8{n,s,m}-seg 12.6 / 42.6 / 110.2, yolo11{n,s,m}-seg 10.4 / 35.5 / 123.3 - ratios to n of 3.4 and 8.7, 3.4 and 11.9.
    Every layer's count scales with the pixel count alike, so the ratios hold at 64 x 96; the class branch (nc = 3 here, 80
    there) is a few per cent of a model: within 25 %."""
    from mtgv import spec
    from mtgv.detector import Detector

    for arch, rs, rm in (("v8", 42.6 / 12.6, 110.2 / 12.6), ("11", 35.5 / 10.4, 123.3 / 10.4)):
        cfg = spec.detector_scale_config(arch, "n", input_hw=S.SMALL_HW)
        fn = Detector(cfg, spec.random_detector_state(cfg, S.WEIGHT_SEED), max_batch=1).flops_per_frame()
        fs = _detector(arch, "s", "seg", S.SMALL_HW, S.SMALL_N).flops_per_frame()
        fm = _detector(arch, "m", "seg", S.SMALL_HW, S.SMALL_N).flops_per_frame()
        print(f"{arch}: flops per 64 x 96 frame n {fn:.4g} s {fs:.4g} ({fs / fn:.2f}x) m {fm:.4g} ({fm / fn:.2f}x)")
        assert 0.75 * rs < fs / fn < 1.25 * rs and 0.75 * rm < fm / fn < 1.25 * rm


# ---------------------------------------------------------------------------
# 2. the stem alone
# ---------------------------------------------------------------------------
def _stem(frames, w4, bias, cout, flip, sp8, wide):
    from mtgv import native as nv

    n, h, w, _ = frames.shape
    out = torch.full((n, h // 2, w // 2, cout), float("nan"), device="cuda")
    nv.check(nv.lib().mtgv_op_stem_u8(nv.ptr(frames), nv.ptr(w4), nv.ptr(bias), nv.ptr(out), n, h, w, cout, int(flip), int(sp8), int(wide), nv.stream()))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _stem_inputs(cout, hw):
    """frames (3, h, w, 3) uint8, weights [cout][3][3][4] with a zero 4th input channel, bias; and the float64 reference
    SiLU(conv(frames / 255)) for flip off and on, (3, h / 2, w / 2, cout)"""
    rng = np.random.default_rng(1000 * cout + hw[0] + hw[1])
    frames = rng.integers(0, 256, (3, hw[0], hw[1], 3), dtype=np.uint8)
    w = (rng.standard_normal((cout, 3, 3, 3)) * 0.4).astype(np.float32)  # [o][kh][kw][c]
    b = (rng.standard_normal(cout) * 0.2).astype(np.float32)
    w4 = np.zeros((cout, 3, 3, 4), np.float32)
    w4[..., :3] = w
    refs = {}
    for flip in (False, True):
        x = torch.from_numpy(np.ascontiguousarray(frames[..., ::-1] if flip else frames)).permute(0, 3, 1, 2).double() / 255.0
        y = torch.nn.functional.conv2d(x, torch.from_numpy(w).double().permute(0, 3, 1, 2), torch.from_numpy(b).double(), stride=2, padding=1)
        refs[flip] = torch.nn.functional.silu(y).permute(0, 2, 3, 1).numpy()
    return frames, w4, b, refs


@pytest.mark.parametrize("sp8", [False, True], ids=["f32", "sp8"])
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("hw", [(64, 96), (32, 8)], ids=["64x96", "32x8"])  # (32 x 8: one thread per output row of the n kernel)
@pytest.mark.parametrize("cout", [16, 32, 48, 64])
def test_stem_against_float64(cout, hw, flip, sp8):
    """Every output is a bias plus 27 FMAs of pixels in [0, 1] (each u / 255 rounded once) and SiLU: with S = max over outputs
    of |b| + sum |w|, the pre-activation is at most S and its float32 error at most (27 + 2) roundings of 2^-24 S, which
    SiLU's slope (below 1.1) carries through: 32 x 2^-24 S.  The fast SiLU itself (act.h: __expf and v_rcp_f32) is within
    1e-6 relative, its own figure.  SP8 output adds the split's 2^-22 |x| and the subnormal floor of its lo half, 2^-25
    (sp8.h)."""
    frames, w4, b, refs = _stem_inputs(cout, hw)
    out = _stem(torch.from_numpy(frames).cuda(), torch.from_numpy(w4).cuda(), torch.from_numpy(b).cuda(), cout, flip, sp8, False).cpu().numpy()
    got = sp8_util.unpack(out) if sp8 else out.astype(np.float64)
    s = float((np.abs(w4).sum((1, 2, 3)) + np.abs(b)).max())
    tol = 32 * 2.0**-24 * s + 1e-6 * s + ((2.0**-22 * s + 2.0**-25) if sp8 else 0.0)
    err = np.abs(got - refs[flip]).max()
    print(f"stem cout {cout} {hw} flip {flip} sp8 {sp8}: err {err:.2e} (tolerance {tol:.2e}, S = {s:.2f})")
    assert np.isfinite(got).all() and err < tol
    if hw == (64, 96):  # flip matters: the two references differ by far more than the tolerance
        assert np.abs(refs[True] - refs[False]).max() > 100 * tol


@pytest.mark.parametrize("sp8", [False, True], ids=["f32", "sp8"])
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("hw", [(64, 96), (32, 8)], ids=["64x96", "32x8"])
def test_wide_stem_at_16_channels_gives_scale_n_bits(hw, flip, sp8):
    """conv0_u8_wide_kernel<16> (two pixels per thread) against conv0_u8_kernel (four): the same bits in either format"""
    frames, w4, b, _ = _stem_inputs(16, hw)
    args = (torch.from_numpy(frames).cuda(), torch.from_numpy(w4).cuda(), torch.from_numpy(b).cuda(), 16, flip, sp8)
    narrow, wide = _stem(*args, False), _stem(*args, True)
    assert torch.equal(narrow.view(torch.int32), wide.view(torch.int32))


def test_stem_errors():
    from mtgv import native as nv

    frames, w4, b, _ = _stem_inputs(32, (32, 8))
    f, w, bb = torch.from_numpy(frames).cuda(), torch.from_numpy(w4).cuda(), torch.from_numpy(b).cuda()
    out = torch.empty((3, 16, 4, 32), device="cuda")
    for n, h, wd, cout in ((3, 32, 8, 24), (3, 32, 8, 80), (3, 31, 8, 32), (3, 32, 12, 32), (0, 32, 8, 32)):
        with pytest.raises(AssertionError, match="stem"):
            nv.check(nv.lib().mtgv_op_stem_u8(nv.ptr(f), nv.ptr(w), nv.ptr(bb), nv.ptr(out), n, h, wd, cout, 0, 0, 0, nv.stream()))


# ---------------------------------------------------------------------------
# 3. NMS, masks, end to end
# ---------------------------------------------------------------------------
def _e2e(key):
    case = (*key, S.SMALL_HW, S.SMALL_N)
    kw = S.E2E_CASES[key]
    cfg, _, frames = S.inputs(*case, **kw)
    ref_dets, _, _ = S.reference(*case, **kw, f32=True)
    return cfg, frames, _detector(*case, **kw), ref_dets


def _forward_np(det, frames, mask_rows=0):
    out = det.forward(torch.from_numpy(frames).cuda(), True, mask_rows)
    pred, protos = det.raw_outputs(len(frames))
    o = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
    return o, pred.cpu().numpy(), None if protos is None else protos.cpu().numpy()


@pytest.mark.parametrize("key", list(S.E2E_CASES), ids=lambda k: f"{k[0]}{k[1]}-{k[2]}")
def test_nms_and_end_to_end(key):
    """the rules of tests/test_gpu_rect.py: the NMS kernel is bit-exact on the predictions it was given; against the float32
    oracle at most one threshold flip per frame, order moves at most 1 + flips, confidences within 1e-4, k > 10"""
    cfg, frames, det, ref_dets = _e2e(key)
    o, pred, _ = _forward_np(det, frames)
    bkey = "rboxes" if cfg.task == "obb" else "boxes"
    for i in range(len(frames)):
        k = int(o["n_det"][i])
        if cfg.task == "obb":
            same_in = obb_ref.nms_rotated_single(pred[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        else:
            same_in = D.nms_single(pred[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        assert k == len(same_in["keep_idx"])
        np.testing.assert_array_equal(o["keep_idx"][i, :k], same_in["keep_idx"])
        np.testing.assert_array_equal(o["cls"][i, :k], same_in["cls"])
        np.testing.assert_array_equal(o[bkey][i, :k], same_in[bkey])
        ref = ref_dets[i]
        got_idx, ref_idx = o["keep_idx"][i, :k], ref["keep_idx"]
        common = np.intersect1d(got_idx, ref_idx)
        flips = max(k, len(ref_idx)) - len(common)
        print(f"{key} frame {i}: kept {k} (reference {len(ref_idx)}), threshold flips {flips}")
        assert k > 10 and flips <= 1
        assert k < cfg.max_det and got_idx.max() < cfg.num_anchors
        gi = {a: j for j, a in enumerate(got_idx)}
        ri = {a: j for j, a in enumerate(ref_idx)}
        gsel = np.asarray([gi[a] for a in common])
        rsel = np.asarray([ri[a] for a in common])
        assert (np.diff(o["conf"][i, :k]) <= 0).all()
        assert np.abs(gsel - rsel).max() <= 1 + flips
        np.testing.assert_array_equal(o["cls"][i, :k][gsel], ref["cls"][rsel])
        assert np.abs(o["conf"][i, :k][gsel] - ref["conf"][rsel]).max() < 1e-4
        assert np.abs(o[bkey][i, :k][gsel][:, :4] - ref[bkey][rsel][:, :4]).max() < max(cfg.in_h, cfg.in_w) * 1e-4
        if cfg.task == "obb":
            assert np.abs(o[bkey][i, :k][gsel][:, 4] - ref[bkey][rsel][:, 4]).max() < 1e-4


@pytest.mark.parametrize("mask_rows", [16, 300])  # <= 16: mask_logits_kernel; above: the batched GEMM with the crop epilogue
def test_mask_logits_v8s(mask_rows):
    """the mask stage keeps its shapes at scale s (nm = 32 prototypes of npr = 128 channels): within 1e-4 of the oracle's masks,
    within 2e-5 of the oracle's mask_logits on the GPU's own pred and protos; rows beyond n_det are zeros"""
    cfg, frames, det, ref_dets = _e2e(("v8", "s", "seg"))
    o, pred, protos = _forward_np(det, frames, mask_rows)
    mh, mw = cfg.in_h // 4, cfg.in_w // 4
    assert o["mask_logits"].shape == (len(frames), mask_rows, mh, mw)
    for i in range(len(frames)):
        kk = min(int(o["n_det"][i]), mask_rows)
        same_in = D.nms_single(pred[i], cfg.nc, cfg.conf, cfg.iou, cfg.max_det, cfg.max_wh)
        first = {key: v[:kk] for key, v in same_in.items()}
        ml = o["mask_logits"][i, :kk]
        own_err = np.abs(ml - D.mask_logits(pred[i], protos[i], first, cfg.nc, (cfg.in_h, cfg.in_w))).max()
        ref = ref_dets[i]
        ri = {a: j for j, a in enumerate(ref["keep_idx"])}
        pairs = [(j, ri[a]) for j, a in enumerate(same_in["keep_idx"][:kk]) if a in ri]
        gsel, rsel = np.asarray([p[0] for p in pairs]), np.asarray([p[1] for p in pairs])
        ref_err = np.abs(ml[gsel] - ref["mask_logits"][rsel]).max()
        print(f"v8s mask_rows {mask_rows} frame {i}: {kk} masks, vs own pred {own_err:.2e}, vs reference {ref_err:.2e}")
        assert len(pairs) >= kk - 1 and kk > 10
        assert own_err < 2e-5 and ref_err < 1e-4
        assert (ml != 0).any() and (o["mask_logits"][i, kk:] == 0).all()


# ---------------------------------------------------------------------------
# 4. scale n is untouched
# ---------------------------------------------------------------------------
# Measured on the parent commit (b963448, before mtgv_detector_cfg had a scale) with this function's code on an MI355X:
# GEMM launches of one 640 x 640 frame, f16x3, fork off, and SHA-256 of `pred`'s bytes.  Weights random_detector_state seed
# 3, frame default_rng(640).
PARENT_N = {
    "v8": (54, "01b79b5622cb55f049d334d88cfa266da51328d47fda16f7e5442d5b86ae5d4e"),
    "11": (84, "d81dc7c71e3178237072f466e733006f8946abfda098ef0a3fa793c694fc0a92"),
}


def scale_n_fingerprint(arch):
    """(GEMM launches, SHA-256 of pred) of one forward of the scale-n detector"""
    from mtgv import native, spec
    from mtgv.detector import Detector

    cfg = spec.yolo11_config() if arch == "11" else spec.DetectorConfig()
    det = Detector(cfg, spec.random_detector_state(cfg, 3), max_batch=1)
    frames = torch.from_numpy(np.random.default_rng(640).integers(0, 256, (1, 640, 640, 3), dtype=np.uint8)).cuda()
    L = native.lib()
    det.set_fork(0)

    def run():
        native.check(L.mtgv_profile_gemm(1))
        try:
            det.forward(frames, True, 0)
            torch.cuda.synchronize()
            ms, fl, nl = C.c_double(), C.c_double(), C.c_int64()
            native.check(L.mtgv_profile_gemm_read(C.byref(ms), C.byref(fl), C.byref(nl)))
        finally:
            native.check(L.mtgv_profile_gemm(0))
        pred, _ = det.raw_outputs(1)
        return int(nl.value), hashlib.sha256(pred.cpu().numpy().tobytes()).hexdigest()

    return _with_mode("f16x3", run)


@pytest.mark.parametrize("arch", ["v8", "11"])
def test_scale_n_is_untouched(arch):
    launches, sha = scale_n_fingerprint(arch)
    print(f"{arch} n: {launches} GEMM launches, pred sha256 {sha}")
    assert (launches, sha) == PARENT_N[arch]


# The same for every (architecture, scale, task), measured on commit b6479f1 - the parent of the change that gave YOLOv8 and
# YOLO11 one CSP block, one neck, one head level and one arena table - with this function's code on an MI355X: GEMM launches of
# one forward of SMALL_N frames of SMALL_HW on a max_batch = 4 handle (f16x3, fork off), mtgv_detector_flops (compared as a
# double, exactly), SHA-256 of `pred`'s bytes and, on a segment handle, of `protos`'.  Weights and frames: scales_common.inputs.
PARENT_ALL = {
    ("v8", "n", "seg"): (60, 170138880.0, '8a8444ac49a683be978887b773bc184075499d68b27d650df9369a42e72f8c95',
                         '2d8ef0a395ccce2d6982d3c12b146f4fdca5ff395f15a79d0cb0b3c7039d6287'),
    ("v8", "n", "obb"): (55, 124938432.0, 'b27a6d0272bc98ebdd526119025df699fff4b7a57573ab827cd6b5dc8f749341',
                         None),
    ("v8", "s", "seg"): (62, 598792704.0, '3507bb69b7ef77debf2240ca0226e468ffa6b8e10347872da70420f12262e108',
                         '7643355e5acecc02c7f2cbae0262cc8e199b289a04356a0e24008284cda915bb'),
    ("v8", "s", "obb"): (58, 441256320.0, 'a5c049ca607a94266b802ca76442fb41badc1641cf761cddbe3581d77cbfb758',
                         None),
    ("v8", "m", "seg"): (85, 1564330752.0, '9ad56e4def622f6b6c7eadc3b2260e7253979d9527e1dbf992429d517165c91d',
                         'd77679b39351bbc5dff0a098839aad9fd6e0ece71e1c769e214b37ec9e4f3369'),
    ("v8", "m", "obb"): (81, 1212420672.0, '45cfc7710c7c6dac71a946b989b2e1b6e7999545f434c1ab6d765837f38096bd',
                         None),
    ("11", "n", "seg"): (84, 143569920.0, 'daada1b81319c471d9df7c4c02f5a091ab6dc0b009746717688b0c8a5d162452',
                         '01b020d220c267764ac575219131d0cea3001f9dac09b68d326ed01ac46bdec2'),
    ("11", "n", "obb"): (79, 98369472.0, 'c7fe6bb65b489eb2431310746707605856e04cd8b50853aec47cdb0371777004',
                         None),
    ("11", "s", "seg"): (83, 491784192.0, '16cd546259906f6c24d85f86fb49755c2d0b4fcc114f2143408e53a5947f1e90',
                         'a032caec62b4b0cfc5df1d97f08d6e7beac9d060300adf556eb31380922596a8'),
    ("11", "s", "obb"): (79, 334247808.0, '46e68edfef55c6f9bf3e3087b2a026ef6af8c61731bbbf4b4579460689716386',
                         None),
    ("11", "m", "seg"): (108, 1693433856.0, '7e76e1b0125661101213c422aaf11f36a72cf4c3b29f09e647769aa68d59e0d2',
                         'bf7f61530dc965cc45511665317fab0a8762bc9f93721ae295c82e87be166237'),
    ("11", "m", "obb"): (104, 1070079744.0, '7e3ca9b8f1c3ec57e83b0097db5cc03b0d3218cdc421ca433d114e7c49e24ad2',
                         None),
}


def small_fingerprint(arch, scale, task):
    """(GEMM launches, flops per frame, SHA-256 of pred, SHA-256 of protos or None) of one forward of the small case"""
    from mtgv import native

    case = (arch, scale, task, S.SMALL_HW, S.SMALL_N)
    _, _, frames = S.inputs(*case)
    det = _detector(*case)
    x = torch.from_numpy(frames).cuda()
    L = native.lib()
    det.set_fork(0)

    def run():
        native.check(L.mtgv_profile_gemm(1))
        try:
            det.forward(x, True, 0)
            torch.cuda.synchronize()
            nl = C.c_int64()
            native.check(L.mtgv_profile_gemm_read(None, None, C.byref(nl)))
        finally:
            native.check(L.mtgv_profile_gemm(0))
        pred, protos = det.raw_outputs(len(frames))
        sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
        return int(nl.value), det.flops_per_frame(), sha(pred), None if protos is None else sha(protos)

    try:
        return _with_mode("f16x3", run)
    finally:
        det.set_fork(-1)  # (the handle is shared with the other tests of this module)


@pytest.mark.parametrize("task", ["seg", "obb"])
@pytest.mark.parametrize("scale", ["n", "s", "m"])
@pytest.mark.parametrize("arch", ["v8", "11"])
def test_every_scale_runs_the_parents_launches(arch, scale, task):
    got = small_fingerprint(arch, scale, task)
    print(f'    ("{arch}", "{scale}", "{task}"): {got!r},')
    assert (got[3] is None) == (task == "obb")
    assert got == PARENT_ALL[(arch, scale, task)]


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------
def _create(scale, arch=8):
    from mtgv import native as nv

    c = nv.DetectorCfg()
    c.nc, c.imgsz, c.max_batch, c.conf, c.iou, c.max_det, c.arch, c.task = 3, 64, 1, 0.25, 0.7, 300, arch, 0
    c.scale = scale
    h = nv.c_vp(0)
    rc = nv.lib().mtgv_detector_create(C.byref(c), C.byref(h))
    msg = nv.lib().mtgv_last_error().decode()
    if h.value:
        nv.lib().mtgv_detector_destroy(h)
    return rc, msg


def test_scale_errors():
    from mtgv import spec
    from mtgv.detector import Detector

    for arch in (8, 11):
        for scale in (0, 1, 2):
            assert _create(scale, arch)[0] == 0
        for scale in (3, 4):  # l, x: known to spec and the oracle, refused by the library
            rc, msg = _create(scale, arch)
            assert rc == 2 and "n, s, m" in msg, (rc, msg)
        for scale in (-1, 5):
            assert _create(scale, arch)[0] == 1
    with pytest.raises(KeyError, match="n, s, m"):
        Detector(spec.detector_scale_config("v8", "l", input_hw=(64, 96)), None, max_batch=1)
    # an s state dict into an n handle: the first weight's element count
    cfg_s = spec.detector_scale_config("v8", "s", input_hw=(64, 96))
    sd = spec.random_detector_state(cfg_s, S.WEIGHT_SEED)
    det = Detector(spec.DetectorConfig(input_hw=(64, 96)), None, max_batch=1)
    from mtgv import native as nv

    a = np.ascontiguousarray(sd["model.0.conv.weight"])
    rc = nv.lib().mtgv_detector_set_param(det._h, b"model.0.conv.weight", a.ctypes.data_as(nv.c_vp), a.size)
    assert rc == 1 and "elements, expected" in nv.lib().mtgv_last_error().decode()
