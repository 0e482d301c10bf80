"""NMS straight from the segment head's raw rows (mtgv_op_nms_raw: the row form of nms_kernel, csrc/nms.hip) against the
two passes it replaces on the same rows: mtgv_op_decode (decode_kernel: every anchor -> pred) and mtgv_nms on that pred.
Both forms take the class scores and the boxes from csrc/head_decode.h, so every output must be the same bits: n_det,
boxes, conf, cls, keep_idx, and the kept detections' coefficients (the pred form's are gathered from pred here).

Rows are synthetic: imgsz 224 (maps 28 / 14 / 7, 1029 anchors), 2 images, nc 3, nm 32, in the detector's row layout
(128 floats: box bins at 0, coefficients at 64, class logits at 96) and once in a 100-float layout with other offsets."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

IMGSZ, N, NC, NM = 224, 2, 3, 32
GRIDS = (28, 14, 7)
NA = sum(g * g for g in GRIDS)
LAYOUT = dict(ct=128, cls=96, coef=64)       # detector.h
LAYOUT_100 = dict(ct=100, cls=64, coef=68)   # class logits in front of the coefficients, rows that share cache lines
CONF, IOU, MAX_WH = 0.25, 0.7, 7680.0


def _fields(seed):
    """per-anchor fields (n, na, *) on the CPU: box logits (64), class logits (nc), coefficients (nm)"""
    g = torch.Generator().manual_seed(seed)
    return {
        "box": torch.randn((N, NA, 64), generator=g) * 2.0,
        "cls": torch.randn((N, NA, NC), generator=g) * 2.0 - 2.0,
        "coef": torch.randn((N, NA, NM), generator=g),
    }


def _peaked(f, bin_, sharp=12.0):
    """box logits with nearly all mass on one bin of each side: boxes 2 * bin_ strides wide around the anchor"""
    f["box"] = torch.randn_like(f["box"]) * 0.1
    f["box"].view(N, NA, 4, 16)[..., bin_] += sharp


def _case(name):
    if name in ("random", "random_layout100"):
        f = _fields(1)
        f["cls"] -= 3.0  # a few percent of the anchors are candidates, as in a real frame
        return f, 300
    if name == "ties":
        # the same best score at 60 anchors of every level (and at two classes of some): ordered by anchor
        f = _fields(2)
        f["cls"][:] = -6.0
        pick = torch.cat([torch.arange(5, 780, 20), torch.arange(790, 980, 19), torch.arange(985, 1029, 4)])
        f["cls"][:, pick, 1] = 1.25
        f["cls"][:, pick[::3], 2] = 1.25
        _peaked(f, 1)
        return f, 300
    if name == "none":
        f = _fields(3)
        f["cls"][:] = -8.0 + 0.1 * torch.randn_like(f["cls"])
        return f, 300
    if name == "all":
        f = _fields(4)
        f["cls"] = 2.0 + 0.3 * torch.randn_like(f["cls"])
        return f, 300
    if name == "max_det":
        # boxes one stride wide do not overlap their neighbours: hundreds survive, 20 are reported
        f = _fields(5)
        f["cls"] = 1.0 + torch.randn_like(f["cls"])
        _peaked(f, 0)
        f["box"].view(N, NA, 4, 16)[..., 1] += 12.0  # bins 0 and 1 equally: distance 0.5 on every side
        return f, 20
    if name == "class_offset":
        # boxes 16 strides wide at neighbouring P3 pixels overlap with IoU 240 / 272 = 0.88: two of different classes are
        # both kept (the class offset moves them apart), of two of the same class the second is suppressed
        f = _fields(6)
        f["cls"][:] = -8.0
        _peaked(f, 8)
        a, b = 10 * 28 + 9, 17 * 28 + 15
        f["cls"][:, a, 0], f["cls"][:, a + 1, 1] = 2.0, 1.9
        f["cls"][:, b, 2], f["cls"][:, b + 1, 2] = 1.8, 1.7
        return f, 300
    raise KeyError(name)


def _rows(fields, lay):
    """the three levels' row tensors (n, g * g, ct) on the GPU, NaN wherever the layout holds no field"""
    out, a0 = [], 0
    for g in GRIDS:
        r = torch.full((N, g * g, lay["ct"]), float("nan"))
        sl = slice(a0, a0 + g * g)
        r[..., :64] = fields["box"][:, sl]
        r[..., lay["cls"]:lay["cls"] + NC] = fields["cls"][:, sl]
        r[..., lay["coef"]:lay["coef"] + NM] = fields["coef"][:, sl]
        out.append(r.cuda().contiguous())
        a0 += g * g
    return out


def _run(fields, lay, max_det):
    from mtgv import native as nv
    from mtgv.detector import nms

    L = nv.lib()
    rows = _rows(fields, lay)
    hr = nv.HeadRows(rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), IMGSZ, lay["ct"], lay["cls"], lay["coef"])
    pred = torch.empty((N, 4 + NC + NM, NA), dtype=torch.float32, device="cuda")
    nv.check(L.mtgv_op_decode(C.byref(hr), N, NC, NM, nv.ptr(pred), nv.stream()))
    ref = nms(pred, NC, CONF, IOU, max_det, MAX_WH)
    ws = torch.empty((int(L.mtgv_nms_workspace_bytes(N, NA)) + 3) // 4, dtype=torch.int32, device="cuda")
    # outputs start as garbage: the kernel writes every slot
    got = {
        "n_det": torch.full((N,), -7, dtype=torch.int32, device="cuda"),
        "boxes": torch.full((N, max_det, 4), float("nan"), device="cuda"),
        "conf": torch.full((N, max_det), float("nan"), device="cuda"),
        "cls": torch.full((N, max_det), -7, dtype=torch.int32, device="cuda"),
        "keep_idx": torch.full((N, max_det), -7, dtype=torch.int32, device="cuda"),
    }
    coef = torch.full((N, max_det, NM), float("nan"), device="cuda")
    nv.check(L.mtgv_op_nms_raw(C.byref(hr), N, NC, NM, CONF, IOU, max_det, MAX_WH, nv.ptr(got["n_det"]), nv.ptr(got["boxes"]),
                               nv.ptr(got["conf"]), nv.ptr(got["cls"]), nv.ptr(got["keep_idx"]), nv.ptr(coef), nv.ptr(ws), ws.numel() * 4,
                               nv.stream()))
    torch.cuda.synchronize()
    # the pred form's coefficients: pred's coefficient rows at the kept anchors, zeros beyond n_det
    ref_coef = torch.zeros_like(coef)
    for i in range(N):
        k = int(ref["n_det"][i])
        ref_coef[i, :k] = pred[i, 4 + NC:, ref["keep_idx"][i, :k].long()].T
    return ref, ref_coef, got, coef, pred


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


CASES = ["random", "random_layout100", "ties", "none", "all", "max_det", "class_offset"]


@pytest.mark.parametrize("name", CASES)
def test_nms_raw_equals_decode_then_nms(name):
    fields, max_det = _case(name)
    ref, ref_coef, got, coef, pred = _run(fields, LAYOUT_100 if name == "random_layout100" else LAYOUT, max_det)
    n_det = ref["n_det"].tolist()
    scores = pred[:, 4:4 + NC].amax(1)
    cand = (scores > CONF).sum(1).tolist()
    print(f"{name}: candidates {cand} n_det {n_det} (raw form {got['n_det'].tolist()})")
    # the case is what its name says (judged on the pred form, the reference)
    if name == "none":
        assert cand == [0, 0] and n_det == [0, 0]
    elif name == "all":
        assert cand == [NA, NA] and min(n_det) > 0
    elif name == "max_det":
        assert n_det == [max_det, max_det] and min(cand) > 4 * max_det
    elif name == "class_offset":
        assert cand == [4, 4] and n_det == [3, 3]
        assert ref["keep_idx"][0, :3].tolist() == [10 * 28 + 9, 10 * 28 + 10, 17 * 28 + 15]
    elif name == "ties":
        k = ref["keep_idx"][0, :n_det[0]].tolist()
        assert min(n_det) >= 30 and k == sorted(k), "equal scores must come out in anchor order"
    else:
        assert min(n_det) > 0 and max(n_det) < max_det
    for key in ("n_det", "boxes", "conf", "cls", "keep_idx"):
        assert torch.equal(_bits(got[key]), _bits(ref[key])), f"{name}: {key} differs between the row form and decode -> nms"
    assert torch.equal(_bits(coef), _bits(ref_coef)), f"{name}: coefficients differ"
