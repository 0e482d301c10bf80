"""ORACLE for the OBB detector family (test infrastructure, never shipped or measured as the product).

CPU restatement of what the OBB tests check the GPU against beside the network itself: ProbIoU, the rotated NMS rule and
this project's card-orientation rule.  The OBB head and its decode sit with the segment head in oracle/detector_ref.py.

[external - recalled] PARITY UNPINNED: head, decode (`dist2rbox`), ProbIoU (`batch_probiou`) and the rotated NMS rule
(`non_max_suppression(rotated=True)` -> `nms_rotated`) are ultralytics 8.3.x's as recalled; the package is absent and the
reference (mtgvision/od_train.py:19, :101 builds `yolo..-obb.yaml` by default; od_datasets.py:244-257 labels card /
card_top / card_bottom) holds no OBB inference code, so the issue that introduced this file is the specification.  The
card rule is this project's own: the reference leaves it "to compute later".

`probiou`, `nms_rotated_single` and `obb_cards` take a `dtype`: float32 is, operation for operation, what the HIP kernels
compute (probiou.h, nms.hip, obb_cards.hip); float64 evaluates the same formulas on the same float32 inputs and is the
yardstick for both.
"""

from __future__ import annotations

import numpy as np

EPS = 1e-7


# ---------------------------------------------------------------------------
# ProbIoU
# ---------------------------------------------------------------------------
def cov(w, h, theta, dtype=np.float32):
    """(a, b, c) of boxes with sides w, h and angle theta: the covariance [[a, c], [c, b]]"""
    f = dtype
    w, h, theta = (np.asarray(v).astype(f) for v in (w, h, theta))
    A, B = w * w / f(12), h * h / f(12)
    cs, sn = np.cos(theta), np.sin(theta)
    cs2, sn2 = cs * cs, sn * sn
    return A * cs2 + B * sn2, A * sn2 + B * cs2, (A - B) * cs * sn


def probiou_cov(x1, y1, a1, b1, c1, x2, y2, a2, b2, c2, dtype=np.float32):
    f = dtype
    eps = f(EPS)
    sa, sb, sc = a1 + a2, b1 + b2, c1 + c2
    D_ = sa * sb - sc * sc
    dy, dx = y1 - y2, x1 - x2
    t1 = (sa * (dy * dy) + sb * (dx * dx)) / (D_ + eps) * f(0.25)
    t2 = (sc * (x2 - x1) * dy) / (D_ + eps) * f(0.5)
    d1 = np.maximum(a1 * b1 - c1 * c1, f(0))
    d2 = np.maximum(a2 * b2 - c2 * c2, f(0))
    t3 = f(0.5) * np.log(D_ / (f(4) * np.sqrt(d1 * d2) + eps) + eps)
    bd = np.minimum(np.maximum(t1 + t2 + t3, eps), f(100))
    hd = np.sqrt(f(1) - np.exp(-bd) + eps)
    return f(1) - hd


def probiou(a, b, dtype=np.float32):
    """ProbIoU of the box pairs a[i], b[i] ((m, 5) x, y, w, h, angle), evaluated in `dtype` on the inputs as given"""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    a1, b1, c1 = cov(a[:, 2], a[:, 3], a[:, 4], dtype)
    a2, b2, c2 = cov(b[:, 2], b[:, 3], b[:, 4], dtype)
    with np.errstate(all="ignore"):
        return probiou_cov(a[:, 0], a[:, 1], a1, b1, c1, b[:, 0], b[:, 1], a2, b2, c2, dtype)


# ---------------------------------------------------------------------------
# rotated NMS
# ---------------------------------------------------------------------------
def _candidates(pred, nc, conf_thres):
    cls_scores = pred[4 : 4 + nc]
    conf = cls_scores.max(0)
    cls = cls_scores.argmax(0).astype(np.int32)  # first maximum on ties
    cand = np.nonzero(conf > np.float32(conf_thres))[0]
    order = cand[np.lexsort((cand, -conf[cand]))]  # score descending, anchor ascending
    return conf, cls, order


def pair_matrix(pred, nc, conf_thres=0.25, max_wh=7680.0, dtype=np.float32, block=512):
    """yields (j0, M) with M[i, j - j0] = probiou(candidate i, candidate j) of the sorted, class-offset candidates"""
    pred = np.asarray(pred, np.float32)
    conf, cls, order = _candidates(pred, nc, conf_thres)
    f = dtype
    off = cls[order].astype(np.float32) * np.float32(max_wh)
    x, y = (pred[0, order] + off).astype(f), (pred[1, order] + off).astype(f)  # the offset add is float32 in either case
    a, b, c = cov(pred[2, order], pred[3, order], pred[4 + nc, order], f)
    n = len(order)
    with np.errstate(all="ignore"):
        for j0 in range(0, n, block):
            s = slice(j0, min(n, j0 + block))
            yield j0, probiou_cov(x[:, None], y[:, None], a[:, None], b[:, None], c[:, None], x[None, s], y[None, s], a[None, s], b[None, s],
                                  c[None, s], f)


def nms_rotated_single(pred, nc, conf_thres=0.25, iou_thres=0.7, max_det=300, max_wh=7680.0):
    """pred (4 + nc + 1, A) float32 of one image -> dict(keep_idx, rboxes (k, 5), conf, cls), score-descending.

    NOT the greedy sweep: candidate j is kept iff no candidate i < j (score order) has probiou(i, j) >= iou, whether or
    not i was itself dropped.  float32, operation for operation what nms_rotated_kernel does."""
    pred = np.asarray(pred, np.float32)
    conf, cls, order = _candidates(pred, nc, conf_thres)
    n = len(order)
    keep = np.ones(n, bool)
    thr = np.float32(iou_thres)
    for j0, M in pair_matrix(pred, nc, conf_thres, max_wh):
        i = np.arange(n)[:, None]
        j = j0 + np.arange(M.shape[1])[None, :]
        keep[j0 : j0 + M.shape[1]] = ~((M >= thr) & (i < j)).any(0)
    k = order[keep][:max_det]
    return {
        "keep_idx": k.astype(np.int32),
        "rboxes": np.stack([pred[0, k], pred[1, k], pred[2, k], pred[3, k], pred[4 + nc, k]], 1).astype(np.float32).reshape(-1, 5),
        "conf": conf[k],
        "cls": cls[k],
    }


def nms_greedy_single(pred, nc, conf_thres=0.25, iou_thres=0.7, max_wh=7680.0):
    """what a greedy sweep with the same measure would keep (only a dropped-by-a-KEPT-box test): for the test that
    tells the two rules apart"""
    pred = np.asarray(pred, np.float32)
    _, _, order = _candidates(pred, nc, conf_thres)
    n = len(order)
    M = np.zeros((n, n), np.float32)
    for j0, blk in pair_matrix(pred, nc, conf_thres, max_wh):
        M[:, j0 : j0 + blk.shape[1]] = blk
    kept = []
    for j in range(n):
        if not any(M[i, j] >= np.float32(iou_thres) for i in kept):
            kept.append(j)
    return order[kept].astype(np.int32)


# ---------------------------------------------------------------------------
# card rule (this project's)
# ---------------------------------------------------------------------------
def _inside_first(rb, cls, nd, want, cx, cy, ux, uy, vx, vy, hw, hh):
    """d.u of the first detection of class `want` whose centre lies inside the card, or None"""
    if want < 0:
        return None
    for t in range(nd):
        if cls[t] != want:
            continue
        dx, dy = rb[t, 0] - cx, rb[t, 1] - cy
        dv, du = dx * vx + dy * vy, dx * ux + dy * uy
        if abs(dv) <= hw and abs(du) <= hh:
            return du
    return None


def obb_cards(n_det, rboxes, conf, cls, pad_boxes, k, card_cls=0, top_cls=1, bottom_cls=2, dtype=np.float32):
    """(F,), (F, md, 5), (F, md), (F, md), (k, 4) -> quads (F*k, 4, 2), sel_boxes (F*k, 4), frame_idx, state, as
    mtgv_obb_cards; every operation in `dtype` on the inputs as given"""
    f = dtype
    F, md = rboxes.shape[0], rboxes.shape[1]
    quads = np.zeros((F * k, 4, 2), f)
    sel = np.zeros((F * k, 4), f)
    fidx = np.zeros(F * k, np.int32)
    state = np.zeros(F * k, np.int32)
    half_pi = f(np.float32(np.pi / 2))  # the kernel's float32 constant in either evaluation
    for i in range(F * k):
        fr, slot = divmod(i, k)
        fidx[i] = fr
        nd = min(max(int(n_det[fr]), 0), md)
        rb, cl = rboxes[fr].astype(f), cls[fr]
        idx = [t for t in range(nd) if cl[t] == card_cls]
        if slot >= len(idx):
            x1, y1, x2, y2 = pad_boxes[slot].astype(f)
            quads[i] = [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]
            sel[i] = [x1, y1, x2, y2]
            continue
        t = idx[slot]
        cx, cy, w, h, th = rb[t]
        if w > h:
            w, h = h, w
            th = th + half_pi
        cs, sn = np.cos(th), np.sin(th)
        ux, uy, vx, vy = -sn, cs, cs, sn
        hw, hh = w * f(0.5), h * f(0.5)
        st = 2
        du = _inside_first(rb, cl, nd, top_cls, cx, cy, ux, uy, vx, vy, hw, hh)
        if du is not None and du != 0:
            sg = f(1) if du > 0 else f(-1)
        else:
            du = _inside_first(rb, cl, nd, bottom_cls, cx, cy, ux, uy, vx, vy, hw, hh)
            if du is not None and du != 0:
                sg = f(-1) if du > 0 else f(1)
            else:
                sg = f(1) if (uy < 0 or (uy == 0 and ux < 0)) else f(-1)
                st = 1
        Ux, Uy = sg * ux, sg * uy
        Rx, Ry = -Uy, Ux
        ax, ay, bx, by = Ux * hh, Uy * hh, Rx * hw, Ry * hw
        q = np.array([[cx + ax - bx, cy + ay - by], [cx + ax + bx, cy + ay + by], [cx - ax + bx, cy - ay + by], [cx - ax - bx, cy - ay - by]], f)
        quads[i] = q
        sel[i] = [q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()]
        state[i] = st
    return quads, sel, fidx, state
