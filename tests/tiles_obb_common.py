"""Shared by test_tiles_obb_cpu.py and test_gpu_tiles_obb.py: the cases of the rotated tile merge as plain numpy tables (what
mtgv.tiles.merge_tiles_obb_host and mtgv_tiles_merge_obb both read), the quad pairs of the pair function, and a float64
evaluation of both written on its own (plain polygon clipping in Python floats).  No GPU needed here."""
import functools
import math

import numpy as np

import tiles_common as tc
from mtgv.tiles import merge_tiles_obb_host, tile_grid

OUTPUTS = ("sel_boxes_src", "quads_src", "frame_idx", "sel_conf", "src_slot", "n_sel", "state", "oriented_by")
WINDOW, OVERLAP, BIG = tc.WINDOW, tc.OVERLAP, tc.BIG
CARD, TOP, BOTTOM = 0, 1, 2


def rq(cx, cy, w, h, th):
    """an upright-assumed card quad TL, TR, BR, BL (float64) of centre, short side w, long side h and angle th"""
    u = np.array([-math.sin(th), math.cos(th)])
    U = -u if u[1] > 0 else u
    R = np.array([-U[1], U[0]])
    c = np.array([cx, cy], np.float64)
    return np.array([c + U * h / 2 - R * w / 2, c + U * h / 2 + R * w / 2, c - U * h / 2 + R * w / 2, c - U * h / 2 - R * w / 2])


# ---------------------------------------------------------------------------
# float64, on its own: Sutherland-Hodgman clipping in Python floats
# ---------------------------------------------------------------------------
def area2_f64(poly):
    """the doubled signed area of a polygon, in Python floats"""
    poly = [(float(x), float(y)) for x, y in poly]
    return sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly)))


def inter_f64(a, b):
    """the area of intersection of two convex quads: b clipped by a's edges"""
    a, b = [(float(x), float(y)) for x, y in a], [(float(x), float(y)) for x, y in b]
    sa = area2_f64(a)
    if sa == 0 or area2_f64(b) == 0:
        return 0.0
    if sa < 0:
        a = a[::-1]
    poly = b
    for e in range(4):
        (ax, ay), (bx, by) = a[e], a[(e + 1) % 4]
        side = [(bx - ax) * (y - ay) - (by - ay) * (x - ax) for x, y in poly]
        out = []
        for i, p in enumerate(poly):
            q, dp, dq = poly[(i + 1) % len(poly)], side[i], side[(i + 1) % len(poly)]
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if len(poly) < 3:
            return 0.0
    return abs(area2_f64(poly)) / 2


def card_pairs(n, seed=0):
    """n card-like pairs: sides 60-90 x 100-140 px, any angle, centres within 80 px, anywhere in 3840 x 2160 -> (n, 4, 2) x 2"""
    rng = np.random.default_rng(seed)
    a, b = np.zeros((n, 4, 2), np.float32), np.zeros((n, 4, 2), np.float32)
    for i in range(n):
        cx, cy = rng.uniform(0, 3840), rng.uniform(0, 2160)
        a[i] = rq(cx, cy, rng.uniform(60, 90), rng.uniform(100, 140), rng.uniform(-np.pi, np.pi))
        b[i] = rq(cx + rng.uniform(-80, 80), cy + rng.uniform(-80, 80), rng.uniform(60, 90), rng.uniform(100, 140), rng.uniform(-np.pi, np.pi))
    return a, b


_SQ = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float64)
ANALYTIC = {  # name -> (a, b, area of the intersection), integer coordinates
    "identical": (_SQ, _SQ, 100),
    "half_shift_x": (_SQ, _SQ + [5, 0], 50),
    "half_shift_y": (_SQ, _SQ + [0, 5], 50),
    "quarter": (_SQ, _SQ + [5, 5], 25),
    "disjoint": (_SQ, _SQ + [20, 0], 0),
    "shared_edge": (_SQ, _SQ + [10, 0], 0),
    "shared_edge_part": (_SQ, _SQ + [10, 4], 0),
    "shared_corner": (_SQ, _SQ + [10, 10], 0),
    "inside": (_SQ, _SQ * 0.4 + [2, 3], 16),
    "inside_swapped": (_SQ * 0.4 + [2, 3], _SQ, 16),
    "inside_touching": (_SQ, _SQ * 0.5, 25),
    "diamond": (_SQ, np.array([[5, 0], [10, 5], [5, 10], [0, 5]], np.float64), 50),
    "diamond_swapped": (np.array([[5, 0], [10, 5], [5, 10], [0, 5]], np.float64), _SQ, 50),
    "zero_area": (_SQ, np.array([[2, 2], [8, 8], [8, 8], [2, 2]], np.float64), 0),
    "zero_area_swapped": (np.array([[2, 2], [8, 8], [8, 8], [2, 2]], np.float64), _SQ, 0),
}


def analytic_pairs():
    """every ANALYTIC case with both windings of either quad, every starting corner of a, at the origin and offset by
    (3000, 2000) -> [(name, a, b, want)]"""
    out = []
    for name, (a, b, want) in sorted(ANALYTIC.items()):
        for ra in (False, True):
            for rb in (False, True):
                for roll in range(4):
                    for off in ((0, 0), (3000, 2000)):
                        qa = np.roll(a[::-1] if ra else a, roll, 0) + off
                        qb = (b[::-1] if rb else b) + off
                        out.append((f"{name} ra={ra} rb={rb} roll={roll} off={off}", qa.astype(np.float32), qb.astype(np.float32), np.float32(want)))
    return out


# ---------------------------------------------------------------------------
# merge cases
# ---------------------------------------------------------------------------
def to_tile(tab, t, quad):
    """camera-pixel corners -> float32 pixels of tile t's detector input (exact where the ratio is 1 and the numbers are small)"""
    _, y0, x0, _, _ = (int(v) for v in tab["tiles"][t])
    _, _, top, left = (int(v) for v in tab["geo"][t])
    q = np.array(quad, np.float64).reshape(4, 2)
    return np.stack([(q[:, 0] - x0) * tab["ratio"][t] + left, (q[:, 1] - y0) * tab["ratio"][t] + top], 1).astype(np.float32)


def case(tab, dets, kt, k, max_det=8, edge=2.0, ios=0.5, markers=(), n_det=None, state=None, max_tiles_per_frame=None, card_cls=CARD):
    """dets: [(global tile, quad TL TR BR BL in camera pixels, conf, state), ...]; markers: [(tile, conf, cls), ...], detections of
    another class with no quad.  Every tile's detections are put in score-descending order like an NMS output; its j-th card
    detection fills slot j < kt (quads, state), as crop.obb_cards does.  n_det: {tile: count} and state: {slot: value} override."""
    NT = tab["tiles"].shape[0]
    conf, cls, nd = np.zeros((NT, max_det), np.float32), np.zeros((NT, max_det), np.int32), np.zeros((NT,), np.int32)
    quads, st = np.zeros((NT * kt, 4, 2), np.float32), np.zeros((NT * kt,), np.int32)
    per = {}
    for t, q, c, s in dets:
        per.setdefault(t, []).append((np.float32(c), card_cls, to_tile(tab, t, q), s))
    for t, c, cl in markers:
        per.setdefault(t, []).append((np.float32(c), cl, None, 0))
    for t, lst in per.items():
        lst.sort(key=lambda e: -float(e[0]))  # (stable: equal scores keep their order)
        assert len(lst) <= max_det
        j = 0
        for d, (c, cl, q, s) in enumerate(lst):
            conf[t, d], cls[t, d] = c, cl
            if q is not None:
                if j < kt:
                    quads[t * kt + j], st[t * kt + j] = q, s
                j += 1
        nd[t] = len(lst)
    for t, n in (n_det or {}).items():
        nd[t] = n
    for slot, s in (state or {}).items():
        st[slot] = s
    return dict(tab, n_det=nd, conf=conf, cls=cls, quads=quads, state=st, kt=kt, k=k, edge=edge, ios=ios, pad_frac=tc.pad_frac(k), card_cls=card_cls,
                max_tiles_per_frame=max_tiles_per_frame)


def host(c):
    return merge_tiles_obb_host(c["n_det"], c["conf"], c["cls"], c["quads"], c["state"], c["tiles"], c["geo"], c["ratio"], c["tile_start"], c["hw"],
                                c["pad_frac"], c["kt"], c["k"], c["edge"], c["ios"], c["card_cls"], c["max_tiles_per_frame"])


def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


UP = np.array([(20, 10), (60, 10), (60, 70), (20, 70)], np.float64)  # an upright card TL, TR, BR, BL
DOWN, SIDE = UP[[2, 3, 0, 1]], UP[[1, 2, 3, 0]]  # the same corners upside down, and turned by a quarter (u perpendicular)
STRIP_A = np.array([(10, 90), (70, 30), (77, 37), (17, 97)], np.float64)  # a thin card at 45 degrees, area 840
STRIP_B = STRIP_A + [10, 10]  # beside it: disjoint, while the bounding boxes overlap by 57 x 57 of 67 x 67


@functools.lru_cache(maxsize=None)
def designed():
    """name -> case.  The 300 x 500 frame has 12 windows, tile t = 4 * row + column; tile 0 is x 0..160, y 0..128, tile 1 is
    x 128..288, tile 4 is y 96..224, tile 5 both.  `three` is one 128 x 160 frame seen by three whole windows (no inner side)."""
    big, one = tc.tables([BIG]), tc.tables([WINDOW])
    full = tc.tables([BIG], with_full=True)  # tile 12 is the whole frame, ratio 0.32
    three = tc.tables([WINDOW], tiles=[[(0, 0, 128, 160)] * 3])
    two = tc.tables([(200, 400), (100, 120)], tiles=[list(tile_grid(200, 400, WINDOW, OVERLAP)) + [(0, 0, 200, 400)], [(0, 0, 100, 120)]])
    small = [(140, 20), (148, 28), (142, 34), (134, 26)]  # inside tiles 0 and 1, more than `edge` from their inner sides
    corner = [(140, 102), (148, 110), (142, 116), (134, 108)]  # inside tiles 0, 1, 4 and 5
    whole = [(100, 30), (220, 40), (215, 110), (95, 100)]
    frag = [(105, 45), (150, 48), (148, 95), (103, 92)]  # inside `whole`, and inside tile 0 away from its inner sides
    wide = [(130, 25), (208, 10), (286, 25), (208, 40)]  # tile 1 is x 128..288: exactly `edge` from both inner sides
    return {
        "side_by_side_45": case(one, [(0, STRIP_A, 0.9, 1), (0, STRIP_B, 0.8, 1)], 4, 4),
        "overlap_two": case(big, [(0, small, 0.8, 1), (1, small, 0.9, 1)], 4, 4),
        "corner_four": case(big, [(0, corner, 0.5, 1), (1, corner, 0.6, 1), (4, corner, 0.95, 2), (5, corner, 0.7, 1)], 4, 4),
        "equal_conf": case(big, [(1, small, 0.75, 1), (0, small, 0.75, 1)], 4, 4),
        "fragment_low": case(full, [(12, whole, 0.9, 1), (0, frag, 0.6, 1)], 4, 4),
        "fragment_high": case(full, [(12, whole, 0.6, 1), (0, frag, 0.9, 1)], 4, 4),
        # the same quad of the tile's own pixels: at the frame's left side in tile 0, at an inner side in tile 1
        "inner_and_frame_side": case(big, [(0, [(0, 25), (10, 10), (20, 25), (10, 40)], 0.9, 1), (1, [(128, 25), (138, 10), (148, 25), (138, 40)], 0.9, 1)], 4, 4),
        "exactly_edge": case(big, [(1, wide, 0.9, 1)], 4, 4),
        "edge_left_strict": case(big, [(1, [(129.75, 25)] + wide[1:], 0.9, 1)], 4, 4),
        "edge_right_strict": case(big, [(1, wide[:2] + [(286.25, 25)] + wide[3:], 0.9, 1)], 4, 4),
        # inter = 32 * 64 = 0.5 * 4096 exactly: both kept; 32.25 * 64 is over: the second is dropped
        "ios_equal": case(one, [(0, _sq(0, 0, 64, 64), 0.9, 1), (0, _sq(32, 0, 96, 64), 0.8, 1), (0, _sq(0, 64, 64, 128), 0.7, 1),
                                (0, _sq(31.75, 64, 95.75, 128), 0.6, 1)], 8, 8),
        "orient_flip": case(three, [(0, UP, 0.9, 1), (1, DOWN, 0.8, 2)], 4, 4),
        "orient_agree": case(three, [(0, UP, 0.9, 1), (1, UP + [1, 0], 0.8, 2)], 4, 4),
        "orient_two_donors": case(three, [(0, UP, 0.9, 1), (1, UP, 0.7, 2), (2, DOWN, 0.8, 2)], 4, 4),
        "orient_kept_oriented": case(three, [(0, UP, 0.9, 2), (1, DOWN, 0.8, 2)], 4, 4),
        "orient_perpendicular": case(three, [(0, UP, 0.9, 1), (1, SIDE, 0.8, 2)], 4, 4),
        # an unoriented duplicate between the kept one and the donor, and a marker in front of every card
        "orient_behind_unoriented": case(three, [(0, UP, 0.9, 1), (1, UP, 0.85, 1), (2, DOWN, 0.8, 2)], 4, 4,
                                         markers=[(0, 0.95, TOP), (1, 0.99, BOTTOM), (2, 0.5, TOP)]),
        # tile 1 detects markers only; its slot 0 claims state 1 all the same: no candidate
        "markers_only": case(three, [(0, UP, 0.9, 1)], 4, 4, markers=[(1, 0.8, TOP), (1, 0.7, BOTTOM)], state={1 * 4: 1}),
        "n_det_over_max_det": case(three, [(0, _sq(4 + 20 * i, 8, 20 + 20 * i, 40), 0.9 - 0.1 * i, 1) for i in range(6)], 4, 8, n_det={0: 99}),
        "n_det_negative": case(three, [(0, UP, 0.9, 1), (1, UP + [70, 0], 0.8, 1)], 4, 4, n_det={1: -3}),
        "state_three": case(three, [(0, UP, 0.9, 1), (0, UP + [70, 0], 0.8, 1)], 4, 4, state={1: 3}),
        "more_than_k": case(one, [(0, _sq(4 + 12 * i, 8, 14 + 12 * i, 40), 0.3 + 0.05 * i, 1 + i % 2) for i in range(12)], 16, 8, max_det=16),
        "none": case(big, [], 4, 8),
        "two_frames": case(two, [(0, _sq(20, 20, 40, 50), 0.9, 1), (6, rq(30, 35, 20, 30, 0.02), 0.8, 2), (1, small, 0.7, 2), (0, small, 0.6, 1),
                                 (7, rq(40, 50, 30, 50, 0.7), 0.5, 1), (7, rq(90, 50, 20, 36, -0.4), 0.4, 2)], 4, 4,
                           markers=[(6, 0.85, TOP), (7, 0.9, BOTTOM), (7, 0.45, TOP)]),
    }


def random_case(seed, kt, k, max_det=64):
    """up to 4 frames of mixed sizes, 1 to 16 tiles each (some with the full-frame window): small cards at any angle, seen -
    with up to a pixel of jitter per corner - by every tile that holds their centre; a card that reaches over a window's side
    is clipped by the mapping and falls to the cut rule at an inner side.  Markers of the other classes are mixed in, states
    1 / 2 and upright / upside down at random, confidences all distinct."""
    rng = np.random.default_rng(seed)
    frames_hw, grids = [], []
    while len(frames_hw) < 4:
        h, w = int(rng.integers(60, 400)), int(rng.integers(60, 600))
        g = tile_grid(h, w, WINDOW, OVERLAP, bool(rng.integers(0, 2)))
        if len(g) <= 16:
            frames_hw.append((h, w)), grids.append(g)
    tab = tc.tables(frames_hw, tiles=grids)
    dets, markers = [], []
    for f, (h, w) in enumerate(frames_hw):
        for _ in range(int(rng.integers(1, 30 if kt > 8 else 10))):
            q = rq(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(8, 14), rng.uniform(14, 22), rng.uniform(-np.pi, np.pi))
            for t in range(int(tab["tile_start"][f]), int(tab["tile_start"][f + 1])):
                _, y0, x0, wh, ww = (int(v) for v in tab["tiles"][t])
                cx, cy = q.mean(0)
                if not (x0 <= cx <= x0 + ww and y0 <= cy <= y0 + wh) or rng.random() < 0.15:
                    continue
                seen = q + rng.uniform(-1, 1, (4, 2)) / max(tab["ratio"][t], 0.25)
                st = 1 + int(rng.integers(0, 2))
                if st == 2 and rng.random() < 0.5:
                    seen = seen[[2, 3, 0, 1]]
                dets.append((t, seen, 0.0, st))
                if rng.random() < 0.4:
                    markers.append((t, 0.0, int(rng.integers(1, 3))))
    confs = (0.3 + 0.6 * (rng.permutation(len(dets) + len(markers)) + 0.5) / max(1, len(dets) + len(markers))).astype(np.float32)
    assert len(set(confs.tolist())) == len(confs)
    dets = [(t, q, confs[i], s) for i, (t, q, _, s) in enumerate(dets)]
    markers = [(t, confs[len(dets) + i], cl) for i, (t, _, cl) in enumerate(markers)]
    per_tile = np.bincount([d[0] for d in dets] + [m[0] for m in markers], minlength=1)
    assert per_tile.max() <= max_det, per_tile.max()
    return case(tab, dets, kt, k, max_det=max_det, markers=markers)


RANDOM = [(11, 1, 4), (12, 8, 8), (13, 64, 64), (14, 8, 1), (15, 64, 16), (16, 1, 64)]  # (seed, kt, k): the margins hold for these (test_tiles_obb_cpu)


def cap_case():
    """one frame at the cap: 16 whole windows of 64 card detections, 1024 disjoint 4 x 3 diamonds on a 32 x 32 grid - every
    candidate survives the cut rule and the suppression; 64 are kept"""
    tab = tc.tables([WINDOW], tiles=[[(0, 0, 128, 160)] * 16])
    rng = np.random.default_rng(5)
    levels = np.linspace(0.3, 0.9, 16).astype(np.float32)
    dets = []
    for i, cell in enumerate(rng.permutation(1024)):
        gy, gx = divmod(int(cell), 32)
        x, y = gx * 5, gy * 4
        dets.append((i // 64, [(x + 2, y), (x + 4, y + 1.5), (x + 2, y + 3), (x, y + 1.5)], levels[int(rng.integers(0, 16))], 1 + i % 2))
    return case(tab, dets, 64, 64, max_det=64)


def nan_case():
    """a NaN and an inf corner among ordinary candidates (three whole windows)"""
    c = designed()["orient_two_donors"]
    c = dict(c, quads=c["quads"].copy(), conf=c["conf"].copy(), cls=c["cls"].copy(), state=c["state"].copy(), n_det=c["n_det"].copy())
    kt = c["kt"]
    for t, bad in ((0, np.nan), (1, np.inf)):  # a second card in tiles 0 and 1
        c["conf"][t, 1], c["cls"][t, 1], c["n_det"][t], c["state"][t * kt + 1] = 0.6 - 0.1 * t, CARD, 2, 1
        c["quads"][t * kt + 1] = UP + [75, 20]
        c["quads"][t * kt + 1, 2, t] = bad
    return c


def garbage_tile_start_cases():
    """two_frames (7 + 1 tiles) with a range that leaves [0, NT], a negative one, a descending one and one longer than
    max_tiles_per_frame = 7: those frames have no candidates -> n_sel [2, 0], [0, 2], [0, 0], [0, 0]"""
    c = designed()["two_frames"]
    return [dict(c, tile_start=np.array(ts, np.int32), max_tiles_per_frame=7) for ts in ([0, 7, 99], [-2, 7, 8], [5, 3, 3], [0, 8, 8])]


# ---------------------------------------------------------------------------
# the same rule in float64, on its own, with the margin of every decision
# ---------------------------------------------------------------------------
def merge_f64(c):
    """-> (per frame [(src_slot, state, oriented_by)] in kept order, margins): margins = the least |inter - ios * min(area)| over
    the pairs compared, the least distance of a bound from a cut line it was compared with, the least confidence gap"""
    kt, k, ios, edge, md = c["kt"], c["k"], float(c["ios"]), float(c["edge"]), c["conf"].shape[1]
    m_inter, m_cut, m_conf = math.inf, math.inf, math.inf
    frames = []
    for f, (h, w) in enumerate(c["hw"]):
        cands = []
        for t in range(int(c["tile_start"][f]), int(c["tile_start"][f + 1])):
            _, y0, x0, wh, ww = (int(v) for v in c["tiles"][t])
            _, _, top, left = (int(v) for v in c["geo"][t])
            r = float(c["ratio"][t])
            nd = min(max(int(c["n_det"][t]), 0), md)
            cards = [d for d in range(nd) if c["cls"][t, d] == c["card_cls"]]
            for j in range(min(kt, len(cards))):
                if int(c["state"][t * kt + j]) not in (1, 2):
                    continue
                q = [(min(max((float(x) - left) / r + x0, x0), x0 + ww), min(max((float(y) - top) / r + y0, y0), y0 + wh)) for x, y in c["quads"][t * kt + j]]
                xs, ys = [p[0] for p in q], [p[1] for p in q]
                lines = [(min(xs) - (x0 + edge), x0 > 0), ((x0 + ww - edge) - max(xs), x0 + ww < w), (min(ys) - (y0 + edge), y0 > 0),
                         ((y0 + wh - edge) - max(ys), y0 + wh < h)]
                m_cut = min([m_cut] + [abs(d) for d, inner in lines if inner])
                if any(inner and d < 0 for d, inner in lines):
                    continue
                cands.append((float(c["conf"][t, cards[j]]), t, j, q, int(c["state"][t * kt + j])))
        cands.sort(key=lambda e: (-e[0], e[1], e[2]))
        for x, y in zip(cands, cands[1:]):
            m_conf = min(m_conf, x[0] - y[0])
        alive, kept = [True] * len(cands), []
        while len(kept) < k and any(alive):
            p = alive.index(True)
            alive[p] = False
            _, t, j, qa, sta = cands[p]
            area_a, by = abs(area2_f64(qa)) / 2, -1
            donor = None
            for i in range(p + 1, len(cands)):
                if not alive[i]:
                    continue
                qb = cands[i][3]
                area_b, inter = abs(area2_f64(qb)) / 2, inter_f64(qa, qb)
                if area_a == 0 or area_b == 0:
                    continue
                m_inter = min(m_inter, abs(inter - ios * min(area_a, area_b)))
                if inter > ios * min(area_a, area_b):
                    alive[i] = False
                    if donor is None and cands[i][4] == 2:
                        donor = cands[i]
            if sta == 1 and donor is not None:
                qb = donor[3]
                ua = [(qa[0][i] + qa[1][i]) - (qa[2][i] + qa[3][i]) for i in range(2)]
                ub = [(qb[0][i] + qb[1][i]) - (qb[2][i] + qb[3][i]) for i in range(2)]
                if ua[0] * ub[0] + ua[1] * ub[1] != 0:
                    sta, by = 2, donor[1] * kt + donor[2]
            kept.append((t * kt + j, sta, by))
        frames.append(kept)
    return frames, (m_inter, m_cut, m_conf)
