"""Shared by test_tiles_cpu.py and test_gpu_tiles.py: the designed cases of the tile merge and the random frames, as plain
numpy tables (what mtgv.tiles.merge_tiles_host and mtgv_tiles_merge both read).  No GPU needed here."""
import numpy as np

from mtgv.detector import fit_geometry
from mtgv.tiles import merge_tiles_host, tile_grid

WINDOW = (128, 160)  # the window and the detector input of the designed cases: a tile is an exact copy (ratio 1)
OVERLAP = 32
BIG = (300, 500)  # x origins 0, 128, 256, 340 and y origins 0, 96, 172: 12 windows in raster order
_PAD = np.array([[40.0, 60.0, 168.0, 252.0], [200.0, 60.0, 328.0, 252.0], [360.0, 60.0, 488.0, 252.0], [500.0, 60.0, 628.0, 252.0],
                 [40.0, 330.0, 168.0, 522.0], [200.0, 330.0, 328.0, 522.0], [360.0, 330.0, 488.0, 522.0], [500.0, 330.0, 628.0, 522.0]], np.float32)

OUTPUTS = ("sel_boxes_src", "quads_src", "frame_idx", "sel_conf", "src_slot", "n_sel")


def pad_frac(k):
    """what Pipeline hands the merge: _PAD_BOXES / 640, repeated to k rows"""
    return np.tile(_PAD / np.float32(640.0), ((k + 7) // 8, 1))[:k].copy()


def tables(frames_hw, window=WINDOW, overlap=OVERLAP, with_full=False, input_hw=WINDOW, tiles=None):
    """-> dict hw (F, 2), tiles (NT, 5), tile_start (F + 1), geo (NT, 4), ratio (NT) of the frames' tile grids (or of the
    caller's own per-frame window lists `tiles`)"""
    grids = [tile_grid(h, w, window, overlap, with_full) for h, w in frames_hw] if tiles is None else [np.array(g, np.int32).reshape(-1, 4) for g in tiles]
    rows = np.concatenate([np.concatenate([np.full((len(g), 1), f, np.int32), g], 1) for f, g in enumerate(grids)]).astype(np.int32)
    g = [fit_geometry(int(t[3]), int(t[4]), input_hw[0], input_hw[1]) for t in rows]
    return {"hw": np.array(frames_hw, np.int32).reshape(-1, 2), "tiles": rows,
            "tile_start": np.concatenate([[0], np.cumsum([len(x) for x in grids])]).astype(np.int32),
            "geo": np.array([t[1:] for t in g], np.int32).reshape(len(g), 4), "ratio": np.array([t[0] for t in g], np.float64)}


def to_tile(tab, t, box):
    """camera-pixel xyxy -> float32 pixels of tile t's detector input (exact where the ratio is 1 and the numbers are small)"""
    _, y0, x0, _, _ = (int(v) for v in tab["tiles"][t])
    _, _, top, left = (int(v) for v in tab["geo"][t])
    r = tab["ratio"][t]
    x = np.array(box, np.float64)
    return np.array([(x[0] - x0) * r + left, (x[1] - y0) * r + top, (x[2] - x0) * r + left, (x[3] - y0) * r + top], np.float32)


def case(tab, dets, kt, k, max_det=8, edge=2.0, ios=0.5, quads=False, n_det=None, tile_px=False, max_tiles_per_frame=None):
    """dets: [(global tile, xyxy in camera pixels (tile_px: in the tile's own input pixels), conf), ...]; every tile's list is
    put in score-descending order like an NMS output.  quads: the candidates also get mask-like quads (their boxes drawn in
    by a pixel, as corners TL TR BR BL).  n_det: {tile: count} overrides (a count above kt)."""
    NT = tab["tiles"].shape[0]
    boxes, conf, nd = np.zeros((NT, max_det, 4), np.float32), np.zeros((NT, max_det), np.float32), np.zeros((NT,), np.int32)
    per = {}
    for t, b, c in dets:
        per.setdefault(t, []).append((np.array(b, np.float32) if tile_px else to_tile(tab, t, b), np.float32(c)))
    for t, lst in per.items():
        lst.sort(key=lambda e: -float(e[1]))  # (stable: equal scores keep their order)
        assert len(lst) <= max_det
        for j, (b, c) in enumerate(lst):
            boxes[t, j], conf[t, j] = b, c
        nd[t] = len(lst)
    for t, n in (n_det or {}).items():
        nd[t] = n
    q = None
    if quads:
        q = np.zeros((NT * kt, 4, 2), np.float32)
        for t in range(NT):
            for j in range(min(int(nd[t]), kt)):
                x0, y0, x1, y1 = boxes[t, j] + np.array([1, 1, -1, -1], np.float32)
                q[t * kt + j] = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    return dict(tab, n_det=nd, boxes=boxes, conf=conf, quads=q, kt=kt, k=k, edge=edge, ios=ios, pad_frac=pad_frac(k),
                max_tiles_per_frame=max_tiles_per_frame)


def host(c):
    return merge_tiles_host(c["n_det"], c["boxes"], c["conf"], c["quads"], c["tiles"], c["geo"], c["ratio"], c["tile_start"], c["hw"], c["pad_frac"],
                            c["kt"], c["k"], c["edge"], c["ios"], c["max_tiles_per_frame"])


def designed():
    """name -> case.  The 300 x 500 frame has 12 windows, tile t = 4 * row + column; tile 0 is x 0..160, y 0..128, tile 1 is
    x 128..288, tile 4 is y 96..224, tile 5 both."""
    big, one = tables([BIG]), tables([WINDOW])
    full = tables([BIG], with_full=True)  # tile 12 is the whole frame, ratio 0.32
    two = tables([(200, 400), (100, 120)])  # 6 tiles and 1 (clipped) tile
    card = (135, 100, 150, 120)  # inside tiles 0, 1, 4 and 5, more than `edge` from their inner sides
    out = {
        "overlap_two": case(big, [(0, (135, 20, 150, 50), 0.8), (1, (135, 20, 150, 50), 0.9)], 4, 4),
        "corner_four": case(big, [(0, card, 0.5), (1, card, 0.6), (4, card, 0.95), (5, card, 0.7)], 4, 4, quads=True),
        "equal_conf": case(big, [(1, (135, 20, 150, 50), 0.75), (0, (135, 20, 150, 50), 0.75)], 4, 4),
        # the same box of the tile's own pixels: at the frame's left side in tile 0, at an inner side in tile 1
        "inner_and_frame_side": case(big, [(0, (0, 10, 20, 40), 0.9), (1, (0, 10, 20, 40), 0.9)], 4, 4, tile_px=True),
        # tile 1 is x 128..288: exactly `edge` from both inner sides (nobody else sees it whole)
        "exactly_edge": case(big, [(1, (130, 10, 286, 40), 0.9)], 4, 4),
        # inter = 32 * 64 = 0.5 * 4096 exactly: both kept; 32.25 * 64 is over: the second is dropped
        "ios_equal": case(one, [(0, (0, 0, 64, 64), 0.9), (0, (32, 0, 96, 64), 0.8), (0, (0, 64, 64, 128), 0.7), (0, (31.75, 64, 95.75, 128), 0.6)], 8, 8),
        # a card larger than the overlap: whole in the full-frame window, a fragment of it in tile 0
        "fragment_low": case(full, [(12, (100, 30, 220, 110), 0.9), (0, (100, 30, 150, 110), 0.6)], 4, 4),
        "fragment_high": case(full, [(12, (100, 30, 220, 110), 0.6), (0, (100, 30, 150, 110), 0.9)], 4, 4),
        "more_than_k": case(one, [(0, (4 + 12 * i, 8, 14 + 12 * i, 40), 0.3 + 0.05 * i) for i in range(12)], 16, 8, max_det=16),
        "none": case(big, [], 4, 8),
        "n_det_over_kt": case(one, [(0, (4 + 20 * i, 8, 20 + 20 * i, 40), 0.9 - 0.1 * i) for i in range(6)], 4, 8, quads=True),
        "full_ratio": case(tables([BIG], tiles=[[(0, 0, 300, 500)]]), [(0, (100, 50, 220, 200), 0.9), (0, (300, 20, 360, 110), 0.5)], 4, 4, quads=True),
        "two_frames": case(two, [(0, (20, 20, 60, 80), 0.9), (1, (140, 20, 150, 80), 0.8), (0, (140, 20, 150, 80), 0.7), (5, (300, 120, 380, 190), 0.6),
                                 (6, (10, 10, 50, 70), 0.5), (6, (60, 10, 100, 70), 0.4)], 4, 4),
    }
    return out


def random_case(seed, kt, k, quads, max_det=64):
    """8 frames of 1 to 16 tiles: cards at quarter pixels, every tile detects the part it sees of the cards that reach into it
    (a cut card keeps a box at the window's side and falls to the cut rule), confidences from 16 values (ties are common)"""
    rng = np.random.default_rng(seed)
    frames_hw, grids = [], []
    while len(frames_hw) < 8:
        h, w = int(rng.integers(40, 400)), int(rng.integers(40, 600))
        g = tile_grid(h, w, WINDOW, OVERLAP, bool(rng.integers(0, 2)))
        if len(g) <= 16:
            frames_hw.append((h, w)), grids.append(g)
    tab = tables(frames_hw, tiles=grids)
    levels = np.linspace(0.3, 0.9, 16).astype(np.float32)
    NT = tab["tiles"].shape[0]
    boxes, conf, nd = np.zeros((NT, max_det, 4), np.float32), np.zeros((NT, max_det), np.float32), np.zeros((NT,), np.int32)
    for f, (h, w) in enumerate(frames_hw):
        n_cards = int(rng.integers(0, 40 if kt > 8 else 14))
        cx, cy = rng.uniform(0, w, n_cards), rng.uniform(0, h, n_cards)
        cw, ch = rng.uniform(8, 50, n_cards), rng.uniform(8, 60, n_cards)
        cards = np.round(np.stack([cx - cw / 2, cy - ch / 2, cx + cw / 2, cy + ch / 2], 1) * 4) / 4
        for t in range(int(tab["tile_start"][f]), int(tab["tile_start"][f + 1])):
            _, y0, x0, wh, ww = (int(v) for v in tab["tiles"][t])
            found = []
            for c in cards:
                b = np.array([max(c[0], x0), max(c[1], y0), min(c[2], x0 + ww), min(c[3], y0 + wh)])
                if b[2] - b[0] < 2 or b[3] - b[1] < 2 or rng.random() < 0.15:
                    continue
                b = b + np.round(rng.uniform(-1, 1, 4) * 4) / 4 * (rng.random() < 0.5)
                tb = np.round(to_tile(tab, t, b).astype(np.float64) * 4) / 4
                found.append((tb.astype(np.float32), levels[int(rng.integers(0, 16))]))
            found.sort(key=lambda e: -float(e[1]))
            found = found[:max_det]
            for j, (b, c) in enumerate(found):
                boxes[t, j], conf[t, j] = b, c
            nd[t] = len(found)
    q = None
    if quads:
        q = np.zeros((NT * kt, 4, 2), np.float32)
        for t in range(NT):
            for j in range(min(int(nd[t]), kt)):
                x0, y0, x1, y1 = boxes[t, j]
                q[t * kt + j] = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float32) + np.round(rng.uniform(-2, 2, (4, 2)) * 4).astype(np.float32) / 4
    return dict(tab, n_det=nd, boxes=boxes, conf=conf, quads=q, kt=kt, k=k, edge=2.0, ios=0.5, pad_frac=pad_frac(k), max_tiles_per_frame=None)


def cap_case():
    """one frame at the cap: 16 tiles (each the whole 128 x 160 frame: no inner side) of 64 detections, 1024 disjoint boxes
    on a 32 x 32 grid - every candidate survives the cut rule and the suppression; 64 are kept"""
    tab = tables([WINDOW], tiles=[[(0, 0, 128, 160)] * 16])
    rng = np.random.default_rng(5)
    levels = np.linspace(0.3, 0.9, 16).astype(np.float32)
    cells = rng.permutation(1024)
    dets = []
    for i, cell in enumerate(cells):
        gy, gx = divmod(int(cell), 32)
        dets.append((i // 64, (gx * 5, gy * 4, gx * 5 + 4, gy * 4 + 3), levels[int(rng.integers(0, 16))]))
    return case(tab, dets, 64, 64, max_det=64)


def blocks_frame(h, w, seed, n_blocks=6):
    """a smooth two-colour gradient with a few flat coloured blocks on it (the cards of the pipeline tests)"""
    rng = np.random.default_rng(seed)
    c0, c1 = rng.integers(60, 200, (2, 3)).astype(np.float64)
    t = (np.arange(h)[:, None] / h + np.arange(w)[None, :] / w)[..., None] / 2
    f = np.round(c0 * (1 - t) + c1 * t).astype(np.uint8)
    for _ in range(n_blocks):
        bh, bw = int(rng.integers(h // 8, h // 3)), int(rng.integers(w // 10, w // 4))
        y, x = int(rng.integers(0, h - bh)), int(rng.integers(0, w - bw))
        f[y : y + bh, x : x + bw] = rng.integers(0, 256, 3, dtype=np.uint8)
    return f
