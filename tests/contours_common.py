"""Cases of the contour tests (tests/test_contours_cpu.py, tests/test_gpu_contours.py) and a plain numpy / Python
restatement of what csrc/contours.hip does: row runs in raster order, union-find on run indices with the smaller index as
the root, a bounded Moore trace that first counts and then writes, CHAIN_APPROX_SIMPLE applied while walking, and the caps.
The CPU test proves the restatement equal to the host specification `mtgv.adapters._mask_segments` on every case, so the
algorithm is checked before anything runs on a GPU; the GPU test compares the kernel with the host function directly.

MAX_RUNS / MAX_BLOBS restate CT_MAX_RUNS / CT_MAX_BLOBS of csrc/contours.hip: keep the two in step."""
import numpy as np

MAX_RUNS = 4096
MAX_BLOBS = 1024
MAX_POINTS = 4096  # the wrappers' default, what every non-overflow case is run with
STRATEGIES = {"all": 0, "largest": 1}

_DY = (0, -1, -1, -1, 0, 1, 1, 1)  # W NW N NE E SE S SW
_DX = (-1, -1, 0, 1, 1, 1, 0, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the device algorithm, restated
# ---------------------------------------------------------------------------------------------------------------------
def _runs(m):
    """row runs (y, x0, x1) in raster order"""
    out = []
    for y in range(m.shape[0]):
        d = np.diff(np.concatenate([[0], m[y].astype(np.int8), [0]]))
        out += [(y, int(a), int(b) - 1) for a, b in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0])]
    return out


def _trace(p, sr, sc, max_steps, write, keep0_in, stop_at_cap, out, pos, cap):
    """ct_trace of contours.hip on the padded boolean image p -> (kept count, keep0, dense points, bad); write True also
    stores the kept points in `out` while pos < cap (point 0 first if keep0_in), and with stop_at_cap ends the walk there"""
    cr, cc, back, npts, fd, pd, cnt, done = sr, sc, 0, 1, 0, 0, 0, False
    dense = [(sr, sc)]

    def put(r, c):
        nonlocal pos
        if pos < cap:
            out[pos] = (c - 1, r - 1)
        pos += 1

    if write and keep0_in:
        put(sr, sc)
    for _ in range(max_steps):
        if write and stop_at_cap and pos >= cap:
            done = True
            break
        d = next((dd for dd in ((back + i) % 8 for i in range(8)) if p[cr + _DY[dd], cc + _DX[dd]]), None)
        if d is None:
            done = True
            break
        nr, nc = cr + _DY[d], cc + _DX[d]
        back = (d + 5) % 8
        if (nr, nc) == (sr, sc):
            done = True
            break
        if npts == 1:
            fd = d
        elif pd != d:
            if write:
                put(cr, cc)
            cnt += 1
        pd, cr, cc, npts = d, nr, nc, npts + 1
        dense.append((nr, nc))
    bad = not done
    if npts == 1:
        return 1, 1, dense, bad
    qy, qx = sr - cr, sc - cc
    keep_last = (_DY[pd], _DX[pd]) != (qy, qx)
    if write and keep_last:
        put(cr, cc)
    keep0 = int((_DY[fd], _DX[fd]) != (qy, qx))
    cnt += int(keep_last) + keep0
    if cnt == 0:
        cnt, keep0 = 1, 1
    return cnt, keep0, dense, bad


def device_contours(mask, strategy="all", max_points=MAX_POINTS):
    """-> dict(points (n_points, 2) int32 x, y; n_points; n_blobs; status; n_runs; dense: per-blob dense chains (y, x) of the
    padded image, as adapters._trace_blob returns them)"""
    m = np.asarray(mask) != 0
    res = dict(points=np.zeros((0, 2), np.int32), n_points=0, n_blobs=0, status=0, n_runs=0, dense=[])
    runs = _runs(m)
    res["n_runs"] = len(runs)
    if len(runs) == 0:
        return res
    if len(runs) > MAX_RUNS:
        res["status"] = 1
        return res
    parent = list(range(len(runs)))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    rowoff = np.searchsorted([r[0] for r in runs], np.arange(m.shape[0] + 1))
    for i, (y, x0, x1) in enumerate(runs):
        if y == 0:
            continue
        for k in range(rowoff[y - 1], rowoff[y]):
            if runs[k][1] > x1 + 1:
                break
            if runs[k][2] < x0 - 1:
                continue
            a, b = find(i), find(k)
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = [i for i in range(len(runs)) if parent[i] == i]
    res["n_blobs"] = len(roots)
    if len(roots) > MAX_BLOBS:
        res["status"] = 1
        return res
    p = np.pad(m, 1)
    max_steps = 8 * int(m.sum())
    out = np.zeros((max_points, 2), np.int32)
    # blob 0 of "all" and a mask's only blob start at offset 0: written during the first walk, point 0 taken as kept
    direct0 = STRATEGIES[strategy] == 0 or len(roots) == 1
    first = []
    for b, i in enumerate(roots):
        if b == 0 and direct0:
            first.append(_trace(p, runs[i][0] + 1, runs[i][1] + 1, max_steps, True, 1, False, out, 0, max_points))
        else:
            first.append(_trace(p, runs[i][0] + 1, runs[i][1] + 1, max_steps, False, 0, False, None, 0, 0))
    res["dense"] = [np.asarray(f[2], np.int64) for f in first]
    bad = any(f[3] for f in first) or (direct0 and first[0][1] != 1)
    counts = [f[0] for f in first]
    if STRATEGIES[strategy] == 0:
        offs, total, todo = np.concatenate([[0], np.cumsum(counts)]), int(np.sum(counts)), range(len(roots))
    else:
        best = int(np.argmax(counts))  # the first maximum
        offs, total, todo = np.zeros(len(roots) + 1, np.int64), counts[best], [best]
    for b in todo:
        if b == 0 and direct0:
            continue
        i = roots[b]
        _trace(p, runs[i][0] + 1, runs[i][1] + 1, max_steps, True, first[b][1], True, out, int(offs[b]), max_points)
    res["n_points"] = min(total, max_points)
    res["points"] = out[: res["n_points"]]
    res["status"] = int(total > max_points or bad)
    return res


def host_contours(mask, strategy="all"):
    """the specification: (points (P, 2) int32, number of blobs) from mtgv.adapters._mask_segments and scipy's labelling"""
    from scipy import ndimage

    from mtgv.adapters import _mask_segments

    pts = _mask_segments(np.asarray(mask) != 0, strategy)
    n_blobs = ndimage.label(np.asarray(mask) != 0, structure=np.ones((3, 3), int))[1]
    assert np.array_equal(pts, np.round(pts))
    return pts.astype(np.int32), int(n_blobs)


# ---------------------------------------------------------------------------------------------------------------------
# cases: small on purpose, each names what can go wrong
# ---------------------------------------------------------------------------------------------------------------------
def _from_pixels(h, w, yx):
    m = np.zeros((h, w), np.uint8)
    for y, x in yx:
        m[y, x] = 1
    return m


def _from_rows(rows):
    return np.asarray([[c != "." for c in r] for r in rows], np.uint8)


def _shifted_starts(m):
    """the same shape turned and mirrored so that another pixel is the trace's start"""
    return [m, m[::-1], m[:, ::-1], m.T, m.T[::-1], m[::-1, ::-1]]


def u_shape(orientation, size=12):
    """a U-shaped card mask (a rectangle with a notch), opening down / up / left / right"""
    m = np.zeros((size, size), np.uint8)
    m[2 : size - 2, 1 : size - 1] = 1
    m[size - 6 : size - 2, 4 : size - 4] = 0  # opens downwards
    return {"down": m, "up": m[::-1], "right": m.T, "left": m.T[:, ::-1]}[orientation].copy()


def card_mask(h=640, w=640, centre=(320.0, 320.0), half=(120.0, 170.0), angle_deg=20.0, notch=30.0):
    """a rotated rectangle with a round notch in the middle of its bottom edge (the reference's U-shaped card masks)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.deg2rad(angle_deg)
    u = (xx - centre[0]) * np.cos(a) + (yy - centre[1]) * np.sin(a)
    v = -(xx - centre[0]) * np.sin(a) + (yy - centre[1]) * np.cos(a)
    m = (np.abs(u) <= half[0]) & (np.abs(v) <= half[1])
    bx, by = centre[0] - half[1] * np.sin(a), centre[1] + half[1] * np.cos(a)  # middle of the bottom edge
    m &= (xx - bx) ** 2 + (yy - by) ** 2 >= notch**2
    return m.astype(np.uint8)


def word_boundary_mask(w):
    """runs that straddle a 32-pixel word boundary of the bit image, end exactly on it, and end on the last column"""
    m = np.zeros((9, w), np.uint8)
    m[0, max(0, w - 8) :] = 1               # ends on the last column
    m[2, 28 : min(w, 36)] = 1               # straddles x = 32 (where the row is wide enough)
    m[4, 20 : min(w, 32)] = 1               # ends exactly on x = 31
    m[6, min(w - 1, 32) : min(w, 40)] = 1   # starts exactly on x = 32
    if w > 60:
        m[8, 58 : min(w, 67)] = 1           # straddles x = 64
        m[6, 50 : min(w, 64)] = 1           # ends exactly on x = 63
    m[2:7, 31:33] = 1                       # a two-pixel bar across x = 32 joins rows 2, 4 and 6 into one blob
    return m


RANDOM_SHAPE = (33, 70)
RANDOM_DENSITIES = (0.05, 0.3, 0.5, 0.6, 0.9)


def random_mask(density, seed, shape=RANDOM_SHAPE):
    return (np.random.default_rng(1000 * seed + int(density * 100)).random(shape) < density).astype(np.uint8)


def stride2_grid(size=66):
    """single pixels on a stride-2 grid: (size / 2)^2 blobs, more than MAX_BLOBS at size 66"""
    m = np.zeros((size, size), np.uint8)
    m[::2, ::2] = 1
    return m


def cases():
    """[(name, mask (h, w) uint8)]: every non-overflow case"""
    out = [
        ("1x1 set", np.ones((1, 1), np.uint8)),
        ("1x1 clear", np.zeros((1, 1), np.uint8)),
        ("pixel in 3x3", _from_pixels(3, 3, [(1, 1)])),
        ("two pixels, horizontal", _from_pixels(3, 4, [(1, 1), (1, 2)])),
        ("two pixels, diagonal", _from_pixels(3, 4, [(0, 1), (1, 2)])),
        ("two pixels, anti-diagonal", _from_pixels(3, 4, [(0, 2), (1, 1)])),
        ("1x5 line", np.ones((1, 5), np.uint8)),
        ("5x1 line", np.ones((5, 1), np.uint8)),
        ("full 4x6", np.ones((4, 6), np.uint8)),
    ]
    corners = np.zeros((9, 9), np.uint8)
    corners[:3, :2] = corners[:2, 6:] = corners[7:, :3] = corners[6:, 7:] = 1
    out.append(("rectangles at the corners of 9x9", corners))
    inv_v = _from_pixels(3, 5, [(0, 2), (1, 1), (2, 0), (1, 3), (2, 4)])  # the walk takes one arm and stops on the apex
    plus = _from_rows([".#.", "###", ".#."])
    diamond = _from_pixels(3, 3, [(0, 1), (1, 0), (1, 2), (2, 1)])
    hook = _from_rows(["..#..", ".#.#.", "#...#", "#....", "##..."])  # an inverted V with a longer, bent left arm
    for name, m in (("inverted V", inv_v), ("plus", plus), ("diamond", diamond), ("hook", hook)):
        for k, v in enumerate(_shifted_starts(m)):
            out.append((f"{name} / turn {k}", np.ascontiguousarray(v)))
            out.append((f"{name} / turn {k} padded", np.pad(v, ((1, 2), (2, 1)))))
    ring = np.ones((5, 5), np.uint8)
    ring[1:4, 1:4] = 0
    out.append(("ring 5x5", ring))
    dot = ring.copy()
    dot[2, 2] = 1
    out.append(("ring with a dot in the hole", dot))
    nested = np.ones((9, 9), np.uint8)
    nested[1:8, 1:8] = 0
    nested[2:7, 2:7] = 1
    nested[3:6, 3:6] = 0
    out.append(("two nested rings", nested))
    for o in ("down", "up", "left", "right"):
        out.append((f"U opening {o}", u_shape(o)))
    for w in (31, 32, 33, 63, 64, 65):
        out.append((f"word boundary, width {w}", word_boundary_mask(w)))
        out.append((f"full rows, width {w}", np.ones((3, w), np.uint8)))
    for d in RANDOM_DENSITIES:
        for seed in range(3):
            out.append((f"random {d} seed {seed}", random_mask(d, seed)))
    out.append(("card 640x640", card_mask()))
    out.append(("card 480x640", card_mask(480, 640, (300.0, 250.0), (100.0, 150.0), -35.0, 25.0)))
    return out


def batches():
    """[(name, masks (n, h, w) uint8)]: several masks in one call"""
    five = np.stack([random_mask(0.3, 0), random_mask(0.9, 1), np.zeros(RANDOM_SHAPE, np.uint8), random_mask(0.05, 2), random_mask(0.6, 0)])
    full = np.ones((7, 40), np.uint8)
    return [("five different masks", five), ("empty between two full", np.stack([full, np.zeros_like(full), full]))]
