"""Yardstick for the labelled bank top-k (test_match_labels_cpu.py, test_gpu_match_labels.py): the brute-force oracle,
a numpy model of the tiled scheme, and the shared inputs.

The contract (include/mtgv.h, mtgv_bank_topk_ex), restated:
  row n is eligible for query m when (tags[n] & all_of) == all_of, and any_of == 0 or (tags[n] & any_of) != 0, and
  (tags[n] & none_of) == 0;  order: score desc, then id asc;  distinct: among the eligible rows a group >= 0 is represented
  by its best row under that order, rows of group -1 never suppress one another;  then k;  then the threshold: a
  representative below it becomes a pad (id -1, score -inf), pads come last.
Scores are the fp64 cosines of oracle.match_ref.scores.
"""
from __future__ import annotations

import numpy as np

N = 421  # three 192-column tiles (the last 37 wide), five 96-column wave ranges, seven 64-column tiles
B_MAX = 130  # crosses the 128-row tile
NO_FILTER = (0, 0, 0)
FULL = 0xFFFFFFFFFFFFFFFF


def eligible(tags: np.ndarray, mask) -> np.ndarray:
    """(N,) bool for one query's (all_of, any_of, none_of)"""
    t = np.asarray(tags, np.uint64)
    a, o, x = (np.uint64(int(v)) for v in mask)
    return ((t & a) == a) & ((o == 0) | ((t & o) != 0)) & ((t & x) == 0)


def _pick(order, groups, distinct, k):
    """walk rows in (score desc, id asc) order; with distinct skip a row whose non-negative group was seen"""
    out, seen = [], set()
    for n in order:
        g = int(groups[n])
        if distinct and g >= 0:
            if g in seen:
                continue
            seen.add(g)
        out.append(int(n))
        if len(out) == k:
            break
    return out


def labelled_topk(s, tags, groups, masks, distinct, k, threshold=None):
    """s (B, N) fp64 scores, tags (N,) uint64, groups (N,) int, masks (B, 3) or one triple -> (ids (B, k) int64, scores
    (B, k) fp64): eligibility, then distinct, then k, then threshold."""
    s = np.asarray(s, np.float64)
    b, n = s.shape
    masks = np.broadcast_to(np.asarray(masks, np.uint64).reshape(-1, 3), (b, 3))
    ids = np.full((b, k), -1, np.int64)
    out = np.full((b, k), -np.inf, np.float64)
    for i in range(b):
        idx = np.nonzero(eligible(tags, masks[i]))[0]
        order = idx[np.lexsort((idx, -s[i, idx]))]
        rows = _pick(order, groups, distinct, k)
        if threshold is not None:
            rows = [r for r in rows if s[i, r] >= threshold]
        ids[i, : len(rows)] = rows
        out[i, : len(rows)] = s[i, rows]
    return ids, out


def labelled_cosine_topk(q, bank, tags, groups, masks, distinct, k, threshold=None):
    from oracle import match_ref as M

    return labelled_topk(M.scores(q, bank), tags, groups, masks, distinct, k, threshold)


def rep_margin(s, tags, groups, masks, distinct, k):
    """per query: the smallest fp64 gap between consecutive representatives among the top k + 1 (inf with fewer than two)"""
    _, sc = labelled_topk(s, tags, groups, masks, distinct, k + 1)
    with np.errstate(invalid="ignore"):  # pads: -inf - -inf
        gap = np.where(np.isfinite(sc[:, 1:]), sc[:, :-1] - sc[:, 1:], np.inf)
    return gap.min(axis=1)


def tiled_topk(s, tags, groups, masks, distinct, k, cols, range_dedupe=True):
    """The kernels' scheme: every range of `cols` columns reports its kt = min(k, cols) best eligible rows - of pairwise
    different groups when range_dedupe - and a merge over the candidates (which always dedupes) takes the top k.
    range_dedupe=False is the WRONG scheme the design rules out: a range full of one group's rows hides the next group."""
    s = np.asarray(s, np.float64)
    b, n = s.shape
    masks = np.broadcast_to(np.asarray(masks, np.uint64).reshape(-1, 3), (b, 3))
    kt = min(k, cols)
    ids = np.full((b, k), -1, np.int64)
    for i in range(b):
        el = eligible(tags, masks[i])
        cand = []
        for c0 in range(0, n, cols):
            idx = np.arange(c0, min(c0 + cols, n))
            idx = idx[el[idx]]
            order = idx[np.lexsort((idx, -s[i, idx]))]
            cand += _pick(order, groups, distinct and range_dedupe, kt)
        cand = np.asarray(cand, np.int64)
        order = cand[np.lexsort((cand, -s[i, cand]))] if len(cand) else cand
        rows = _pick(order, groups, distinct, k)
        ids[i, : len(rows)] = rows
    return ids


# ---- shared inputs ----
# seeds chosen on the CPU (test_match_labels_cpu.py::test_seeds_leave_no_near_ties re-checks them): for every query, k and
# label variant the tests use, the oracle's gap between consecutive representatives among the top k + 1 exceeds 1e-5
SEEDS = {768: 259, 64: 0, 36: 12}
K_MAX = 8
# bits 60..63 of the random tags are designed: which rows carry them
ROWS_BIT63 = [57, 333]  # fewer than k rows for k = 3, 8
ROWS_BIT62 = [390, 397, 400, 405, 411, 414, 418, 419, 420]  # all in the ragged last tile (rows >= 384)
ROWS_BIT61 = [3, 20, 41, 100, 250, 251, 300]  # row 100 is alone in the 96-column range 96..191 and the 64-column tile 64..127
N_SPECIAL = 5  # queries 0..4: a random selective mask, no row, fewer than k, ragged tile only, one row in a range


def random_case(d: int):
    """bank (N, d), queries (B_MAX, d) float32; tags (N,) uint64 = AND of two random words (every bit set in a quarter of
    the rows: all_of masks are selective) with the designed bits above; groups (N,) int32: about a third of the rows
    ungrouped, the rest in 60 groups scattered over the tiles; masks (B_MAX, 3) uint64 per query."""
    rng = np.random.default_rng(1000 * d + SEEDS[d])
    bank = rng.standard_normal((N, d)).astype(np.float32)
    q = (rng.standard_normal((B_MAX, d)) * 3).astype(np.float32)
    tags = rng.integers(0, 2**64, N, dtype=np.uint64) & rng.integers(0, 2**64, N, dtype=np.uint64)
    tags &= np.uint64(FULL >> 4)
    for bit, rows in ((63, ROWS_BIT63), (62, ROWS_BIT62), (61, ROWS_BIT61)):
        tags[rows] |= np.uint64(1 << bit)
    groups = rng.integers(0, 60, N).astype(np.int32)
    groups[rng.random(N) < 0.33] = -1
    masks = np.zeros((B_MAX, 3), np.uint64)
    for i in range(B_MAX):
        kind = i % 4
        bits = [int(x) for x in rng.choice(60, 3, replace=False)]
        if kind == 0:  # one required bit, one forbidden
            masks[i] = (1 << bits[0], 0, 1 << bits[1])
        elif kind == 1:  # two required bits: about 1 row in 16
            masks[i] = ((1 << bits[0]) | (1 << bits[1]), 0, 0)
        elif kind == 2:  # any of two, none of a third
            masks[i] = (0, (1 << bits[0]) | (1 << bits[1]), 1 << bits[2])
        else:
            masks[i] = (1 << bits[0], (1 << bits[1]) | (1 << bits[2]), 0)
    masks[1] = (FULL, 0, 0)  # no row has every bit
    masks[2] = (1 << 63, 0, 0)
    masks[3] = (0, 1 << 62, 0)
    masks[4] = (1 << 61, 0, 0)
    return bank, q, tags, groups, masks


def variant_labels(case, variant):
    """(masks or NO_FILTER, distinct) of the label variants the random-bank tests run"""
    masks = case[4]
    return {"filter": (masks, False), "distinct": (NO_FILTER, True), "both": (masks, True)}[variant]


def hiding_case(d: int):
    """Case 3 of the issue: every score is 0.1 except rows 200..204 (0.90..0.94, group 7), row 210 (0.8, group 8), row 30
    (0.5) and row 400 (0.4), both ungrouped.  Rows 200..210 share one 64-column tile (192..255) and one 96-column range
    (192..287).  k = 3, distinct: [204, 210, 30]; a merge-only dedupe answers [204, 30, 400].
    Rows are c e0 + sqrt(1 - c^2) e1 and the query is e0: the cosines are c to rounding, gaps >= 1e-2."""
    c = np.full(N, 0.1)
    c[200:205] = 0.90 + 0.01 * np.arange(5)
    c[210], c[30], c[400] = 0.8, 0.5, 0.4
    groups = np.full(N, -1, np.int32)
    groups[200:205] = 7
    groups[210] = 8
    return _two_axis_bank(c, d), _e0(d), groups


def ties_case(d: int):
    """Case 4: exact duplicate rows decide by id.  Rows 10 and 12 (0.9) share group 3 -> 10 represents it; rows 20 (group 4)
    and 21 (group 5) tie at 0.8 -> both, 20 first; group 6 spans five tiles, its best is row 150 (0.75) beside 0.7s that
    tie with one another; every other row scores 0.1 in one of seven groups 100 + row % 7, which span every tile: 11
    representatives in all, so k = 100 (more than a range holds, more than there are groups) ends in pads."""
    c = np.full(N, 0.1)
    groups = (100 + np.arange(N) % 7).astype(np.int32)
    c[[10, 12]], groups[[10, 12]] = 0.9, 3
    c[20], groups[20] = 0.8, 4
    c[21], groups[21] = 0.8, 5
    for r, v in ((5, 0.7), (70, 0.7), (150, 0.75), (300, 0.7), (415, 0.72)):
        c[r], groups[r] = v, 6
    return _two_axis_bank(c, d), _e0(d), groups


def _e0(d):
    q = np.zeros(d, np.float32)
    q[0] = 2.0
    return q


def _two_axis_bank(c, d):
    bank = np.zeros((len(c), d), np.float32)
    bank[:, 0] = c
    bank[:, 1] = np.sqrt(1.0 - np.asarray(c, np.float64) ** 2)
    return bank


BIG_N, BIG_B, BIG_K, BIG_D, BIG_SEED = 5000, 129, 3, 768, 0


def big_case():
    """Case 6: a bank and batch the unlabelled match sends through the two-pass pre-pass (>= 4096 rows, >= 128 queries,
    k <= 4, dim % 64 == 0): bank, queries, tags (bits set in half of the rows), groups (about 1500 of them, a fifth of the
    rows ungrouped), one (all_of, any_of, none_of) per query.  Seed chosen like SEEDS."""
    rng = np.random.default_rng(77000 + BIG_SEED)
    bank = rng.standard_normal((BIG_N, BIG_D)).astype(np.float32)
    q = (rng.standard_normal((BIG_B, BIG_D)) * 3).astype(np.float32)
    tags = rng.integers(0, 2**64, BIG_N, dtype=np.uint64)
    groups = rng.integers(0, 1500, BIG_N).astype(np.int32)
    groups[rng.random(BIG_N) < 0.2] = -1
    masks = np.zeros((BIG_B, 3), np.uint64)
    for i in range(BIG_B):
        bits = [int(x) for x in rng.choice(64, 3, replace=False)]
        masks[i] = (1 << bits[0], 0, 1 << bits[1]) if i % 2 else (0, (1 << bits[0]) | (1 << bits[1]), 1 << bits[2])
    return bank, q, tags, groups, masks
