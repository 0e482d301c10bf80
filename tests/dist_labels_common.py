"""The labelled sharded match (mtgv.dist, include/mtgv.h: mtgv_bank_topk_packed_ex / mtgv_topk_merge_gathered_ex) restated
in numpy for test_dist_labels_cpu.py and test_gpu_dist_labels.py.  Inputs, seeds and the brute-force oracle are those of
match_labels_common.py.

The scheme:
  1. every shard (rows shard_rows(N, r, R)) runs the labelled top-k over its own rows - eligibility, and with distinct one
     row per group >= 0 - and writes k results in the exchange format packed[b][k][2] int64: word 0 the GLOBAL id or -1,
     word 1 = (group as uint32) << 32 | float32 bits of the score; pads are (-1, group -1, -inf);
  2. the merge walks the R * k candidates of a query in (score desc, id asc) order; with distinct a picked candidate
     retires every other candidate of its non-negative group; then k; then the threshold (a representative below it
     becomes a pad and is not replaced).
local_dedupe=False and merge_dedupe=False are the two WRONG variants the design rules out (negative controls).
"""
from __future__ import annotations

import numpy as np

import match_labels_common as L

NEG_INF_BITS = 0xFF800000
PAD_WORD = np.uint64((0xFFFFFFFF << 32) | NEG_INF_BITS)


def shards(n: int, R: int):
    from mtgv.dist import shard_rows

    return [shard_rows(n, r, R) for r in range(R)]


def pack(ids, scores, groups):
    """ids (.., k) int64 global or -1, scores (.., k) float, groups (.., k) int of the results -> (.., k, 2) int64 exchange
    words; a result with id -1 becomes the pad whatever its score and group say"""
    ids = np.asarray(ids, np.int64)
    bits = np.ascontiguousarray(scores, np.float32).view(np.uint32).astype(np.uint64)
    g = np.ascontiguousarray(np.broadcast_to(groups, ids.shape), np.int32)
    w1 = (g.view(np.uint32).astype(np.uint64) << np.uint64(32)) | bits
    w1 = np.where(ids >= 0, w1, PAD_WORD)
    return np.stack([ids, w1.view(np.int64)], -1)


def unpack(packed):
    """(.., 2) int64 -> (ids int64, scores float32, groups int32); the score is read as the unlabelled merge reads it"""
    packed = np.asarray(packed, np.int64)
    w1 = packed[..., 1]
    scores = w1.astype(np.uint32).view(np.float32)  # test_dist_cpu.py's merge_gathered: the low half
    groups = (w1 >> 32).astype(np.int32)
    return packed[..., 0], scores, groups


def local_packed(s_shard, lo, tags_shard, groups_shard, masks, distinct, k, local_dedupe=True):
    """step 1 for one shard: s_shard (B, n_shard) scores of ALL queries against the shard's rows -> (B, k, 2) int64"""
    b = s_shard.shape[0]
    if s_shard.shape[1] == 0:
        ids, sc = np.full((b, k), -1, np.int64), np.full((b, k), -np.inf)
    else:
        ids, sc = L.labelled_topk(s_shard, tags_shard, groups_shard, masks, distinct and local_dedupe, k)
    g = np.asarray(groups_shard, np.int64)[np.maximum(ids, 0)] if len(groups_shard) else -1
    return pack(np.where(ids >= 0, ids + lo, -1), sc, g)


def merge(gathered, row0, b, k, distinct, threshold=None, merge_dedupe=True):
    """step 2: gathered (R, B_total, k, 2) int64 -> (ids (b, k) int64, scores (b, k) float32) of queries [row0, row0 + b)"""
    gathered = np.asarray(gathered, np.int64)
    mine = gathered[:, row0 : row0 + b].transpose(1, 0, 2, 3).reshape(b, -1, 2)
    ci, cs, cg = unpack(mine)
    ids = np.full((b, k), -1, np.int64)
    out = np.full((b, k), -np.inf, np.float32)
    for i in range(b):
        idx = np.nonzero((ci[i] >= 0) & (cs[i] > -np.inf))[0]
        order = idx[np.lexsort((ci[i, idx], -cs[i, idx].astype(np.float64)))]
        rows = L._pick(order, cg[i], distinct and merge_dedupe, k)
        if threshold is not None:
            rows = [r for r in rows if cs[i, r] >= np.float32(threshold)]
        ids[i, : len(rows)] = ci[i, rows]
        out[i, : len(rows)] = cs[i, rows]
    return ids, out


def exchange(s, tags, groups, masks, distinct, k, R, local_dedupe=True):
    """step 1 on every shard of a bank whose scores are s (B, N): the all-gathered buffer (R, B, k, 2) int64"""
    s = np.asarray(s, np.float64)
    tags, groups = np.asarray(tags, np.uint64), np.asarray(groups)
    parts = [local_packed(s[:, lo:hi], lo, tags[lo:hi], groups[lo:hi], masks, distinct, k, local_dedupe) for lo, hi in shards(s.shape[1], R)]
    return np.stack(parts)


def sharded_labelled_topk(s, tags, groups, masks, distinct, k, R, threshold=None, local_dedupe=True, merge_dedupe=True):
    """the whole scheme over R row shards -> (ids (B, k) int64, scores (B, k) float32)"""
    g = exchange(s, tags, groups, masks, distinct, k, R, local_dedupe)
    return merge(g, 0, g.shape[1], k, distinct, threshold, merge_dedupe)


# ---- the designed cross-shard case ----
CROSS_K, CROSS_R, CROSS_THR = 4, 3, 0.7
CROSS_WANT = [200, 60, 350, 100]  # distinct, k = 4
CROSS_WANT_NO_MERGE_DEDUPE = [200, 40, 300, 60]
CROSS_WANT_THR = [200, 60, -1, -1]  # threshold 0.7: pads are not refilled


def cross_shard_case(d: int):
    """N = 421 over R = 3 shards [0, 141), [141, 281), [281, 421).  Group 9 has a row on every shard - 40 (0.90), 200
    (0.95), 300 (0.90) - so every shard reports one and the merge must retire two; group 11 is rows 60 and 360 (0.80 each),
    exact duplicates on different shards: the lower id represents it; rows 350 (0.6) and 100 (0.5) are ungrouped; every
    other row scores 0.1, ungrouped.  Built like hiding_case: bank, query, groups."""
    c = np.full(L.N, 0.1)
    groups = np.full(L.N, -1, np.int32)
    for r, v, g in ((40, 0.90, 9), (200, 0.95, 9), (300, 0.90, 9), (60, 0.80, 11), (360, 0.80, 11), (350, 0.6, -1), (100, 0.5, -1)):
        c[r], groups[r] = v, g
    return L._two_axis_bank(c, d), L._e0(d), groups
