"""Shared by test_match_edges_cpu.py and test_gpu_match_edges.py: the cases of the direct test of the bank match
(match.hip, gemm_sp_epi_topk.h, the convert-on-load kernel's fused top-k) at its tile, range and bound edges, their seeded
draws, their fp64 references (oracle/match_ref.py, computed from the f32 inputs) and a restatement of the two-pass match's
fp16 first pass.  No GPU needed here.

Paths.  "split": one pass on the split kernel (f16x3 mode, b >= 128, N >= 192; 128 x 192 tile, one candidate group per
96-column wave range).  "col": one pass on the convert-on-load kernel (f32 mode at b >= 128, b < 128 in either mode; one
group per 64-column tile).  "two": fp16 first pass + exact re-rank (f16x3 mode, b >= 128, K % 64 == 0, N >= 4096, k <= 4).

The first pass restated (first_pass): rows and queries normalised in f32 as l2norm_rows_kernel does it (l2norm_f32 follows
its summation order, so the result is meant to equal the device's bit for bit - the GPU test checks that on the stored
rows); a bank row times the power of two that sp8_pack_rows_kernel picks (row maximum in [2^13, 2^14)); both operands rounded
to fp16; products summed in fp64; un-scaled.  The kernel sums the same (exact) products in f32.

Judging (judge): a probe query returns the oracle's ids in order on its planted ranks; every other (query, rank) returns
the oracle's id where the fp64 gaps to both neighbouring ranks exceed ID_MARGIN = 2e-5 - which holds every query to exact
ids whose smallest gap among its top k + 1 exceeds 2e-5, test_gpu_match._check's rule, and a query with one near-tie still
to exact ids on its other ranks; elsewhere the returned id's fp64 score must explain the rank within SCORE_TOL = 2e-6, the
bound the existing match tests hold f32 accumulation of unit vectors to.  Returned scores: within SCORE_TOL everywhere.
weak_fraction() is the share of a case's queries with a gap <= ID_MARGIN among their top k + 1; the cap of 5 % is held by
every case with k <= 16, by its seed (among 0..7; the k = 16 cases with many queries measure 0.039, 0.043, 0.031, 0.039 and
0.008, every other case at most 0.016).  At k = 70 and 100 no seed holds it: the top 71 or 101 of at most 383 N(0, 1/K)
scores lie about 1e-3 apart on average, so a gap below 2e-5 somewhere among them is the rule (0.44 to 0.88 of the queries
over seeds 0..7 in the four such cases with 128 or more queries; the three of one or three queries reach 0 at some seeds,
which says nothing at that batch size) - which is why the judgement is per rank, and at k >= 70 the share of (query, rank) slots under the weaker rule is
capped at 5 % instead (measured: at most 0.037).

Planted probes: the probe queries are rows 0, 31, 32, 127, 128 and b - 1 of the batch where they exist; each has its top
p = min(k + 1, N // (probes + 1)) rows planted at cosines 0.9, 0.9 - 2e-5, ... (p = k + 1 wherever the bank has the rows for
it), on the delicate columns first: N - 1, 0, 95, 96, 191, 192, the first column of the last candidate group."""
import functools
from collections import namedtuple

import numpy as np

from oracle import match_ref as M

PRE_KP, PRE_R, PRE_EPS = 2, 8, 1.1e-3  # match.hip
RANGE = 96       # columns per candidate group of the split kernel (a wave range of the 128 x 192 tile)
COL_GROUP = 64   # of the convert-on-load kernel (its 128 x 64 top-k tile)
ID_MARGIN = 2e-5
SCORE_TOL = 2e-6
WEAK_CAP = 0.05
STEP = 2e-5      # spacing of planted cosines
TOP = 0.9
SP_OF = {"split": 1, "col": 0, "two": 3}  # the launch profiler's sp column

Case = namedtuple("Case", "name path mode N K b k seed")


def _cases(path, rows):
    """rows: (N, K, b, k, seed[, mode]); the seeds are among 0..7, chosen per case where the near-tie cap needs it"""
    out = []
    for r in rows:
        N, K, b, k, seed = r[:5]
        mode = r[5] if len(r) > 5 else "f16x3"
        out.append(Case(f"{path}-N{N}-K{K}-b{b}-k{k}-{mode}", path, mode, N, K, b, k, seed))
    return out


TABLE = {
    "split": dict(N=(192, 193, 288, 289, 383), K=(64, 72, 200), b=(128, 129, 257), k=(1, 4, 16, 100)),
    "col": dict(N=(63, 64, 65, 130, 193), K=(32, 72), b=(1, 3, 127, 129), k=(1, 16, 70)),
    "two": dict(N=(4096, 4128, 4129, 4224), K=(64, 128), b=(128, 131), k=(1, 3, 4)),
}
CASES = (
    _cases("split", [(192, 64, 128, 1, 0), (193, 72, 128, 4, 1), (288, 200, 129, 16, 6), (289, 72, 257, 100, 3), (383, 64, 129, 100, 4),
                     (383, 200, 257, 4, 5), (192, 72, 257, 16, 5), (193, 200, 128, 100, 7), (289, 64, 128, 4, 0), (288, 72, 129, 1, 1),
                     (193, 64, 257, 1, 2), (383, 72, 128, 16, 0)])
    + _cases("col", [(63, 32, 1, 16, 0), (63, 72, 127, 1, 1, "f32"), (64, 72, 3, 16, 2, "f32"), (64, 32, 129, 1, 3, "f32"),
                     (65, 72, 129, 16, 1, "f32"), (65, 32, 3, 70, 5), (63, 72, 3, 70, 6), (130, 72, 127, 16, 0), (130, 32, 1, 70, 0, "f32"),
                     (193, 72, 129, 70, 1, "f32"), (193, 32, 127, 1, 2), (193, 72, 3, 16, 3)])
    + _cases("two", [(4096, 64, 128, 1, 0), (4096, 128, 131, 4, 1), (4128, 64, 131, 3, 2), (4128, 128, 128, 1, 3), (4129, 64, 128, 4, 4),
                     (4129, 128, 131, 3, 5), (4129, 64, 131, 1, 6), (4224, 128, 128, 4, 7), (4224, 64, 131, 3, 0), (4096, 64, 131, 3, 1),
                     (4224, 128, 131, 1, 2), (4128, 128, 128, 4, 3)])
)
BY_NAME = {c.name: c for c in CASES}


def group_cols(path):
    return COL_GROUP if path == "col" else RANGE


def expected_topk(c):
    """the topk column of the one GEMM row the launch profiler must show"""
    return PRE_KP if c.path == "two" else min(c.k, group_cols(c.path))


def slots_of(N):
    """candidate ranges of the first pass: two per 192-column tile, the last ones possibly short or empty"""
    return -(-N // (2 * RANGE)) * 2


def probes_of(b):
    return sorted({p for p in (0, 31, 32, 127, 128, b - 1) if 0 <= p < b})


def delicate_columns(N, path):
    g = group_cols(path)
    first_last = (N - 1) // g * g
    out = []
    for col in (N - 1, 0, 95, 96, 191, 192, first_last):
        if 0 <= col < N and col not in out:
            out.append(col)
    return out


# ---- draws ----
def _unit64(q):
    q = np.asarray(q, np.float64)
    return q / np.sqrt((q * q).sum())


def planted_row(qh, c, rng):
    """c qh + sqrt(1 - c^2) u with u a random unit vector orthogonal to the unit vector qh (fp64), as f32"""
    g = rng.standard_normal(qh.shape[0])
    u = g - (g @ qh) * qh
    u /= np.sqrt((u * u).sum())
    return (c * qh + np.sqrt(1.0 - c * c) * u).astype(np.float32)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def draw(name):
    """(q f32 [b][K], bank f32 [N][K], plan): plan[probe] = the planted columns in rank order"""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    bank = rng.standard_normal((c.N, c.K)).astype(np.float32)
    q = (rng.standard_normal((c.b, c.K)) * 2).astype(np.float32)
    probes = probes_of(c.b)
    p = min(c.k + 1, c.N // (len(probes) + 1))
    deli = delicate_columns(c.N, c.path)
    cols = {pr: [] for pr in probes}
    for i, col in enumerate(deli):  # rank 1 of probe 0 at N - 1, of probe 1 at column 0; the others take the next free rank in turn
        pr = probes[i % len(probes)]
        if len(cols[pr]) < p:
            cols[pr].append(col)
    used = {col for v in cols.values() for col in v}
    free = [int(x) for x in rng.permutation(c.N) if int(x) not in used]
    for pr in probes:
        while len(cols[pr]) < p:
            cols[pr].append(free.pop())
    for pr in probes:
        qh = _unit64(q[pr])
        for j, col in enumerate(cols[pr]):
            bank[col] = planted_row(qh, TOP - STEP * j, rng)
    _freeze(q, bank)
    return q, bank, {pr: tuple(v) for pr, v in cols.items()}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(fp64 scores [b][N], oracle ids [b][k], oracle scores [b][k]) - pads id -1 / -inf where k > N"""
    q, bank, _ = _draw_any(name)
    k = _k_any(name)
    s = M.scores(q, bank)
    ids, sc = M.topk_from_scores(s, k)
    _freeze(s, ids, sc)
    return s, ids, sc


def planted_margin(name):
    """smallest fp64 gap between a probe's lowest planted row and its best row that is not planted for it"""
    c = BY_NAME[name]
    _, _, plan = draw(name)
    s, _, _ = oracle(name)
    worst = np.inf
    for pr, cols in plan.items():
        rest = np.delete(s[pr], list(cols))
        worst = min(worst, s[pr, list(cols)].min() - (rest.max() if rest.size else -np.inf))
    return worst


# ---- judging ----
def rank_gaps(s, k):
    """fp64 [b][kk] each: gap from rank r to rank r - 1 and to rank r + 1 (inf at the ends), kk = min(k, N)"""
    b, n = s.shape
    kk = min(k, n)
    top = -np.sort(-s, axis=1)[:, : kk + 1]
    d = top[:, :-1] - top[:, 1:]  # d[r] = s_r - s_(r+1), r < top.shape[1] - 1
    nxt = np.full((b, kk), np.inf)
    nxt[:, : d.shape[1]] = d[:, :kk]
    prv = np.full((b, kk), np.inf)
    prv[:, 1:] = d[:, : kk - 1]
    return prv, nxt


def planted_ranks(cols, k, n):
    """how many of a probe's leading ranks are judged against its plan: the planted ranks with a planted row below them"""
    return min(len(cols) - 1, k, n)


def exact_ranks(s, k, plan=None):
    """bool [b][kk]: the ranks whose id is judged exactly - a probe's planted ranks always (their gaps are STEP by
    construction: planted_gap() holds them above STEP / 2), any other rank where both gaps exceed ID_MARGIN"""
    prv, nxt = rank_gaps(s, k)
    exact = (prv > ID_MARGIN) & (nxt > ID_MARGIN)
    for pr, cols in (plan or {}).items():
        exact[pr, : planted_ranks(cols, k, s.shape[1])] = True
    return exact


def weak_fraction(s, k, plan=None):
    """share of queries with a rank judged by score only; without probes: the queries with a gap <= ID_MARGIN among their
    top k + 1, those test_gpu_match._check's rule judges by score"""
    return float((~exact_ranks(s, k, plan).all(axis=1)).mean())


def weak_slot_fraction(s, k, plan=None):
    return float((~exact_ranks(s, k, plan)).mean())


def planted_gap(s, plan):
    """smallest fp64 gap between consecutive planted rows of a probe"""
    return min(float(-np.diff(s[pr, list(cols)]).max()) for pr, cols in plan.items() if len(cols) > 1)


def judge(s, rid, rsc, ids, sc, k, plan=None, id_base=0):
    """asserts the judging rule of the module docstring on a result (ids int64 [b][k], sc f32 [b][k]); returns the largest
    |score - oracle score|"""
    b, n = s.shape
    kk = min(k, n)
    ids = np.asarray(ids)
    sc = np.asarray(sc)
    assert ids.shape == (b, k) and sc.shape == (b, k)
    assert (ids[:, kk:] == -1).all() and np.isneginf(sc[:, kk:]).all(), "slots beyond the bank's rows must be pads"
    got = ids[:, :kk] - id_base
    assert ((got >= 0) & (got < n)).all(), "an id outside the bank (or a pad where a row exists)"
    exact = exact_ranks(s, k, plan)
    for pr, cols in (plan or {}).items():
        m = planted_ranks(cols, k, n)
        assert got[pr, :m].tolist() == list(cols[:m]) == rid[pr, :m].tolist(), (pr, got[pr, :m].tolist(), cols[:m])
    bad = exact & (got != rid[:, :kk])
    assert not bad.any(), ("ids differ from the oracle outside near-ties", np.argwhere(bad)[:8].tolist())
    for r in range(b):
        assert len(set(got[r].tolist())) == kk, ("a row returned twice", r)
    explained = np.abs(np.take_along_axis(s, got, axis=1) - rsc[:, :kk])
    assert explained.max() < SCORE_TOL, explained.max()
    err = np.abs(sc[:, :kk].astype(np.float64) - rsc[:, :kk])
    assert err.max() < SCORE_TOL, err.max()
    assert (np.diff(sc[:, :kk], axis=1) <= 0).all()
    return float(err.max())


# ---- the first pass restated ----
def l2norm_f32(x):
    """rows / max(|row|, 1e-12) in f32, summed as l2norm_rows_kernel sums: lane l accumulates x[l], x[l + 64], ... with
    fused multiply-adds, then a 64-lane butterfly"""
    x = np.ascontiguousarray(x, np.float32)
    rows, d = x.shape
    sq = np.zeros((rows, 64), np.float32)
    for i0 in range(0, d, 64):
        w = min(64, d - i0)
        ch = x[:, i0 : i0 + w].astype(np.float64)
        sq[:, :w] = (ch * ch + sq[:, :w].astype(np.float64)).astype(np.float32)  # the product of two f32 is exact in fp64
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        sq = sq + sq[:, lanes ^ m]
    nrm = np.maximum(np.sqrt(sq[:, :1]), np.float32(1e-12))
    assert nrm.dtype == np.float32
    return x / nrm


def row_scale(bn):
    """the power of two sp8_pack_rows_kernel multiplies a (normalised, f32) row by: its maximum lands in [2^13, 2^14)"""
    mx = np.abs(bn).max(axis=1)
    _, ex = np.frexp(mx)
    e = np.where(mx > 0, np.clip(14 - ex, -100, 100), 0)
    return np.ldexp(np.float32(1.0), e).astype(np.float32)


def first_pass(q, bank):
    """approximate scores fp64 [b][N] of the fp16 x fp16 first pass"""
    qn = l2norm_f32(q)
    bn = l2norm_f32(bank)
    sc = row_scale(bn)
    q16 = qn.astype(np.float16).astype(np.float64)
    b16 = (bn * sc[:, None]).astype(np.float16).astype(np.float64)
    return (q16 @ b16.T) / sc.astype(np.float64)[None, :]


def range_candidates(approx):
    """(scores fp64 [b][slots][PRE_KP], columns int [b][slots][PRE_KP], in-range margin fp64 [b][slots][PRE_KP]): per range
    its PRE_KP best approximate scores (score desc, column asc), pads (-inf, -1); margin[j] = gap from reported entry j to
    the next best score of the range (inf where there is none)"""
    b, n = approx.shape
    slots = slots_of(n)
    pad = np.full((b, slots * RANGE), -np.inf)
    pad[:, :n] = approx
    pad = pad.reshape(b, slots, RANGE)
    order = np.argsort(-pad, axis=2, kind="stable")[:, :, : PRE_KP + 1]
    top = np.take_along_axis(pad, order, axis=2)
    cols = order[:, :, :PRE_KP] + (np.arange(slots) * RANGE)[None, :, None]
    cs = top[:, :, :PRE_KP]
    cols = np.where(np.isneginf(cs), -1, cols)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isneginf(top[:, :, 1:]), np.inf, top[:, :, :PRE_KP] - top[:, :, 1:])
    margin = np.where(np.isneginf(cs), np.inf, margin)
    return cs, cols, margin


def proof_slack(approx, s, k):
    """per query: s_kth - max(a_R, cut) as rerank_kernel forms it from the restated candidates (fp64 [b]) - the proof holds
    where this exceeds PRE_EPS, the query is scanned where it does not - and the re-ranked columns [b][PRE_R]"""
    cs, cols, _ = range_candidates(approx)
    b = approx.shape[0]
    cut = cs[:, :, PRE_KP - 1].max(axis=1)
    flat_s, flat_c = cs.reshape(b, -1), cols.reshape(b, -1)
    slack = np.empty(b)
    sel = np.empty((b, PRE_R), np.int64)
    for r in range(b):
        order = np.lexsort((flat_c[r], -flat_s[r]))[:PRE_R]  # score desc, column asc; pads (-inf) last
        sel[r] = flat_c[r][order]
        a_r = flat_s[r][order[-1]]
        ex = np.sort(s[r, sel[r][sel[r] >= 0]].astype(np.float32))[::-1]
        kth = ex[k - 1] if ex.size >= k else -np.inf
        slack[r] = kth - max(a_r, cut[r])
    return slack, sel


# ---- cluster cases (two-pass): 12 rows 2e-5 apart in exact cosine, scrambled by the fp16 pass ----
CLUSTER_N, CLUSTER_B, CLUSTER_Q, DUP_Q = 4096, 128, 31, 127
CLUSTER_KS = (1, 3, 4)
LAST_RANGE0 = (CLUSTER_N - 1) // RANGE * RANGE  # 4032: the last, partial range holds 64 columns
PLACEMENTS = {
    "one-range": tuple(480 + 7 * i + 3 for i in range(12)),                 # all inside range 5
    "twelve-ranges": tuple(RANGE * (2 + 3 * i) + (7 * i) % RANGE for i in range(12)),
    "straddle-last": tuple(range(LAST_RANGE0 - 6, LAST_RANGE0 + 6)),       # six columns on either side of the boundary
}
DUP_COLS = (4090, 4040, 4063, 4095)  # exact duplicates in the last partial range, more than PRE_KP of them
CLUSTER_SEED = {64: 4, 128: 0}  # the draws whose fp16 pass misorders the cluster's best k + 1 = 5 rows (test_match_edges_cpu)
Cluster = namedtuple("Cluster", "name K placement")
CLUSTERS = [Cluster(f"cluster-K{K}-{p}", K, p) for K in (64, 128) for p in PLACEMENTS]
CLUSTER_BY_NAME = {c.name: c for c in CLUSTERS}


@functools.lru_cache(maxsize=None)
def cluster_draw(name):
    """(q, bank, cluster columns in exact rank order, duplicate columns ascending)"""
    c = CLUSTER_BY_NAME[name]
    rng = np.random.default_rng(CLUSTER_SEED[c.K])
    bank = rng.standard_normal((CLUSTER_N, c.K)).astype(np.float32)
    q = (rng.standard_normal((CLUSTER_B, c.K)) * 2).astype(np.float32)
    cols = [int(x) for x in rng.permutation(np.array(PLACEMENTS[c.placement]))]  # ranks do not follow the columns
    qh = _unit64(q[CLUSTER_Q])
    for j, col in enumerate(cols):
        bank[col] = planted_row(qh, TOP - STEP * j, rng)
    dup = planted_row(_unit64(q[DUP_Q]), 0.95, rng)
    for col in DUP_COLS:
        bank[col] = dup
    _freeze(q, bank)
    return q, bank, tuple(cols), tuple(sorted(DUP_COLS))


# ---- bound case (two-pass, K = 64, k = 1): the winner is hidden and the proof's slack lies inside (PRE_EPS / 2, PRE_EPS) ----
BOUND_N, BOUND_B, BOUND_K, BOUND_Q = 4096, 128, 64, 32
BOUND_W, BOUND_H, BOUND_D = 1950, (1925, 2000), 100  # W and its two hiders in range 20, D in range 1
BOUND_SLACK = 6.2e-4                                  # aimed at: above PRE_EPS / 2 = 5.5e-4 with room for the f32 sums
Bound = namedtuple("Bound", "q bank n c deficit slack gap")


def _sparse_row(n, c, K):
    """c q^ + sqrt(1 - c^2) e_n for q^ = n components of 1 / sqrt(n): W's shape, its component along q^ the same fp16
    rounding n times over"""
    w = np.zeros(K, np.float64)
    w[:n] = c / np.sqrt(n)
    w[n] = np.sqrt(1.0 - c * c)
    return w.astype(np.float32)


def _tune(make, value, lo, hi, target, tol):
    """c in [lo, hi] with |value(make(c)) - target| <= tol, by bisection on the trend and a scan of the last interval"""
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if value(make(mid)) < target:
            lo = mid
        else:
            hi = mid
    for c in np.linspace(lo - 2e-5, hi + 2e-5, 201):
        if abs(value(make(c)) - target) <= tol:
            return c
    raise AssertionError("no row hits the target")


@functools.lru_cache(maxsize=None)
def bound_case():
    """W = c q^ + sqrt(1 - c^2) e_n for the sparse-constant query q^ (n components of 1 / sqrt(n)), n and c found by scanning
    n in [2, 62] and c in [0.80, 0.99] for the largest exact - approximate score; two hiders of its range tuned to approximate
    scores just above W's; D elsewhere tuned to an exact score BOUND_SLACK above the lower hider's approximate score; every
    other query with a clear winner of its own.
    Measured (restatement, seed 0; the device's first pass agrees with the restatement to 1e-7): n = 62, c = 0.9876, W's
    deficit 8.31e-4, slack s_kth - max(a_R, cut) = 6.15e-4, W's exact score 1.85e-4 above D's, every other query's slack
    above 0.31.  The hiders and D lose about 4e-4 themselves: the query's fp16 rounding is common to every row, so D's
    approximate score cannot sit beside its exact score - what the proof sees is D's exact score and the hiders' approximate ones."""
    K = BOUND_K
    rng = np.random.default_rng(0)
    # the sparse-constant query and W's component along it whose fp16 roundings lose the most
    best = (-1.0, 0, 0.0)
    cs = np.arange(0.80, 0.99, 1e-4)
    for n in range(2, K - 1):
        q = np.zeros((1, K), np.float32)
        q[0, :n] = 1.0
        rows = np.stack([_sparse_row(n, c, K) for c in cs])
        d = (M.scores(q, rows) - first_pass(q, rows))[0]
        j = int(d.argmax())
        if d[j] > best[0]:
            best = (float(d[j]), n, float(cs[j]))
    deficit, n, c = best
    bank = rng.standard_normal((BOUND_N, K)).astype(np.float32)
    q = (rng.standard_normal((BOUND_B, K)) * 2).astype(np.float32)
    q[BOUND_Q] = 0.0
    q[BOUND_Q, :n] = 1.0
    qx = q[BOUND_Q : BOUND_Q + 1]
    qh = _unit64(q[BOUND_Q])
    for j in range(BOUND_B):  # every other query has a clear winner outside the ranges of W and D: its proof holds
        if j != BOUND_Q:
            bank[2100 + 13 * j] = planted_row(_unit64(q[j]), 0.8, rng)
    W = _sparse_row(n, c, K)
    bank[BOUND_W] = W
    eW = float(M.scores(qx, W[None])[0, 0])
    aW = float(first_pass(qx, W[None])[0, 0])

    def approx_of(row):
        return float(first_pass(qx, row[None])[0, 0])

    def exact_of(row):
        return float(M.scores(qx, row[None])[0, 0])

    for i, col in enumerate(BOUND_H):  # approximately just above W, exactly below it
        g = rng.standard_normal(K)
        u = g - (g @ qh) * qh
        u /= np.sqrt((u * u).sum())
        make = lambda cc, u=u: (cc * qh + np.sqrt(1.0 - cc * cc) * u).astype(np.float32)
        bank[col] = make(_tune(make, approx_of, 0.7, 0.999, aW + 3e-5 + 2e-5 * i, 6e-6))
    cut = min(approx_of(bank[col]) for col in BOUND_H)
    g = rng.standard_normal(K)
    u = g - (g @ qh) * qh
    u /= np.sqrt((u * u).sum())
    make = lambda cc: (cc * qh + np.sqrt(1.0 - cc * cc) * u).astype(np.float32)
    bank[BOUND_D] = make(_tune(make, exact_of, 0.7, 0.999, cut + BOUND_SLACK, 5e-6))
    _freeze(q, bank)
    approx = first_pass(q, bank)
    s = M.scores(q, bank)
    slack, _ = proof_slack(approx, s, 1)
    return Bound(q, bank, n, c, deficit, slack, eW - float(s[BOUND_Q, BOUND_D]))


# ---- a_R case: the winner IS reported, but nine reported rows of other ranges score approximately higher, so it is not among
# the PRE_R re-ranked; every range's cut-off is a random row's.  Only the a_R term of the bound sends the block to the scan. ----
AR_DECOYS = tuple(RANGE * (2 + 2 * i) + 5 * i for i in range(PRE_R + 1))  # nine rows in ranges 2, 4, ..., 18, none W's or a query's winner


@functools.lru_cache(maxsize=None)
def ar_case():
    """(q, bank): the bound case's queries and bank with W alone in its range (its hiders and D are random rows again) and
    the decoys at exact cosines 1.0e-4, 1.1e-4, ... below W's"""
    bc = bound_case()
    rng = np.random.default_rng(1)
    q, bank = bc.q, bc.bank.copy()
    qx = q[BOUND_Q : BOUND_Q + 1]
    qh = _unit64(q[BOUND_Q])
    for col in BOUND_H + (BOUND_D,):
        bank[col] = rng.standard_normal(BOUND_K).astype(np.float32)
    eW = float(M.scores(qx, bank[BOUND_W][None])[0, 0])
    for i, col in enumerate(AR_DECOYS):
        g = rng.standard_normal(BOUND_K)
        u = g - (g @ qh) * qh
        u /= np.sqrt((u * u).sum())
        make = lambda cc, u=u: (cc * qh + np.sqrt(1.0 - cc * cc) * u).astype(np.float32)
        bank[col] = make(_tune(make, lambda row: float(M.scores(qx, row[None])[0, 0]), 0.7, 0.999, eW - 1.0e-4 - 1e-5 * i, 4e-6))
    _freeze(bank)
    return q, bank


def _draw_any(name):
    if name in BY_NAME:
        return draw(name)
    if name in CLUSTER_BY_NAME:
        return cluster_draw(name)[:2] + (None,)
    if name == "a_R":
        return ar_case() + (None,)
    assert name == "bound"
    bc = bound_case()
    return bc.q, bc.bank, None


def _k_any(name):
    return BY_NAME[name].k if name in BY_NAME else 4 if name in CLUSTER_BY_NAME else 1
