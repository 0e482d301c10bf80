"""Scenarios and the host yardstick for the wide device tracker (test_track_wide_cpu.py, test_gpu_track_wide.py): up to 256
tracks per stream and 64 cards per frame, on the multi-wave update kernel.

The pieces of track_common are reused by import; its module constants S, K and MAX_TRACKS are not touched: a wide
scenario carries its own stream count, cards per frame and slot count, and `layout` / `run_host` here take them from the
scenario.  Corner coordinates are integer pixels, so ties are exact in fp64.  Unrelated cards sit on a grid of 700 px
pitch: further apart than the 300 px distance threshold, so that nothing matches by accident.

Sizes (T slots, K cards per frame): W2 = (65, 17), W3 = (128, 33), W4 = (256, 64); slot t lives in wave t // 64.
"""
from __future__ import annotations

import copy
import dataclasses
import functools

import numpy as np

from track_common import DT, CappedTracker, Scenario, Step, _Enc, _Seg, _Vecs, ewma32, quad  # noqa: F401 (re-exported)

DIM, BANK_ROWS, TOP_K = 32, 64, 3
SIZES = {"W2": (65, 17), "W3": (128, 33), "W4": (256, 64)}
PITCH = 700
# tracks that survive eight frames without a sighting and get their id on the first re-match (8 <= 10: born initialising)
LONG = dict(period=8, hit_counter_max=15, initialization_delay=10)
# tracks shown every third frame stay (+4 per hit, cap 9), a track that misses its turn is dropped; ids at creation
ROTATE = dict(period=2, hit_counter_max=9, initialization_delay=0)


@dataclasses.dataclass
class WideScenario(Scenario):
    k: int = 64  # cards per frame
    n_streams: int = 3

    def z(self):
        """embeddings (steps, streams, k, DIM) float32: what the encoder would give for the crop in slot k"""
        return np.random.default_rng(2000 + self.seed).standard_normal((len(self.steps), self.n_streams, self.k, DIM)).astype(np.float32)


def grid(n, row0=2):
    """card n of the grid: 32 per row, 700 px pitch, rows from `row0` (rows 0 and 1 are left to a scenario's own cards)"""
    return quad(100 + PITCH * (n % 32), 100 + PITCH * (row0 + n // 32))


def _steps(n, per_stream, streams_of=None, dt=DT, t0=100.0):
    S = len(per_stream)
    out = []
    for i in range(n):
        ss = list(range(S)) if streams_of is None else list(streams_of(i))
        out.append(Step(ss, [t0 + i * dt + 0.001 * s for s in ss], [list(per_stream[s](i)) for s in ss]))
    return out


def _few(s):
    """a light stream beside the heavy one: three drifting cards"""
    return lambda i: [quad(100 + PITCH * c + 3 * i, 120 + 40 * s + 2 * i) for c in range(3)]


# ---- 1. fill: disjoint sets of K cards in rotation until every slot is taken, then one set more --------------------
def fill(size, extra):
    T, K = SIZES[size]
    n_sets = T // K + (1 if extra and T % K else 0)  # W2: 4 sets of 17 = 68 > 65, the fourth set overflows by itself

    def heavy(i):
        if extra and T % K == 0 and i == 2 * n_sets:
            return [grid(n_sets * K + c) for c in range(K)]  # W4: a fifth set finds no slot at all
        r = i % n_sets
        return [grid(r * K + c) for c in range(K)]

    return WideScenario(f"fill_{size}", _steps(2 * n_sets + 3, [_few(0), heavy, _few(2)]), policy=dict(LONG), max_tracks=T, k=K, capped=extra,
                        seed=20 + len(size) + T)


# ---- 2. / 3. ties --------------------------------------------------------------------------------------------------
TIE_P = (3000, 100)  # rows 0 and 1 of the grid are free for these


def ties():
    """stream 0: A (older) in slot 64, B (younger) in the recycled slot 0, one detection in the middle (step 7): A wins.
    stream 1: A (older) in slot 0, B (younger) in slot 64: A wins.  stream 2: three stationary tracks, each in turn with
    two detections at 50 px, at detection indices (15, 16), (31, 32), (62, 63): the lower index wins."""
    a, b, mid = quad(*TIE_P), quad(TIE_P[0] + 100, TIE_P[1]), quad(TIE_P[0] + 50, TIE_P[1])

    def high_older(i):
        if i == 0:
            return [grid(c) for c in range(64)]  # fillers take slots 0..63 and starve: dropped at the start of step 3
        if i < 3:
            return [a]  # born in step 1 into slot 64
        return [mid] if i == 7 else [a, b]  # B born in step 3 into slot 0

    def low_older(i):
        if i == 0:
            return [a] + [grid(c) for c in range(63)]  # A in slot 0, fillers in 1..63
        return [mid] if i == 7 else [a, b]  # B born in step 1 while the fillers still live: slot 64

    P = [(1000, 100), (3000, 100), (5000, 100)]

    def det_ties(i):
        if i in (4, 5, 6):
            j, lo = i - 4, (15, 31, 62)[i - 4]
            p = P[j]
            pair = [quad(p[0] + 50, p[1]), quad(p[0] + 30, p[1] + 40)]
            if j == 1:
                pair.reverse()  # which of the two quads sits at the lower index does not matter: the index does
            d = [grid(c) for c in range(64)]
            d[lo], d[lo + 1] = pair
            for jj in range(j + 1, 3):
                d[jj] = quad(*P[jj])  # the tracks whose turn is still to come stay where they are
            return d
        return [quad(*p) for p in P]

    return WideScenario("ties", _steps(10, [high_older, low_older, det_ties]), max_tracks=256, k=64, seed=31)


# ---- 4. / 6. a full frame: 64 rounds with winners from all waves, ids handed out across waves in one frame -----------
def _off(j):
    return (j * 37) % 41 - 20  # integer displacements, |off| <= 20


def line_card(ln, p, dx=0, dy=0):
    """card p of line ln: 100 px pitch, so a detection is within the threshold of five tracks; the lines are 700 px apart"""
    return quad(100 + 100 * p + dx, 100 + PITCH * ln + dy)


FULL_SHOWN = [(ln, p) for ln in range(3) for p in range(0, 64, 3)][:64]  # every third card of each line: 22 + 22 + 20
FULL_LATE = [(0, 1), (0, 4), (1, 1), (2, 4)]  # cards that are still initialising in step 5


def full():
    """Stream 1.  Step 0: 32 fillers take slots 0..31.  Steps 1..3: the 64 cards of line 0, 1, 2 are born into slots
    32..95, 96..159, 160..223: every line straddles two waves, and detection d of a line is card 2 (d % 32) + d // 32, so
    neighbours on a line live in different waves.  Step 4 shows every third card of each line, displaced: 64 initialising
    tracks in four waves are matched in 64 rounds of phase 1 and get their ids in the order of the matches.  Step 5 shows 60
    of them again (initialised now: phase 0) and four cards whose tracks are still initialising (phase 1)."""

    def heavy(i):
        if i == 0:
            return [grid(c, row0=4) for c in range(32)]
        if i < 4:
            return [line_card(i - 1, 2 * (d % 32) + d // 32) for d in range(64)]
        if i == 4:
            return [line_card(ln, p, _off(p + 7 * ln), 3 * ln) for ln, p in FULL_SHOWN]
        if i == 5:
            return [line_card(ln, p, _off(2 * p + ln) // 2, -2) for ln, p in FULL_SHOWN[:60]] + [line_card(ln, p, 5, 5) for ln, p in FULL_LATE]
        return [line_card(ln, p, 2 * (i - 5), 0) for ln, p in FULL_SHOWN]

    return WideScenario("full", _steps(8, [_few(0), heavy, _few(2)]), policy=dict(LONG), max_tracks=256, k=64, seed=41)


# ---- 5. slot allocation across waves ---------------------------------------------------------------------------------
ALLOC_SLOT_OF_BIRTH = {180: 3, 181: 70, 182: 130, 183: 178}  # the tracks born into recycled slots


def alloc():
    """Stream 1, T = 180 (three waves): three sets of 60 cards in rotation fill every slot (card n: birth n, slot n).  The
    cards of slots 3, 70 and 130 miss their second turn and are dropped; in step 6 three new cards take 3, 70 and 130 in
    ascending detection order.  The card of slot 178 misses step 8 and is dropped in step 10, where the one new card finds
    the only free slot in the last wave."""
    gone = {3: 3, 70: 4, 130: 5, 178: 8}  # card: the step from which it is missing
    joined = {0: [(6, 300), (6, 301), (6, 302)], 1: [(10, 310)]}  # set: (from step, card) shown behind the set's own cards

    def heavy(i):
        r = i % 3
        d = [grid(60 * r + c) for c in range(60) if not (60 * r + c in gone and i >= gone[60 * r + c])]
        return d + [grid(n) for since, n in joined.get(r, []) if i >= since]

    return WideScenario("alloc", _steps(12, [_few(0), heavy, _few(2)]), policy=dict(ROTATE), max_tracks=180, k=64, seed=51)


# ---- 7. layouts with holes over all 64 slots; 8. a NaN corner at a detection index >= 16 -------------------------------
def _drift(s, n):
    return lambda i: [quad(100 + PITCH * (c % 8) + 3 * i, 100 + PITCH * (c // 8) + 40 * s + 2 * i) for c in range(n - (s % 2))]


def holes(mode):
    return WideScenario(f"holes_{mode}", _steps(8, [_drift(s, 24) for s in range(3)]), max_tracks=128, k=64, mode=mode, seed=61 + len(mode))


def nan_high():
    def nan(s):
        def f(i):
            d = list(_drift(s, 20)(i))
            if 3 <= i <= 5:
                q = quad(350, 6000)
                q[1, 0] = np.nan
                d.insert(17, q)
            return d

        return f

    return WideScenario("nan_high", _steps(10, [nan(s) for s in range(3)]), max_tracks=65, k=33, seed=71)


def gating():
    """0.2 s steps with the 0.5 s wait, 40 still cards per stream in 64 slots with holes: due at the id, then every third
    step, and steps in which nothing is due"""
    def still(s):
        return lambda i: [quad(100 + PITCH * (c % 8), 100 + PITCH * (c // 8) + 50 * s) for c in range(40)]

    return WideScenario("gating", _steps(10, [still(s) for s in range(3)], dt=0.2), max_tracks=65, k=64, mode="state", seed=81)


@functools.lru_cache(None)
def scenarios():
    sc = [fill("W2", True), fill("W3", False), fill("W4", True), ties(), full(), alloc(), holes("state"), holes("both"), nan_high(), gating()]
    return {s.name: s for s in sc}


def layout(scn: WideScenario, i: int):
    """track_common.layout for the scenario's own K: quads (F, K, 4, 2), n_det or None, state or None, slot_of_det[f][di]"""
    st, K = scn.steps[i], scn.k
    F = len(st.streams)
    rng = np.random.default_rng(50 + 97 * scn.seed + i)
    quads = np.empty((F, K, 4, 2), np.float32)
    n_det, state, where = np.zeros((F,), np.int32), np.zeros((F, K), np.int32), []
    for f, dets in enumerate(st.dets):
        assert len(dets) <= K
        decoy = dets[0] if dets else quad(200, 200)
        quads[f] = decoy
        if scn.mode == "n_det":
            ks = list(range(len(dets)))
            n_det[f] = len(dets)
        else:
            ks = sorted(rng.choice(K, size=len(dets), replace=False).tolist())
            n_det[f] = (max(ks) + 1) if ks else 0
            if scn.mode == "both" and n_det[f] < K:
                state[f, n_det[f]:] = 1  # valid by state, cut off by n_det
        for k, d in zip(ks, dets):
            quads[f, k] = d
            state[f, k] = 1 + int(rng.integers(0, 2))
        where.append(ks)
    return quads, (None if scn.mode == "state" else n_det), (None if scn.mode == "n_det" else state), where


def _run_host(scn: WideScenario, capped: bool):
    from mtgv.tracker import KalmanPointTracker, TrackerCtx

    S, Z = scn.n_streams, scn.z()
    ctxs, encs, vecs, clocks, births = [], [], [], [], [0] * S
    for s in range(S):
        e, v, c = _Enc(), _Vecs(), [0.0]
        ctx = TrackerCtx(scn.update_wait_sec, scn.ewma_weight, segmenter=lambda fr: [_Seg(q, di) for di, q in enumerate(fr)], encoder=e, vecs=v,
                         clock=(lambda c=c: c[0]), thumbnails=False)
        ctx.tracker = CappedTracker(scn.max_tracks, **scn.policy) if capped else KalmanPointTracker(**scn.policy)
        ctxs.append(ctx), encs.append(e), vecs.append(v), clocks.append(c)
    out, peak = [], [0] * S
    for i, st in enumerate(scn.steps):
        where = layout(scn, i)[3]
        frames = []
        for f, s in enumerate(st.streams):
            ctx = ctxs[s]
            clocks[s][0] = st.now[f]
            encs[s].z = {di: Z[i, s, k] for di, k in enumerate(where[f])}
            vecs[s].queries = []
            before = {t.id: (None if t.avg_z is None else t.avg_z.copy(), t.last_update_time) for t in ctx.tracked_data.values()}
            next_id = ctx.tracker._next_id
            objs = ctx.update(st.dets[f])
            for t in ctx.tracker.tracks:  # new tracks are appended in ascending detection index: the creation order
                if not hasattr(t, "birth"):
                    t.birth = births[s]
                    births[s] += 1
            by_id = {t.id: t.last_detection for t in ctx.tracker.tracks if t.id is not None}
            matched = [(o.id, by_id[o.id]) for o in objs]
            due = [o for o in objs if o.last_update_time == st.now[f]]
            assert len(due) == len(vecs[s].queries) and all((o.avg_z == q).all() for o, q in zip(due, vecs[s].queries))
            peak[s] = max(peak[s], len(ctx.tracker.tracks))
            frames.append(dict(matched=matched, due=[(o.id, by_id[o.id]) for o in due], avg={o.id: o.avg_z.copy() for o in due},
                               prev={o.id: before.get(o.id, (None, None))[0] for o in due}, last={o.id: o.last_update_time for o in objs},
                               tracks=[copy.deepcopy(t) for t in ctx.tracker.tracks], n_live=len(ctx.tracker.tracks),
                               new_ids={t.id: t.birth for t in ctx.tracker.tracks if t.id is not None and t.id >= next_id}))
        out.append(frames)
    return out, peak, [c.tracker for c in ctxs]


@functools.lru_cache(None)
def run_host(name: str, capped=None):
    """track_common.run_host for a wide scenario, once per (scenario, yardstick): per step, per frame a dict (matched, due,
    avg, prev, last, tracks, n_live, new_ids {id given in this frame: birth}); the peak of live tracks per stream; the
    trackers.  Callers do not change what they get."""
    scn = scenarios()[name]
    return _run_host(scn, scn.capped if capped is None else capped)
