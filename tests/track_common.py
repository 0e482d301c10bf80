"""Scenarios and the host yardstick for the device tracker tests (test_track_cpu.py, test_gpu_track.py).

A scenario is a list of steps; a step names the streams it carries (in the order of its frames), one clock per frame and
each frame's detection list.  `run_host` feeds every stream's frames to a `mtgv.tracker.TrackerCtx` of its own (the
existing host code: KalmanPointTracker + the gating + the EWMA) and records what the device has to reproduce.  Corner
coordinates are integer pixels, so the tie cases are exact in fp64.  `ewma32` is the float32 restatement of the EWMA.
"""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

S, K, DIM, BANK_ROWS, TOP_K, MAX_TRACKS = 3, 4, 32, 64, 3, 8
DT = 1.0 / 30.0


def quad(cx, cy, w=80, h=120):
    return np.array([[cx - w / 2, cy - h / 2], [cx + w / 2, cy - h / 2], [cx + w / 2, cy + h / 2], [cx - w / 2, cy + h / 2]], np.float32)


@dataclasses.dataclass
class Step:
    streams: list  # stream of each frame
    now: list  # clock of each frame
    dets: list  # per frame: list of (4, 2) float32 quads, the frame's detection list


@dataclasses.dataclass
class Scenario:
    name: str
    steps: list
    policy: dict = dataclasses.field(default_factory=dict)  # KalmanPointTracker's arguments
    update_wait_sec: float = 0.5
    ewma_weight: float = 0.1
    max_tracks: int = MAX_TRACKS
    mode: str = "n_det"  # how the detection list is laid out in the K slots: "n_det" (a prefix), "state" (holes), "both"
    capped: bool = False  # (j): the yardstick is the host tracker with the slot limit
    seed: int = 0

    def z(self):
        """embeddings (steps, S, K, DIM) float32: what the encoder would give for the crop in slot k"""
        return np.random.default_rng(1000 + self.seed).standard_normal((len(self.steps), S, K, DIM)).astype(np.float32)


def _steps(n, per_stream, streams_of=None, dt=DT, t0=100.0):
    """per_stream[s](i) -> detection list of stream s in frame i; streams_of(i) -> the streams of step i in frame order"""
    out = []
    for i in range(n):
        ss = list(range(S)) if streams_of is None else list(streams_of(i))
        out.append(Step(ss, [t0 + i * dt + 0.001 * s for s in ss], [list(per_stream[s](i)) for s in ss]))
    return out


def _scenarios():
    P = (200, 200)
    sc = []

    # (a) steady drift of 2-3 cards per stream
    def drift(s):
        return lambda i: [quad(100 + 150 * c + 3 * i, 120 + 40 * s + 2 * i + 150 * (c % 2)) for c in range(2 + (s % 2))]

    sc.append(Scenario("a_drift", _steps(12, [drift(s) for s in range(S)]), seed=1))

    # (b) births and drop-outs of 1..7 frames: short gaps are bridged by the prediction, a long one ends the track
    def gaps(s):
        gone = {0: set(range(5, 6)) | set(range(8, 11)), 1: set(range(6, 13)), 2: set(range(4, 9))}[s]  # 1 + 3, 7, 5 frames

        def f(i):
            d = [quad(120 + 4 * i, 150 + 30 * s)]
            if i not in gone:
                d.append(quad(420 - 3 * i, 400))
            if i >= 3 + s:
                d.append(quad(300, 100 + 2 * i))  # a late birth
            return d

        return f

    sc.append(Scenario("b_gaps", _steps(16, [gaps(s) for s in range(S)]), mode="state", seed=2))

    # (c) exact ties.  Stationary tracks keep their position exactly (innovation 0), so the distances below are exact.
    def tie_dets(i):  # one initialised track at P; then two detections 50 px from it: the lower detection index wins
        if i < 4:
            return [quad(*P)]
        if i == 4:
            return [quad(P[0] + 50, P[1]), quad(P[0] + 30, P[1] + 40)]
        return [quad(P[0] + 30, P[1] + 40), quad(P[0] + 50, P[1])] if i == 5 else [quad(*P)]

    def tie_tracks(i):  # two initialised tracks 100 px apart, one detection in the middle: the older track wins
        if i < 4:
            return [quad(*P), quad(P[0] + 100, P[1])]
        return [quad(P[0] + 50, P[1])] if i == 4 else [quad(*P), quad(P[0] + 100, P[1])]

    def tie_phase(i):  # A (older) is still initialising, B (younger) initialised; equal distance: the initialised one goes first
        a, b, mid = quad(*P), quad(P[0] + 100, P[1]), quad(P[0] + 50, P[1])
        return {0: [a], 1: [a, b], 2: [b], 3: [b], 4: [mid]}.get(i, [b])

    sc.append(Scenario("c_ties", _steps(10, [tie_dets, tie_tracks, tie_phase]), seed=3))

    # (d) a detection at distance exactly 300 (not admitted: `<` is strict), then one just below
    def thr(s):
        def f(i):
            if i < 4:
                return [quad(*P)]
            if i == 4:
                return [quad(P[0] + 180, P[1] + 240)]
            if i == 5:
                return [quad(P[0] + 180, P[1] + 239)]
            return [quad(P[0] + 180, P[1] + 239), quad(*P)]

        return f

    sc.append(Scenario("d_threshold", _steps(10, [thr(s) for s in range(S)]), seed=4))

    # (e) slot recycling: A, B born together; A dies; C is born into A's (lower) slot; then B and C tie for one detection
    def recycle(s):
        a, b, c, mid = quad(100, 100), quad(500, 300), quad(600, 300), quad(550, 300)

        def f(i):
            if i < 2:
                return [a, b]
            if i < 9:
                return [b]  # A starves and is dropped
            if i < 13:
                return [b, c]  # C takes the free slot 0 and gets its id
            return [mid] if i == 13 else [b, c]

        return f

    sc.append(Scenario("e_recycle", _steps(16, [recycle(s) for s in range(S)]), seed=5))

    # (f) no initialisation delay; and a period beyond the delay: both give the id at creation
    sc.append(Scenario("f_delay0", _steps(10, [gaps(s) for s in range(S)]), policy=dict(initialization_delay=0, period=1), seed=6))
    sc.append(Scenario("f_period3", _steps(10, [gaps(s) for s in range(S)]), policy=dict(initialization_delay=2, period=3), mode="both", seed=7))

    # (g) one quad with a NaN corner among ordinary ones: it never matches and its track dies on its own
    def nan(s):
        def f(i):
            d = list(drift(s)(i))
            if 3 <= i <= 5:
                q = quad(350, 350)
                q[1, 0] = np.nan
                d.insert(1, q)
            return d

        return f

    sc.append(Scenario("g_nan", _steps(11, [nan(s) for s in range(S)]), seed=8))

    # (h) the frames of a step in permuted stream order, and steps that carry only two of the three streams
    orders = [(2, 0, 1), (1, 2), (0, 1, 2), (2, 1), (1, 0, 2), (0, 2)]
    sc.append(Scenario("h_order", _steps(14, [gaps(s) for s in range(S)], streams_of=lambda i: orders[i % len(orders)]), mode="state", seed=9))

    # (i) gating: 0.2 s clock steps with the 0.5 s wait - a track is due when it gets its id, then every third step, and
    # there are steps in which nothing is due
    def still(s):
        return lambda i: [quad(150 + 200 * c, 200 + 50 * s) for c in range(2)]

    sc.append(Scenario("i_gating", _steps(14, [still(s) for s in range(S)], dt=0.2), seed=10))

    # (j) overflow: stream 1 gets 4 detections that jump by more than 300 px every frame with 4 slots; streams 0 and 2 run on
    def jump(i):
        return [quad(1000 * (i % 5) + 100 + 2000 * c, 5000 * (i % 7) + 100) for c in range(4)]

    sc.append(Scenario("j_overflow", _steps(12, [drift(0), jump, drift(2)]), max_tracks=4, capped=True, seed=11))
    return sc


SCENARIOS = {s.name: s for s in _scenarios()}


def layout(scn: Scenario, i: int):
    """step i as the device sees it: quads (F, K, 4, 2) float32, n_det (F,) int32 or None, state (F, K) int32 or None, and
    slot_of_det[f][di] = k.  Slots that are no detection hold a quad that sits right on a real card: using one shows."""
    st = scn.steps[i]
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
            n_det[f] = (max(ks) + 1) if ks else 0  # "both": a prefix bound and holes inside it
            if scn.mode == "both" and n_det[f] < K:
                state[f, n_det[f]:] = 1  # valid by state, cut off by n_det
        for k, d in zip(ks, dets):
            quads[f, k] = d
            state[f, k] = 1 + int(rng.integers(0, 2))
        where.append(ks)
    return quads, (None if scn.mode == "state" else n_det), (None if scn.mode == "n_det" else state), where


def output_keys(quad_source, tracked=False, sources=False, thumbs=False):
    """(keys of the dict that Pipeline.run or - tracked - TrackedPipeline.run returns, keys of its "det"), as the code
    returned them when the crop stage still wrote its quads into the detector's dict: the detector's own outputs, quads and
    card_state for "obb", quads_src for SourceFrames, the thumbnails with a thumbnail quality"""
    out = {"ids", "scores", "n_det", "boxes", "crops", "det"}
    out |= {"track_ids", "n_due", "due_idx", "quads"} if tracked else {"z"}
    det = {"n_det", "conf", "cls", "keep_idx"} | ({"rboxes"} if quad_source == "obb" else {"boxes", "mask_logits"})
    if quad_source == "obb":
        out, det = out | {"quads", "card_state"}, det | {"quads", "card_state"}
    if sources:
        out, det = out | {"quads_src"}, det | {"quads_src"}
    if thumbs:
        out |= {"thumbs", "thumb_offsets"}
    return out, det


def ewma32(prev, z, w):
    """TrackerCtx's `avg = w * z + (1 - w) * avg` on float32 vectors, restated with explicit float32 scalars (a Python
    float times a float32 array is a float32 product with the scalar rounded to float32); prev None: avg starts as z"""
    z = np.asarray(z, np.float32)
    prev = z if prev is None else np.asarray(prev, np.float32)
    return np.float32(w) * z + np.float32(1 - w) * prev


class CappedTracker:
    """KalmanPointTracker with the device's one limit: an unmatched detection that finds `max_tracks` tracks alive is
    dropped (and counted).  Everything else is the host class's own code."""

    def __new__(cls, max_tracks, **policy):
        from mtgv.tracker import KalmanPointTracker, _KalmanTrack

        class _Capped(KalmanPointTracker):
            dropped = 0

            def update(self, detections):
                self.tracks = [t for t in self.tracks if t.hit_counter >= 0]
                for t in self.tracks:
                    t.last_detection = -1
                    t.step()
                free = list(range(len(detections)))
                free = self._match([t for t in self.tracks if not t.is_initializing], detections, free)
                free = self._match([t for t in self.tracks if t.is_initializing], detections, free)
                for di in free:
                    if len(self.tracks) >= max_tracks:
                        self.dropped += 1
                        continue
                    t = _KalmanTrack(detections[di], self.period, self.initialization_delay)
                    if not t.is_initializing:
                        t.id = self._next_id
                        self._next_id += 1
                    t.last_detection = di
                    self.tracks.append(t)
                return sorted((t.id, t.last_detection) for t in self.tracks if t.id is not None and t.last_detection >= 0 and t.hit_counter >= 0)

        return _Capped(**policy)


class _Seg:
    def __init__(self, q, di):
        self.xyxyxyxy, self.di = q, di

    def extract_dewarped(self, frame):
        return np.array([self.di])


class _Enc:
    def __init__(self):
        self.z = None

    def encode(self, crops):
        import torch

        return torch.from_numpy(np.stack([self.z[int(c[0])] for c in crops]))


class _Vecs:
    def __init__(self):
        self.queries = []

    def query_nearby_batch(self, qs, k, with_payload, with_vectors):
        self.queries = [np.array(q, copy=True) for q in qs]
        return [[] for _ in qs]


def run_host(scn: Scenario, capped=None):
    """every stream through its own TrackerCtx -> per step, per frame a dict: matched [(id, di)], due [(id, di)] in the
    host's order, avg {id: avg_z} of the due tracks after the step, tracks (a snapshot of the filter state in creation
    order, each with its creation serial `birth`), n_live; and per stream the peak of n_live and the trackers themselves"""
    from mtgv.tracker import KalmanPointTracker, TrackerCtx

    capped = scn.capped if capped is None else capped
    Z = scn.z()
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
            objs = ctx.update(st.dets[f])
            for t in ctx.tracker.tracks:  # new tracks are appended in ascending detection index: the creation order
                if not hasattr(t, "birth"):
                    t.birth = births[s]
                    births[s] += 1
            by_id = {t.id: t.last_detection for t in ctx.tracker.tracks if t.id is not None}
            matched = [(o.id, by_id[o.id]) for o in objs]
            # the clock of a stream only moves forward: exactly the tracks embedded in this frame carry its time stamp
            due = [o for o in objs if o.last_update_time == st.now[f]]
            assert len(due) == len(vecs[s].queries) and all((o.avg_z == q).all() for o, q in zip(due, vecs[s].queries))
            peak[s] = max(peak[s], len(ctx.tracker.tracks))
            frames.append(dict(matched=matched, due=[(o.id, by_id[o.id]) for o in due], avg={o.id: o.avg_z.copy() for o in due},
                               prev={o.id: before.get(o.id, (None, None))[0] for o in due}, last={o.id: o.last_update_time for o in objs},
                               tracks=[copy.deepcopy(t) for t in ctx.tracker.tracks], n_live=len(ctx.tracker.tracks)))
        out.append(frames)
    return out, peak, [c.tracker for c in ctxs]
