"""The lock-step host yardstick of the embed budget (test_track_budget_cpu.py, test_gpu_track_budget.py).

`track_common.run_host` runs every stream through a TrackerCtx of its own, one after the other; a budget couples the
streams of a step, so here one `KalmanPointTracker` per stream is stepped together: every frame of the step is associated,
the reported tracks are gated as `TrackerCtx.update` gates them (`now - last_update_time > update_wait_sec or avg_z is
None`), `mtgv.tracker.select_due` chooses among the candidates of the whole step, and only the chosen tracks get
`last_update_time = now` and an embedding.  Scenarios are track_common's (and track_wide_common's steps): imported, not
edited.
"""
from __future__ import annotations

import numpy as np

import track_common as tc


def tie_heavy_keys(n, seed, straddle_budget=None):
    """n float64 keys for the selection tests: NaN (no candidate) or one of five values and +inf, so that ties dominate.
    straddle_budget E: the keys are arranged so that the group of equal keys that holds the E-th largest candidate has
    members on both sides of the cut (when there are more than E candidates and n >= 3)."""
    rng = np.random.default_rng(seed)
    values = np.array([np.inf, 0.75, 0.5, 0.5 + 2.0 ** -52, 1.0 / 30.0, -0.25])
    w = values[rng.integers(0, len(values), n)]
    w[rng.random(n) < 0.2] = np.nan
    if straddle_budget is not None and n >= 3:
        cand = np.flatnonzero(~np.isnan(w))
        e = int(straddle_budget)
        if 1 <= e < cand.size:
            order = cand[np.lexsort((cand, -w[cand]))]
            w[order[e - 1]] = w[order[e]] = 0.5  # the E-th and the (E + 1)-th candidate tie ...
            w[order[:e - 1]] = np.inf  # ... below everything in front of them
            w[order[e + 1:]] = np.where(rng.random(order.size - e - 1) < 0.5, 0.5, -0.25)  # and more of the group behind
    return w


def brute_force(waited, budget):
    """sorted(key=(-waited, index))[:E] in ascending index: the statement of the rule that select_due is tested against"""
    w = np.asarray(waited, np.float64)
    cand = [i for i in range(w.size) if not np.isnan(w[i])]
    return np.array(sorted(sorted(cand, key=lambda i: (-w[i], i))[: int(budget)]), dtype=np.int64)


def select_outputs(waited, budget):
    """what track_select_kernel has to write for `waited`: due_idx (n) with -1 behind n_due, rank_of (n), n_due, n_deferred"""
    from mtgv.tracker import select_due

    w = np.asarray(waited, np.float64)
    sel = select_due(w, budget)
    due_idx = np.full(w.size, -1, np.int32)
    due_idx[: sel.size] = sel
    rank_of = np.full(w.size, -1, np.int32)
    rank_of[sel] = np.arange(sel.size)
    return due_idx, rank_of, int(sel.size), int((~np.isnan(w)).sum() - sel.size)


def run_lockstep(steps, where, K, budget, update_wait_sec=0.5, policy=None, max_tracks=None, n_streams=None):
    """steps: track_common.Step's; where[i][f][di] = the slot k of detection di of frame f in step i (track_common.layout's
    fourth result); budget E.  max_tracks: the capped tracker (scenario j).
    -> per step a dict: matched [per frame [(id, di)]], waited (F * K,) float64 (NaN: no candidate), due (the selected flat
    slots, ascending), n_deferred, last {(stream, id): last_update_time of every track reported in the step, after it}"""
    from mtgv.tracker import KalmanPointTracker, select_due

    policy = policy or {}
    S = (1 + max(s for st in steps for s in st.streams)) if n_streams is None else n_streams
    trackers = [tc.CappedTracker(max_tracks, **policy) if max_tracks is not None else KalmanPointTracker(**policy) for _ in range(S)]
    data = {}  # (stream, id) -> [last_update_time, has_z]: TrackedData's two gating fields
    out = []
    for i, st in enumerate(steps):
        F = len(st.streams)
        waited = np.full(F * K, np.nan)
        owner, matched_all = {}, []
        for f, s in enumerate(st.streams):
            matched = trackers[s].update(list(st.dets[f]))
            matched_all.append(matched)
            now = st.now[f]
            for tid, di in matched:
                d = data.setdefault((s, tid), [now, False])  # a new TrackedData is stamped with the frame's clock
                j = f * K + where[i][f][di]
                owner[j] = (s, tid, now)
                if now - d[0] > update_wait_sec or not d[1]:
                    waited[j] = (now - d[0]) if d[1] else np.inf
        due = select_due(waited, budget)
        for j in due:
            s, tid, now = owner[int(j)]
            data[(s, tid)] = [now, True]
        out.append(dict(matched=matched_all, waited=waited, due=due, n_deferred=int((~np.isnan(waited)).sum() - due.size),
                        last={(s, tid): data[(s, tid)][0] for s, tid, _ in owner.values()}))
    return out, trackers


def run_lockstep_scenario(scn, budget):
    """a track_common scenario through the lock-step yardstick"""
    where = [tc.layout(scn, i)[3] for i in range(len(scn.steps))]
    return run_lockstep(scn.steps, where, tc.K, budget, scn.update_wait_sec, scn.policy, scn.max_tracks if scn.capped else None, tc.S)


def binding_scenario(n_steps=26):
    """track_common's shape (S 3, K 4) with four still cards per stream, no initialisation delay and a negative wait: every
    one of the 12 slots is a candidate in every step"""
    def cards(s):
        return lambda i: [tc.quad(150 + 400 * c + i, 200 + 50 * s) for c in range(4)]

    return tc.Scenario("budget_binds", tc._steps(n_steps, [cards(s) for s in range(tc.S)]), policy=dict(initialization_delay=0),
                       update_wait_sec=-1.0, seed=21)
