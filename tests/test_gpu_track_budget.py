"""The embed budget of the device tracker (csrc/track.hip: track_select_kernel; mtgv/track.py: embed_budget, run_many)
against its host statement: mtgv.tracker.select_due for the selection, track_budget_common's lock-step yardstick for whole
steps.  Everything is compared exactly: the kernel finds the budget-th largest fp64 key by a radix select, no tolerance."""
import functools

import numpy as np
import pytest
import torch

import track_budget_common as tb
import track_common as tc
import track_wide_common as tw

pytestmark = pytest.mark.gpu

FIELDS = ("live", "hit_counter", "is_initializing", "id", "birth", "has_z", "pos", "vel", "pp", "pv", "vv", "last_update_time", "avg_z",
          "match_ids", "match_scores")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(None)
def _matcher():
    from mtgv.matcher import Matcher

    m = Matcher(tc.DIM, capacity=tc.BANK_ROWS)
    m.add(np.random.default_rng(77).standard_normal((tc.BANK_ROWS, tc.DIM)).astype(np.float32))
    return m


def _tracker(scn, **kw):
    from mtgv.track import DeviceTracker

    return DeviceTracker(tc.S, tc.K, tc.DIM, tc.TOP_K, max_tracks=scn.max_tracks, update_wait_sec=scn.update_wait_sec, ewma_weight=scn.ewma_weight,
                         **{**scn.policy, **kw})


def _select(w, budget):
    from mtgv import native

    n = w.size
    wd = _cu(w)
    due_idx, rank_of = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    n_due, n_def = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    native.check(native.lib().mtgv_op_track_select(native.ptr(wd), n, int(budget), native.ptr(due_idx), native.ptr(rank_of), native.ptr(n_due),
                                                   native.ptr(n_def), native.stream()))
    return due_idx.cpu().numpy(), rank_of.cpu().numpy(), int(n_due.item()), int(n_def.item())


# ---- 1. the selection kernel alone

@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 8192])
def test_select_kernel(n):
    straddled = 0
    for e in sorted({1, 5, n - 1, n, n + 1} - {0}):
        for seed, straddle in ((0, None), (1, e)):
            w = tb.tie_heavy_keys(n, 7000 * n + 10 * e + seed, straddle)
            want = tb.select_outputs(w, e)
            got = _select(w, e)
            for name, g, x in zip(("due_idx", "rank_of", "n_due", "n_deferred"), got, want):
                assert np.array_equal(g, x), f"n {n} E {e} seed {seed}: {name} {g} vs {x}"
            sel = want[0][: want[2]]
            if want[3] and sel.size:
                lo = w[sel].min()
                straddled += int(((w == lo).sum() > (w[sel] == lo).sum()))
    assert n < 63 or straddled > 0, "no case in which the group of tied keys straddles the budget"


def test_select_kernel_no_candidate_and_signed_zero():
    assert _select(np.full(70, np.nan), 3)[2:] == (0, 0)
    w = np.array([-0.0, 0.0, np.nan, 0.0, -0.0, -1.0])  # -0.0 == 0.0: one group, taken by index
    got, want = _select(w, 3), tb.select_outputs(w, 3)
    assert all(np.array_equal(g, x) for g, x in zip(got, want)) and want[0][:3].tolist() == [0, 1, 3]


def test_refusals():
    from mtgv import native
    from mtgv.track import DeviceTracker

    for n, e in ((0, 1), (8193, 1), (8, 0), (8, 65536)):
        buf = torch.zeros((max(n, 1),), dtype=torch.float64, device="cuda")
        out = torch.zeros((max(n, 1),), dtype=torch.int32, device="cuda")
        assert native.lib().mtgv_op_track_select(native.ptr(buf), n, e, native.ptr(out), native.ptr(out), native.ptr(out), native.ptr(out),
                                                 native.stream()) == 1, (n, e)
    for e in (0, 65536):
        with pytest.raises(AssertionError):
            DeviceTracker(2, 4, 8, 1, max_tracks=8, embed_budget=e)
    # 2731 frames x 3 cards = 8193 flat slots on a budget handle: status 1; 2730 x 3 = 8190 runs
    trk = DeviceTracker(2731, 3, 4, 1, max_tracks=4, embed_budget=5)
    quads = torch.zeros((2731, 3, 4, 2), dtype=torch.float32, device="cuda")
    n_det = torch.zeros((2731,), dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError, match="8192"):
        trk.update(quads, range(2731), 1.0, n_det=n_det)
    _, _, n_due = trk.update(quads[:2730], range(2730), 1.0, n_det=n_det[:2730])
    assert int(n_due.item()) == 0 and int(trk.n_deferred.item()) == 0
    plain = DeviceTracker(2, 4, 8, 1, max_tracks=8)
    with pytest.raises(AssertionError):
        plain.gather(torch.zeros((8, 16), dtype=torch.uint8, device="cuda"), pad=True)
    # commit: a handle without a budget takes any number of rows, as it always did; a budget handle one block per row
    small = torch.zeros((2, 4, 4, 2), dtype=torch.float32, device="cuda")
    z = torch.zeros((70000, 8), dtype=torch.float32, device="cuda")
    budget = DeviceTracker(2, 4, 8, 1, max_tracks=8, embed_budget=5)
    for t in (plain, budget):
        t.update(small, range(2), 1.0, n_det=n_det[:2])
    assert plain.commit(z).shape == z.shape and budget.commit(z[:65535]).shape == (65535, 8)
    with pytest.raises(AssertionError, match="65535"):
        budget.commit(z[:65536])


# ---- 2. a budget that never binds changes nothing

@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_budget_that_never_binds_changes_nothing(name):
    scn = tc.SCENARIOS[name]
    E = tc.S * tc.K
    plain, budget, m, Z = _tracker(scn), _tracker(scn, embed_budget=E), _matcher(), scn.z()
    n_due_total = 0
    for i, st in enumerate(scn.steps):
        quads, n_det, state, _ = tc.layout(scn, i)
        tid_p, due_p, nd_p = plain.update(_cu(quads), st.streams, st.now, n_det=_cu(n_det), state=_cu(state))
        tid_b, due_b, nd_b = budget.update(_cu(quads), st.streams, st.now, n_det=_cu(n_det), state=_cu(state))
        n_due, due = int(nd_p.item()), due_p.cpu().numpy()
        assert torch.equal(tid_p, tid_b) and torch.equal(due_p, due_b) and int(nd_b.item()) == n_due, (name, i)
        assert int(budget.n_deferred.item()) == 0, (name, i)
        z = np.zeros((E, tc.DIM), np.float32)
        for r, j in enumerate(due[:n_due]):
            z[r] = Z[i, st.streams[j // tc.K], j % tc.K]
        if n_due:
            out_p = plain.store(*m.match(plain.commit(_cu(z[:n_due])), tc.TOP_K))
        else:
            out_p = plain.store()
        q = budget.commit(_cu(z))
        assert not q[n_due:].any(), (name, i)
        out_b = budget.store(*m.match(q, tc.TOP_K))
        assert torch.equal(out_p[0], out_b[0]) and (_bits(out_p[1].cpu().numpy()) == _bits(out_b[1].cpu().numpy())).all(), (name, i)
        for s in range(tc.S):
            a, b = plain.state(s), budget.state(s)
            for k in FIELDS:
                assert (_bits(a[k]) == _bits(b[k])).all(), (name, i, s, k)
            assert (a["next_id"], a["next_birth"], a["overflow"]) == (b["next_id"], b["next_birth"], b["overflow"])
        n_due_total += n_due
    assert n_due_total > 0


# ---- 3. a budget that binds

@pytest.mark.parametrize("E", [1, 5])
def test_budget_that_binds(E):
    scn = tb.binding_scenario()
    host, _ = tb.run_lockstep_scenario(scn, E)
    trk = _tracker(scn, embed_budget=E)
    bound = -(-12 // E)
    z = torch.from_numpy(np.random.default_rng(5).standard_normal((E, tc.DIM)).astype(np.float32)).cuda()
    taken_at, before = {}, [trk.state(s) for s in range(tc.S)]
    for i, (st, h) in enumerate(zip(scn.steps, host)):
        quads, n_det, _, _ = tc.layout(scn, i)
        tid, due_idx, n_due_dev = trk.update(_cu(quads), st.streams, st.now, n_det=_cu(n_det))
        tid, due, n_due, n_def = tid.cpu().numpy(), due_idx.cpu().numpy(), int(n_due_dev.item()), int(trk.n_deferred.item())
        assert due[:n_due].tolist() == h["due"].tolist() and (due[n_due:] == -1).all(), (i, due, h["due"])
        cand = int((~np.isnan(h["waited"])).sum())
        assert cand == 12 and n_due + n_def == cand and n_due == E
        after = [trk.state(s) for s in range(tc.S)]
        for f, s in enumerate(st.streams):
            assert sorted((int(tid[f, k]), k) for k in range(tc.K) if tid[f, k] > 0) == h["matched"][f]
            for k in range(tc.K):  # every slot is a candidate: selected -> the frame's clock, deferred -> untouched
                t = int(np.flatnonzero((after[s]["id"] == tid[f, k]) & (after[s]["live"] != 0))[0])
                if f * tc.K + k in due[:n_due]:
                    assert after[s]["last_update_time"][t] == st.now[f], (i, f, k)
                    taken_at.setdefault((s, int(tid[f, k])), []).append(i)
                else:
                    assert _bits(after[s]["last_update_time"])[t] == _bits(before[s]["last_update_time"])[t], (i, f, k)
                    if after[s]["has_z"][t]:  # embedded before: the time of that embed, as on the host
                        assert after[s]["last_update_time"][t] == h["last"][(s, int(tid[f, k]))]
        q = trk.commit(z)
        assert not q[n_due:].any()
        trk.store()
        before = [trk.state(s) for s in range(tc.S)]
    assert len(taken_at) == 12 and len(scn.steps) >= 8
    for key, steps in taken_at.items():  # nobody starves
        assert steps[0] < bound and max(np.diff(steps), default=0) <= bound and len(scn.steps) - steps[-1] <= bound, (key, steps)


# ---- 4. the wide form

def test_wide_budget():
    from mtgv.track import DeviceTracker

    S, K, E = 6, 64, 100
    cards = [[tw.grid(c, row0=0) for c in range(K)] for _ in range(S)]
    # stream s's clock runs 1 ms per step faster than stream s - 1's: from step 1 on the keys differ by stream
    steps = [tc.Step(list(range(S)), [100.0 + i / 30.0 + 0.001 * s * i for s in range(S)], cards) for i in range(4)]
    where = [[list(range(K)) for _ in range(S)] for _ in steps]
    host, _ = tb.run_lockstep(steps, where, K, E, update_wait_sec=-1.0, policy=dict(initialization_delay=0), n_streams=S)
    trk = DeviceTracker(S, K, 8, 1, max_tracks=K, embed_budget=E, initialization_delay=0, update_wait_sec=-1.0)
    assert trk.wide
    quads = _cu(np.stack([np.stack(c) for c in cards]))
    n_det = torch.full((S,), K, dtype=torch.int32, device="cuda")
    z = torch.ones((E, 8), dtype=torch.float32, device="cuda")
    for i, (st, h) in enumerate(zip(steps, host)):
        _, due_idx, n_due = trk.update(quads, st.streams, st.now, n_det=n_det)
        due, n_due = due_idx.cpu().numpy(), int(n_due.item())
        assert n_due == E and int(trk.n_deferred.item()) == S * K - E == h["n_deferred"]
        assert due[:n_due].tolist() == h["due"].tolist() and (due[n_due:] == -1).all(), i
        if i == 0:
            assert due[:n_due].tolist() == list(range(E))  # all +inf: the first E by index
        trk.commit(z)
        trk.store()
    finite = host[-1]["waited"][host[-1]["due"]]
    assert np.isinf(finite).sum() == S * K - 3 * E and len(set(finite[np.isfinite(finite)].tolist())) == 1  # the oldest keys, all of one stream's clock


# ---- 5. padding

def test_padding_and_prepass_fallbacks(monkeypatch):
    from mtgv.matcher import Matcher
    from mtgv.track import DeviceTracker

    F, K, E, DIM = 3, 4, 128, 64
    m = Matcher(DIM, capacity=4096)  # 128 queries, dim % 64 == 0, 4096 rows: the two-pass match with its fallback counter
    m.add(np.random.default_rng(3).standard_normal((4096, DIM)).astype(np.float32))
    trk = DeviceTracker(F, K, DIM, 1, max_tracks=8, embed_budget=E, initialization_delay=0)
    cards = np.stack([np.stack([tc.quad(100 + 150 * c, 100 + 10 * f) for c in range(K)]) for f in range(F)])
    n_det = torch.full((F,), K, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    counts = []
    for step, t in enumerate((10.0, 10.1)):
        _, due_idx, n_due = trk.update(_cu(cards), range(F), t, n_det=n_det)
        n, due = int(n_due.item()), due_idx.cpu().numpy()
        counts.append(n)
        for shape in ((F * K, 8, 8, 3), (F * K, 5, 7, 3)):  # the 16-byte and the bytewise path
            src = torch.randint(0, 256, shape, generator=g, device="cuda", dtype=torch.uint8)
            out = torch.full((E, *shape[1:]), 7, dtype=torch.uint8, device="cuda")
            assert trk.gather(src, out=out, pad=True) is out and trk.gather(src, pad=True).shape == out.shape
            assert (out[:n] == src[torch.from_numpy(due[:n]).long().cuda()]).all() and not out[n:].any()
        z = torch.randn((E, DIM), generator=g, device="cuda")
        q = torch.full_like(z, float("nan"))
        from mtgv import native

        native.check(native.lib().mtgv_tracker_commit(trk._h, native.ptr(z), native.ptr(q), E, native.stream()))
        assert not q[n:].any() and bool(torch.isfinite(q).all()) and (n == 0 or bool(q[:n].any()))
        fb = m.prepass_fallbacks()
        ids, scores = m.match(q, 1)
        trk.store(ids, scores)
        torch.cuda.synchronize()
        if n == 0:
            assert m.prepass_fallbacks() == fb, f"{m.prepass_fallbacks() - fb} zero queries took the match's exact fallback"
        # a pad row's answer is the exact one: what the one-pass match gives for the same queries, bit for bit
        monkeypatch.setenv("MTGV_MATCH_PREPASS", "0")
        ids1, scores1 = m.match(q, 1)
        monkeypatch.setenv("MTGV_MATCH_PREPASS", "1")
        assert torch.equal(ids, ids1) and torch.equal(scores[n:].view(torch.int32), scores1[n:].view(torch.int32))
        assert (ids[n:] == 0).all() and (scores[n:] == 0).all()
    assert counts == [F * K, 0]


# ---- 6, 7. the pipeline

@functools.lru_cache(None)
def _pipeline():
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline

    F, K = 4, 4
    det_cfg = spec.DetectorConfig()
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=256)
    m.add(np.random.default_rng(5).standard_normal((200, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F),
                    Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1, quad_source="mask")
    # test_gpu_track's frames: bright cards on noise that move two pixels per step
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (F, 640, 640, 3), dtype=np.uint8)
    for f in range(F):
        for c in range(3):
            x, y = 60 + 190 * c, 100 + 120 * f
            base[f, y : y + 180, x : x + 120] = 200 + 10 * c
    # Step 0 carries two of the four cameras, so the tracks of cameras 2 and 0 get their ids (and are due) one step before
    # those of cameras 3 and 1: at most 8 slots are due at once and a budget of 8 defers nothing through step 6.  Step 7
    # comes a second later: every track is due at once, the budget binds, and step 8 embeds what it left.
    steps = []
    for i in range(9):
        n = 2 if i == 0 else F
        t = 50.0 + 0.2 * i + (1.0 if i >= 7 else 0.0)
        steps.append((torch.from_numpy(np.roll(base, 2 * i, axis=2)[:n]).cuda(), [2, 0, 3, 1][:n], [t + 0.01 * f for f in range(n)]))
    return pipe, steps


def _same(a, b, path):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif a is None or b is None:
        assert a is None and b is None, path
    else:
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), path


def _sync_debug_honoured():
    x = torch.ones((1,), device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_pipeline_runs_without_a_synchronisation():
    """With a budget `run` reads nothing back, and while the budget has not deferred anything it is the budget-less step.
    After the first deferral the two trackers differ by construction - a deferred track is embedded a step later, so a
    later step in which nothing is deferred still has another due set - and the comparison with the budget-less pipeline
    ends there.  Every step, before and after, is compared with the lock-step host yardstick fed with the quads the
    pipeline saw: track ids, the selected slots and the number deferred."""
    from mtgv.track import TrackedPipeline

    pipe, steps = _pipeline()
    E = 8
    tp, ref = TrackedPipeline(pipe, streams=4, top_k=3, embed_budget=E), TrackedPipeline(pipe, streams=4, top_k=3)
    first = tp.run(*steps[0])  # (workspaces are allocated on the first step)
    ref.run(*steps[0])
    honoured = _sync_debug_honoured()
    deferred, compared_due, n_due_total = False, 0, 0
    seen = [first]
    for i, step in enumerate(steps[1:], 1):
        if honoured:
            torch.cuda.set_sync_debug_mode("error")
        try:
            out = tp.run(*step)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        want = ref.run(*step)
        assert set(out) == set(want) | {"n_deferred"} and out["n_due"].shape == (1,) and out["n_due"].dtype == torch.int32
        assert out["n_deferred"].shape == (1,) and out["n_deferred"].dtype == torch.int32
        n_due, n_def = int(out["n_due"].item()), int(out["n_deferred"].item())
        print(f"step {i}: n_due {n_due} n_deferred {n_def} (budget-less: {want['n_due']})")
        assert n_due <= E and tuple(tp.last_z.shape) == (E, 768)
        due = out["due_idx"].cpu().numpy()
        assert (due[:n_due] >= 0).all() and (np.diff(due[:n_due]) > 0).all() and (due[n_due:] == -1).all()
        padded = torch.zeros((E, *out["crops"].shape[1:]), dtype=torch.uint8, device="cuda")
        padded[:n_due] = out["crops"][torch.from_numpy(due[:n_due]).long().cuda()]
        assert torch.equal(tp.last_z, pipe.encoder.encode(padded)), "the committed embeddings are not encode(padded crops[due_idx])"
        deferred = deferred or n_def > 0
        if not deferred:
            assert n_due == want["n_due"]
            for k in set(want) - {"n_due"}:
                _same(out[k], want[k], k)
            if n_due:
                assert torch.equal(tp.last_z[:n_due], ref.last_z)
            compared_due += n_due
        n_due_total += n_due
        seen.append(out)
    assert compared_due > 0, "no due track was compared with the budget-less pipeline"
    assert deferred and n_due_total > compared_due, "the budget never bound"
    # all nine steps against the lock-step host yardstick on the pipeline's own quads (slot k is detection k: a prefix)
    K, host_steps, where = pipe.K, [], []
    for (_, sof, now), out in zip(steps, seen):
        quads, n_det = out["quads"].cpu().numpy(), np.minimum(out["n_det"].cpu().numpy(), K)
        host_steps.append(tc.Step(list(sof), list(now), [[quads[f, k] for k in range(n_det[f])] for f in range(len(sof))]))
        where.append([list(range(n_det[f])) for f in range(len(sof))])
    host, _ = tb.run_lockstep(host_steps, where, K, E, update_wait_sec=0.5, n_streams=4)
    after_deferral = 0
    for i, (out, h) in enumerate(zip(seen, host)):
        tids, n_due = out["track_ids"].cpu().numpy(), int(out["n_due"].item())
        for f in range(tids.shape[0]):
            assert sorted((int(tids[f, k]), k) for k in range(K) if tids[f, k] > 0) == h["matched"][f], (i, f)
        assert out["due_idx"].cpu().numpy()[:n_due].tolist() == h["due"].tolist(), (i, h["due"])
        assert int(out["n_deferred"].item()) == h["n_deferred"], i
        after_deferral += n_due if any(x["n_deferred"] for x in host[:i]) else 0
    assert after_deferral > 0, "no step behind the first deferral had a due track"


def test_run_many_overlapped_is_sequential_run(monkeypatch):
    from mtgv.track import TrackedPipeline

    pipe, steps = _pipeline()
    with pytest.raises(AssertionError, match="embed_budget"):
        TrackedPipeline(pipe, streams=4, top_k=3).run_many(steps)
    seq, par = TrackedPipeline(pipe, streams=4, top_k=3, embed_budget=8), TrackedPipeline(pipe, streams=4, top_k=3, embed_budget=8)
    want, want_z = [], []
    for step in steps:
        want.append(seq.run(*step))
        want_z.append(seq.last_z)
    monkeypatch.setenv("MTGV_OVERLAP", "on")
    got = par.run_many(steps)
    torch.cuda.synchronize()
    assert len(got) == len(want) == len(steps) >= 6
    for i, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"step {i}")
    assert torch.equal(par.last_z, want_z[-1])
    assert sum(int(o["n_due"].item()) for o in got) > 0 and sum(int(o["n_deferred"].item()) for o in got) > 0
    monkeypatch.setenv("MTGV_CROP_STAGE", "enc")  # the crop stage on the embed stream, as Pipeline.run_many has it
    for i, (a, b) in enumerate(zip(TrackedPipeline(pipe, streams=4, top_k=3, embed_budget=8).run_many(steps), want)):
        _same(a, b, f"crop stage on the embed stream, step {i}")
    monkeypatch.delenv("MTGV_CROP_STAGE")
    monkeypatch.setenv("MTGV_OVERLAP", "off")  # the opt-in: sequential run on the current stream
    again = TrackedPipeline(pipe, streams=4, top_k=3, embed_budget=8).run_many(steps[:2])
    for i, (a, b) in enumerate(zip(again, want)):
        _same(a, b, f"sequential step {i}")
