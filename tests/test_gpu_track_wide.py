"""The wide device tracker (MTGV_TRACKER_WIDE: up to 256 tracks per stream and 64 cards per frame on the multi-wave update
kernel of csrc/track.hip) against the host code it restates, as test_gpu_track.py does for the one-wave kernel: one
mtgv.tracker.TrackerCtx with a KalmanPointTracker per stream (CappedTracker where a scenario overflows).  Ids, due sets,
counters and the fp64 filter state have no tolerance.  test_track_wide_cpu.py shows on the host alone that the scenarios
reach the waves, ties and slots they are named for."""
import functools

import numpy as np
import pytest
import torch

import track_common as tc
import track_wide_common as tw

pytestmark = pytest.mark.gpu

KAL = ("pos", "vel", "pp", "pv", "vv")
STATE_KEYS = KAL + ("live", "hit_counter", "is_initializing", "id", "birth", "has_z", "avg_z", "match_ids", "match_scores", "last_update_time")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _cu(a):
    return None if a is None else torch.from_numpy(a).cuda()


@functools.lru_cache(None)
def _matcher():
    from mtgv.matcher import Matcher

    m = Matcher(tw.DIM, capacity=tw.BANK_ROWS)
    m.add(np.random.default_rng(77).standard_normal((tw.BANK_ROWS, tw.DIM)).astype(np.float32))
    return m


def _device_pass(scn, S, K, layout, wide):
    """one pass of a scenario through a fresh device tracker: per step the outputs and every stream's state"""
    from mtgv.track import DeviceTracker

    trk = DeviceTracker(S, K, tw.DIM, tw.TOP_K, max_tracks=scn.max_tracks, wide=wide, update_wait_sec=scn.update_wait_sec,
                        ewma_weight=scn.ewma_weight, **scn.policy)
    assert trk.wide == (wide is not False)
    m, Z, dev = _matcher(), scn.z(), []
    for i, st in enumerate(scn.steps):
        quads, n_det, state, where = layout(scn, i)
        tid, due_idx, n_due_dev = trk.update(_cu(quads), st.streams, st.now, n_det=_cu(n_det), state=_cu(state))
        n_due, due = int(n_due_dev.item()), due_idx.cpu().numpy()
        rec = dict(track_ids=tid.cpu().numpy(), due=due, n_due=n_due, where=where, q=None)
        if n_due:
            z = np.stack([Z[i, st.streams[j // K], j % K] for j in due[:n_due]])
            q = trk.commit(torch.from_numpy(z).cuda())
            ids, scores = trk.store(*m.match(q, tw.TOP_K))
            rec.update(z=z, q=q.cpu().numpy())
        else:
            ids, scores = trk.store()
        rec.update(ids=ids.cpu().numpy(), scores=scores.cpu().numpy(), states=[trk.state(s) for s in range(S)])
        dev.append(rec)
    return dev


@functools.lru_cache(None)
def _run(name):
    """a wide scenario through the host yardstick and the device, shared by the tests below"""
    scn = tw.scenarios()[name]
    host, _, host_trackers = tw.run_host(name)
    return scn, scn.n_streams, scn.k, host, host_trackers, _device_pass(scn, scn.n_streams, scn.k, tw.layout, None)


@functools.lru_cache(None)
def _run_forced(name):
    """a scenario of track_common (T 8 or 4, K 4) through wide=True: the new kernel with one wave"""
    scn = tc.SCENARIOS[name]
    host, _, host_trackers = tc.run_host(scn)
    return scn, tc.S, tc.K, host, host_trackers, _device_pass(scn, tc.S, tc.K, tc.layout, True)


def _check_state(st, tracks, tag):
    """the live slots of one stream against the host's track list, mapped by creation serial; bit for bit"""
    live = np.flatnonzero(st["live"])
    by_birth = {int(st["birth"][t]): int(t) for t in live}
    assert len(by_birth) == len(live), f"{tag}: a birth twice"
    assert sorted(by_birth) == sorted(t.birth for t in tracks), f"{tag}: live births {sorted(by_birth)} vs host {[t.birth for t in tracks]}"
    for t in tracks:
        sl = by_birth[t.birth]
        assert int(st["hit_counter"][sl]) == t.hit_counter and bool(st["is_initializing"][sl]) == t.is_initializing, f"{tag} birth {t.birth}"
        assert int(st["id"][sl]) == (t.id or 0), f"{tag} birth {t.birth}: id {st['id'][sl]} vs {t.id}"
        for n in KAL:
            assert (_bits(st[n][sl]) == _bits(getattr(t, n))).all(), f"{tag} birth {t.birth}: {n} {st[n][sl]} vs {getattr(t, n)}"


def _check_association(name, run):
    scn, S, K, host, host_trackers, dev = run
    prev = [None] * S
    for i, (st, rec) in enumerate(zip(scn.steps, dev)):
        assert (rec["due"][: rec["n_due"]] >= 0).all() and (np.diff(rec["due"][: rec["n_due"]]) > 0).all() and (rec["due"][rec["n_due"]:] == -1).all()
        due_dev = {(int(j) // K, int(j) % K) for j in rec["due"][: rec["n_due"]]}
        due_host = set()
        for f, s in enumerate(st.streams):
            h, ks, tag = host[i][f], rec["where"][f], f"{name} step {i} stream {s}"
            got = sorted((int(rec["track_ids"][f, k]), ks.index(k)) for k in range(K) if rec["track_ids"][f, k] > 0 and k in ks)
            assert got == h["matched"], f"{tag}: {got} vs host {h['matched']}"
            assert all(rec["track_ids"][f, k] == 0 for k in range(K) if k not in ks), f"{tag}: an id on a slot that is no detection"
            due_host |= {(f, ks[di]) for _, di in h["due"]}
            stt = rec["states"][s]
            _check_state(stt, h["tracks"], tag)
            by_id = {int(v): t for t, v in enumerate(stt["id"]) if stt["live"][t] and v > 0}
            for tid_, last in h["last"].items():
                assert stt["last_update_time"][by_id[tid_]] == last, f"{tag}: last_update_time of id {tid_}"
        assert due_dev == due_host, f"{name} step {i}: due {sorted(due_dev)} vs host {sorted(due_host)}"
        for s in range(S):  # a stream that the step does not carry is not touched
            if s not in st.streams and prev[s] is not None:
                assert all((_bits(prev[s][k]) == _bits(rec["states"][s][k])).all() for k in KAL + ("live", "hit_counter", "id", "birth", "avg_z")), (name, i, s)
            prev[s] = rec["states"][s]
    for s in range(S):
        last = dev[-1]["states"][s]
        assert last["next_id"] == host_trackers[s]._next_id, (name, s)
        assert last["overflow"] == getattr(host_trackers[s], "dropped", 0), (name, s)
        # every detection that found a slot has a creation serial: the host's count of tracks ever made
        made = [t.birth for i, st in enumerate(scn.steps) for f, ss in enumerate(st.streams) if ss == s for t in host[i][f]["tracks"]]
        assert last["next_birth"] == max(made, default=-1) + 1, (name, s)


@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_forced_wide_equals_the_host(name):
    """T = 8 (4 in j_overflow), K = 4: every scenario of the one-wave tests through wide=True; and the one-wave kernel leaves
    the same state behind, array for array and bit for bit (the two kernels share one per-slot body, csrc/track.hip)"""
    _check_association(name, _run_forced(name))
    scn, S, K, _, _, wide = _run_forced(name)
    narrow = _device_pass(scn, S, K, tc.layout, False)
    for i, (a, b) in enumerate(zip(narrow, wide)):
        for s in range(S):
            assert a["states"][s].keys() == b["states"][s].keys()
            for key, v in a["states"][s].items():
                assert np.array_equal(_bits(np.asarray(v)), _bits(np.asarray(b["states"][s][key]))), (name, i, s, key)


@pytest.mark.parametrize("name", sorted(tw.scenarios()))
def test_association(name):
    _check_association(name, _run(name))


def test_fill_overflow_and_counters():
    """W2 and W4: the further set overflows, exactly as the capped host drops; the light streams are untouched by it"""
    for name in ("fill_W2", "fill_W4"):
        scn, S, K, host, capped, dev = _run(name)
        last = dev[-1]["states"]
        assert capped[1].dropped > 0 and last[1]["overflow"] == capped[1].dropped
        assert last[0]["overflow"] == 0 and last[2]["overflow"] == 0
        assert int(last[1]["live"].sum()) == scn.max_tracks
    scn, S, K, host, _, dev = _run("fill_W3")
    assert int(dev[-1]["states"][1]["live"].sum()) == 99 and dev[-1]["states"][1]["overflow"] == 0


def test_tie_slots():
    """the tie of two tracks is between waves: stream 0, the older track in slot 64 and the younger in slot 0; stream 1 the
    other way round; the older one wins both times (test_association compares the outcome with the host)"""
    scn, S, K, host, _, dev = _run("ties")
    for s, older, younger in ((0, 64, 0), (1, 0, 64)):
        st = dev[6]["states"][s]
        assert st["live"][older] and st["live"][younger] and st["id"][older] == 1 and st["id"][younger] == 2
        assert st["birth"][older] < st["birth"][younger]
        assert dev[7]["track_ids"][scn.steps[7].streams.index(s), 0] == 1
    for step, lo in ((4, 15), (5, 31), (6, 62)):
        f = scn.steps[step].streams.index(2)
        assert dev[step]["track_ids"][f, lo] == step - 3 and dev[step]["track_ids"][f, lo + 1] == 0


def test_full_frame_slots():
    """nothing is recycled in `full`: slot == birth, which is what test_track_wide_cpu.py reads the waves from"""
    _, _, _, _, _, dev = _run("full")
    st = dev[5]["states"][1]
    live = np.flatnonzero(st["live"])
    assert len(live) == 224 and (st["birth"][live] == live).all()
    got_id = st["id"][live] > 0
    assert {int(t) // 64 for t in live[got_id]} == {0, 1, 2, 3}


def test_alloc_slots():
    """unmatched detections in ascending index take the lowest free slot over the whole workgroup: 3, 70, 130; and the
    only free slot in the last wave"""
    _, _, _, _, _, dev = _run("alloc")
    st = dev[6]["states"][1]
    slot_of = {int(st["birth"][t]): int(t) for t in np.flatnonzero(st["live"])}
    assert {b: slot_of[b] for b in (180, 181, 182)} == {b: tw.ALLOC_SLOT_OF_BIRTH[b] for b in (180, 181, 182)}
    assert all(slot_of[b] == b for b in slot_of if b < 180)
    free = np.flatnonzero(dev[9]["states"][1]["live"] == 0)
    assert free.tolist() == [], free
    st = dev[10]["states"][1]
    assert int(np.flatnonzero(st["birth"] == 183)[0]) == tw.ALLOC_SLOT_OF_BIRTH[183] == 178 and st["live"].all() and st["overflow"] == 0


@pytest.mark.parametrize("name", ["gating", "holes_both", "full"])
def test_ewma_and_matches(name):
    """gating, EWMA and store with up to 3 x 64 rows through commit, the production Matcher.match and store"""
    scn, S, K, host, _, dev = _run(name)
    m = _matcher()
    avg, kept, n_kept, n_due_total, n_due_max = {}, {}, 0, 0, 0
    for i, (st, rec) in enumerate(zip(scn.steps, dev)):
        due = [int(j) for j in rec["due"][: rec["n_due"]]]
        rank = {j: r for r, j in enumerate(due)}
        want_q = []
        for r, j in enumerate(due):
            f, k = divmod(j, K)
            key = (st.streams[f], int(rec["track_ids"][f, k]))
            avg[key] = tw.ewma32(avg.get(key), rec["z"][r], scn.ewma_weight)
            want_q.append(avg[key])
            assert (_bits(avg[key]) == _bits(host[i][f]["avg"][key[1]])).all()
        if due:
            assert (_bits(np.stack(want_q)) == _bits(rec["q"])).all(), f"{name} step {i}: avg_z"
            ids, scores = m.match(torch.from_numpy(np.stack(want_q)).cuda(), tw.TOP_K)
            ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        n_due_total += len(due)
        n_due_max = max(n_due_max, len(due))
        for f, s in enumerate(st.streams):
            stt = rec["states"][s]
            slot_of_id = {int(v): t for t, v in enumerate(stt["id"]) if stt["live"][t] and v > 0}
            for k in range(K):
                tid, j = int(rec["track_ids"][f, k]), f * K + k
                if tid == 0:
                    assert (rec["ids"][f, k] == -1).all() and np.isneginf(rec["scores"][f, k]).all(), f"{name} step {i} slot {j}"
                    continue
                if j in rank:
                    r = rank[j]
                    kept[(s, tid)] = (ids[r].copy(), scores[r].copy())
                    slot = slot_of_id[tid]
                    assert stt["has_z"][slot] == 1 and (_bits(stt["avg_z"][slot]) == _bits(avg[(s, tid)])).all()
                    assert (stt["match_ids"][slot] == ids[r]).all() and (_bits(stt["match_scores"][slot]) == _bits(scores[r])).all()
                else:
                    n_kept += 1
                assert (rec["ids"][f, k] == kept[(s, tid)][0]).all() and (_bits(rec["scores"][f, k]) == _bits(kept[(s, tid)][1])).all(), \
                    f"{name} step {i} slot {j} (due: {j in rank})"
    assert n_due_total > 4 and n_kept > 4
    if name == "gating":
        assert n_due_max == 120 and any(r["n_due"] == 0 and (r["track_ids"] > 0).any() for r in dev)
    if name == "full":
        assert n_due_max >= 64


def test_twice_the_same():
    """one wide scenario on two fresh handles: every output and the whole state bitwise equal"""
    scn, S, K, _, _, dev = _run("full")
    again = _device_pass(scn, S, K, tw.layout, None)
    for i, (a, b) in enumerate(zip(dev, again)):
        for key in ("track_ids", "due", "ids", "scores"):
            assert (_bits(a[key]) == _bits(b[key])).all(), (i, key)
        assert a["n_due"] == b["n_due"] and (a["q"] is None) == (b["q"] is None)
        assert a["q"] is None or (_bits(a["q"]) == _bits(b["q"])).all()
        for s in range(S):
            # (dead slots keep whatever their last track left: the same on both handles)
            assert all((_bits(a["states"][s][key]) == _bits(b["states"][s][key])).all() for key in STATE_KEYS), (i, s)
            assert all(a["states"][s][key] == b["states"][s][key] for key in ("next_id", "next_birth", "overflow")), (i, s)


def test_more_frames_than_one_launch():
    """W2 (T 65, K 17): 40 streams in reversed frame order, 17 drifting cards each, against one host tracker per stream;
    the streams on both sides of the 32-frame launch boundary are compared in full"""
    from mtgv.tracker import KalmanPointTracker
    from mtgv.track import DeviceTracker

    S, (T, K) = 40, tw.SIZES["W2"]
    trk = DeviceTracker(S, K, 4, 1, max_tracks=T)
    assert trk.wide
    hosts = [KalmanPointTracker() for _ in range(S)]
    order = list(range(S))[::-1]
    n_det = torch.full((S,), K, dtype=torch.int32, device="cuda")
    for step in range(4):
        quads = np.stack([np.stack([tw.quad(100 + 7 * s + 3 * step + tw.PITCH * (c % 6), 100 + tw.PITCH * (c // 6) + (s % 5) * step) for c in range(K)])
                          for s in order])
        tid, due_idx, n_due = trk.update(torch.from_numpy(quads).cuda(), order, 10.0 + step, n_det=n_det)
        tid, due = tid.cpu().numpy(), due_idx.cpu().numpy()[: int(n_due.item())]
        want_due = []
        for f, s in enumerate(order):
            matched = hosts[s].update(list(quads[f]))
            assert sorted((int(tid[f, k]), k) for k in range(K) if tid[f, k] > 0) == matched, (step, s)
            want_due += [f * K + di for _, di in matched]  # never committed: a reported track stays due
        assert sorted(want_due) == due.tolist(), step
        for s in (0, 7, 8, 39):  # frames 39, 32 (second launch) and 31, 0 (first)
            st = trk.state(s)
            for birth, t in enumerate(hosts[s].tracks):
                t.birth = birth
            _check_state(st, hosts[s].tracks, f"step {step} stream {s}")
        trk.store()
    assert (tid[:, 16] > 0).all()  # detection index 16 carries a track


def test_refusals_through_the_wrapper():
    from mtgv.track import DeviceTracker

    with pytest.raises(AssertionError, match="max_tracks"):
        DeviceTracker(2, 4, 8, 1, max_tracks=65, wide=False)
    with pytest.raises(AssertionError, match="cards_per_frame"):
        DeviceTracker(2, 17, 8, 1, max_tracks=8, wide=False)
    with pytest.raises(AssertionError, match="max_tracks"):
        DeviceTracker(2, 4, 8, 1, max_tracks=257)
    with pytest.raises(AssertionError, match="cards_per_frame"):
        DeviceTracker(2, 65, 8, 1, max_tracks=8)
    trk = DeviceTracker(2, 4, 8, 1, max_tracks=65)
    assert trk.wide and trk.state(1)["live"].shape == (65,) and not trk.state(1)["live"].any()
    assert not DeviceTracker(2, 16, 8, 1, max_tracks=64).wide


def _host_ctx(policy, wait, w):
    from mtgv.tracker import KalmanPointTracker, TrackerCtx

    e, v, c = tc._Enc(), tc._Vecs(), [0.0]
    ctx = TrackerCtx(wait, w, segmenter=lambda fr: [tc._Seg(q, di) for di, q in enumerate(fr)], encoder=e, vecs=v, clock=lambda: c[0], thumbnails=False)
    ctx.tracker = KalmanPointTracker(**policy)
    return ctx, e, v, c


E2E = {"mask": dict(cls_bias=None), "obb": dict(cls_bias=-0.9)}


@pytest.mark.parametrize("source", ["mask", "obb"])
def test_tracked_pipeline_end_to_end(source):
    """TrackedPipeline over Pipeline(cards_per_frame=24) with 96 tracks per stream: the comparison of
    test_gpu_track.py::test_tracked_pipeline_end_to_end, on frames that carry 17 or more valid slots"""
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline
    from mtgv.track import TrackedPipeline

    F, K, TOP, order = 2, 24, 3, [1, 0]
    policy = {}
    det_cfg = spec.yolo11_config(task="obb") if source == "obb" else spec.DetectorConfig()
    kw = {} if E2E[source]["cls_bias"] is None else dict(cls_bias=E2E[source]["cls_bias"])
    det_sd = spec.random_detector_state(det_cfg, 3, **kw)
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=256)
    m.add(np.random.default_rng(5).standard_normal((200, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, det_sd, max_batch=F), Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1,
                    quad_source=source)
    tp = TrackedPipeline(pipe, streams=F, top_k=TOP, max_tracks=96, **policy)
    assert tp.tracker.wide and tp.tracker.K == K
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (F, 640, 640, 3), dtype=np.uint8)
    for f in range(F):
        for c in range(24):  # a binder page and a half: 6 x 4 bright cards on noise
            x, y = 20 + 102 * (c % 6), 20 + 150 * (c // 6) + 10 * f
            base[f, y : y + 130, x : x + 90] = 180 + 3 * c
    hosts = [_host_ctx(policy, 0.5, 0.1) for _ in range(F)]
    kept, n_due_total, n_kept, most_valid = {}, 0, 0, 0
    for step in range(5):
        frames = torch.from_numpy(np.roll(base, 2 * step, axis=2)).cuda()
        now = [50.0 + 0.2 * step + 0.01 * f for f in range(F)]
        out = tp.run(frames, order, now)
        ref = pipe.run(frames)
        assert (set(out), set(out["det"])) == tc.output_keys(source, tracked=True)
        assert (set(ref), set(ref["det"])) == tc.output_keys(source)
        for k in ("crops", "boxes", "n_det"):
            assert torch.equal(out[k], ref[k]), k
        n_due, due = out["n_due"], out["due_idx"].cpu().numpy()
        assert (due[:n_due] >= 0).all() and (due[n_due:] == -1).all()
        rank = {int(j): r for r, j in enumerate(due[:n_due])}
        z = None
        if n_due:
            z = pipe.encoder.encode(out["crops"][torch.from_numpy(due[:n_due]).long().cuda()])
            assert torch.equal(tp.last_z, z), "the committed embeddings are not encode(crops[due_idx])"
            z = z.cpu().numpy()
        quads, tids = out["quads"].cpu().numpy(), out["track_ids"].cpu().numpy()
        valid = (out["card_state"].cpu().numpy() > 0) if source == "obb" else (np.arange(K)[None] < np.minimum(out["n_det"].cpu().numpy(), K)[:, None])
        most_valid = max(most_valid, int(valid.sum(axis=1).max()))
        ids, scores = out["ids"].cpu().numpy(), out["scores"].cpu().numpy()
        due_host, queries = set(), {}
        for f, s in enumerate(order):
            ctx, e, v, c = hosts[s]
            ks = [k for k in range(K) if valid[f, k]]
            c[0] = now[f]
            e.z = {di: z[rank[f * K + k]] for di, k in enumerate(ks) if f * K + k in rank}  # a KeyError: the host embeds a slot the device did not
            v.queries = []
            objs = ctx.update([quads[f, k] for k in ks])
            by_id = {t.id: t.last_detection for t in ctx.tracker.tracks if t.id is not None}
            assert sorted((int(tids[f, k]), di) for di, k in enumerate(ks) if tids[f, k] > 0) == [(o.id, by_id[o.id]) for o in objs], (step, s)
            assert all(tids[f, k] == 0 for k in range(K) if k not in ks)
            for o in objs:
                if o.last_update_time == now[f]:
                    due_host.add(f * K + ks[by_id[o.id]])
                    queries[f * K + ks[by_id[o.id]]] = o.avg_z
        assert due_host == set(rank), (step, sorted(due_host), due[:n_due])
        if n_due:
            want_ids, want_scores = m.match(torch.from_numpy(np.stack([queries[int(j)] for j in due[:n_due]])).cuda(), TOP)
            want_ids, want_scores = want_ids.cpu().numpy(), want_scores.cpu().numpy()
        n_due_total += n_due
        for f, s in enumerate(order):
            for k in range(K):
                j, tid = f * K + k, int(tids[f, k])
                if tid == 0:
                    assert (ids[f, k] == -1).all() and np.isneginf(scores[f, k]).all()
                    continue
                if j in rank:
                    kept[(s, tid)] = (want_ids[rank[j]], want_scores[rank[j]])
                else:
                    n_kept += 1
                assert (ids[f, k] == kept[(s, tid)][0]).all() and (_bits(scores[f, k]) == _bits(kept[(s, tid)][1])).all(), (step, j)
    print(f"{source}: most valid slots in a frame {most_valid}, {n_due_total} embeds in 5 steps of {F * K} crops, {n_kept} slots served from kept matches")
    assert most_valid >= 17, f"no frame carried 17 or more valid slots ({most_valid}): nothing the narrow tracker could not do"
    assert n_due_total > 0, "no track ever became due: the run checked nothing"
