"""The device tracker (csrc/track.hip, mtgv/track.py) against the host code it restates: mtgv.tracker's KalmanPointTracker
and TrackerCtx, run per stream on the CPU over the scenarios of track_common.  Ids, due sets and the fp64 filter state have
no tolerance: both sides do the same IEEE operations in the same order (the kernel is built without FMA contraction).  The
EWMA is compared with the float32 restatement of the helper, the matches with Matcher.match on the same vectors."""
import functools

import numpy as np
import pytest
import torch

import track_common as tc

pytestmark = pytest.mark.gpu

KAL = ("pos", "vel", "pp", "pv", "vv")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


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


@functools.lru_cache(None)
def _run(name):
    """one pass of a scenario through the host yardstick and through the device, shared by the tests below"""
    scn = tc.SCENARIOS[name]
    host, _, host_trackers = tc.run_host(scn)
    trk, m, Z = _tracker(scn), _matcher(), scn.z()
    dev = []
    for i, st in enumerate(scn.steps):
        quads, n_det, state, where = tc.layout(scn, i)
        cu = lambda a: None if a is None else torch.from_numpy(a).cuda()
        tid, due_idx, n_due_dev = trk.update(cu(quads), st.streams, st.now, n_det=cu(n_det), state=cu(state))
        n_due, due = int(n_due_dev.item()), due_idx.cpu().numpy()
        rec = dict(track_ids=tid.cpu().numpy(), due=due, n_due=n_due, where=where, q=None)
        if n_due:
            z = np.stack([Z[i, st.streams[j // tc.K], j % tc.K] for j in due[:n_due]])
            q = trk.commit(torch.from_numpy(z).cuda())
            ids, scores = trk.store(*m.match(q, tc.TOP_K))
            rec.update(z=z, q=q.cpu().numpy())
        else:
            ids, scores = trk.store()
        rec.update(ids=ids.cpu().numpy(), scores=scores.cpu().numpy(), states=[trk.state(s) for s in range(tc.S)])
        dev.append(rec)
    return scn, host, host_trackers, dev


def _check_state(st, tracks, tag):
    """the live slots of one stream against the host's track list, mapped by creation serial; bit for bit"""
    live = np.flatnonzero(st["live"])
    by_birth = {int(st["birth"][t]): int(t) for t in live}
    assert sorted(by_birth) == sorted(t.birth for t in tracks), f"{tag}: live births {sorted(by_birth)} vs host {[t.birth for t in tracks]}"
    for t in tracks:
        sl = by_birth[t.birth]
        assert int(st["hit_counter"][sl]) == t.hit_counter and bool(st["is_initializing"][sl]) == t.is_initializing, f"{tag} birth {t.birth}"
        assert int(st["id"][sl]) == (t.id or 0), f"{tag} birth {t.birth}: id {st['id'][sl]} vs {t.id}"
        for n in KAL:
            assert (_bits(st[n][sl]) == _bits(getattr(t, n))).all(), f"{tag} birth {t.birth}: {n} {st[n][sl]} vs {getattr(t, n)}"


@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_association(name):
    scn, host, host_trackers, dev = _run(name)
    prev = [None] * tc.S
    for i, (st, rec) in enumerate(zip(scn.steps, dev)):
        assert (rec["due"][: rec["n_due"]] >= 0).all() and (np.diff(rec["due"][: rec["n_due"]]) > 0).all() and (rec["due"][rec["n_due"]:] == -1).all()
        due_dev = {(int(j) // tc.K, int(j) % tc.K) for j in rec["due"][: rec["n_due"]]}
        due_host = set()
        for f, s in enumerate(st.streams):
            h, ks, tag = host[i][f], rec["where"][f], f"{name} step {i} stream {s}"
            got = sorted((int(rec["track_ids"][f, k]), ks.index(k)) for k in range(tc.K) if rec["track_ids"][f, k] > 0 and k in ks)
            assert got == h["matched"], f"{tag}: {got} vs host {h['matched']}"
            assert all(rec["track_ids"][f, k] == 0 for k in range(tc.K) if k not in ks), f"{tag}: an id on a slot that is no detection"
            due_host |= {(f, ks[di]) for _, di in h["due"]}
            _check_state(rec["states"][s], h["tracks"], tag)
            by_id = {int(v): t for t, v in enumerate(rec["states"][s]["id"]) if rec["states"][s]["live"][t] and v > 0}
            for tid_, last in h["last"].items():
                assert rec["states"][s]["last_update_time"][by_id[tid_]] == last, f"{tag}: last_update_time of id {tid_}"
        assert due_dev == due_host, f"{name} step {i}: due {sorted(due_dev)} vs host {sorted(due_host)}"
        for s in range(tc.S):  # a stream that the step does not carry is not touched
            if s not in st.streams and prev[s] is not None:
                assert all((_bits(prev[s][k]) == _bits(rec["states"][s][k])).all() for k in KAL + ("live", "hit_counter", "id", "birth", "avg_z")), (name, i, s)
            prev[s] = rec["states"][s]
    for s in range(tc.S):
        last = dev[-1]["states"][s]
        assert last["next_id"] == host_trackers[s]._next_id
        assert last["overflow"] == getattr(host_trackers[s], "dropped", 0)


def test_overflow_counts_what_the_host_accepted():
    """(j): the device drops exactly the detections for which the uncapped host tracker makes a track and the capped one
    cannot; the other streams run as if nothing happened (test_association compares their state)"""
    scn, _, capped, dev = _run("j_overflow")
    _, peak, _ = tc.run_host(scn, capped=False)
    # nothing ever matches in stream 1, so every detection is a new track for the host: 4 per frame
    n_host = 4 * len(scn.steps)
    n_dev = dev[-1]["states"][1]["next_birth"]
    assert peak[1] > scn.max_tracks and capped[1].dropped > 0
    assert dev[-1]["states"][1]["overflow"] == capped[1].dropped == n_host - n_dev
    assert dev[-1]["states"][0]["overflow"] == 0 and dev[-1]["states"][2]["overflow"] == 0


@pytest.mark.parametrize("name", ["a_drift", "b_gaps", "h_order", "i_gating", "f_delay0"])
def test_ewma_and_matches(name):
    scn, host, _, dev = _run(name)
    m = _matcher()
    avg, kept, n_kept, n_due_total = {}, {}, 0, 0
    for i, (st, rec) in enumerate(zip(scn.steps, dev)):
        due = [int(j) for j in rec["due"][: rec["n_due"]]]
        want_q = []
        for r, j in enumerate(due):
            f, k = divmod(j, tc.K)
            key = (st.streams[f], int(rec["track_ids"][f, k]))
            avg[key] = tc.ewma32(avg.get(key), rec["z"][r], scn.ewma_weight)
            want_q.append(avg[key])
            assert (_bits(avg[key]) == _bits(host[i][f]["avg"][key[1]])).all()  # the helper's restatement is the host's arithmetic
        if due:
            assert (_bits(np.stack(want_q)) == _bits(rec["q"])).all(), f"{name} step {i}: avg_z"
            ids, scores = m.match(torch.from_numpy(np.stack(want_q)).cuda(), tc.TOP_K)  # the production match, called directly
            ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        n_due_total += len(due)
        for f, s in enumerate(st.streams):
            stt = rec["states"][s]
            for k in range(tc.K):
                tid, j = int(rec["track_ids"][f, k]), f * tc.K + k
                if tid == 0:
                    assert (rec["ids"][f, k] == -1).all() and np.isneginf(rec["scores"][f, k]).all(), f"{name} step {i} slot {j}"
                    continue
                if j in due:
                    r = due.index(j)
                    kept[(s, tid)] = (ids[r].copy(), scores[r].copy())
                    slot = [t for t in range(scn.max_tracks) if stt["live"][t] and stt["id"][t] == tid][0]
                    assert stt["has_z"][slot] == 1 and (_bits(stt["avg_z"][slot]) == _bits(avg[(s, tid)])).all()
                    assert (stt["match_ids"][slot] == ids[r]).all() and (_bits(stt["match_scores"][slot]) == _bits(scores[r])).all()
                else:
                    n_kept += 1
                assert (rec["ids"][f, k] == kept[(s, tid)][0]).all() and (_bits(rec["scores"][f, k]) == _bits(kept[(s, tid)][1])).all(), \
                    f"{name} step {i} slot {j} (due: {j in due})"
    assert n_due_total > 4 and n_kept > 4
    if name == "i_gating":
        assert any(r["n_due"] == 0 and (r["track_ids"] > 0).any() for r in dev)


def test_gather():
    """packed rows == crops[due_idx] bytewise: n_due == F * K, n_due == 0 (nothing written) and one in between; both the
    16-byte and the bytewise path"""
    from mtgv.track import DeviceTracker

    F, K = 3, 4
    trk = DeviceTracker(F, K, 8, 1, max_tracks=8, initialization_delay=0)
    cards = np.stack([np.stack([tc.quad(100 + 150 * c, 100 + 10 * f) for c in range(K)]) for f in range(F)])
    n_det = torch.full((F,), K, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    steps = []
    for step, t in enumerate((10.0, 10.1, 10.2)):
        q = cards.copy()
        if step == 2:
            q[1, 2] = tc.quad(5000, 5000)  # one card jumps away: a new track, the only one due
        _, due_idx, n_due = trk.update(torch.from_numpy(q).cuda(), range(F), t, n_det=n_det)
        steps.append(int(n_due.item()))
        due = due_idx.cpu().numpy()
        for shape in ((F * K, 8, 8, 3), (F * K, 5, 7, 3)):
            src = torch.randint(0, 256, shape, generator=g, device="cuda", dtype=torch.uint8)
            out = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
            assert trk.gather(src, out=out) is out
            n = steps[-1]
            assert (out[:n] == src[torch.from_numpy(due[:n]).long().cuda()]).all() and (out[n:] == 7).all()
        if steps[-1]:  # a track stays due until it has an embedding
            trk.commit(torch.ones((steps[-1], 8), device="cuda"))
        trk.store()
    assert steps == [F * K, 0, 1] and due[0] == 1 * K + 2


def test_reset():
    scn = tc.SCENARIOS["f_delay0"]
    trk = _tracker(scn)

    def feed(i):
        quads, n_det, state, _ = tc.layout(scn, i)
        st = scn.steps[i]
        return trk.update(torch.from_numpy(quads).cuda(), st.streams, st.now, n_det=torch.from_numpy(n_det).cuda())[0].cpu().numpy()

    for i in range(4):
        feed(i)
    before = [trk.state(s) for s in range(tc.S)]
    assert all(b["live"].any() and b["next_id"] > 1 for b in before)
    trk.reset(1)
    after = [trk.state(s) for s in range(tc.S)]
    for s in (0, 2):
        assert all((_bits(before[s][k]) == _bits(after[s][k])).all() for k in KAL + ("live", "hit_counter", "is_initializing", "id", "birth", "has_z", "avg_z",
                                                                                  "match_ids", "match_scores", "last_update_time"))
        assert after[s]["next_id"] == before[s]["next_id"] and after[s]["next_birth"] == before[s]["next_birth"]
    assert not after[1]["live"].any() and after[1]["next_id"] == 1 and after[1]["next_birth"] == 0
    trk.reset(-1)
    assert all(not trk.state(s)["live"].any() and trk.state(s)["next_id"] == 1 for s in range(tc.S))
    ids = feed(0)
    assert sorted(ids[0][ids[0] > 0].tolist()) == list(range(1, 1 + int((ids[0] > 0).sum()))) and (ids > 0).any()


def test_more_frames_than_one_launch():
    """update takes 32 frames per launch: 40 streams in reversed frame order, two drifting cards each, against one host
    tracker per stream (ids, due set, filter state of the streams on both sides of the launch boundary)"""
    from mtgv.tracker import KalmanPointTracker
    from mtgv.track import DeviceTracker

    S, K = 40, 2
    trk = DeviceTracker(S, K, 4, 1, max_tracks=4)
    hosts = [KalmanPointTracker() for _ in range(S)]
    order = list(range(S))[::-1]
    n_det = torch.full((S,), K, dtype=torch.int32, device="cuda")
    for step in range(5):
        quads = np.stack([np.stack([tc.quad(100 + 7 * s + 3 * step, 100 + 300 * c + (s % 5) * step) for c in range(K)]) for s in order])
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


def _host_ctx(policy, wait, w):
    from mtgv.tracker import KalmanPointTracker, TrackerCtx

    e, v, c = tc._Enc(), tc._Vecs(), [0.0]
    ctx = TrackerCtx(wait, w, segmenter=lambda fr: [tc._Seg(q, di) for di, q in enumerate(fr)], encoder=e, vecs=v, clock=lambda: c[0], thumbnails=False)
    ctx.tracker = KalmanPointTracker(**policy)
    return ctx, e, v, c


@pytest.mark.parametrize("source", ["mask", "obb"])
def test_tracked_pipeline_end_to_end(source):
    from mtgv import spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher
    from mtgv.pipeline import Pipeline
    from mtgv.track import TrackedPipeline

    F, K, TOP = 3, 4, 3
    policy = {}  # the reference's: ids on a track's third frame, due then and 0.6 s later
    det_cfg = spec.yolo11_config(task="obb") if source == "obb" else spec.DetectorConfig()
    det_sd = spec.random_detector_state(det_cfg, 3, cls_bias=-0.9) if source == "obb" else spec.random_detector_state(det_cfg, 3)
    enc_cfg = spec.encoder_config("cnvnxt2ae_nano", (192, 128), "conv+linear")
    m = Matcher(768, capacity=256)
    m.add(np.random.default_rng(5).standard_normal((200, 768)).astype(np.float32))
    pipe = Pipeline(Detector(det_cfg, det_sd, max_batch=F), Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K), m, K, 1,
                    quad_source=source)
    tp = TrackedPipeline(pipe, streams=F, top_k=TOP, max_tracks=64, **policy)
    # synthetic frames with bright cards on noise that move two pixels per step
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (F, 640, 640, 3), dtype=np.uint8)
    for f in range(F):
        for c in range(3):
            x, y = 60 + 190 * c, 100 + 120 * f
            base[f, y : y + 180, x : x + 120] = 200 + 10 * c
    hosts = [_host_ctx(policy, 0.5, 0.1) for _ in range(F)]
    kept, n_due_total, n_kept = {}, 0, 0
    for step in range(6):
        frames = torch.from_numpy(np.roll(base, 2 * step, axis=2)).cuda()
        now = [50.0 + 0.2 * step + 0.01 * f for f in range(F)]
        out = tp.run(frames, [2, 0, 1], now)
        ref = pipe.run(frames)
        assert (set(out), set(out["det"])) == tc.output_keys(source, tracked=True)
        assert (set(ref), set(ref["det"])) == tc.output_keys(source)
        for k in ("crops", "boxes", "n_det"):
            assert torch.equal(out[k], ref[k]), k
        n_due, due = out["n_due"], out["due_idx"].cpu().numpy()
        assert (due[:n_due] >= 0).all() and (due[n_due:] == -1).all()
        z = None
        if n_due:
            z = pipe.encoder.encode(out["crops"][torch.from_numpy(due[:n_due]).long().cuda()])
            assert torch.equal(tp.last_z, z), "the committed embeddings are not encode(crops[due_idx])"
            z = z.cpu().numpy()
        quads, tids = out["quads"].cpu().numpy(), out["track_ids"].cpu().numpy()
        valid = (out["card_state"].cpu().numpy() > 0) if source == "obb" else (np.arange(K)[None] < np.minimum(out["n_det"].cpu().numpy(), K)[:, None])
        ids, scores = out["ids"].cpu().numpy(), out["scores"].cpu().numpy()
        due_host, queries = set(), {}
        for f, s in enumerate([2, 0, 1]):
            ctx, e, v, c = hosts[s]
            ks = [k for k in range(K) if valid[f, k]]
            c[0] = now[f]
            e.z = {di: z[list(due[:n_due]).index(f * K + k)] for di, k in enumerate(ks) if f * K + k in due[:n_due]}  # a KeyError: the host embeds a slot the device did not
            v.queries = []
            objs = ctx.update([quads[f, k] for k in ks])
            by_id = {t.id: t.last_detection for t in ctx.tracker.tracks if t.id is not None}
            assert sorted((int(tids[f, k]), di) for di, k in enumerate(ks) if tids[f, k] > 0) == [(o.id, by_id[o.id]) for o in objs], (step, s)
            assert all(tids[f, k] == 0 for k in range(K) if k not in ks)
            for o in objs:
                if o.last_update_time == now[f]:
                    due_host.add(f * K + ks[by_id[o.id]])
                    queries[f * K + ks[by_id[o.id]]] = o.avg_z
        assert due_host == set(int(j) for j in due[:n_due]), (step, sorted(due_host), due[:n_due])
        if n_due:  # the host restatement's averaged embeddings through the production match
            want_ids, want_scores = m.match(torch.from_numpy(np.stack([queries[int(j)] for j in due[:n_due]])).cuda(), TOP)
            want_ids, want_scores = want_ids.cpu().numpy(), want_scores.cpu().numpy()
        n_due_total += n_due
        for f, s in enumerate([2, 0, 1]):
            for k in range(K):
                j, tid = f * K + k, int(tids[f, k])
                if tid == 0:
                    assert (ids[f, k] == -1).all() and np.isneginf(scores[f, k]).all()
                    continue
                if j in due[:n_due]:
                    r = list(due[:n_due]).index(j)
                    kept[(s, tid)] = (want_ids[r], want_scores[r])
                else:
                    n_kept += 1
                assert (ids[f, k] == kept[(s, tid)][0]).all() and (_bits(scores[f, k]) == _bits(kept[(s, tid)][1])).all(), (step, j)
    assert n_due_total > 0, "no track ever became due: the run checked nothing"
    print(f"{source}: {n_due_total} embeds in 6 steps of {F * K} crops, {n_kept} slots served from kept matches")
