"""CPU-only checks around the wide device tracker: mtgv_tracker_create_ex refuses what it must before any HIP call, and the
wide scenarios of track_wide_common are what their names promise, read off the host tracker alone - a wide GPU test that
never leaves wave 0 would show nothing."""
import ctypes as C

import numpy as np
import pytest

import track_wide_common as tw

WIDE = 1  # MTGV_TRACKER_WIDE


def _create_ex(flags, **kw):
    from mtgv import native

    cfg = native.TrackerCfg(streams=3, max_tracks=8, cards_per_frame=4, dim=32, top_k=3)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = native.c_vp(0)
    return native.lib().mtgv_tracker_create_ex(C.byref(cfg), flags, C.byref(h)), h


@pytest.mark.parametrize("flags,bad", [(0, dict(max_tracks=65)), (0, dict(cards_per_frame=17)), (WIDE, dict(max_tracks=257)),
                                       (WIDE, dict(cards_per_frame=65)), (WIDE, dict(max_tracks=0)), (WIDE, dict(cards_per_frame=0)), (2, {}),
                                       (3, {}), (-1, {})])
def test_create_ex_refuses_without_a_gpu(flags, bad):
    from mtgv import native

    rc, h = _create_ex(flags, **bad)
    assert rc == 1 and not h.value and b"tracker" in native.lib().mtgv_last_error(), native.lib().mtgv_last_error()


def test_create_ex_null_arguments_and_version():
    from mtgv import native

    L = native.lib()
    assert L.mtgv_version() >= 110
    assert native.TRACKER_WIDE == WIDE
    h = native.c_vp(0)
    assert L.mtgv_tracker_create_ex(None, WIDE, C.byref(h)) == 1 and b"tracker" in L.mtgv_last_error() and not h.value
    cfg = native.TrackerCfg(streams=1, max_tracks=200, cards_per_frame=40, dim=4, top_k=1)
    assert L.mtgv_tracker_create_ex(C.byref(cfg), WIDE, None) == 1 and b"tracker" in L.mtgv_last_error()


def test_the_wrapper_chooses_the_handle_by_size(monkeypatch):
    """wide=None: the wide handle iff max_tracks > 64 or cards_per_frame > 16; True / False force it (no GPU: the create
    call is recorded, not made)"""
    import torch

    from mtgv import native, track

    calls = []

    class _Lib:
        def mtgv_tracker_create_ex(self, cfg, flags, out):
            calls.append(flags)
            return 0

    monkeypatch.setattr(native, "require_gpu", lambda: None)
    monkeypatch.setattr(native, "lib", lambda: _Lib())
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    monkeypatch.setattr(track.DeviceTracker, "__del__", lambda self: None)
    for kw, want in ((dict(max_tracks=64), 0), (dict(max_tracks=65), WIDE), (dict(cards=17), WIDE), (dict(wide=True), WIDE),
                     (dict(max_tracks=65, wide=False), 0), (dict(cards=64, max_tracks=256), WIDE)):
        kw = dict(kw)
        t = track.DeviceTracker(2, kw.pop("cards", 16), 8, 1, device="cuda:0", **kw)
        assert calls[-1] == want and t.wide == bool(want), kw


def test_sizes():
    assert tw.SIZES == {"W2": (65, 17), "W3": (128, 33), "W4": (256, 64)}
    for scn in tw.scenarios().values():
        assert len(scn.steps) <= 16 and scn.n_streams <= 3 and 1 <= scn.max_tracks <= 256 and 1 <= scn.k <= 64
        assert all(len(d) <= scn.k for st in scn.steps for d in st.dets)
        for st in scn.steps:  # integer pixels
            for d in st.dets:
                a = np.stack(d) if d else np.zeros((0,))
                assert (a[~np.isnan(a)] == np.round(a[~np.isnan(a)])).all()


@pytest.mark.parametrize("name", sorted(tw.scenarios()))
def test_scenario_respects_the_slot_cap(name):
    """the uncapped host tracker holds more than T tracks only where the scenario is meant to overflow, and there only in
    stream 1"""
    scn = tw.scenarios()[name]
    _, peak, _ = tw.run_host(name, False)
    if scn.capped:
        assert peak[1] > scn.max_tracks and peak[0] <= scn.max_tracks and peak[2] <= scn.max_tracks, peak
        assert tw.run_host(name)[2][1].dropped > 0
    else:
        assert max(peak) <= scn.max_tracks, peak


def test_fill_reaches_every_wave():
    """the live count of stream 1 climbs past 64 (W2, W3), past 128 and 192 to T (W4), and the sets keep being re-matched"""
    for name, above in (("fill_W2", (64,)), ("fill_W3", (64,)), ("fill_W4", (64, 128, 192))):
        scn = tw.scenarios()[name]
        host, peak, _ = tw.run_host(name)
        live = [fr[1]["n_live"] for fr in host]
        assert all(any(n > a for n in live) for a in above), (name, live)
        assert max(live) == (scn.max_tracks if scn.capped else (scn.max_tracks // scn.k) * scn.k), (name, live)
        assert live == sorted(live)  # nothing dies: every set is seen again in time
        n_sets = -(-max(live) // scn.k)
        assert all(len(host[i][1]["matched"]) >= scn.k - 3 for i in (n_sets, n_sets + 1)), name  # re-matched, with ids
    assert tw.run_host("fill_W4")[2][1].dropped == 64 and tw.run_host("fill_W2")[2][1].dropped > 0


def _mean_dist(q, pos):
    return float(np.linalg.norm(np.asarray(q, np.float64) - np.asarray(pos, np.float64).reshape(4, 2), axis=1).mean())


def test_ties_are_ties():
    scn, (host, _, _) = tw.scenarios()["ties"], tw.run_host("ties")
    for s, (birth_a, birth_b) in ((0, (64, 65)), (1, (0, 64))):  # streams 0 and 1: two initialised tracks, one detection
        before = {t.birth: t for t in host[6][s]["tracks"]}
        a, b = before[birth_a], before[birth_b]
        assert a.id == 1 and b.id == 2 and not a.is_initializing and not b.is_initializing
        assert (a.vel == 0).all() and (b.vel == 0).all()  # stationary: the prediction of step 7 is the position itself
        mid = scn.steps[7].dets[s][0]
        assert _mean_dist(mid, a.pos) == _mean_dist(mid, b.pos) == 50.0
        assert host[7][s]["matched"] == [(1, 0)], "the older track takes the detection"
    # stream 0: the fillers of slots 0..63 are gone when B is born, stream 1: they are alive (so B is born behind them)
    assert host[2][0]["n_live"] == 65 and host[3][0]["n_live"] == 2 and host[1][1]["n_live"] == 65
    for j, (step, lo) in enumerate(((4, 15), (5, 31), (6, 62))):  # stream 2: one track, two detections
        t = [t for t in host[step - 1][2]["tracks"] if t.id == j + 1][0]
        d = scn.steps[step].dets[2]
        assert (t.vel == 0).all() and _mean_dist(d[lo], t.pos) == _mean_dist(d[lo + 1], t.pos) == 50.0
        assert not np.array_equal(d[lo], d[lo + 1]) and (j + 1, lo) in host[step][2]["matched"], "the lower index wins"
        assert len(d) == 64


def test_full_frame_crosses_the_waves():
    host, _, _ = tw.run_host("full")
    wave = lambda birth: birth // 64  # nothing is recycled in this scenario: slot == birth (the GPU test checks it)
    # step 4: 64 initialising tracks of all four waves get their ids in one frame, in the order of the matches
    new = host[4][1]["new_ids"]
    assert len(new) == 64 and {wave(b) for b in new.values()} == {0, 1, 2, 3}
    order = [wave(new[i]) for i in sorted(new)]
    assert sum(a != b for a, b in zip(order, order[1:])) >= 16, "successive winners come from different waves"
    assert [new[i] for i in sorted(new)] != sorted(new.values()), "ids follow the matches, not the slots"
    # step 5: 60 initialised tracks (phase 0) from all four waves, and four initialising ones take what is left (phase 1)
    got = host[5][1]
    old = {t.id: t.birth for t in host[4][1]["tracks"] if t.id is not None}
    assert len(got["matched"]) == 64 and len(got["new_ids"]) == 4
    assert {wave(old[i]) for i, _ in got["matched"] if i in old} == {0, 1, 2, 3}
    assert len({wave(b) for b in got["new_ids"].values()}) >= 2
    # each detection of step 5 is within the threshold of several tracks
    tracks = host[4][1]["tracks"]
    for q in tw.scenarios()["full"].steps[5].dets[1]:
        assert sum(_mean_dist(q, t.pos + t.vel) < 300.0 for t in tracks) >= 3


def test_alloc_recycles_in_three_waves():
    host, peak, _ = tw.run_host("alloc")
    live = [fr[1]["n_live"] for fr in host]
    assert live[2] == 180 and live[3] == 180 and live[4] == 179 and live[5] == 178 and live[6] == 180, live
    assert live[9] == 180 and live[10] == 180 and peak[1] == 180, live
    births = lambda i: {t.birth for t in host[i][1]["tracks"]}
    assert births(6) - births(5) == {180, 181, 182} and births(5) - births(6) == {130} and births(10) - births(9) == {183}
    assert births(9) - births(10) == {178}
    assert sorted(tw.ALLOC_SLOT_OF_BIRTH) == [180, 181, 182, 183]


def test_layouts_and_nan():
    for name in ("holes_state", "holes_both"):
        scn = tw.scenarios()[name]
        ks = [k for i in range(len(scn.steps)) for w in tw.layout(scn, i)[3] for k in w]
        assert min(ks) == 0 and max(ks) == 63 and len(set(ks)) > 48  # holes over all 64 slots
    scn = tw.scenarios()["holes_both"]
    assert any((state[f, n:] > 0).any() for i in range(len(scn.steps)) for _, n_det, state, _ in [tw.layout(scn, i)] for f, n in enumerate(n_det))
    host, _, _ = tw.run_host("nan_high")
    assert np.isnan(tw.scenarios()["nan_high"].steps[3].dets[0][17]).any()
    nan_tracks = [t for t in host[4][0]["tracks"] if np.isnan(t.pos).any()]
    assert nan_tracks and all(t.id is None for t in nan_tracks)
    host, _, _ = tw.run_host("gating")
    assert any(all(f["matched"] and not f["due"] for f in fr) for fr in host) and max(len(f["due"]) for fr in host for f in fr) == 40
