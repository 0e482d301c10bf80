"""CPU-only checks around the device tracker: the scenarios respect the slot cap the tests may rely on, the library refuses
bad tracker configurations without a GPU, the Python wrapper refuses bad stream lists before it calls the library, and the
float32 EWMA restatement of the test helper is TrackerCtx's arithmetic."""
import ctypes as C

import numpy as np
import pytest

import track_common as tc


@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_scenario_respects_the_slot_cap(name):
    """(a)-(i): the host tracker never holds more than max_tracks tracks per stream, so the device may not differ;
    (j): it does, and only there"""
    scn = tc.SCENARIOS[name]
    _, peak, _ = tc.run_host(scn, capped=False)
    assert len(scn.steps) <= 16 and all(len(d) <= tc.K for st in scn.steps for d in st.dets)
    if scn.capped:
        assert max(peak) > scn.max_tracks and peak[0] <= scn.max_tracks and peak[2] <= scn.max_tracks, peak
    else:
        assert max(peak) <= scn.max_tracks, peak


def test_scenarios_hit_their_cases():
    """what the scenario names promise, read off the host tracker alone"""
    host = {n: tc.run_host(s)[0] for n, s in tc.SCENARIOS.items()}
    # (b) a track survives a short gap under its id and comes back under a new one after the long gap
    ids_b = [sorted(i for i, _ in fr[1]["matched"]) for fr in host["b_gaps"]]  # stream 1: the 7-frame gap
    assert max(max(i, default=0) for i in ids_b) >= 4
    # (c) the tie between two tracks goes to the older one: in frame 4 of stream 1 id 1 is matched, id 2 is not
    assert [i for i, _ in host["c_ties"][4][1]["matched"]] == [1]
    assert host["c_ties"][4][0]["matched"] == [(1, 0)]  # two detections, equal distance: the lower index
    assert host["c_ties"][4][2]["matched"] == [(1, 0)]  # the initialised (younger) track wins against the initialising one
    # (d) exactly 300 is not a match
    assert host["d_threshold"][4][0]["matched"] == [] and host["d_threshold"][5][0]["matched"] == [(1, 0)]
    # (e) the tie goes to B (id 1, born first) although C (id 2) would sit in the lower slot
    assert host["e_recycle"][13][0]["matched"] == [(1, 0)] and any(i == 2 for i, _ in host["e_recycle"][12][0]["matched"])
    # (f) ids at creation
    assert host["f_delay0"][0][0]["matched"] and host["f_period3"][0][0]["matched"]
    # (g) the NaN quad makes tracks that never get an id
    assert any(np.isnan(t.pos).any() for fr in host["g_nan"][4] for t in fr["tracks"])
    # (i) steps with matched tracks and nothing due, and tracks due when they get their id
    empties = [i for i, fr in enumerate(host["i_gating"]) if all(f["matched"] and not f["due"] for f in fr)]
    assert empties and host["i_gating"][2][0]["due"] == host["i_gating"][2][0]["matched"] != []


def _create(**kw):
    from mtgv import native

    cfg = native.TrackerCfg(streams=3, max_tracks=8, cards_per_frame=4, dim=32, top_k=3)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = native.c_vp(0)
    return native.lib().mtgv_tracker_create(C.byref(cfg), C.byref(h)), h


@pytest.mark.parametrize("bad", [dict(streams=0), dict(max_tracks=65), dict(max_tracks=0), dict(cards_per_frame=17), dict(cards_per_frame=0),
                                 dict(top_k=0), dict(top_k=9), dict(dim=0), dict(distance_threshold=-1.0), dict(distance_threshold=float("nan")),
                                 dict(hit_counter_max=-1), dict(period=-1), dict(initialization_delay=-2), dict(ewma_weight=1.5),
                                 dict(update_wait_sec=float("nan"))])
def test_create_refuses_bad_configurations_without_a_gpu(bad):
    from mtgv import native

    rc, h = _create(**bad)
    assert rc == 1 and not h.value and b"tracker" in native.lib().mtgv_last_error()
    with pytest.raises(AssertionError):
        native.check(rc)


def test_create_null_cfg_and_version():
    from mtgv import native

    L = native.lib()
    assert L.mtgv_version() >= 104
    h = native.c_vp(0)
    assert L.mtgv_tracker_create(None, C.byref(h)) == 1 and b"null" in L.mtgv_last_error()
    assert L.mtgv_tracker_create(C.byref(native.TrackerCfg(streams=1, max_tracks=1, cards_per_frame=1, dim=4, top_k=1)), None) == 1
    assert L.mtgv_tracker_reset(None, -1, None) == 1 and L.mtgv_tracker_commit(None, None, None, 1, None) == 1
    assert L.mtgv_tracker_gather_u8(None, 0, 16, None, None, 4, None, None) == 1


def test_wrapper_refuses_bad_stream_lists_before_the_library(monkeypatch):
    from mtgv import native
    from mtgv.track import DeviceTracker, check_streams

    assert check_streams([2, 0, 1], 3).tolist() == [2, 0, 1] and check_streams([1], 3).dtype == np.int32
    for bad in ([0, 0], [0, 1, 1], [3], [-1, 0], []):
        with pytest.raises(AssertionError):
            check_streams(bad, 3)
    monkeypatch.setattr(native, "lib", lambda: pytest.fail("the library was called"))
    trk = object.__new__(DeviceTracker)  # no GPU here: the argument check comes before anything that needs one
    trk.streams, trk.K, trk._h = 3, 4, None
    for bad in ([1, 1], [0, 5]):
        with pytest.raises(AssertionError, match="stream"):
            trk.update(None, bad, 0.0)


def test_policy_zero_forms():
    """0 in mtgv_tracker_cfg means `the reference's value`: the wrapper sends the two policies where 0 is a value of its own
    in the forms the header names for them, and refuses zeros that cannot be expressed"""
    from mtgv import native
    from mtgv.track import _policy_cfg

    cfg = native.TrackerCfg()
    _policy_cfg(cfg, dict(initialization_delay=0, update_wait_sec=0.0, period=3, ewma_weight=None))
    assert cfg.initialization_delay == -1 and 0.0 < cfg.update_wait_sec < 1e-300 and cfg.period == 3 and cfg.ewma_weight == 0.0
    with pytest.raises(AssertionError):
        _policy_cfg(native.TrackerCfg(), dict(distance_threshold=0))
    with pytest.raises(AssertionError):
        _policy_cfg(native.TrackerCfg(), dict(threshold=3))


def test_ewma_restatement_is_tracker_ctx_arithmetic():
    rng = np.random.default_rng(0)
    for w in (0.1, 0.25, 0.5, 1.0 / 3.0):
        z = rng.standard_normal((64, tc.DIM)).astype(np.float32) * 10
        avg = None
        for row in z:
            a = row if avg is None else avg
            want = w * row + (1 - w) * a  # mtgv/tracker.py:303-305
            avg = tc.ewma32(avg, row, w)
            assert want.dtype == np.float32 and (want.view(np.int32) == avg.view(np.int32)).all()
    # and the host run of a scenario carries exactly these vectors
    scn = tc.SCENARIOS["i_gating"]
    host, _, _ = tc.run_host(scn)
    Z, seen = scn.z(), 0
    for i, frames in enumerate(host):
        for f, fr in enumerate(frames):
            s, where = scn.steps[i].streams[f], tc.layout(scn, i)[3][f]
            for tid, di in fr["due"]:
                want = tc.ewma32(fr["prev"][tid], Z[i, s, where[di]], scn.ewma_weight)
                assert (want.view(np.int32) == fr["avg"][tid].view(np.int32)).all()
                seen += 1
    assert seen > 6
