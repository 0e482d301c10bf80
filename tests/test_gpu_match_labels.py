"""GPU: bank row labels - filtered and distinct-card top-k (mtgv_bank_topk_ex) against the brute-force oracle of
match_labels_common.py.  Ids must be exact; scores within 2e-6 of the fp64 oracle, the existing match tests' bar.

Bank N = 421: three 192-column tiles (the last 37 wide), five 96-column wave ranges, seven 64-column tiles.  b = 130 crosses
the 128-row tile and (with dim % 8 == 0, f16x3) takes the LDS-DMA kernel; b = 1, 5, dim 36 and the f32 mode take the
convert-on-load kernel."""
import functools
import os

import numpy as np
import pytest
import torch

import match_labels_common as L

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
BS, DS, KS = [1, 5, 130], [768, 64, 36], [1, 3, 8]


@pytest.fixture(params=MODES)
def mode(request):
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision(request.param)
    yield request.param
    native.set_gemm_precision(before)


@pytest.fixture
def no_prepass():
    old = os.environ.get("MTGV_MATCH_PREPASS")
    os.environ["MTGV_MATCH_PREPASS"] = "0"
    yield
    if old is None:
        os.environ.pop("MTGV_MATCH_PREPASS", None)
    else:
        os.environ["MTGV_MATCH_PREPASS"] = old


@functools.lru_cache(maxsize=None)
def _case(d):
    """the random bank of dimension d and its fp64 scores, computed once and left unchanged"""
    from oracle import match_ref as M

    case = L.random_case(d)
    return case, M.scores(case[1], case[0])


def _matcher(bank, tags=None, groups=None, capacity=None):
    from mtgv.matcher import Matcher

    m = Matcher(bank.shape[1], capacity=capacity or len(bank) + 3)
    m.add(bank)
    if tags is not None or groups is not None:
        m.set_labels(0, tags, groups)
    return m


def _compare(got, want, what):
    ids, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
    wid, wsc = want
    real = wid >= 0
    err = np.abs(sc[real] - wsc[real]).max() if real.any() else 0.0
    print(f"{what}: {int((ids != wid).sum())} ids differ, max score error {err:.3g}, {int(real.sum())} hits, {int((~real).sum())} pads")
    assert (ids == wid).all(), f"{what}: ids differ from the oracle in rows {sorted(set(np.nonzero(ids != wid)[0].tolist()))[:8]}"
    assert err < 2e-6, what
    assert np.isneginf(sc[~real]).all(), f"{what}: pads must score -inf"


def _check(m, q, s64, tags, groups, masks, distinct, k, thr=None, rows=None, what=""):
    """the labelled match of queries `rows` against the oracle; before it the host check that no query is a near-tie"""
    rows = slice(None) if rows is None else rows
    q, s64 = q[rows], s64[rows]
    flt = None
    if masks is not L.NO_FILTER:
        masks = flt = np.ascontiguousarray(masks[rows])
    assert (L.rep_margin(s64, tags, groups, masks, distinct, k) > 1e-5).all(), "the oracle itself has a near-tie: choose another seed"
    want = L.labelled_topk(s64, tags, groups, masks, distinct, k, thr)
    if thr is not None:
        free = L.labelled_topk(s64, tags, groups, masks, distinct, k)[1]
        assert np.abs(free[np.isfinite(free)] - thr).min() > 1e-5, "a score sits on the threshold"
    got = m.match(q, k, threshold=thr, filter=flt, distinct=distinct)
    _compare(got, want, what)
    return got


def _threshold(s64, tags, groups, masks, distinct, k):
    """a threshold in the widest gap of the central half of the oracle's scores: some hits fall below it, none sits on it"""
    sc = L.labelled_topk(s64, tags, groups, masks, distinct, k)[1]
    v = np.unique(sc[np.isfinite(sc)])
    lo, hi = len(v) // 4, max(len(v) // 4 + 2, 3 * len(v) // 4)
    v = v[lo:hi]
    i = int(np.argmax(np.diff(v)))
    return float((v[i] + v[i + 1]) / 2)


# ---- 1. nothing changes ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("b", BS)
def test_default_labels_change_nothing(mode, no_prepass, b, d, k):
    (bank, q, tags, groups, masks), _ = _case(d)
    m = _matcher(bank)
    qd = torch.from_numpy(q[:b]).cuda()
    ids0, sc0 = m.match(qd, k)
    ids1, sc1 = m.match(qd, k, filter=L.NO_FILTER, distinct=True)  # the labelled kernels on an unlabelled bank
    assert torch.equal(ids0, ids1) and torch.equal(sc0, sc1), "all-default labels must not change a single bit"
    m.set_labels(0, tags, groups)
    m.match(qd, k, filter=masks[:b], distinct=True)
    ids2, sc2 = m.match(qd, k)  # a plain match after labelled ones, on a labelled bank
    assert torch.equal(ids0, ids2) and torch.equal(sc0, sc2)
    m.set_labels(0, np.zeros(L.N, np.uint64), np.full(L.N, -1, np.int32))
    ids3, sc3 = m.match(qd, k, filter=L.NO_FILTER, distinct=True)
    assert torch.equal(ids0, ids3) and torch.equal(sc0, sc3)


# ---- 2. filter ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("b", BS)
def test_filter(mode, b, d, k):
    (bank, q, tags, groups, masks), s64 = _case(d)
    m = _matcher(bank, tags, groups)
    if b == 1:  # every designed query as a batch of its own: no row, fewer than k, ragged tile only, one row in a range
        for i in range(L.N_SPECIAL):
            got = _check(m, q, s64, tags, groups, masks, False, k, rows=slice(i, i + 1), what=f"query {i}")
            if i == 1:
                assert (got[0] == -1).all()
    else:
        got = _check(m, q, s64, tags, groups, masks, False, k, rows=slice(0, b), what=f"b={b}")
        ids = got[0].cpu().numpy()
        assert (ids[1] == -1).all() and (ids[2] >= 0).sum() == min(k, 2)
        assert (ids[3][ids[3] >= 0] >= 384).all() and set(ids[4][ids[4] >= 0]) <= set(L.ROWS_BIT61)


def test_filter_forms(mode):
    """one triple of ints broadcast to all queries, a numpy uint64 array and a torch int64 bit pattern are the same filter"""
    (bank, q, tags, groups, masks), s64 = _case(64)
    m = _matcher(bank, tags, groups)
    b, k = 5, 3
    mk = np.ascontiguousarray(masks[:b])
    a = m.match(q[:b], k, filter=mk)
    t = m.match(q[:b], k, filter=torch.from_numpy(mk.view(np.int64)).cuda())
    assert torch.equal(a[0], t[0]) and torch.equal(a[1], t[1])
    triple = tuple(int(v) for v in masks[4])  # bit 61 alone: a Python int beyond int64's positive range is not needed here
    one = m.match(q[:b], k, filter=triple)
    _compare(one, L.labelled_topk(s64[:b], tags, groups, np.asarray(triple, np.uint64), False, k), "broadcast triple")
    hi = m.match(q[:b], k, filter=(1 << 63, 0, 0))  # the sign bit of the int64 pattern
    assert set(hi[0].cpu().numpy().ravel().tolist()) <= set(L.ROWS_BIT63) | {-1}


# ---- 3. distinct: the hiding case ----
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("b", [1, 130])
def test_distinct_hiding_case(mode, b, d):
    """rows 200..204 (one group) fill their range's three candidates; a merge-only dedupe then answers [204, 30, 400]"""
    from oracle import match_ref as M

    bank, q1, groups = L.hiding_case(d)
    q = np.repeat(q1[None], b, 0) * np.linspace(0.5, 2.0, b, dtype=np.float32)[:, None]
    m = _matcher(bank, None, groups)
    ids, sc = m.match(q, 3, distinct=True)
    print("hiding case:", ids[0].tolist(), sc[0].tolist())
    assert (ids.cpu().numpy() == np.array([204, 210, 30])).all()
    _compare((ids, sc), L.labelled_topk(M.scores(q, bank), np.zeros(L.N, np.uint64), groups, L.NO_FILTER, True, 3), "hiding case")
    ids, _ = m.match(q, 3)  # without distinct: three printings of the best card
    assert (ids.cpu().numpy() == np.array([204, 203, 202])).all()


# ---- 4. distinct: exact ties ----
@pytest.mark.parametrize("k", [3, 100])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("b", [1, 130])
def test_distinct_ties(mode, b, d, k):
    """exact duplicates decide by id inside one group and across two; a group over several tiles; k beyond a range and
    beyond the number of groups pads.  (The deliberate ties are exempt from the gap check; the oracle orders them by id.)"""
    from oracle import match_ref as M

    bank, q1, groups = L.ties_case(d)
    q = np.repeat(q1[None], b, 0)
    m = _matcher(bank, None, groups)
    got = m.match(q, k, distinct=True)
    want = L.labelled_topk(M.scores(q, bank), np.zeros(L.N, np.uint64), groups, L.NO_FILTER, True, k)
    _compare(got, want, f"ties k={k}")
    ids = got[0].cpu().numpy()
    assert ids[0, :3].tolist() == [10, 20, 21]
    if k == 100:
        assert ids[0, 3] == 150 and (ids[:, :11] >= 0).all() and (ids[:, 11:] == -1).all()


# ---- 5. combined ----
@pytest.mark.parametrize("variant", ["distinct", "both"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("b", BS)
def test_filter_distinct_threshold(mode, b, d, k, variant):
    case, s64 = _case(d)
    bank, q, tags, groups, _ = case
    masks, distinct = L.variant_labels(case, variant)
    m = _matcher(bank, tags, groups)
    rows = slice(0, b) if b > 1 else slice(5, 6)  # (b = 1: an ordinary query; test_filter runs the designed ones)
    got = _check(m, q, s64, tags, groups, masks, distinct, k, rows=rows, what=f"{variant}")
    g = groups[np.maximum(got[0].cpu().numpy(), 0)]
    for row_ids, row_g in zip(got[0].cpu().numpy(), g):
        kept = row_g[(row_ids >= 0) & (row_g >= 0)]
        assert len(kept) == len(set(kept.tolist())), "two hits share a group"
    mk = masks if masks is L.NO_FILTER else masks[rows]
    thr = _threshold(s64[rows], tags, groups, mk, distinct, max(k, 3))
    _check(m, q, s64, tags, groups, masks, distinct, k, thr=thr, rows=rows, what=f"{variant} thr={thr:.4f}")


def test_id_base_is_added_and_labels_are_local():
    from mtgv.matcher import Matcher

    (bank, q, tags, groups, masks), s64 = _case(64)
    m = Matcher(64, capacity=L.N, id_base=1000)
    m.add(bank)
    m.set_labels(0, tags, groups)
    ids, sc = m.match(q[:5], 3, filter=masks[:5], distinct=True)
    wid, wsc = L.labelled_topk(s64[:5], tags, groups, masks[:5], True, 3)
    _compare((ids, sc), (np.where(wid >= 0, wid + 1000, -1), wsc), "id_base")


# ---- 6. the pre-pass is bypassed ----
def _launches(fn, csv):
    """(sp, topk) of the GEMM launches fn makes (the launch profiler's table)"""
    from mtgv import native as nv

    lib = nv.lib()
    nv.check(lib.mtgv_profile_gemm(1))
    try:
        out = fn()
        torch.cuda.synchronize()
        nv.check(lib.mtgv_profile_gemm_dump(csv.encode()))
    finally:
        nv.check(lib.mtgv_profile_gemm(0))
    lines = open(csv).read().split()
    col = {name: i for i, name in enumerate(lines[0].split(","))}
    rows = [ln.split(",") for ln in lines[1:]]
    return out, [(int(r[col["sp"]]), int(r[col["topk"]])) for r in rows]


def test_labelled_match_bypasses_the_prepass(tmp_path):
    from mtgv import native
    from oracle import match_ref as M

    before = native.get_gemm_precision()
    native.set_gemm_precision("f16x3")
    old = os.environ.pop("MTGV_MATCH_PREPASS", None)
    try:
        bank, q, tags, groups, masks = L.big_case()
        m = _matcher(bank, tags, groups, capacity=L.BIG_N)
        qd = torch.from_numpy(q).cuda()
        _, plain = _launches(lambda: m.match(qd, L.BIG_K), str(tmp_path / "plain.csv"))
        assert plain == [(3, 2)], plain  # the fp16 first pass: two candidates per wave range
        got, lab = _launches(lambda: m.match(qd, L.BIG_K, filter=masks, distinct=True), str(tmp_path / "lab.csv"))
        assert lab == [(1, L.BIG_K)], lab  # the one-pass exact kernel on the LDS-DMA path
        s64 = M.scores(q, bank)
        assert (L.rep_margin(s64, tags, groups, masks, True, L.BIG_K) > 1e-5).all()
        _compare(got, L.labelled_topk(s64, tags, groups, masks, True, L.BIG_K), "5000 x 768, b = 129")
    finally:
        if old is not None:
            os.environ["MTGV_MATCH_PREPASS"] = old
        native.set_gemm_precision(before)


# ---- 7. lifecycle ----
def test_labels_lifecycle():
    (bank, q, tags, groups, masks), s64 = _case(36)
    m = _matcher(bank[:300], capacity=L.N)
    t, g = m.labels(0, 300)
    assert (t == 0).all() and (g == -1).all() and t.dtype == np.uint64 and g.dtype == np.int32  # never labelled: defaults
    m.set_labels(10, tags[10:300], None)  # tags alone: groups stay
    m.set_labels(0, None, groups[:300])
    t, g = m.labels(0, 300)
    assert (t[10:] == tags[10:300]).all() and (t[:10] == 0).all() and (g == groups[:300]).all()
    m.set_labels(0, tags[:10])
    m.add(bank[300:])  # appended rows get the defaults
    t, g = m.labels(300, L.N - 300)
    assert (t == 0).all() and (g == -1).all()
    m.set_labels(300, tags[300:], groups[300:])
    _check(m, q, s64, tags, groups, masks, True, 3, rows=slice(0, 5), what="after append")
    # set_row keeps the row's labels: an upsert changes the vector, not the card
    m.set_row(57, bank[58])
    t, g = m.labels(57, 1)
    assert t[0] == tags[57] and g[0] == groups[57]
    m.clear()
    assert len(m) == 0
    m.add(bank)
    t, g = m.labels(0, L.N)
    assert (t == 0).all() and (g == -1).all(), "clear must reset the labels"
    ids0 = m.match(q[:5], 3)[0]
    assert torch.equal(ids0, m.match(q[:5], 3, filter=L.NO_FILTER, distinct=True)[0])


def _store12():
    from mtgv.adapters import QdrantPoint, VectorStoreQdrant

    rng = np.random.default_rng(21)
    base = rng.standard_normal((4, 768)).astype(np.float32)
    store = VectorStoreQdrant(capacity=32)
    pts = []
    for i in range(12):  # four cards, three printings each, the printings close to their card; the last point has no oracle_id
        v = base[i % 4] + 0.05 * (1 + i // 4) * rng.standard_normal(768).astype(np.float32)
        payload = {"oracle_id": f"card-{i % 4}", "set": f"s{i // 4}"} if i < 11 else {"set": "s2"}
        pts.append(QdrantPoint(id=f"00000000-0000-0000-0000-{i:012d}", vector=v.tolist(), payload=payload))
    store.save_points(pts)
    return store, pts, base


def test_store_groups_save_load(tmp_path):
    from mtgv.bank import load_store, save_store

    store, pts, base = _store12()
    save_store(store, str(tmp_path / "plain"))
    assert sorted(np.load(str(tmp_path / "plain.npz")).files) == ["ids", "vectors"]  # unlabelled: the file of before
    table = store.group_by_payload("oracle_id")
    assert table == {f"card-{c}": c for c in range(4)}
    t, g = store._bank.labels(0, 12)
    assert g.tolist() == [0, 1, 2, 3] * 2 + [0, 1, 2, -1]
    store.set_labels([p.id for p in pts], tags=[1 << (i // 4) for i in range(12)])  # bit = the printing's set
    q = base[0].tolist()
    plain = store.query_nearby(q, k=3)
    assert [p.payload.get("oracle_id") for p in plain] == ["card-0"] * 3  # three printings of one card
    hits = store.query_nearby(q, k=3, distinct=True)
    assert hits[0].id == plain[0].id and len(hits) == 3
    keys = [h.payload.get("oracle_id") for h in hits]
    assert len([x for x in keys if x is not None]) == len(set(x for x in keys if x is not None))
    only_s1 = store.query_nearby(q, k=12, tags_all=1 << 1)
    assert len(only_s1) == 4 and all(h.payload["set"] == "s1" for h in only_s1)
    not_s0 = store.query_nearby_batch([q, base[1].tolist()], k=2, tags_none=1 << 0, distinct=True)
    assert all(h.payload["set"] != "s0" for hs in not_s0 for h in hs) and not_s0[1][0].payload["oracle_id"] == "card-1"
    with pytest.raises(KeyError):
        store.set_labels(["no-such-id"], tags=[1])
    save_store(store, str(tmp_path / "lab"))
    again = load_store(str(tmp_path / "lab"), capacity=32)
    t2, g2 = again._bank.labels(0, 12)
    assert (t2 == store._bank.labels(0, 12)[0]).all() and (g2 == g).all()
    assert [h.id for h in again.query_nearby(q, k=3, distinct=True)] == [h.id for h in hits]
    old = load_store(str(tmp_path / "plain"), capacity=32)  # a file without labels loads as before
    assert [h.id for h in old.query_nearby(q, k=3)] == [h.id for h in plain] and not old._bank.labelled


class _StubPipeline:
    """what TrackedPipeline touches of a Pipeline, fed by a tracker scenario: the detector reports the step's quads, a crop
    carries its (stream, slot) in its first two bytes and the encoder turns that into the scenario's embedding"""

    quad_source = "mask"

    def __init__(self, scn, matcher, tc):
        self.scn, self.matcher, self.K, self.step, self.tc = scn, matcher, tc.K, 0, tc
        self.z = torch.from_numpy(scn.z()).cuda()
        stub = self

        class Det:
            device = torch.device("cuda", torch.cuda.current_device())

            def forward(self, frames, flip_rgb, mask_rows=0):
                quads, n_det, _, _ = tc.layout(stub.scn, stub.step)
                return {"n_det": torch.from_numpy(n_det).cuda(), "quads": torch.from_numpy(quads).cuda()}

        class Enc:
            class cfg:
                z_size = tc.DIM

            def encode(self, crops):
                return stub.z[stub.step, crops[:, 0].long(), crops[:, 1].long()].contiguous()

        self.detector, self.encoder = Det(), Enc()

    def crop(self, frames_u8, det, lease=None, src=None):
        from mtgv.pipeline import Cropped

        streams = self.scn.steps[self.step].streams
        crops = torch.zeros((len(streams) * self.K, 4), dtype=torch.uint8, device="cuda")
        crops[:, 0] = torch.tensor(streams, device="cuda").repeat_interleave(self.K)
        crops[:, 1] = torch.arange(self.K, device="cuda").repeat(len(streams))
        return Cropped(None, crops, det["quads"].reshape(-1, 4, 2))

    def _thumbnails(self, cropped):
        return cropped


def test_tracked_pipeline_distinct_matches():
    """TrackedPipeline(match_opts={"distinct": True}) on the steady-drift scenario: every track's kept matches have pairwise
    different groups, and they are what the matcher answers for the track's query"""
    import track_common as tc
    from mtgv.matcher import Matcher
    from mtgv.track import TrackedPipeline

    scn = tc.SCENARIOS["a_drift"]
    rng = np.random.default_rng(31)
    cards = rng.standard_normal((8, tc.DIM)).astype(np.float32)
    bank = np.repeat(cards, 8, 0) + 0.05 * rng.standard_normal((64, tc.DIM)).astype(np.float32)  # 8 cards x 8 printings
    groups = np.repeat(np.arange(8), 8).astype(np.int32)
    m = Matcher(tc.DIM, capacity=tc.BANK_ROWS)
    m.add(bank)
    m.set_labels(0, None, groups)
    results = {}
    for opts in (None, {"distinct": True}):
        pipe = _StubPipeline(scn, m, tc)
        tp = TrackedPipeline(pipe, streams=tc.S, top_k=tc.TOP_K, max_tracks=tc.MAX_TRACKS, match_opts=opts)
        kept = []
        for i, st in enumerate(scn.steps):
            pipe.step = i
            out = tp.run(torch.zeros((len(st.streams), 1, 1, 3), dtype=torch.uint8, device="cuda"), st.streams, st.now)
            kept.append(out["ids"].cpu().numpy())
        results[bool(opts)] = np.concatenate([k.reshape(-1, tc.TOP_K) for k in kept])
    plain, dist = results[False], results[True]
    assert (dist[:, 0] >= 0).sum() > 10, "no track ever got matches"
    assert (plain[:, 0] == dist[:, 0]).all()  # the best hit is the same row
    for row in dist[dist[:, 0] >= 0]:
        assert (row >= 0).all() and len(set(groups[row].tolist())) == tc.TOP_K, row
    shared = [len(set(groups[row].tolist())) < tc.TOP_K for row in plain[plain[:, 0] >= 0]]
    assert any(shared), "the plain match never returned two printings of one card: the scenario shows nothing"


# ---- 8. errors ----
def test_errors():
    (bank, q, tags, groups, masks), _ = _case(36)
    m = _matcher(bank)
    with pytest.raises(AssertionError, match="group"):
        m.set_labels(0, None, [0, -2, 3])
    assert (m.labels(0, 3)[1] == -1).all()  # refused as a whole
    with pytest.raises(AssertionError, match="outside"):
        m.set_labels(L.N - 1, [1, 2])
    with pytest.raises(AssertionError, match="outside"):
        m.labels(L.N, 1)
    with pytest.raises(AssertionError, match="NaN"):
        m.match(q[:2], 3, threshold=float("nan"), distinct=True)
    for bad in (masks[:3], masks[:2, :2], masks[:2].astype(np.int64), torch.zeros((2, 3), dtype=torch.int32), (1, 2)):
        with pytest.raises(AssertionError, match="filter"):
            m.match(q[:2], 3, filter=bad)
