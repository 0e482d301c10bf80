"""GPU: row labels across the sharded exchange - Matcher.match_packed(filter=, distinct=) on every shard, the packed words
stacked as an all-gather would deliver them, merge_gathered(distinct=) - against the single-bank labelled match
(mtgv_bank_topk_ex: ids and score bits identical) and the fp64 oracle of match_labels_common.py (ids).  Shards are separate
Matcher handles on one GPU; the last test runs ShardedMatcher and Pipeline(match_opts=) through RCCL with one rank."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dist_labels_common as D
import match_labels_common as L
from conftest import ROOT

pytestmark = pytest.mark.gpu

B = L.B_MAX
VARIANTS = ["filter", "distinct", "both"]


@functools.lru_cache(maxsize=None)
def _case(d):
    """the random bank of dimension d, its fp64 scores and its queries on the device: computed once, left unchanged"""
    from oracle import match_ref as M

    case = L.random_case(d)
    return case, M.scores(case[1], case[0]), torch.from_numpy(case[1]).cuda()


def _matcher(bank, tags, groups, lo=0, hi=None):
    """rows [lo, hi) of a bank as a Matcher with id_base lo, labelled by global row through its own slice"""
    from mtgv.matcher import Matcher

    hi = len(bank) if hi is None else hi
    m = Matcher(bank.shape[1], capacity=max(1, hi - lo), id_base=lo)
    if hi > lo:
        m.add(bank[lo:hi])
        m.set_labels(0, None if tags is None else tags[lo:hi], groups[lo:hi])
    return m


@functools.lru_cache(maxsize=None)
def _random_matchers(d, R):
    (bank, _, tags, groups, _), _, _ = _case(d)
    return [_matcher(bank, tags, groups, lo, hi) for lo, hi in D.shards(L.N, R)]


def _exchange(shards, q, k, flt, distinct):
    """what the all-gather of the packed candidates delivers: (R, B, k, 2) int64"""
    return torch.stack([m.match_packed(q, k, filter=flt, distinct=distinct) for m in shards]).contiguous()


def _same(got, want, what):
    """ids and score BITS identical"""
    assert torch.equal(got[0], want[0]), f"{what}: ids differ in queries {torch.nonzero((got[0] != want[0]).any(1)).flatten()[:8].tolist()}"
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), f"{what}: score bits differ"


def _groups_carried(gathered, groups):
    """the high halves of the packed words are the rows' groups; pads carry id -1, -inf and group -1"""
    ids, sc, g = D.unpack(gathered.cpu().numpy())
    assert (g == np.where(ids >= 0, np.asarray(groups)[np.maximum(ids, 0)], -1)).all()
    assert np.isneginf(sc[ids < 0]).all() and np.isfinite(sc[ids >= 0]).all()


# ---- 1. the labelled exchange against the single bank ----
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("R", [2, 3, 7])
@pytest.mark.parametrize("d", [768, 36])
def test_exchange_equals_single_bank(d, R, k):
    from mtgv.matcher import merge_gathered

    (bank, q, tags, groups, masks), s64, qd = _case(d)
    full = _random_matchers(d, 1)[0]
    shards = _random_matchers(d, R)
    for variant in VARIANTS:
        mk, distinct = L.variant_labels((None, None, tags, groups, masks), variant)
        flt = None if mk is L.NO_FILTER else mk
        assert (L.rep_margin(s64, tags, groups, mk, distinct, k) > 1e-5).all(), "the oracle itself has a near-tie: choose another seed"
        want = full.match(qd, k, filter=flt, distinct=distinct)
        gathered = _exchange(shards, qd, k, flt, distinct)
        _groups_carried(gathered, groups)
        got = merge_gathered(gathered, 0, B, k, distinct=distinct)
        _same(got, want, f"{variant} d={d} R={R} k={k}")
        oracle = L.labelled_topk(s64, tags, groups, mk, distinct, k)[0]
        assert (got[0].cpu().numpy() == oracle).all(), f"{variant}: ids differ from the fp64 oracle"
        _same(merge_gathered(gathered, 100, 30, k, distinct=distinct), (want[0][100:], want[1][100:]), f"{variant}: a rank's slice")
        thr = float(want[1][:, 0].median())
        _same(merge_gathered(gathered, 0, B, k, threshold=thr, distinct=distinct), full.match(qd, k, threshold=thr, filter=flt, distinct=distinct),
              f"{variant} thr={thr:.4f}")


# ---- 2. the designed cases ----
@pytest.mark.parametrize("name,k,R", [("hiding", 3, 3), ("ties", 3, 3), ("ties", 100, 7), ("cross", D.CROSS_K, D.CROSS_R)])
def test_designed_cases(name, k, R):
    from mtgv.matcher import merge_gathered
    from oracle import match_ref as M

    bank, q1, groups = {"hiding": L.hiding_case, "ties": L.ties_case, "cross": D.cross_shard_case}[name](64)
    q = torch.from_numpy(np.repeat(q1[None], 3, 0)).cuda()
    full = _matcher(bank, None, groups)
    shards = [_matcher(bank, None, groups, lo, hi) for lo, hi in D.shards(L.N, R)]
    gathered = _exchange(shards, q, k, None, True)
    assert gathered.shape == (R, 3, k, 2)
    _groups_carried(gathered, groups)
    got = merge_gathered(gathered, 0, 3, k, distinct=True)
    _same(got, full.match(q, k, distinct=True), name)
    ids = got[0].cpu().numpy()
    want = L.labelled_topk(M.scores(q1[None], bank), np.zeros(L.N, np.uint64), groups, L.NO_FILTER, True, k)[0]
    print(name, ids[0][:12].tolist())
    assert (ids == want[0]).all()
    if name == "hiding":
        assert ids[0].tolist() == [204, 210, 30]
    if name == "ties":
        assert ids[0, :3].tolist() == [10, 20, 21]
        if k == 100:  # shards of 60 rows hold fewer than k: the 700 candidates include pads
            assert (gathered[..., 0] < 0).any() and ids[0, 3] == 150 and (ids[:, :11] >= 0).all() and (ids[:, 11:] == -1).all()
    if name == "cross":
        assert ids[0].tolist() == D.CROSS_WANT
        plain = merge_gathered(gathered, 0, 3, k)  # the merge that does not dedupe: both 0.90 rows of group 9 come back
        assert plain[0][0].tolist() == D.CROSS_WANT_NO_MERGE_DEDUPE
        ti, ts = merge_gathered(gathered, 0, 3, k, threshold=D.CROSS_THR, distinct=True)
        assert ti[0].tolist() == D.CROSS_WANT_THR and torch.isneginf(ts[:, 2:]).all()  # pads are not refilled
        _same((ti, ts), full.match(q, k, threshold=D.CROSS_THR, distinct=True), "cross thr")


# ---- 3. a bank and batch the unlabelled match sends through the two-pass pre-pass ----
def test_big_case():
    from mtgv.matcher import merge_gathered

    bank, q, tags, groups, masks = L.big_case()
    qd = torch.from_numpy(q).cuda()
    full = _matcher(bank, tags, groups)
    want = full.match(qd, L.BIG_K, filter=masks, distinct=True)
    shards = [_matcher(bank, tags, groups, lo, hi) for lo, hi in D.shards(L.BIG_N, 3)]
    gathered = _exchange(shards, qd, L.BIG_K, masks, True)
    _groups_carried(gathered, groups)
    _same(merge_gathered(gathered, 0, L.BIG_B, L.BIG_K, distinct=True), want, "5000 x 768, b = 129, R = 3")


# ---- 4. defaults and edges ----
def test_defaults_make_the_same_calls():
    from mtgv.matcher import merge_gathered

    (bank, q, tags, groups, masks), _, qd = _case(768)
    shards = _random_matchers(768, 3)
    for k in (1, 3):
        a = [m.match_packed(qd, k) for m in shards]
        b = [m.match_packed(qd, k, filter=None, distinct=False) for m in shards]
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert all(((x[..., 1] >> 32) == 0).all() for x in a), "the unlabelled format keeps its zero high half"
        g = torch.stack(a).contiguous()
        x, y = merge_gathered(g, 0, B, k), merge_gathered(g, 0, B, k, distinct=False)
        _same(x, y, "merge defaults")
        # a filter-only exchange needs no other merge: the unlabelled merge ignores the high half
        lab = _exchange(shards, qd, k, masks, False)
        assert ((lab[..., 1] >> 32) != 0).any()
        _same(merge_gathered(lab, 0, B, k), _random_matchers(768, 1)[0].match(qd, k, filter=masks), "filter-only")


def test_candidate_cap():
    """n_ranks * k = 4096 candidates per query is the cap: exactly 4096 merge (against the numpy restatement), 4098 are refused"""
    from mtgv.matcher import merge_gathered

    rng = np.random.default_rng(5)
    R, b, k = 2, 2, 2048
    ids = rng.permutation(10 * R * b * k)[: R * b * k].reshape(R, b, k).astype(np.int64)
    sc = rng.integers(0, 500, (R, b, k)).astype(np.float32) / 500  # many exact ties: the id decides
    gr = rng.integers(-1, 300, (R, b, k))
    ids[rng.random((R, b, k)) < 0.05] = -1
    packed = D.pack(ids, sc, gr)
    for distinct in (True, False):
        want_i, want_s = D.merge(packed, 0, b, k, distinct)
        got_i, got_s = merge_gathered(torch.from_numpy(packed).cuda(), 0, b, k, distinct=distinct)
        assert (got_i.cpu().numpy() == want_i).all() and (got_s.cpu().numpy() == want_s).all(), f"distinct={distinct}"
        rev_i, rev_s = merge_gathered(torch.from_numpy(packed[::-1].copy()).cuda(), 0, b, k, distinct=distinct)
        assert torch.equal(rev_i, got_i) and torch.equal(rev_s, got_s), "the order of the ranks must not matter"
    for distinct in (True, False):
        with pytest.raises(AssertionError, match="4096"):
            merge_gathered(torch.zeros((3, 1, 1366, 2), dtype=torch.int64, device="cuda"), 0, 1, 1366, distinct=distinct)


def _tied_candidates(k, R=3, b=2):
    """(R, b, k, 2) packed candidates: distinct ids, scores on a grid of eight values (exact ties are common), every group
    -1, about 5 % pads - two of them placed by hand per query, one of which keeps a finite score word (2.0, above every real
    score) that no merge may look at"""
    rng = np.random.default_rng(11)
    ids = rng.permutation(10 * R * b * k)[: R * b * k].reshape(R, b, k).astype(np.int64)
    sc = rng.integers(0, 8, (R, b, k)).astype(np.float32) / 8
    ids[rng.random((R, b, k)) < 0.05] = -1
    ids[0, :, 1] = ids[R - 1, :, k - 1] = -1
    packed = D.pack(ids, sc, -1)
    loud = ids < 0
    loud[R - 1] = False  # the last rank's pads stay the canonical pad word
    packed[..., 1].view(np.uint64)[loud] = np.uint64((0xFFFFFFFF << 32) | int(np.float32(2.0).view(np.uint32)))
    assert loud.any() and (ids[R - 1] < 0).any()
    return packed


@pytest.mark.parametrize("k", [5, 100])
def test_every_merge_form_gives_one_answer(k):
    """One candidate set, one answer (ids and score bits) through every form of the merge - merge_topk on the flattened
    candidates (64-bit ids in HBM), the plain gathered merge and the distinct gathered merge with every group -1 - with and
    without a threshold that cuts inside the list, and that answer is dist_labels_common.merge's.  R * k = 15 candidates
    are fewer than one per thread; 300 make the strided scan take a second, partial pass."""
    from mtgv.matcher import merge_gathered, merge_topk

    R, b = 3, 2
    packed = _tied_candidates(k, R, b)
    want = D.merge(packed, 0, b, k, False)
    assert len(np.unique(want[1][0])) < k, "no exact tie among the results: choose another seed"
    thr = float(want[1][0, k // 2])
    g = torch.from_numpy(packed).cuda()
    flat = g.permute(1, 0, 2, 3).reshape(b, R * k, 2)
    flat_i, flat_s = flat[..., 0].contiguous(), flat[..., 1].to(torch.int32).contiguous().view(torch.float32)
    for t in (None, thr):
        want_i, want_s = D.merge(packed, 0, b, k, False, t)
        dis_i, dis_s = D.merge(packed, 0, b, k, True, t)
        assert (dis_i == want_i).all() and (dis_s.view(np.int32) == want_s.view(np.int32)).all()
        if t is not None:
            assert (want_i[0] >= 0).any() and (want_i[0] < 0).any(), "the threshold must cut inside the list"
        want_t = (torch.from_numpy(want_i).cuda(), torch.from_numpy(want_s).cuda())
        _same(merge_topk(flat_s, flat_i, k, t), want_t, f"merge_topk k={k} thr={t}")
        _same(merge_gathered(g, 0, b, k, t, distinct=False), want_t, f"plain gathered k={k} thr={t}")
        _same(merge_gathered(g, 0, b, k, t, distinct=True), want_t, f"distinct gathered k={k} thr={t}")


def test_empty_shard_and_missing_labels():
    from mtgv import native
    from mtgv.matcher import Matcher, merge_gathered

    (bank, q, tags, groups, masks), _, qd = _case(36)
    empty = Matcher(36, capacity=4, id_base=77)
    p = empty.match_packed(qd[:5].contiguous(), 3, distinct=True)
    assert (p[..., 0] == -1).all() and (p[..., 1].cpu().numpy().view(np.uint64) == D.PAD_WORD).all()
    with pytest.raises(RuntimeError, match="empty"):
        empty.match_packed(qd[:5].contiguous(), 3)  # the unlabelled call keeps its error
    # an empty shard beside two real ones
    full = _random_matchers(36, 1)[0]
    two = _random_matchers(36, 2)
    g = torch.stack([two[0].match_packed(qd, 3, filter=masks, distinct=True), empty.match_packed(qd, 3, filter=masks, distinct=True),
                     two[1].match_packed(qd, 3, filter=masks, distinct=True)]).contiguous()
    _same(merge_gathered(g, 0, B, 3, distinct=True), full.match(qd, 3, filter=masks, distinct=True), "empty shard")
    # neither masks nor distinct: status 1, as in mtgv_bank_topk_ex's labelled form
    out = torch.empty((5, 3, 2), dtype=torch.int64, device="cuda")
    rc = native.lib().mtgv_bank_topk_packed_ex(full._h, native.ptr(qd[:5].contiguous()), 5, 3, 0, None, 0, native.ptr(out), native.stream())
    assert rc == 1 and b"masks or distinct" in native.lib().mtgv_last_error()


def test_masks_that_admit_rows_on_one_shard_only():
    """query 3 admits rows >= 390 only (bit 62), query 1 none at all: the first shards answer with pads"""
    from mtgv.matcher import merge_gathered

    (bank, q, tags, groups, masks), _, qd = _case(768)
    shards = _random_matchers(768, 3)
    gathered = _exchange(shards, qd, 3, masks, True)
    last = gathered[2, 3, :, 0]
    assert (gathered[:2, 3, :, 0] == -1).all() and last[0] >= 390 and ((last >= 390) | (last == -1)).all() and (gathered[:, 1, :, 0] == -1).all()
    got = merge_gathered(gathered, 0, B, 3, distinct=True)
    _same(got, _random_matchers(768, 1)[0].match(qd, 3, filter=masks, distinct=True), "one shard only")
    assert (got[0][1] == -1).all() and torch.isneginf(got[1][1]).all()


@pytest.mark.parametrize("n", [60, 141])
def test_small_bank_labelled_match_against_oracle(n):
    """a labelled match of >= 128 queries over fewer rows than one 192-column tile (what a shard of a small bank is) runs the
    kernel the whole bank runs: ids exact and scores within 2e-6 of the fp64 oracle, the labelled match tests' bar"""
    (bank, q, tags, groups, masks), s64, qd = _case(768)
    m = _matcher(bank, tags, groups, 0, n)
    for variant in VARIANTS:
        mk, distinct = L.variant_labels((None, None, tags, groups, masks), variant)
        assert (L.rep_margin(s64[:, :n], tags[:n], groups[:n], mk, distinct, 3) > 1e-5).all(), "the oracle itself has a near-tie"
        wid, wsc = L.labelled_topk(s64[:, :n], tags[:n], groups[:n], mk, distinct, 3)
        ids, sc = m.match(qd, 3, filter=None if mk is L.NO_FILTER else mk, distinct=distinct)
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        err = np.abs(sc[wid >= 0] - wsc[wid >= 0]).max()
        print(f"n={n} {variant}: max score error {err:.3g}")
        assert (ids == wid).all() and err < 2e-6 and np.isneginf(sc[wid < 0]).all()


# ---- 5. ShardedMatcher and Pipeline(match_opts=) through RCCL, one rank ----
_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "mtg-vision_amd"), os.path.join(%(root)r, "tests")]
import numpy as np, torch, torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
import match_labels_common as L
import mtgv
from mtgv import dist as mdist, spec
from mtgv.matcher import Matcher
bank, q, tags, groups, masks = L.random_case(64)
sm = mtgv.ShardedMatcher(64, L.N)
assert sm.issues_collectives and len(sm) == L.N and sm.rows == range(0, L.N) and sm.local.id_base == 0
assert sm.add_local(bank) == range(0, L.N)
sm.set_labels(0, tags, groups)          # global rows
sm.set_labels(400, None, groups[400:])  # a part of them
t, g = sm.local.labels(0, L.N)
assert (t == tags).all() and (g == groups).all()
calls = []
orig = mdist._all_gather_cat
def spy(x, group=None):
    calls.append(tuple(x.shape))
    assert x.is_cuda
    return orig(x, group)
mdist._all_gather_cat = spy
qd = torch.from_numpy(q[:37]).cuda()
def same(a, b):
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
same(sm.match(qd, 3, filter=masks[:37], distinct=True), sm.local.match(qd, 3, filter=masks[:37], distinct=True))
assert calls == [(37, 64), (37, 3), (37, 3, 2)], calls   # queries, masks, one packed message
del calls[:]
same(sm.match(qd, 3, 0.2, distinct=True), sm.local.match(qd, 3, 0.2, distinct=True))
assert calls == [(37, 64), (37, 3, 2)], calls
del calls[:]
same(sm.match(qd, 3), sm.local.match(qd, 3))              # unlabelled: the lean exchange as before
assert calls == [(37, 64), (37, 3, 2)], calls
same(sm.match(q[0], 3, filter=(1 << 61, 0, 0)), sm.local.match(q[0], 3, filter=(1 << 61, 0, 0)))

# Pipeline(matcher=ShardedMatcher, match_opts=) against the same pipeline with a plain Matcher
from mtgv.detector import Detector
from mtgv.encoder import Encoder
from mtgv.pipeline import Pipeline
det_cfg = spec.DetectorConfig()
enc_cfg = spec.EncoderConfig("ae", (192, 128), 3, 48, (1, 1, 1, 1), (8, 16, 32, 64), "pool+linear", True)
F, K = 4, 4
det = Detector(det_cfg, spec.random_detector_state(det_cfg, 3), max_batch=F)
enc = Encoder(enc_cfg, spec.random_encoder_state(enc_cfg, 1), max_batch=F * K)
rng = np.random.default_rng(9)
bank48 = rng.standard_normal((L.N, 48)).astype(np.float32)
groups48 = (np.arange(L.N) %% 5).astype(np.int32)   # five cards: the plain top 3 would repeat one
plain, sharded = Matcher(48, capacity=L.N), mtgv.ShardedMatcher(48, L.N)
plain.add(bank48); plain.set_labels(0, None, groups48)
sharded.add_local(bank48); sharded.set_labels(0, None, groups48)
frames = torch.from_numpy(rng.integers(0, 256, (F, 640, 640, 3), dtype=np.uint8)).cuda()
opts = {"distinct": True}
p_sh = Pipeline(det, enc, sharded, K, 3, match_opts=opts)
p_pl = Pipeline(det, enc, plain, K, 3, match_opts=opts)
assert p_pl._plain_match and not p_sh._plain_match
del calls[:]
a, b = p_sh.run(frames), p_pl.run(frames)
torch.cuda.synchronize()
assert calls == [(F * K, 48), (F * K, 3, 2)], calls
assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["scores"], b["scores"])
ids = a["ids"].cpu().numpy().reshape(-1, 3)
assert (ids >= 0).all() and all(len(set(groups48[r].tolist())) == 3 for r in ids), "three different cards per crop"
c = Pipeline(det, enc, plain, K, 3).run(frames)   # match_opts=None: the call as before
torch.cuda.synchronize()
assert torch.equal(c["ids"][..., 0], b["ids"][..., 0])
dist.barrier()
dist.destroy_process_group()
print("SHARDED_LABELS_OK")
"""


# ---- 6. ShardedMatcher on two ranks that share the GPU (gloo: the messages staged through host memory) ----
_CHILD2 = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "mtg-vision_amd"), os.path.join(%(root)r, "tests")]
import numpy as np, torch, torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
import match_labels_common as L
import mtgv
from mtgv.dist import shard_rows
from mtgv.matcher import Matcher
bank, q, tags, groups, masks = L.random_case(64)
sm = mtgv.ShardedMatcher(64, L.N)
lo, hi = shard_rows(L.N, rank, world)
assert sm.rows == range(lo, hi) and sm.local.id_base == lo and len(sm) == L.N
assert sm.add_local(bank[lo:hi]) == range(lo, hi)
sm.set_labels(0, None, groups)          # global rows: each rank keeps its part
sm.set_labels(100, tags[100:], None)    # a span that starts inside rank 0's shard and covers rank 1's
sm.set_labels(0, tags[:100])
t, g = sm.local.labels(0, hi - lo)
assert (t == tags[lo:hi]).all() and (g == groups[lo:hi]).all()
full = Matcher(64, capacity=L.N)
full.add(bank)
full.set_labels(0, tags, groups)
b = L.B_MAX // world
mine = slice(rank * b, (rank + 1) * b)
qd = torch.from_numpy(q).cuda()
for flt, distinct, thr in ((masks, True, None), (None, True, 0.3), (masks, False, None), (None, False, None)):
    got = sm.match(q[mine], 3, thr, filter=None if flt is None else flt[mine], distinct=distinct)
    want = full.match(qd, 3, thr, filter=flt, distinct=distinct)   # the batch the shards see: all ranks' queries
    torch.cuda.synchronize()
    assert got[0].is_cuda and torch.equal(got[0], want[0][mine]), (rank, distinct)
    assert torch.equal(got[1].view(torch.int32), want[1][mine].view(torch.int32)), (rank, distinct)
dist.barrier()
dist.destroy_process_group()
sys.stdout.write("SHARDED_TWO_RANKS_OK\n")   # (one write: the two ranks share the pipe)
"""


def test_sharded_matcher_two_ranks_gloo(tmp_path):
    script = tmp_path / "child2.py"
    script.write_text(_CHILD2 % {"root": ROOT})
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MTGV_FORCE_COLLECTIVE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("SHARDED_TWO_RANKS_OK") == 2, r.stdout[-2000:]  # both ranks reached the end


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_matcher_through_rccl_one_rank(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"root": ROOT})
    env = dict(os.environ, MTGV_FORCE_COLLECTIVE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "SHARDED_LABELS_OK" in r.stdout
