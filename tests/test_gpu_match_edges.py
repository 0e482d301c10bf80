"""The bank match on the GPU at its tile, range and bound edges against the fp64 oracle (cases, draws, references and the
restated first pass: match_edges_common.py; what the cases claim about themselves: test_match_edges_cpu.py).

Every case of the shape table runs through one path - the split kernel's fused top-k, the convert-on-load kernel's, or the
fp16 first pass + re-rank - chosen with the operand precision and MTGV_MATCH_PREPASS, under the launch profiler, whose
table must show exactly one GEMM row with the case's M, N, K and the path's sp and topk: no case passes by running another
kernel.  Outputs are prefilled with garbage.  `pytest -s` prints the path and the measured maximum score error per case.

Measured on an MI355X (restated on the host, confirmed on the device): the bound case's winner W loses 8.31e-4 to the fp16
roundings, the proof's slack is 6.15e-4 (PRE_EPS = 1.1e-3, half of it 5.5e-4), W stands 1.85e-4 above the best reported row."""
import contextlib
import os
import tempfile

import numpy as np
import pytest
import torch

import match_edges_common as mc
from oracle import match_ref as M

pytestmark = pytest.mark.gpu

COL_M, COL_N, COL_K, COL_TOPK, COL_SP = 1, 2, 3, 10, 17  # columns of the profiler's table (gemm_profile_dump)
CANARY_ID = -7777
TWO_BANK = "two-N4129-K64-b131-k1-f16x3"  # the bank the cross-path, threshold and upkeep tests share: one column in the last range


@pytest.fixture(autouse=True)
def _restore_precision():
    from mtgv import native

    before = native.get_gemm_precision()
    yield
    native.set_gemm_precision(before)


@contextlib.contextmanager
def prepass(on):
    old = os.environ.get("MTGV_MATCH_PREPASS")
    os.environ["MTGV_MATCH_PREPASS"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MTGV_MATCH_PREPASS", None)
        else:
            os.environ["MTGV_MATCH_PREPASS"] = old


def matcher_of(bank, **kw):
    from mtgv.matcher import Matcher

    m = Matcher(bank.shape[1], capacity=bank.shape[0], **kw)
    m.add(np.array(bank, dtype=np.float32))  # (a copy: the draws are read-only)
    return m


def match_into(m, q, k, path, mode="f16x3", threshold=None):
    """Matcher.match's library call (mtgv_bank_topk, made directly so that the outputs can be prefilled with garbage:
    Matcher.match's own tensor and threshold plumbing is not on the tested path) on the given path, under the launch
    profiler: its table must show exactly one GEMM row, of that path's kernel.  numpy (ids, scores, the profiler's row)"""
    from mtgv import native as nv

    L = nv.lib()
    nv.set_gemm_precision(mode)
    qd = torch.from_numpy(np.array(q, dtype=np.float32)).cuda()
    ids = torch.full((qd.shape[0], k), CANARY_ID, dtype=torch.int64, device="cuda")
    sc = torch.full((qd.shape[0], k), float("nan"), dtype=torch.float32, device="cuda")
    thr = float("-inf") if threshold is None else float(threshold)
    with tempfile.TemporaryDirectory() as tmp:
        csv = os.path.join(tmp, "gemm.csv")
        nv.check(L.mtgv_profile_gemm(1))
        try:
            with prepass(path == "two"):
                nv.check(L.mtgv_bank_topk(m._h, nv.ptr(qd), qd.shape[0], k, m.id_base, thr, nv.ptr(ids), nv.ptr(sc), nv.stream()))
            torch.cuda.synchronize()
            nv.check(L.mtgv_profile_gemm_dump(csv.encode()))
        finally:
            nv.check(L.mtgv_profile_gemm(0))
        rows = [ln.split(",") for ln in open(csv).read().split()[1:]]
    assert len(rows) == 1, rows
    assert int(rows[0][COL_SP]) == mc.SP_OF[path], ("ran on another kernel", path, rows[0])
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert (ids != CANARY_ID).all() and not np.isnan(sc).any(), "a result slot was not written"
    return ids, sc, rows[0]


def match2(*a, **kw):
    return match_into(*a, **kw)[:2]


# ---- every case of the table ----
@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_case_against_oracle(case):
    q, bank, plan = mc.draw(case.name)
    s, rid, rsc = mc.oracle(case.name)
    m = matcher_of(bank)
    ids, sc, r = match_into(m, q, case.k, case.path, case.mode)
    assert (int(r[COL_M]), int(r[COL_N]), int(r[COL_K])) == (case.b, case.N, case.K), r
    assert int(r[COL_SP]) == mc.SP_OF[case.path], ("ran on another kernel", r)
    assert int(r[COL_TOPK]) == mc.expected_topk(case), r
    err = mc.judge(s, rid, rsc, ids, sc, case.k, plan)
    print(f"\n{case.name}: path {case.path} (sp {r[COL_SP]}, topk {r[COL_TOPK]}), max score error {err:.2e}")


# ---- the three paths on one bank ----
def test_paths_agree_and_id_base_shifts_ids_only():
    c = mc.BY_NAME[TWO_BANK]
    q, bank, plan = mc.draw(c.name)
    k = 4
    s = mc.oracle(c.name)[0]
    rid, rsc = M.topk_from_scores(s, k)
    exact = mc.exact_ranks(s, k)  # (no plan: the planted rows beyond this case's own k are judged like any row)
    m = matcher_of(bank)
    res = {p: match2(m, q, k, p, mode) for p, mode in (("two", "f16x3"), ("split", "f16x3"), ("col", "f32"))}
    for p, (ids, sc) in res.items():
        mc.judge(s, rid, rsc, ids, sc, k)
        assert (ids[exact] == res["two"][0][exact]).all(), p
    # id_base: every id shifted, pads untouched (a threshold between the planted and the random rows leaves both)
    mb = matcher_of(bank, id_base=1000)
    for p, mode in (("two", "f16x3"), ("split", "f16x3"), ("col", "f32")):
        i0, s0 = match2(m, q, k, p, mode, threshold=0.7)
        i1, s1 = match2(mb, q, k, p, mode, threshold=0.7)
        assert (i0 == -1).any() and (i0 >= 0).any()
        assert (i1 == np.where(i0 >= 0, i0 + 1000, -1)).all(), p
        assert (s1.view(np.int32) == s0.view(np.int32)).all()
        assert np.isneginf(s0[i0 < 0]).all()
        assert ((s >= 0.7 + 1e-5).sum(1).clip(max=k) <= (i0 >= 0).sum(1)).all() and ((i0 >= 0).sum(1) <= (s >= 0.7 - 1e-5).sum(1)).all()


# ---- the first pass on its own ----
FIRST_PASS = [c.name for c in mc.CASES if c.path == "two" and c.k == max(x.k for x in mc.CASES if x.path == "two" and x.N == c.N)] + ["bound"]


def device_rows(x):
    """rows of x as the device normalises them (the bank's own kernel)"""
    return matcher_of(x).rows(0, x.shape[0])


@pytest.mark.parametrize("name", FIRST_PASS)
def test_first_pass_candidates(name):
    from mtgv import native as nv

    q, bank, _ = mc._draw_any(name)
    s = mc.oracle(name)[0]
    b, n = s.shape
    # the restatement normalises as the device does, bit for bit - so its fp16 operands are the kernel's
    assert (device_rows(bank).view(np.int32) == mc.l2norm_f32(bank).view(np.int32)).all()
    assert (device_rows(q).view(np.int32) == mc.l2norm_f32(q).view(np.int32)).all()
    approx = mc.first_pass(q, bank)
    ref_s, ref_c, margin = mc.range_candidates(approx)
    m = matcher_of(bank)
    nv.set_gemm_precision("f16x3")
    cs, ci, range_cols = m.prepass_candidates(torch.from_numpy(np.array(q)).cuda())
    torch.cuda.synchronize()
    cs, ci = cs.cpu().numpy(), ci.cpu().numpy()
    assert range_cols == mc.RANGE and cs.shape == (b, mc.slots_of(n), mc.PRE_KP) == ref_s.shape
    assert ci.max() < n, "a column past N was reported"
    pads = np.isneginf(ref_s)
    assert (np.isneginf(cs) == pads).all() and ((ci == -1) == pads).all()  # short and empty ranges pad, no other range does
    w_last = (n - 1) // mc.RANGE
    if n % mc.RANGE == 1:
        assert (ci[:, w_last, 0] == n - 1).all() and (ci[:, w_last, 1] == -1).all()
    assert (ci[:, w_last + 1 :] == -1).all()
    lo = (np.arange(cs.shape[1]) * mc.RANGE)[None, :, None]
    assert ((ci == -1) | ((ci >= lo) & (ci < lo + mc.RANGE))).all(), "a candidate outside its range"
    err = np.abs(np.where(pads, 0.0, cs.astype(np.float64) - np.where(pads, 0.0, ref_s)))
    assert err.max() < mc.SCORE_TOL, err.max()
    clear = margin > mc.SCORE_TOL
    clear[:, :, 1:] &= clear[:, :, :-1]  # an entry's column is decided where the gaps above and below it are
    assert (ci[clear] == ref_c[clear]).all()
    exact = np.take_along_axis(s, np.maximum(ci, 0).reshape(b, -1), axis=1).reshape(ci.shape)
    off = np.abs(np.where(pads, 0.0, cs - exact))
    assert off.max() < mc.PRE_EPS
    print(f"\n{name}: first pass vs restatement {err.max():.2e}, vs fp64 exact {off.max():.2e}, {int(clear.sum())} of {clear.size} columns decided")
    if name == "bound":
        x = mc.BOUND_Q
        assert sorted(ci[x, mc.BOUND_W // mc.RANGE].tolist()) == sorted(mc.BOUND_H) and mc.BOUND_W not in ci[x].reshape(-1).tolist()
        assert mc.BOUND_D in ci[x].reshape(-1).tolist()


def test_first_pass_refusals_leave_the_buffers_alone():
    from mtgv import native as nv

    rng = np.random.default_rng(3)

    def refused(m, b, mode="f16x3"):
        nv.set_gemm_precision(mode)
        q = torch.from_numpy(rng.standard_normal((b, m.dim)).astype(np.float32)).cuda()
        n = b * mc.slots_of(max(len(m), 1)) * mc.PRE_KP + 64
        cs = torch.full((n,), 12345.0, dtype=torch.float32, device="cuda")
        ci = torch.full((n,), CANARY_ID, dtype=torch.int32, device="cuda")
        with pytest.raises(AssertionError, match="no fp16 first pass"):
            m.prepass_candidates(q, out=(cs, ci))
        torch.cuda.synchronize()
        assert (cs == 12345.0).all() and (ci == CANARY_ID).all()

    big = matcher_of(rng.standard_normal((4096, 64)).astype(np.float32))
    refused(big, 127)                      # fewer than 128 queries
    refused(big, 128, mode="f32")          # f32 mode: no split kernel
    refused(matcher_of(rng.standard_normal((4095, 64)).astype(np.float32)), 128)  # fewer than 4096 rows
    refused(matcher_of(rng.standard_normal((4096, 72)).astype(np.float32)), 128)  # dim % 64 != 0 (and so no fp16 copy)
    nv.set_gemm_precision("f16x3")
    cs, ci, _ = big.prepass_candidates(torch.from_numpy(rng.standard_normal((128, 64)).astype(np.float32)).cuda())
    assert cs.shape == (128, 44, 2) and int(ci.max()) < 4096  # and the same bank is served at 128 queries


# ---- clusters 2e-5 apart: the fallback scan's ordering ----
@pytest.mark.parametrize("cl", mc.CLUSTERS, ids=lambda c: c.name)
def test_cluster_comes_back_in_exact_order(cl):
    q, bank, cols, dups = mc.cluster_draw(cl.name)
    s = mc.oracle(cl.name)[0]
    m = matcher_of(bank)
    before = m.prepass_fallbacks()
    for k in mc.CLUSTER_KS:
        rid, rsc = M.topk_from_scores(s, k)
        ids, sc = match2(m, q, k, "two")
        assert ids[mc.CLUSTER_Q].tolist() == list(cols[:k]), (k, ids[mc.CLUSTER_Q].tolist())
        assert ids[mc.DUP_Q].tolist() == list(dups[:k]), (k, ids[mc.DUP_Q].tolist())
        assert (sc[mc.DUP_Q] == sc[mc.DUP_Q, 0]).all()
        err = mc.judge(s, rid, rsc, ids, sc, k)
    assert m.prepass_fallbacks() >= before + 2 * len(mc.CLUSTER_KS)  # both planted queries need the scan, at every k
    print(f"\n{cl.name}: max score error {err:.2e}, {m.prepass_fallbacks() - before} scans over {len(mc.CLUSTER_KS)} calls")


# ---- the bound ----
def test_bound_case_hidden_winner_is_found_by_the_scan():
    """W is not reported, the best re-ranked row D is 1.85e-4 below it, and D's exact score clears max(a_R, cut) by 6.15e-4:
    only PRE_EPS = 1.1e-3 in the proof sends the block to the scan that finds W (W's fp16 deficit: 8.31e-4)"""
    bc = mc.bound_case()
    s, rid, rsc = mc.oracle("bound")
    m = matcher_of(bc.bank)
    before = m.prepass_fallbacks()
    ids, sc = match2(m, bc.q, 1, "two")
    assert ids[mc.BOUND_Q, 0] == mc.BOUND_W, ("the hidden winner was missed", ids[mc.BOUND_Q].tolist())
    mc.judge(s, rid, rsc, ids, sc, 1)
    assert m.prepass_fallbacks() == before + 1  # that query's block and no other
    one, _ = match2(m, bc.q, 1, "split")
    assert (one == ids).all()


def test_a_r_case_reported_winner_outside_the_re_ranked():
    """W is reported by its range but nine rows of other ranges score approximately higher, and no range's cut-off comes
    near: only the a_R term of max(a_R, cut) sends the block to the scan, which re-scores W as a reported candidate"""
    q, bank = mc.ar_case()
    s, rid, rsc = mc.oracle("a_R")
    m = matcher_of(bank)
    before = m.prepass_fallbacks()
    ids, sc = match2(m, q, 1, "two")
    assert ids[mc.BOUND_Q, 0] == mc.BOUND_W, ("the winner outside the re-ranked was missed", ids[mc.BOUND_Q].tolist())
    mc.judge(s, rid, rsc, ids, sc, 1)
    assert m.prepass_fallbacks() == before + 1


# ---- threshold ----
@pytest.mark.parametrize("path", ["two", "split"])
def test_threshold_at_the_kth_score(path):
    c = mc.BY_NAME[TWO_BANK]
    q, bank, plan = mc.draw(c.name)
    m = matcher_of(bank)
    k, pr = 3, 31
    ids, sc = match2(m, q, k, path)
    kth = sc[pr, k - 1]
    assert sc[pr, k - 2] > kth  # (nothing ties with the k-th score)
    i_eq, s_eq = match2(m, q, k, path, threshold=float(kth))
    assert (i_eq[pr] == ids[pr]).all() and (s_eq[pr].view(np.int32) == sc[pr].view(np.int32)).all()
    up = np.nextafter(kth, np.float32(np.inf), dtype=np.float32)
    i_up, s_up = match2(m, q, k, path, threshold=float(up))
    assert i_up[pr].tolist() == ids[pr, : k - 1].tolist() + [-1], "exactly the k-th slot becomes a pad and is not replaced"
    assert (s_up[pr, : k - 1].view(np.int32) == sc[pr, : k - 1].view(np.int32)).all() and np.isneginf(s_up[pr, k - 1])
    # the whole batch: a slot is kept exactly when its score reaches the threshold
    for thr, (it, st) in ((kth, (i_eq, s_eq)), (up, (i_up, s_up))):
        keep = sc >= thr
        assert (it == np.where(keep, ids, -1)).all()
        assert (st[keep].view(np.int32) == sc[keep].view(np.int32)).all() and np.isneginf(st[~keep]).all()


@pytest.mark.parametrize("path", ["two", "split"])
def test_zero_query_in_a_batch(path):
    bc = mc.bound_case()  # at k = 1 every query but one has a clear winner (test_match_edges_cpu): none of them needs the scan
    q = bc.q.copy()
    q[mc.BOUND_Q] = 0.0
    m = matcher_of(bc.bank)
    before = m.prepass_fallbacks()
    ids, sc = match2(m, q, 1, path)
    assert ids[mc.BOUND_Q].tolist() == [0] and (sc[mc.BOUND_Q] == 0.0).all()
    assert m.prepass_fallbacks() == before, "a zero query counted as a scan"
    others = np.arange(mc.BOUND_B) != mc.BOUND_Q
    assert (ids[others, 0] == 2100 + 13 * np.arange(mc.BOUND_B)[others]).all()
    k = 3
    ids, sc = match2(m, q, k, path)
    assert ids[mc.BOUND_Q].tolist() == [0, 1, 2] and (sc[mc.BOUND_Q] == 0.0).all()
    ids, sc = match2(m, q, k, path, threshold=1e-6)
    assert ids[mc.BOUND_Q].tolist() == [-1] * k and np.isneginf(sc[mc.BOUND_Q]).all()
    ids, sc = match2(m, q, k, path, threshold=0.0)
    assert ids[mc.BOUND_Q].tolist() == [0, 1, 2]


# ---- upkeep of the fp16 copy (two-pass, N = 4129) ----
def test_set_row_refreshes_the_fp16_copy():
    c = mc.BY_NAME[TWO_BANK]
    q, bank, plan = mc.draw(c.name)
    k, pr = 3, 31
    m = matcher_of(bank)
    ids0, _ = match2(m, q, k, "two")
    old1 = plan[pr][0]
    assert ids0[pr, 0] == old1
    planted = {col for cols in plan.values() for col in cols}
    new1 = next(col for col in range(2000, c.N) if col not in planted)
    assert new1 not in ids0[pr].tolist()
    rng = np.random.default_rng(11)
    edited = bank.copy()
    edited[new1] = mc.planted_row(mc._unit64(q[pr]), 0.95, rng)  # a row that was nowhere becomes the best match
    edited[old1] = rng.standard_normal(c.K).astype(np.float32)   # and the former best match is gone
    m.set_row(new1, edited[new1])
    m.set_row(old1, edited[old1])
    s = M.scores(q, edited)
    rid, rsc = M.topk_from_scores(s, k)
    for path in ("two", "split"):
        ids, sc = match2(m, q, k, path)
        assert ids[pr, 0] == new1 and old1 not in ids[pr].tolist(), (path, ids[pr].tolist())
        assert ids[pr].tolist() == rid[pr].tolist()
        mc.judge(s, rid, rsc, ids, sc, k)


def test_uneven_appends_equal_one_append():
    from mtgv.matcher import Matcher

    c = mc.BY_NAME[TWO_BANK]
    q, bank, plan = mc.draw(c.name)
    s = mc.oracle(c.name)[0]
    k = 4
    rid, rsc = M.topk_from_scores(s, k)
    whole = matcher_of(bank)
    parts = Matcher(c.K, capacity=c.N)
    for lo, hi in ((0, 1000), (1000, 1001), (1001, c.N)):
        parts.add(np.array(bank[lo:hi]))
    assert len(parts) == c.N == 1000 + 1 + 3128
    iw, sw = match2(whole, q, k, "two")
    ip, sp = match2(parts, q, k, "two")
    assert (iw == ip).all() and (sw.view(np.int32) == sp.view(np.int32)).all()
    mc.judge(s, rid, rsc, ip, sp, k)
