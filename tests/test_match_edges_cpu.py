"""CPU-only: everything match_edges_common.py claims about its own cases - table coverage, planted margins, the cap on
near-tie judgements, the clusters' fp16 misordering, the bound case's conditions, and that the restated first pass never
errs by PRE_EPS.  test_gpu_match_edges.py runs the same cases on the device.  `pytest -s` prints the figures."""
import numpy as np
import pytest

import match_edges_common as mc
from oracle import match_ref as M

TWO = [c for c in mc.CASES if c.path == "two"]


def test_table_coverage():
    """every value of the shape table appears in a case of its path, the N and K edges meet, about a dozen cases per path"""
    for path, table in mc.TABLE.items():
        cases = [c for c in mc.CASES if c.path == path]
        assert 10 <= len(cases) <= 14
        for field, values in table.items():
            assert {getattr(c, field) for c in cases} == set(values), (path, field)
    have = {(c.path, c.N, c.K, c.k) for c in mc.CASES}
    assert any(p == "split" and n == 193 and k_ == 72 for p, n, k_, _ in have)       # a one-column last range with a K tail
    assert any(p == "split" and n == 383 and kk == 100 for p, n, _, kk in have)      # k beyond a range's columns, ragged N
    assert any(p == "two" and n == 4129 and kk == 4 for p, n, _, kk in have)         # one column in the last range, largest k
    assert any(p == "col" and n == 65 and kk == 70 for p, n, _, kk in have)          # k > N: pads
    for c in mc.CASES:
        if c.path == "split":
            assert c.mode == "f16x3" and c.b >= 128 and c.N >= 192 and c.K % 8 == 0
        elif c.path == "two":
            assert c.mode == "f16x3" and c.b >= 128 and c.N >= 4096 and c.K % 64 == 0 and c.k <= 4
        else:
            assert c.b < 128 or c.mode == "f32"
    assert {c.mode for c in mc.CASES if c.path == "col" and c.b < 128} == {"f32", "f16x3"}
    # the two-pass N reach: last range of 64 columns and an empty one after it, exactly full, one column, whole tiles
    assert [(n % 192) for n in mc.TABLE["two"]["N"]] == [64, 96, 97, 0]
    assert mc.slots_of(4096) == 44 and mc.slots_of(4129) == 44 and mc.slots_of(4224) == 44 and mc.slots_of(4225) == 46


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_planted_probes_and_near_tie_cap(case):
    q, bank, plan = mc.draw(case.name)
    s, rid, rsc = mc.oracle(case.name)
    assert sorted(plan) == mc.probes_of(case.b)
    probes = sorted(plan)
    p = len(plan[probes[0]])
    assert p == case.k + 1 or p == case.N // (len(probes) + 1), "fewer planted rows only where the bank cannot hold k + 1 per probe"
    assert plan[probes[0]][0] == case.N - 1                       # rank 1 at the bank's last row
    assert len(probes) < 2 or plan[probes[1]][0] == 0              # and at its first
    planted = [col for cols in plan.values() for col in cols]
    assert len(set(planted)) == len(planted)
    assert set(mc.delicate_columns(case.N, case.path)) <= set(planted) or p * len(probes) < len(mc.delicate_columns(case.N, case.path))
    margin, gap = mc.planted_margin(case.name), mc.planted_gap(s, plan)
    assert margin > 0.25, "a planted row must stand far above every row that is not planted for its probe"
    assert mc.STEP / 2 < gap < 2 * mc.STEP
    for pr, cols in plan.items():
        m = mc.planted_ranks(cols, case.k, case.N)
        assert rid[pr, :m].tolist() == list(cols[:m])
    weak_q, weak_slots = mc.weak_fraction(s, case.k, plan), mc.weak_slot_fraction(s, case.k, plan)
    print(f"\n{case.name}: planted {p} per probe, margin {margin:.3f}, gap {gap:.2e}, near-tie queries {weak_q:.3f}, slots {weak_slots:.4f}")
    if case.k <= 16:
        assert weak_q <= mc.WEAK_CAP
    else:  # (module docstring: no seed can hold the per-query cap at k = 70 and 100; the judgement is per rank, the cap per slot)
        assert weak_slots <= mc.WEAK_CAP
    # the oracle passes its own judgement, and a result with two neighbouring planted ranks swapped does not
    mc.judge(s, rid, rsc, rid, rsc.astype(np.float32), case.k, plan)
    if case.k >= 2 and p >= 3:
        wrong = rid.copy()
        wrong[probes[0], [0, 1]] = wrong[probes[0], [1, 0]]
        with pytest.raises(AssertionError):
            mc.judge(s, rid, rsc, wrong, rsc.astype(np.float32), case.k, plan)


def test_restated_first_pass_error_stays_below_pre_eps():
    worst = 0.0
    names = [c.name for c in TWO] + [c.name for c in mc.CLUSTERS] + ["bound", "a_R"]
    for name in names:
        q, bank, _ = mc._draw_any(name)
        s, _, _ = mc.oracle(name)
        err = np.abs(mc.first_pass(q, bank) - s).max()
        worst = max(worst, err)
    print(f"\nworst restated |approximate - exact| over {len(names)} banks: {worst:.3e} (PRE_EPS {mc.PRE_EPS:.1e})")
    assert worst < mc.PRE_EPS


@pytest.mark.parametrize("cl", mc.CLUSTERS, ids=lambda c: c.name)
def test_cluster_is_misordered_by_the_fp16_pass(cl):
    q, bank, cols, dups = mc.cluster_draw(cl.name)
    s, rid, rsc = mc.oracle(cl.name)
    approx = mc.first_pass(q, bank)
    assert len(cols) == 12 and rid[mc.CLUSTER_Q].tolist() == list(cols[:4])
    exact12 = s[mc.CLUSTER_Q, list(cols)]
    assert (np.diff(exact12) < -mc.STEP / 2).all() and (np.diff(exact12) > -2 * mc.STEP).all()
    order = np.lexsort((np.array(cols), -approx[mc.CLUSTER_Q, list(cols)])).tolist()
    print(f"\n{cl.name}: approximate order of the exact ranks {order}")
    top = max(mc.CLUSTER_KS) + 1
    assert order[:top] != list(range(top)), "the fp16 pass keeps the exact order of the best k + 1: the case checks no ordering"
    assert order[0] != 0, "the best row also leads approximately: k = 1 checks no ordering"
    ranges = {col // mc.RANGE for col in cols}
    assert len(ranges) == {"one-range": 1, "twelve-ranges": 12, "straddle-last": 2}[cl.placement]
    if cl.placement == "straddle-last":
        assert max(ranges) == mc.slots_of(mc.CLUSTER_N) - 2 and mc.CLUSTER_N - mc.LAST_RANGE0 < mc.RANGE  # into the last, partial range
    # the duplicates: one vector, more than PRE_KP copies, all in the last partial range
    assert len(dups) > mc.PRE_KP and min(dups) >= mc.LAST_RANGE0
    assert all((bank[d] == bank[dups[0]]).all() for d in dups)
    assert rid[mc.DUP_Q].tolist() == list(dups[:4])
    assert s[mc.DUP_Q, dups[0]] - np.delete(s[mc.DUP_Q], list(dups)).max() > 0.25


def test_bound_case():
    bc = mc.bound_case()
    approx = mc.first_pass(bc.q, bc.bank)
    s, rid, _ = mc.oracle("bound")
    x, w = mc.BOUND_Q, mc.BOUND_W
    cs, cols, _ = mc.range_candidates(approx)
    slack, sel = mc.proof_slack(approx, s, 1)
    print(f"\nbound case: {bc.n} non-zeros, c = {bc.c:.4f}, W's deficit {bc.deficit:.3e}, slack {slack[x]:.3e}, W over D {bc.gap:.3e}, "
          f"smallest slack of the other queries {np.delete(slack, x).min():.3f}")
    assert s[x, w] - approx[x, w] >= 6e-4                              # W's approximate score falls short of its exact score
    assert sorted(cols[x, w // mc.RANGE].tolist()) == sorted(mc.BOUND_H)  # two hiders are reported for W's range: W is not
    assert w not in cols[x].reshape(-1).tolist()
    assert 4e-4 <= slack[x] <= 9e-4                                    # below PRE_EPS, above half of it
    assert slack[x] > mc.PRE_EPS / 2 + 4e-5                            # ... with room for the device's f32 sums
    assert rid[x, 0] == w and bc.gap > 2 * mc.ID_MARGIN                # the oracle's answer is W, clearly
    assert mc.BOUND_D in sel[x].tolist()                               # D is re-ranked: it is the answer of a proof that holds wrongly
    assert s[x, mc.BOUND_D] == np.delete(s[x], w).max()
    assert (np.delete(slack, x) > 0.1).all()                           # no other query of the batch comes near a scan
    assert np.abs(approx - s).max() < mc.PRE_EPS


def test_a_r_case():
    """the winner is reported but not re-ranked, and no range's cut-off comes near: the proof fails through a_R alone"""
    q, bank = mc.ar_case()
    approx = mc.first_pass(q, bank)
    s, rid, _ = mc.oracle("a_R")
    x, w = mc.BOUND_Q, mc.BOUND_W
    cs, cols, _ = mc.range_candidates(approx)
    slack, sel = mc.proof_slack(approx, s, 1)
    assert cols[x, w // mc.RANGE, 0] == w                                  # reported: the best of its range
    assert set(sel[x].tolist()) < set(mc.AR_DECOYS)                        # the re-ranked: eight of the nine decoys
    assert w not in sel[x].tolist()                                        # but nine rows come before it
    assert rid[x, 0] == w and s[x, w] - np.delete(s[x], w).max() > 2 * mc.ID_MARGIN
    kth = np.float32(s[x, sel[x]].max())
    cut = cs[x, :, mc.PRE_KP - 1].max()
    print(f"\na_R case: slack {slack[x]:.3e}, s_kth - cut {kth - cut:.3f}, W's approximate score {approx[x, w] - (kth - mc.PRE_EPS):.3e} above the scan's threshold")
    assert slack[x] < mc.PRE_EPS - 1e-4                                    # the proof fails ...
    assert kth - cut > 0.1                                                 # ... and would hold on the cut-offs alone
    assert approx[x, w] > kth - mc.PRE_EPS + 1e-4                          # the scan re-scores W as a reported candidate
    assert (np.delete(slack, x) > 0.1).all()
    assert np.abs(approx - s).max() < mc.PRE_EPS


def test_restatement_pieces():
    """l2norm_f32 against fp64 (one ulp), row_scale's window, range_candidates' pads"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((37, 200)).astype(np.float32)
    n = mc.l2norm_f32(x)
    assert n.dtype == np.float32
    np.testing.assert_allclose(n, M.l2_normalize(x.astype(np.float64)), rtol=3e-7, atol=0)
    sc = mc.row_scale(n)
    mx = np.abs(n).max(1) * sc
    assert ((mx >= 2**13) & (mx < 2**14)).all() and (np.frexp(sc)[0] == 0.5).all()
    approx = rng.standard_normal((2, 4129))
    cs, cols, margin = mc.range_candidates(approx)
    assert cs.shape == (2, 44, 2)
    assert cols[0, 43].tolist() == [4128, -1] and np.isneginf(cs[0, 43, 1]) and cs[0, 43, 0] == approx[0, 4128]
    cs, cols, _ = mc.range_candidates(approx[:, :4096])
    assert cols[1, 43].tolist() == [-1, -1] and (cols[:, 42] >= 4032).all() and (cols < 4096).all()
