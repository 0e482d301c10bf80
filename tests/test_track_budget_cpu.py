"""The embed budget's selection rule on the host (mtgv.tracker.select_due) and the lock-step yardstick that the GPU tests
compare the device with (track_budget_common).  No GPU."""
import numpy as np
import pytest

import track_budget_common as tb
import track_common as tc


@pytest.mark.parametrize("n", [1, 12, 65, 300])
def test_select_due_is_the_brute_force_rule(n):
    from mtgv.tracker import select_due

    straddled = 0
    for e in sorted({1, max(1, n - 1), n, n + 1}):
        for seed, straddle in ((0, None), (1, None), (2, e), (3, e)):
            w = tb.tie_heavy_keys(n, 1000 * n + 10 * e + seed, straddle)
            got, want = select_due(w, e), tb.brute_force(w, e)
            assert got.dtype == np.int64 and (got == want).all(), (n, e, seed, got, want)
            assert (np.diff(got) > 0).all() and got.size == min(e, int((~np.isnan(w)).sum()))
            out = np.setdiff1d(np.flatnonzero(~np.isnan(w)), got)
            if got.size and out.size:  # nothing left out beats anything taken; an equal key only from a larger index
                lo = w[got].min()
                assert w[out].max() <= lo
                tied_in, tied_out = got[w[got] == lo], out[w[out] == lo]
                if tied_out.size:
                    straddled += 1
                    assert tied_in.max() < tied_out.min()
    assert n < 12 or straddled > 0, "no case in which the group of tied keys straddles the budget"


def test_select_due_corner_cases():
    from mtgv.tracker import select_due

    assert select_due([np.nan, np.nan], 3).size == 0
    assert select_due([np.inf, np.inf, np.inf], 2).tolist() == [0, 1]  # never embedded: the first by index
    assert select_due([0.6, np.inf, np.nan, 0.7], 2).tolist() == [1, 3]
    assert select_due([0.6, np.inf, np.nan, 0.7], 9).tolist() == [0, 1, 3]  # a budget that does not bind: today's due set
    with pytest.raises(AssertionError):
        select_due([1.0], 0)


@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_lockstep_without_a_binding_budget_is_run_host(name):
    """with E >= S * K the lock-step yardstick reproduces the per-stream TrackerCtx's matches, due sets and time stamps"""
    scn = tc.SCENARIOS[name]
    host, _, _ = tc.run_host(scn)
    lock, _ = tb.run_lockstep_scenario(scn, tc.S * tc.K)
    n_due = 0
    for i, (st, rec) in enumerate(zip(scn.steps, lock)):
        where = tc.layout(scn, i)[3]
        want = set()
        for f, s in enumerate(st.streams):
            assert rec["matched"][f] == host[i][f]["matched"], (name, i, s)
            want |= {f * tc.K + where[f][di] for _, di in host[i][f]["due"]}
            for tid, last in host[i][f]["last"].items():
                assert rec["last"][(s, tid)] == last, (name, i, s, tid)
        assert set(rec["due"].tolist()) == want and rec["n_deferred"] == 0, (name, i)
        n_due += len(want)
    assert n_due > 0


@pytest.mark.parametrize("budget", [1, 5])
def test_lockstep_with_a_binding_budget(budget):
    """12 candidates in every step: min(E, 12) are taken, the never-embedded first, and nobody starves: a track is taken
    again after at most ceil(12 / E) steps"""
    scn = tb.binding_scenario()
    lock, _ = tb.run_lockstep_scenario(scn, budget)
    bound = -(-12 // budget)
    taken_at = {}
    for i, rec in enumerate(lock):
        cand = np.flatnonzero(~np.isnan(rec["waited"]))
        assert cand.size == 12 and rec["due"].size == budget and rec["n_deferred"] == 12 - budget
        for j in rec["due"]:
            taken_at.setdefault(int(j), []).append(i)  # (still cards: a slot is a track)
    assert len(taken_at) == 12
    for j, steps in taken_at.items():
        assert steps[0] < bound and max(np.diff(steps), default=0) <= bound and len(scn.steps) - steps[-1] <= bound, (j, steps)
