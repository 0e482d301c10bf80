"""CPU-only: the labelled top-k oracle (match_labels_common.py) against a second statement of the contract, the exactness
of the tiled scheme the kernels use (range-level dedupe + merge dedupe) and the counter-example against a merge-only
dedupe, the chosen seeds, and the status convention of the new entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_labels_common as L
from conftest import ROOT


@pytest.fixture(scope="module")
def libpath():
    from mtgv import native

    if not os.path.exists(native.LIB_PATH):
        subprocess.run([sys.executable, os.path.join(ROOT, "mtg-vision_amd", "build.py")], check=True)
    return native.LIB_PATH


def _second_statement(s, tags, groups, mask, distinct, k, threshold):
    """per-group argmax, then sort: independent of the oracle's ordered walk"""
    el = L.eligible(tags, mask)
    rows = [n for n in range(len(s)) if el[n] and (not distinct or groups[n] < 0)]
    if distinct:
        for g in sorted(set(int(x) for x in groups[el] if x >= 0)):
            members = [n for n in range(len(s)) if el[n] and groups[n] == g]
            best = max(s[n] for n in members)
            rows.append(min(n for n in members if s[n] == best))
    rows.sort(key=lambda n: (-s[n], n))
    rows = rows[:k]
    return [n for n in rows if threshold is None or s[n] >= threshold]


def _random_problem(rng, n, b, ties=True):
    s = rng.standard_normal((b, n))
    if ties:
        s = np.round(s * 4) / 4  # a handful of distinct values: many exact ties
    tags = rng.integers(0, 16, n).astype(np.uint64)
    groups = rng.integers(-1, max(2, n // 6), n).astype(np.int32)
    masks = np.stack([rng.integers(0, 16, b), rng.integers(0, 16, b), rng.integers(0, 16, b)], 1).astype(np.uint64)
    masks[rng.random(b) < 0.5, 1] = 0
    masks[rng.random(b) < 0.5, 2] = 0
    masks[rng.random(b) < 0.3, 0] = 0
    return s, tags, groups, masks


@pytest.mark.parametrize("distinct", [False, True])
def test_oracle_equals_second_statement(distinct):
    rng = np.random.default_rng(7)
    for trial in range(40):
        n, b, k = int(rng.integers(1, 80)), 4, int(rng.integers(1, 12))
        s, tags, groups, masks = _random_problem(rng, n, b)
        thr = None if trial % 2 else 0.25
        ids, sc = L.labelled_topk(s, tags, groups, masks, distinct, k, thr)
        for i in range(b):
            want = _second_statement(s[i], tags, groups, masks[i], distinct, k, thr)
            assert ids[i].tolist() == want + [-1] * (k - len(want)), (trial, i)
            assert sc[i, : len(want)].tolist() == [s[i, r] for r in want] and np.isneginf(sc[i, len(want):]).all()
            if distinct:
                g = [int(groups[r]) for r in want if groups[r] >= 0]
                assert len(g) == len(set(g))


def test_defaults_are_the_plain_topk():
    from oracle import match_ref as M

    rng = np.random.default_rng(8)
    s, tags, _, _ = _random_problem(rng, 50, 6)
    ids, sc = L.labelled_topk(s, tags, np.full(50, -1, np.int32), L.NO_FILTER, True, 7, 0.0)
    rid, rsc = M.topk_from_scores(s, 7, 0.0)
    assert (ids == rid).all() and (sc == rsc).all()


@pytest.mark.parametrize("cols", [64, 96])
def test_partition_property(cols):
    """range-level dedupe + merge dedupe is exact; merge-only dedupe is not"""
    rng = np.random.default_rng(100 + cols)
    wrong = 0
    for trial in range(200):
        n, k = int(rng.integers(cols, 5 * cols)), int(rng.integers(1, 9))
        s, tags, groups, masks = _random_problem(rng, n, 2)
        groups = rng.integers(-1, 6, n).astype(np.int32)  # few groups: ranges fill up with one group's rows
        want, _ = L.labelled_topk(s, tags, groups, masks, True, k)
        assert (L.tiled_topk(s, tags, groups, masks, True, k, cols) == want).all(), trial
        assert (L.tiled_topk(s, tags, groups, masks, False, k, cols) == L.labelled_topk(s, tags, groups, masks, False, k)[0]).all(), trial
        wrong += int((L.tiled_topk(s, tags, groups, masks, True, k, cols, range_dedupe=False) != want).any())
    assert wrong > 0, "the wrong scheme never showed: the trials do not exercise the hiding case"


@pytest.mark.parametrize("cols", [64, 96])
def test_hiding_counter_example(cols):
    from oracle import match_ref as M

    bank, q, groups = L.hiding_case(64)
    s = M.scores(q[None], bank)
    top = np.sort(s[0])[::-1]
    # 0.94 .. 0.90, 0.8, 0.5, 0.4: gaps of 1e-2 and more, up to the float32 rounding of the stored rows (6e-8)
    assert (top[:7] - top[1:8]).min() >= 1e-2 - 1e-7
    tags = np.zeros(L.N, np.uint64)
    assert L.labelled_topk(s, tags, groups, L.NO_FILTER, True, 3)[0][0].tolist() == [204, 210, 30]
    assert L.tiled_topk(s, tags, groups, L.NO_FILTER, True, 3, cols)[0].tolist() == [204, 210, 30]
    assert L.tiled_topk(s, tags, groups, L.NO_FILTER, True, 3, cols, range_dedupe=False)[0].tolist() == [204, 30, 400]
    assert 200 // cols == 210 // cols  # one range holds rows 200..210


def test_ties_case_has_pads_at_k_100():
    from oracle import match_ref as M

    bank, q, groups = L.ties_case(36)
    ids, _ = L.labelled_topk(M.scores(q[None], bank), np.zeros(L.N, np.uint64), groups, L.NO_FILTER, True, 100)
    assert ids[0, :4].tolist() == [10, 20, 21, 150] and (ids[0, :11] >= 0).all() and (ids[0, 11:] == -1).all()


@pytest.mark.parametrize("d", [768, 64, 36])
def test_seeds_leave_no_near_ties(d):
    """what the GPU tests assert on the host before they compare ids, for every query, k and variant at once"""
    from oracle import match_ref as M

    case = L.random_case(d)
    bank, q, tags, groups, masks = case
    s = M.scores(q, bank)
    for variant in ("filter", "distinct", "both"):
        m, distinct = L.variant_labels(case, variant)
        assert L.rep_margin(s, tags, groups, m, distinct, L.K_MAX).min() > 1e-5, variant
    # the designed queries are what their names say
    el = [L.eligible(tags, masks[i]) for i in range(L.N_SPECIAL)]
    assert el[0].sum() > L.K_MAX and el[1].sum() == 0 and el[2].sum() == 2
    assert np.nonzero(el[3])[0].min() >= 384 and np.nonzero(el[4])[0].tolist() == L.ROWS_BIT61


def test_new_entry_points_status_without_gpu(libpath):
    from mtgv import native

    lib = native.lib()
    assert lib.mtgv_version() >= 105
    for rc in (
        lib.mtgv_bank_set_labels(None, 0, 1, None, None, None),
        lib.mtgv_bank_get_labels(None, 0, 1, None, None),
        lib.mtgv_bank_topk_ex(None, None, 1, 1, 0, 0.0, None, 1, None, None, None),
    ):
        assert rc == 1 and b"null" in lib.mtgv_last_error()
        with pytest.raises(AssertionError):
            native.check(rc)
