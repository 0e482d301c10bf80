"""CPU-only companion of test_gpu_dwconv_ln_direct.py (cases, draws, reference: dwconv_ln_common.py).
  - Every case reaches the kernel form the table names, by mtgv_op_dwconv7_ln_form - the launcher's own rule, read without
    a GPU - so a change of that rule cannot take a form out of the direct test unnoticed; together the cases reach all
    eight forms the rule can pick.
  - Every shape and format of the refusal table, and null pointers, are status 1 from both entry points.
  - The cases can tell the likely mistakes of such a kernel apart, shown on the fp64 reference alone: for every case each
    mistake that can show there moves the reference by more than dwconv_ln_common.separation() - 100 x the GPU test's
    tolerance; 2 x for the one-pass variance, with the measurements behind that there.  Cases of 128 images and more: on
    two images of the same draw.
  taps transposed; kernel flipped; horizontal padding read from the adjacent row; vertical padding read from the
  neighbouring image (n > 1); conv bias dropped; variance over C - 1; eps outside the square root and eps dropped (the
  eps = 0.5 case); one-pass variance in f32."""
import ctypes as C

import numpy as np
import pytest

import dwconv_ln_common as cc
from dwconv_ln_common import CASES, REFUSALS, Switches


def _few(index):
    """(case, draw, reference) of CASES[index], cut to two images where the case has 128 or more"""
    case = CASES[index]
    d, ref = cc.drawn(index)
    k = 2 if case.n >= 128 else case.n
    return case._replace(n=k), d, ref[:k]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_case_reaches_its_form(index):
    case = CASES[index]
    with Switches(case.env):
        rc, form = cc.form_of(case.n, case.h, case.w, case.c)
    assert rc == 0 and form == case.form, (index, rc, form, case.form)
    with Switches(case.env, MTGV_DW_ROWS="0"):  # what the GPU test compares every case's bits with
        rc, form = cc.form_of(case.n, case.h, case.w, case.c)
    assert rc == 0 and form == (cc.ROWS, 8 if case.w >= 8 else 4 if case.w >= 4 else 2, 1, 0), (index, rc, form)


def test_cases_reach_every_form():
    rows = {c.form[1:] for c in CASES if c.form[0] == cc.ROWS}
    assert rows == {(4, 3, 1), (8, 3, 0), (4, 3, 0), (8, 1, 0), (4, 1, 0), (2, 1, 0)}
    assert {(c.form[0], c.c) for c in CASES if c.form[0] != cc.ROWS} == {(cc.STREAM, 96), (cc.STREAM, 192), (cc.IMAGE, 384), (cc.IMAGE, 768)}
    assert sum(c.c % 8 != 0 for c in CASES) == 1  # one case that only the f32 output takes
    assert all(CASES[i].n > 1 and CASES[i].n < 128 for i in cc.BATCH_CASES) and {CASES[i].form[0] for i in cc.BATCH_CASES} == {cc.ROWS, cc.IMAGE}


def test_tap_table_limit():
    """C = 280 is the largest C whose row-group block - partial sums, statistics and the 49 x C tap table - fits the
    default 64 KB of LDS: asked of dwconv7_ln_rows_lds_bytes itself, through the rule that calls it (WL = 1 exactly while
    dwconv7_ln_rows_lds_bytes(4, 3, true, C) <= 65536), at every C the launch admits"""
    with Switches(()):
        for c in range(16, 1028, 4):
            assert cc.form_of(2, 5, 4, c) == (0, (cc.ROWS, 4, 3, int(c <= 280))), c
        assert cc.form_of(2, 5, 8, 284)[1] == (cc.ROWS, 8, 3, 0)
        # the batch thresholds of the streaming and whole-image forms
        assert cc.form_of(127, 14, 32, 96)[1] == (cc.ROWS, 4, 3, 1) and cc.form_of(127, 12, 8, 384)[1] == (cc.ROWS, 8, 3, 0)
    with Switches((), MTGV_DW_IMAGE="0"):
        assert cc.form_of(128, 12, 8, 384)[1] == (cc.ROWS, 8, 3, 0)


def test_refusals_without_gpu():
    from mtgv import native

    L = native.lib()
    assert L.mtgv_version() >= 113
    buf = np.zeros(64, np.float32)  # never read: every call below is refused before anything is launched
    p = C.c_void_p(buf.ctypes.data)
    form = (C.c_int32 * 4)(-1, -1, -1, -1)
    for what, (n, h, w, c), fmt in REFUSALS:
        rc = L.mtgv_op_dwconv7_ln(p, p, p, p, p, p, n, h, w, c, 1e-6, fmt, form, None)
        assert rc == 1 and b"dwconv7_ln" in L.mtgv_last_error(), (what, rc)
        if fmt == 0:  # (the form does not depend on the output format)
            rc, f = cc.form_of(n, h, w, c)
            assert rc == 1 and f == (-1, -1, -1, -1), (what, rc, f)
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert L.mtgv_op_dwconv7_ln(*args, 2, 7, 6, 16, 1e-6, 0, form, None) == 1 and b"null" in L.mtgv_last_error()
    assert L.mtgv_op_dwconv7_ln(p, p, p, p, p, p, 2, 7, 6, 16, 1e-6, 0, None, None) == 1 and b"null" in L.mtgv_last_error()
    assert L.mtgv_op_dwconv7_ln_form(2, 7, 6, 16, None) == 1 and b"null" in L.mtgv_last_error()
    assert L.mtgv_op_dwconv7_ln(p, p, p, p, p, p, 2, 7, 6, 16, 1e-6, 2, form, None) == 1  # no such format
    assert tuple(form) == (-1, -1, -1, -1)


@pytest.mark.parametrize("index", range(len(CASES)))
def test_cases_separate_the_mutations(index):
    case, d, ref = _few(index)
    assert np.isfinite(ref).all() and ref.shape == (case.n, case.h, case.w, case.c)
    for m in cc.MUTATIONS:
        if not cc.applies(m, case):
            continue
        diff = np.abs(cc.reference(case, d, m, images=case.n) - ref)
        print(f"dwconv7_ln case {index} {m}: max |mutated - reference| = {diff.max():.3g}, required {cc.separation(m):.3g}")
        assert diff.max() > cc.separation(m), (index, m, diff.max())
        if m in ("hpad_adjacent_row", "vpad_neighbour_image") and min(case.h, case.w) > 6:  # these show within 3 of a border only
            inner = diff[:, 3:-3] if m == "vpad_neighbour_image" else diff[:, :, 3:-3]
            assert inner.max() < 1e-9, (index, m)


def test_every_mutation_is_exercised():
    for m in cc.MUTATIONS:
        assert sum(cc.applies(m, c) for c in CASES) >= (1 if m.startswith("eps") else 8), m


def test_draw():
    case = CASES[13]
    d, _ = cc.drawn(13)
    assert 7.0 < d.x[:, :3].std() < 9.0 and 7.0 < d.x[:, :, -3:].std() < 9.0 and 0.9 < d.x[:, 3:-3, 3:-3].std() < 1.1
    assert abs(d.bias[1:].mean() - cc.BIAS_OFFSET) < 0.5 and d.bias[0] > cc.BIAS_OFFSET + cc.OUTLIER * np.sqrt(case.c) - 4
    assert cc.reference(case, d, images=2).tobytes() == cc.drawn(13)[1][:2].tobytes()  # images of a batch do not depend on each other
