"""CPU-only: the cases of test_gpu_c2f_tail_direct.py can tell the likely mistakes of a fused C2f tail apart, shown on the
fp64 reference alone (c2f_tail_common.py).  For every case the correct reference differs somewhere by more than 100 x
the GPU test's tolerance from the reference with
  - t not zeroed outside the frame (the second conv over the 3x3 conv of a zero-padded input extended by one pixel: the
    trap the P2 comment of c2f_tail_kernel.h names),
  - the shortcut flag flipped,
  - W1 and W2 exchanged,
  - the slices of cat in front of y_last in the wrong order (nb = 2: there is one such slice otherwise),
  - the images stacked without the zero padding between them, a cross-image halo (n > 1: no neighbour otherwise).
Also: the ctypes descriptor matches the header's struct, the version, and the table itself against c2f_tail_ok's rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import c2f_tail_common as cc
from conftest import ROOT

SEPARATION = 100 * cc.TOL


@pytest.mark.parametrize("index", range(len(cc.CASES)))
def test_cases_separate_the_mutations(index):
    case = cc.CASES[index]
    d, ref = cc.drawn(index)
    assert np.isfinite(ref).all() and ref.shape == (case.n * case.h * case.w, 2 * case.ch)
    for m in cc.MUTATIONS:
        if not cc.applies(m, case):
            continue
        diff = np.abs(cc.reference(case, d, m) - ref)
        print(f"c2f tail case {index} {m}: max |mutated - reference| = {diff.max():.3g}")
        assert diff.max() > SEPARATION, (index, m, diff.max())
        if m in ("t_not_zeroed", "cross_image_halo"):  # these two show at a border only: the inner pixels agree (in fp64)
            img = diff.reshape(case.n, case.h, case.w, -1)
            inner = img[:, 1:-1, 1:-1] if m == "t_not_zeroed" else img[:, 2:-2]
            assert inner.max() < 1e-9, (index, m)


def test_every_mutation_and_combination_is_exercised():
    for m in cc.MUTATIONS:
        assert sum(cc.applies(m, c) for c in cc.CASES) >= 2, m
    # all six (ch, nb, shortcut) combinations c2f_tail_ok admits
    assert {(c.ch, c.nb, c.shortcut) for c in cc.CASES} == {(16, 1, True), (16, 1, False), (32, 1, True), (32, 1, False), (32, 2, True), (32, 2, False)}


def test_cases_meet_the_kernel_predicate():
    """c2f_tail_ok's geometry rules (c2f_tail.hip), restated: a case the launch would refuse tests nothing"""
    for c in cc.CASES:
        tw = 32 if c.ch == 16 else 16
        assert c.h >= 80 and c.w >= 80 and c.h % 8 == 0 and c.w % tw == 0, c
        assert all(v % 8 == 0 for v in (c.cat_ct, c.cat_co, c.out_ct, c.out_co)), c
        assert c.cat_ct >= c.cat_co + (1 + c.nb) * c.ch and c.out_ct >= c.out_co + 2 * c.ch, c
    assert min(c.n * c.h * c.w for c in cc.CASES) == 80 * 80 and max(c.n * c.h * c.w for c in cc.CASES) == 3 * 80 * 80


def test_border_rows_are_scaled():
    case = cc.CASES[1]
    d, _ = cc.drawn(1)
    x = d.x.reshape(case.n, case.h, case.w, -1)
    border = np.concatenate([x[:, :2], x[:, -2:]], 1)
    assert 7.0 < border.std() < 9.0 and 0.9 < x[:, 2:-2].std() < 1.1


def test_descriptor_matches_header():
    from mtgv import native

    src = open(os.path.join(ROOT, "include", "mtgv.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mtgv_c2f_tail;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        for name in re.sub(r"^(const\s+)?\w+\s*", "", decl).split(","):
            names.append(name.strip(" *"))
            kinds.append(C.c_void_p if pointer else C.c_int32)
    assert [(n, t) for n, t in native.C2fTail._fields_] == list(zip(names, kinds))
    assert native.lib().mtgv_version() >= 112


def test_null_descriptor_is_status_1_without_gpu():
    from mtgv import native

    L = native.lib()
    assert L.mtgv_op_c2f_tail(None, None) == 1 and b"c2f_tail" in L.mtgv_last_error()
    d = native.C2fTail()
    assert L.mtgv_op_c2f_tail(C.byref(d), None) == 1 and b"null" in L.mtgv_last_error()
