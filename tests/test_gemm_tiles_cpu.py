"""CPU-only companion of test_gpu_gemm_tiles.py (cases, draws, references: gemm_tiles_common.py).  It checks the case
table itself, so that an edit which quietly takes a path of the kernel out of the GPU test fails here:
  - per case and built tile, from BM = 128, BN = 32 tn and BK: a tile wholly inside the problem, a ragged last row tile, a
    ragged last column tile and a K tail exactly where the case's labels say, and over the table every tile width gets
    all four;
  - no case can be planned onto the LDS-DMA split kernel in f16x3 mode (gemm_sp_plan's refusals as arithmetic);
  - the reductions stay within what the 3e-5 bound was established for (dense K <= 316, conv K <= 512), every launch
    within 768 x 331 x 288;
  - the crop reference is oracle.detector_ref.mask_logits' rule: equal to it on a random input, and the placed boxes decide
    the pixels their comments name;
  - mtgv_op_mask_logits refuses what it cannot run before it touches the device."""
import numpy as np
import pytest

import gemm_tiles_common as gc


def _label_check(name, M, N, K, interior, ragged_m, ragged_n, k_tail):
    for t in gc.TILES:
        f = gc.tile_facts(M, N, K, t)
        tn, bk = t[1], t[2]
        assert f["interior"] == (tn in interior), (name, t, f)
        assert f["ragged_m"] == ragged_m, (name, t, f)
        assert f["ragged_n"] == (tn in ragged_n), (name, t, f)
        assert f["k_tail"] == k_tail[0 if bk == 16 else 1], (name, t, f)


@pytest.mark.parametrize("case", gc.DENSE, ids=lambda c: c.name)
def test_dense_case_reaches_what_it_claims(case):
    _label_check(case.name, case.M, case.N, case.K, case.interior, case.ragged_m, case.ragged_n, case.k_tail)
    assert gc.sp_refusals(gc.dense_launch(case)), f"{case.name}: an f16x3 launch could be planned onto the split kernel"
    assert case.K <= 316 and case.K % 4 == 0 and case.M <= 768 and case.N <= 331
    if case.hw:
        assert case.M % case.hw == 0 and (case.scale or case.grn)
    assert not (case.scale and case.act != gc.NONE), "the GRN prologue has a linear epilogue only"


@pytest.mark.parametrize("case", gc.CONV, ids=lambda c: c.name)
def test_conv_case_reaches_what_it_claims(case):
    L = gc.conv_launch(case)
    # every conv case: whole tiles and ragged ones both ways under every tile (297 rows, 168 columns)
    _label_check(case.name, L["M"], L["N"], L["K"], gc.ALL_TN, True, gc.ALL_TN, case.k_tail)
    assert 257 <= L["M"] <= 383 and L["K"] <= 512
    assert gc.sp_refusals(L), f"{case.name}: an f16x3 launch could be planned onto the split kernel"
    assert L["K"] % 4 == 0 and case.cin % 4 == 0 and case.x_ct % 4 == 0 and case.x_co % 4 == 0  # gemm_launch's own demands
    assert case.x_co + case.cin <= case.x_ct and case.out_co + case.cout <= case.out_ct
    if case.res:
        assert case.res[1] + case.cout <= case.res[0]
    if case.os > 1:
        assert 0 <= case.oy < case.os and 0 <= case.ox < case.os and (case.oy, case.ox) != (0, 0)


@pytest.mark.parametrize("case", gc.MASK, ids=lambda c: c.name)
def test_mask_case_reaches_what_it_claims(case):
    L = gc.mask_launch(case)
    assert "batch > 1" in gc.sp_refusals(L)
    for t in gc.TILES:
        assert (case.mh * case.mw) % (32 * t[1]) != 0, "a ragged last column tile at every width"
    rows = [min(nd, case.mask_rows) for nd in case.n_det]
    assert rows[0] == 0, "a frame whose tiles all return"
    assert rows[2] == case.mask_rows < case.n_det[2], "a frame cut at mask_rows"
    assert len(gc.placed_boxes(case)) > rows[1] > 0
    if case.mask_rows > gc.BM:
        assert rows[1] <= gc.BM, "a frame whose second row tile returns"
    assert case.max_det >= max(case.n_det) and case.nm % 4 == 0


def test_table_covers_every_path_under_every_tile():
    """over the table, each built tile sees: a fast + interior block, a K tail, whole and ragged column tiles, each activation
    instance of the dense and the conv kernel, the residual in the interior and in the edge epilogue, the GRN prologue and
    the GRN partials with one and with several images per tile"""
    for t in gc.TILES:
        tn, bk = t[1], t[2]
        dense = [(c, gc.tile_facts(c.M, c.N, c.K, t)) for c in gc.DENSE]
        assert {c.act for c, f in dense if f["interior"] and not f["k_tail"] and not c.scale} == {gc.NONE, gc.GELU, gc.MISH, gc.SILU, gc.SIGMOID}
        assert any(c.res and f["interior"] and f["ragged_m"] and f["ragged_n"] for c, f in dense)
        assert any(f["k_tail"] and f["interior"] for c, f in dense) and any(not f["ragged_n"] for c, f in dense) == (tn in (1, 2, 5))
        assert {c.hw for c, f in dense if c.scale and f["interior"]} == {1, 24, 130}
        assert any(c.scale and c.res for c, f in dense) and any(c.shift for c, f in dense)
        grn = [c for c, f in dense if c.grn and f["interior"]]
        assert any(c.hw >= 2 * gc.BM and c.hw % gc.BM == 0 for c in grn) and any(c.hw < gc.BM for c in grn) and any(gc.BM < c.hw < 2 * gc.BM for c in grn)
        if bk == 32:
            assert any(f["k_tail"] and c.K % 16 == 0 for c, f in dense), "a K that is whole at BK 16 and has a tail at BK 32"
    assert {c.act for c in gc.CONV} == {gc.SILU, gc.NONE, gc.MISH}
    assert {(c.k, c.stride, c.pad) for c in gc.CONV} >= {(3, 1, 1), (3, 2, 1), (2, 2, 0), (4, 4, 0), (1, 1, 0)}
    assert any(c.res for c in gc.CONV) and any(c.os > 1 for c in gc.CONV) and any(c.x_co > 0 and c.out_co > 0 for c in gc.CONV)
    assert len({c.name for c in gc.DENSE}) == len(gc.DENSE) and len({c.name for c in gc.CONV}) == len(gc.CONV)
    assert len(gc.TILES) == 6 and not set(gc.TILES) & set(gc.UNBUILT)


def test_sp_refusals_restate_the_planner():
    """a launch the split kernel takes in f16x3 (pwconv-shaped f32 rows) has no refusal; each listed reason alone refuses"""
    ok = dict(M=293, N=328, K=96, conv=False, remap=False, batch=1, c_total=96, c_off=0, ldo=328, o_off=0, ldr=None)
    assert gc.sp_refusals(ok) == []
    for change in (dict(ldo=331), dict(K=100), dict(batch=3), dict(conv=True), dict(remap=True), dict(N=63), dict(M=127)):
        assert len(gc.sp_refusals({**ok, **change})) == 1, change
    # the 1x1 conv with slices is a dense launch: only its 194-float output pixel keeps it off the split kernel
    assert gc.sp_refusals(gc.conv_launch(gc.CONV_BY_NAME["1x1-slices-silu"])) == ["ldo % 4 != 0"]
    assert not gc.is_conv(1, 1, 1, 0) and gc.is_conv(1, 1, 2, 0) and gc.is_conv(3, 3, 1, 1)


def test_references_are_finite_and_shaped():
    for c in gc.DENSE:
        ref, sums = gc.dense_ref(c.name)
        assert ref.shape == (c.M, c.N) and np.isfinite(ref).all() and (sums is None) == (not c.grn)
        if c.grn:
            assert sums.shape == (c.M // c.hw, c.N) and (sums > 0).all()
    for c in gc.CONV:
        oh, ow = gc.conv_out_hw(c)
        assert (oh, ow) == (11, 9)
        ref = gc.conv_ref(c.name)
        assert ref.shape == (c.n * oh * ow, c.cout) and np.isfinite(ref).all()
        rows = gc.scatter_rows(c)
        assert len(set(rows.tolist())) == len(rows) and rows.max() < c.n * oh * ow * c.os * c.os
        if c.os == 1:
            assert (rows == np.arange(len(rows))).all()


def test_conv_reference_is_the_gather_the_kernel_defines():
    """A(m, k) = in[img][oh s + kh - p][ow s + kw - p][c], k ordered (kh, kw, c), zero outside: a few rows by hand"""
    c = gc.CONV_BY_NAME["3x3s2-cin12-silu"]
    d, ref = gc.conv_draw(c.name), gc.conv_ref(c.name)
    oh, ow = gc.conv_out_hw(c)
    x = d["x"].astype(np.float64).reshape(c.n, c.h, c.w, c.cin)
    w = d["w"].astype(np.float64).reshape(c.cout, -1)
    for m in (0, ow - 1, oh * ow - 1, oh * ow, c.n * oh * ow - 1):
        img, rem = divmod(m, oh * ow)
        y, xx = divmod(rem, ow)
        a = np.zeros((c.k, c.k, c.cin))
        for kh in range(c.k):
            for kw in range(c.k):
                ih, iw = y * c.stride + kh - c.pad, xx * c.stride + kw - c.pad
                if 0 <= ih < c.h and 0 <= iw < c.w:
                    a[kh, kw] = x[img, ih, iw]
        v = w @ a.reshape(-1) + d["b"]
        v = v / (1 + np.exp(-v))
        assert np.abs(v - ref[m]).max() < 1e-12


def test_crop_reference_is_the_oracles():
    from oracle import detector_ref

    rng = np.random.default_rng(3)
    nm, mh, mw, in_h, in_w, nd, nc = 32, 10, 20, 42, 84, 40, 1  # 5 / 21 both ways: a scale that is not a power of two
    coef = rng.standard_normal((nd, nm)).astype(np.float32)
    protos = rng.standard_normal((mh * mw, nm)).astype(np.float32)
    xy = rng.random((nd, 2)) * [in_w, in_h] - 4
    boxes = np.concatenate([xy, xy + rng.random((nd, 2)) * [in_w / 2, in_h / 2]], 1).astype(np.float32)
    boxes[:8] = np.round(boxes[:8] / 4.2) * 4.2  # edges that land on (or a rounding beside) whole mask pixels
    pred = np.zeros((4 + nc + nm, nd), dtype=np.float32)
    pred[4 + nc :] = coef.T
    want = detector_ref.mask_logits(pred, protos.T.reshape(nm, mh, mw), {"keep_idx": np.arange(nd), "boxes": boxes}, nc, (in_h, in_w))
    got, ins = gc.mask_reference(coef[None], protos[None], [nd], boxes[None], np.float32(mw / in_w), nd, mh, mw)
    assert ((want.reshape(nd, -1) != 0) == ins[0]).all()
    w32 = want.reshape(nd, -1)  # (the oracle rounds its fp64 sums to f32: equal up to that rounding)
    assert (np.abs(got[0].astype(np.float32) - w32) <= np.spacing(np.abs(w32))).all()
    # rows at and beyond n_det, or beyond mask_rows, are zero
    got, ins = gc.mask_reference(coef[None], protos[None], [5], boxes[None], np.float32(mw / in_w), 16, mh, mw)
    assert got.shape == (1, 16, mh * mw) and not got[0, 5:].any() and not ins[0, 5:].any()


def test_placed_boxes_decide_the_pixels_they_name():
    c = gc.MASK[0]
    ins = gc.crop_inside(gc.placed_boxes(c), np.float32(c.mw / c.in_w), c.mh, c.mw).reshape(-1, c.mh, c.mw)

    def block(y0, y1, x0, x1):
        m = np.zeros((c.mh, c.mw), dtype=bool)
        m[y0:y1, x0:x1] = True
        return m

    assert (ins[0] == block(1, 6, 2, 10)).all()   # integer edges: low inclusive, high exclusive
    assert (ins[1] == block(2, 6, 3, 8)).all()    # half-integers
    assert ins[2].all() and not ins[3].any() and not ins[4].any()
    assert (ins[5] == block(c.mh - 1, c.mh, c.mw - 1, c.mw)).all() and (ins[6] == block(0, 1, 0, 1)).all()
    d = gc.mask_draw(c.name)
    _, inside = gc.mask_ref(c.name)
    assert not inside[0].any() and inside[1, :5].any() and not inside[1, 5:].any() and inside[2, gc.BM :].any()
    frac = inside[2].mean()
    assert 0.02 < frac < 0.5, frac  # the random boxes cut: neither everything nor nothing is inside
    assert d["crop_scale"] == np.float32(0.25)


def test_mask_logits_refusals_without_gpu():
    """status 1 and a message before anything is launched: the checks run on the host"""
    import ctypes as C

    from mtgv import native as nv

    L = nv.lib()
    assert L.mtgv_version() >= 116
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(nm, mask_rows, form, out=p, max_det=300, n=1):
        return L.mtgv_op_mask_logits(p, p, p, p, n, max_det, nm, 12, 20, 0.25, mask_rows, form, out, None)

    for args in ((64, 16, gc.FORM_PIXELS), (32, 17, gc.FORM_PIXELS)):
        assert call(*args) == 1 and b"per-pixel" in L.mtgv_last_error(), args
    assert call(32, 16, 3) == 1 and b"form" in L.mtgv_last_error()
    assert call(32, 16, gc.FORM_GEMM, out=None) == 1 and b"null" in L.mtgv_last_error()
    assert call(32, 301, gc.FORM_GEMM) == 1 and b"mask_rows" in L.mtgv_last_error()
    assert call(32, 0, gc.FORM_AUTO) == 1 and call(32, 16, gc.FORM_AUTO, n=0) == 1
