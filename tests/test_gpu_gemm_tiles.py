"""The convert-on-load implicit-GEMM kernel (gemm_kernel.h) one launch at a time against fp64, under each of the six tiles
it is built for and in both operand precisions (cases, draws and references: gemm_tiles_common.py; what each case reaches
under each tile is checked by test_gemm_tiles_cpu.py).

Every launch
  - is forced onto its tile with MTGV_GEMM_TILE=tm,tn,bk (read per launch; restored afterwards) and runs under the launch
    profiler, whose table must show exactly one GEMM launch, sp == 0 (not the LDS-DMA split kernel) and the forced tile:
    no case passes by running another kernel;
  - writes into an allocation prefilled with a NaN canary, with guard floats before and after and the pixel's other channels
    where the output is a channel slice: every word outside the tensor must be unchanged, every value inside finite.  Conv
    inputs sit among NaNs likewise (the pixel's other channels, w + 2 pixels before the first and after the last image), so a
    tap that should have been padding poisons the output;
  - is compared with torch fp64 on the CPU at 3e-5 absolute (gemm_tiles_common.TOL);
and within one precision the output words under the six tiles must be identical (the GRN partial sums too): the property
test_detector_batch32_equals_single_frames and test_encoder_batch256_consistency_and_oracle_sample rely on, since the
cost model picks different tiles for different M.

`pytest -s` prints the measured maximum error per (case, precision, tile).  In f16x3 mode the single-op entry points
register only the split kernel's copy of the weights, so B is split on the fly in every case here; the pre-split B of
registered weights is reached through the handles only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gemm_tiles_common as gc

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x3"]
CANARY = 0x7FC17FC1  # a NaN as f32
GUARD_ROWS = 8       # rows (pixels) of canary before and after an output tensor
# columns of the profiler's table (gemm_profile_dump)
COL_M, COL_N, COL_K, COL_BATCH, COL_TM, COL_TN, COL_BK, COL_SP = 1, 2, 3, 6, 11, 12, 13, 17


@pytest.fixture(autouse=True)
def _restore_precision():
    from mtgv import native

    before = native.get_gemm_precision()
    yield
    native.set_gemm_precision(before)


class forced_tile:
    """MTGV_GEMM_TILE for the launches inside, the former value (or none) after"""

    def __init__(self, tile):
        self.value = gc.tile_id(tile)

    def __enter__(self):
        self.before = os.environ.get("MTGV_GEMM_TILE")
        os.environ["MTGV_GEMM_TILE"] = self.value

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop("MTGV_GEMM_TILE", None)
        else:
            os.environ["MTGV_GEMM_TILE"] = self.before


def profiled(tmp_path, tile, launch, batch=1):
    """runs launch() under the forced tile and the launch profiler; returns the one row of the profiler's table after
    checking that it names the convert-on-load kernel on that tile"""
    from mtgv import native as nv

    L = nv.lib()
    csv = str(tmp_path / "gemm.csv")
    with forced_tile(tile):
        nv.check(L.mtgv_profile_gemm(1))
        try:
            launch()
            torch.cuda.synchronize()
            nv.check(L.mtgv_profile_gemm_dump(csv.encode()))
        finally:
            nv.check(L.mtgv_profile_gemm(0))
    rows = [ln.split(",") for ln in open(csv).read().split()[1:]]
    assert len(rows) == 1, rows
    r = rows[0]
    assert r[COL_SP] == "0", ("ran on the LDS-DMA split kernel", r)
    assert (int(r[COL_TM]), int(r[COL_TN]), int(r[COL_BK])) == tile, (tile, r)
    assert int(r[COL_BATCH]) == batch, r
    return r


class Out:
    """rows x ct floats of canary with GUARD_ROWS more rows either side; channels [co, co + c) of the rows in `written`
    (all of them unless given) are the tensor"""

    def __init__(self, rows, ct, co=0, c=None, written=None):
        self.rows, self.ct, self.co, self.c = rows, ct, co, ct if c is None else c
        self.written = np.arange(rows) if written is None else np.asarray(written)
        self.dev = torch.full((rows + 2 * GUARD_ROWS, ct), CANARY, dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD_ROWS * self.ct * 4

    def read(self):
        """(values fp64 [written][c], their words) after checking that nothing else changed and all of it is finite"""
        got = self.dev.cpu().numpy().view(np.uint32)
        body = got[GUARD_ROWS : GUARD_ROWS + self.rows]
        words = np.ascontiguousarray(body[self.written, self.co : self.co + self.c])
        rest = got.copy()
        rest[GUARD_ROWS + self.written, self.co : self.co + self.c] = CANARY
        assert (rest == CANARY).all(), "words outside the output tensor changed"
        vals = words.view(np.float32).astype(np.float64)
        assert np.isfinite(vals).all(), "output not finite (unwritten, or poisoned by a NaN the kernel must not read)"
        return vals, words


def among_nans(values, ct, co, guard_rows):
    """[rows][c] f32 as channels [co, co + c) of ct, NaN in every other channel and in guard_rows rows either side;
    (device tensor, pointer to row 0)"""
    rows, c = values.shape
    host = np.full((rows + 2 * guard_rows, ct), np.nan, dtype=np.float32)
    host[guard_rows : guard_rows + rows, co : co + c] = values
    dev = torch.from_numpy(host).cuda()
    return dev, dev.data_ptr() + guard_rows * ct * 4


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()


def report(kind, name, mode, errs):
    print(f"gemm_tiles {kind} {name} [{mode}]: max_err " + "  ".join(f"{gc.tile_id(t)}: {e:.3g}" for t, e in errs.items()))


def assert_same_bits(name, mode, words):
    first = gc.TILES[0]
    for t in gc.TILES[1:]:
        same = torch.equal(torch.from_numpy(words[t].view(np.int32)), torch.from_numpy(words[first].view(np.int32)))
        assert same, f"{name} [{mode}]: tile {gc.tile_id(t)} and tile {gc.tile_id(first)} differ in {int((words[t] != words[first]).sum())} words"


# ---- dense ----
def run_dense(tmp_path, case, tile, T):
    """one launch of the case under `tile`: (values, words, per-image GRN sums or None, the partials' words or None)"""
    from mtgv import native as nv

    L = nv.lib()
    out = Out(case.M, case.N)
    part = None
    if case.grn:
        part = torch.zeros(int(L.mtgv_op_linear_ex_part_floats(case.M, case.N, case.K, case.act, case.hw)) + 4, device="cuda")

    def launch():
        if case.hw:
            nv.check(L.mtgv_op_linear_ex(nv.ptr(T["a"]), nv.ptr(T["w"]), nv.ptr(T["b"]), nv.ptr(T["r"]), out.ptr, case.M, case.N, case.K, case.act,
                                         case.hw, nv.ptr(T["sc"]), nv.ptr(T["sh"]), nv.ptr(part), nv.stream()))
        else:
            nv.check(L.mtgv_op_linear(nv.ptr(T["a"]), nv.ptr(T["w"]), nv.ptr(T["b"]), nv.ptr(T["r"]), out.ptr, case.M, case.N, case.K, case.act, nv.stream()))

    r = profiled(tmp_path, tile, launch)
    assert (int(r[COL_M]), int(r[COL_N]), int(r[COL_K])) == (case.M, case.N, case.K), r
    vals, words = out.read()
    sums = pwords = None
    if case.grn:
        ur, sm = C.c_int32(0), C.c_int32(0)
        nv.check(L.mtgv_op_last_grn_layout(C.byref(ur), C.byref(sm)))
        unit, segmax = ur.value, sm.value
        assert unit == gc.BM * tile[0] and segmax == (unit - 1) // case.hw + 2
        units = -(-case.M // unit)
        assert units * segmax * case.N <= part.numel() - 4
        assert not part[units * segmax * case.N :].any(), "partials written beyond their layout"
        p = part[: units * segmax * case.N].cpu().view(units, segmax, case.N)
        sums = np.zeros((case.M // case.hw, case.N))
        used = []
        for t in range(units):
            first, last = (t * unit) // case.hw, (min((t + 1) * unit, case.M) - 1) // case.hw
            for s in range(last - first + 1):
                sums[first + s] += p[t, s].double().numpy()
                used.append(p[t, s].numpy())
        pwords = np.stack(used).view(np.uint32)
    return vals, words, sums, pwords


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", gc.DENSE, ids=lambda c: c.name)
def test_dense(tmp_path, case, mode):
    from mtgv import native as nv

    nv.set_gemm_precision(mode)
    ref, ref_sums = gc.dense_ref(case.name)
    T = {k: dev(v) for k, v in gc.dense_draw(case.name).items()}
    errs, words, pwords, sum_errs = {}, {}, {}, {}
    for tile in gc.TILES:
        vals, words[tile], sums, pwords[tile] = run_dense(tmp_path, case, tile, T)
        errs[tile] = float(np.abs(vals - ref).max())
        if case.grn:
            r = vals  # (mish, no residual: the output is the value whose squares are summed)
            own = (r * r).reshape(case.M // case.hw, case.hw, case.N).sum(1)
            sum_errs[tile] = (float((np.abs(sums - ref_sums) / (np.abs(ref_sums) + 1e-3)).max()), float((np.abs(sums - own) / (np.abs(own) + 1e-3)).max()))
    report("dense", case.name, mode, errs)
    if case.grn:
        print(f"gemm_tiles dense {case.name} [{mode}]: GRN sums, relative error vs fp64 / vs the launch's own output " +
              "  ".join(f"{gc.tile_id(t)}: {a:.3g} / {b:.3g}" for t, (a, b) in sum_errs.items()))
    for tile in gc.TILES:
        assert errs[tile] < gc.TOL, (case.name, mode, tile, errs[tile])
        if case.grn:
            assert max(sum_errs[tile]) < gc.GRN_RTOL, (case.name, mode, tile, sum_errs[tile])
    assert_same_bits(case.name, mode, words)
    if case.grn:
        assert_same_bits(case.name + " GRN partials", mode, pwords)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tile", gc.UNBUILT, ids=gc.tile_id)
def test_tile_that_is_not_built_is_an_error(tile, mode):
    """status 1 naming the tile, nothing written: never another tile in its place"""
    from mtgv import native as nv

    L = nv.lib()
    nv.set_gemm_precision(mode)
    case = gc.DENSE_BY_NAME[gc.UNBUILT_CASE]
    T = {k: dev(v) for k, v in gc.dense_draw(case.name).items()}
    out = Out(case.M, case.N)
    with forced_tile(tile):
        rc = L.mtgv_op_linear(nv.ptr(T["a"]), nv.ptr(T["w"]), nv.ptr(T["b"]), None, out.ptr, case.M, case.N, case.K, case.act, nv.stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"no kernel for tile" in L.mtgv_last_error(), (rc, L.mtgv_last_error())
    assert (out.dev.cpu().numpy().view(np.uint32) == CANARY).all(), "the refused launch wrote to its output"


@pytest.mark.parametrize("mode", MODES)
def test_refused_tile_leaves_no_row_in_the_profile(tmp_path, mode):
    """the tile is refused before the launch profiler records anything: a refused launch followed by a real one leaves
    the real one's row alone in the table, so a row's shape and tile always belong to the time beside them"""
    from mtgv import native as nv

    L = nv.lib()
    nv.set_gemm_precision(mode)
    case = gc.DENSE_BY_NAME[gc.UNBUILT_CASE]
    T = {k: dev(v) for k, v in gc.dense_draw(case.name).items()}
    out = Out(case.M, case.N)
    csv = str(tmp_path / "gemm.csv")

    def launch():
        return L.mtgv_op_linear(nv.ptr(T["a"]), nv.ptr(T["w"]), nv.ptr(T["b"]), None, out.ptr, case.M, case.N, case.K, case.act, nv.stream())

    nv.check(L.mtgv_profile_gemm(1))
    try:
        with forced_tile((1, 2, 32)):
            rc = launch()
        assert rc == 1 and b"no kernel for tile" in L.mtgv_last_error(), (rc, L.mtgv_last_error())
        with forced_tile((1, 2, 16)):
            nv.check(launch())
        torch.cuda.synchronize()
        nv.check(L.mtgv_profile_gemm_dump(csv.encode()))
        ms, flops, launches = C.c_double(0), C.c_double(0), C.c_int64(0)
        nv.check(L.mtgv_profile_gemm_read(C.byref(ms), C.byref(flops), C.byref(launches)))
    finally:
        nv.check(L.mtgv_profile_gemm(0))
    rows = [ln.split(",") for ln in open(csv).read().split()[1:]]
    assert len(rows) == 1, rows
    r = rows[0]
    assert (int(r[COL_TM]), int(r[COL_TN]), int(r[COL_BK])) == (1, 2, 16) and r[COL_SP] == "0", r
    assert (int(r[COL_M]), int(r[COL_N]), int(r[COL_K])) == (case.M, case.N, case.K), r
    assert launches.value == 1, launches.value
    assert np.isfinite(out.read()[0]).all()


# ---- conv ----
def run_conv(tmp_path, case, tile, T):
    from mtgv import native as nv

    oh, ow = gc.conv_out_hw(case)
    out = Out(case.n * oh * ow * case.os * case.os, case.out_ct, case.out_co, case.cout, written=gc.scatter_rows(case))
    d = nv.ConvEx()
    d.x, d.n, d.h, d.w, d.x_ct, d.x_co, d.cin, d.x_fmt = T["x_ptr"], case.n, case.h, case.w, case.x_ct, case.x_co, case.cin, 0
    d.wt, d.bias = T["w"].data_ptr(), T["b"].data_ptr()
    d.cout, d.kh, d.kw, d.stride, d.pad, d.act = case.cout, case.k, case.k, case.stride, case.pad, case.act
    d.out, d.out_ct, d.out_co, d.out_fmt = out.ptr, case.out_ct, case.out_co, 0
    if case.res:
        d.res, d.res_ct, d.res_co, d.res_fmt = T["r_ptr"], case.res[0], case.res[1], 0
    d.os, d.oy, d.ox, d.os_nq = case.os, case.oy, case.ox, 0
    path = (C.c_int32 * 4)(-9, -9, -9, -9)
    r = profiled(tmp_path, tile, lambda: nv.check(nv.lib().mtgv_op_conv2d_ex(C.byref(d), path, nv.stream())))
    assert path[0] == -1, ("the library reports the LDS-DMA split kernel", tuple(path))
    assert (int(r[COL_M]), int(r[COL_N]), int(r[COL_K])) == (case.n * oh * ow, case.cout, case.k * case.k * case.cin), r
    return out.read()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", gc.CONV, ids=lambda c: c.name)
def test_conv(tmp_path, case, mode):
    from mtgv import native as nv

    nv.set_gemm_precision(mode)
    ref, draw = gc.conv_ref(case.name), gc.conv_draw(case.name)
    T = {"w": dev(draw["w"]), "b": dev(draw["b"])}
    T["x"], T["x_ptr"] = among_nans(draw["x"], case.x_ct, case.x_co, case.w + 2)
    if case.res:
        T["r"], T["r_ptr"] = among_nans(draw["r"], case.res[0], case.res[1], GUARD_ROWS)
    errs, words = {}, {}
    for tile in gc.TILES:
        vals, words[tile] = run_conv(tmp_path, case, tile, T)
        errs[tile] = float(np.abs(vals - ref).max())
    report("conv", case.name, mode, errs)
    for tile in gc.TILES:
        assert errs[tile] < gc.TOL, (case.name, mode, tile, errs[tile])
    assert_same_bits(case.name, mode, words)


# ---- mask logits: the batched GEMM with m_count, batch strides, the crop epilogue and B split on the fly ----
def run_mask(case, T, form, tmp_path=None, tile=None):
    from mtgv import native as nv

    L = nv.lib()
    npx = case.mh * case.mw
    out = Out(case.n * case.mask_rows, npx)

    def launch():
        nv.check(L.mtgv_op_mask_logits(nv.ptr(T["coef"]), nv.ptr(T["protos"]), nv.ptr(T["n_det"]), nv.ptr(T["boxes"]), case.n, case.max_det, case.nm,
                                       case.mh, case.mw, float(T["crop_scale"]), case.mask_rows, form, out.ptr, nv.stream()))

    if tile is not None:
        r = profiled(tmp_path, tile, launch, batch=case.n)
        assert (int(r[COL_M]), int(r[COL_N]), int(r[COL_K])) == (case.mask_rows, npx, case.nm), r
    else:
        launch()
        torch.cuda.synchronize()
    vals, words = out.read()
    return vals.reshape(case.n, case.mask_rows, npx), words


def check_mask(case, label, vals, ref, inside):
    err = float(np.abs(vals - ref).max())
    assert ((vals != 0) <= inside).all(), f"{label}: a value outside its box, or in a row at or beyond min(n_det, mask_rows)"
    # (a logit inside the box that is exactly 0.0 would be a draw's accident: there is none, so the patterns are equal)
    assert ((vals != 0) == inside).all(), f"{label}: zero / non-zero pattern differs from the crop rule"
    for z, nd in enumerate(case.n_det):
        assert not vals[z, min(nd, case.mask_rows) :].any(), (label, z)
    return err


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", gc.MASK, ids=lambda c: c.name)
def test_mask_logits(tmp_path, case, mode):
    from mtgv import native as nv

    nv.set_gemm_precision(mode)
    ref, inside = gc.mask_ref(case.name)
    assert (ref[inside] != 0).all()
    draw = gc.mask_draw(case.name)
    T = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in draw.items()}
    errs, words = {}, {}
    for tile in gc.TILES:
        vals, words[tile] = run_mask(case, T, gc.FORM_GEMM, tmp_path, tile)
        errs[tile] = check_mask(case, f"{case.name} [{mode}] {gc.tile_id(tile)}", vals, ref, inside)
    report("mask", case.name, mode, errs)
    for tile in gc.TILES:
        assert errs[tile] < gc.TOL, (case.name, mode, tile, errs[tile])
    assert_same_bits(case.name, mode, words)
    gemm_vals = words[gc.TILES[0]].view(np.float32).astype(np.float64).reshape(ref.shape)
    L = nv.lib()
    if case.nm == 32 and case.mask_rows <= 16:
        # the per-pixel kernel on the same inputs: another summation order, so the bound and the pattern, not the bits;
        # and it is what form 0 runs at this size
        pv, pw = run_mask(case, T, gc.FORM_PIXELS)
        e = check_mask(case, f"{case.name} [{mode}] per-pixel", pv, ref, inside)
        d = float(np.abs(pv - gemm_vals).max())
        print(f"gemm_tiles mask {case.name} [{mode}]: per-pixel kernel max_err {e:.3g}, against the GEMM {d:.3g}")
        assert e < gc.TOL and d < gc.TOL
        _, aw = run_mask(case, T, gc.FORM_AUTO)
        assert np.array_equal(aw, pw), "form 0 did not run the per-pixel kernel"
    else:
        out = Out(case.n * case.mask_rows, case.mh * case.mw)
        rc = L.mtgv_op_mask_logits(nv.ptr(T["coef"]), nv.ptr(T["protos"]), nv.ptr(T["n_det"]), nv.ptr(T["boxes"]), case.n, case.max_det,
                                   case.nm, case.mh, case.mw, float(T["crop_scale"]), case.mask_rows, gc.FORM_PIXELS, out.ptr, nv.stream())
        torch.cuda.synchronize()
        assert rc == 1 and b"per-pixel" in L.mtgv_last_error()
        assert (out.dev.cpu().numpy().view(np.uint32) == CANARY).all(), "the refused form wrote to its output"
        _, aw = run_mask(case, T, gc.FORM_AUTO)  # form 0 at this size: the batched GEMM under the cost model's tile
        assert np.array_equal(aw, words[gc.TILES[0]]), "form 0 differs from the batched GEMM"
