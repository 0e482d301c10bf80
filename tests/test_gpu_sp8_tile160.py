"""The 128 x 160 tile of the LDS-DMA split GEMM (SP_CFG_N160, csrc/gemm_sp_cfg.h tile 7): the window conv of the detector
heads' stacked first 3x3 convs (64 box + 64 class + 32 coefficient columns) in one column tile.  One launch at a time
through mtgv_op_conv2d_ex, in the manner of test_gpu_sp8_conv.py and with its helpers: input channels between fp16-NaN
guard bands, the 160 output columns inside a NaN canary, the reported {tile, A mode, epilogue, ring} asserted, fp64
reference at that file's 3e-5, and bit-identity with the same launch on the 128 x 96 tile (MTGV_SP_CFG=2), the
planner's choice before this tile existed.

Maps: one partial tile (M = 49), two images of 12 x 20 (M = 480: a tile spans both images), three of 28 x 28 (M = 2352:
19 tiles, the last one ragged).  Cin 64 / 128 / 256: two, four and eight 32-channel slices, as at P3 / P4 / P5.

The planner names the tile only for launches of more than one round of its tiles (512; gemm_sp.hip: a launch of one
round lasts as long as one tile, and there the narrower tiles win), so the small maps force it
with MTGV_SP_CFG=7 - which the planner honours only where the tile's one instance can run - and two maps on either side
of that threshold run unforced."""
import numpy as np
import pytest

from test_gpu_sp8_conv import (A_CONV, A_SP8, A_WINDOW, CFG_96, EPI_SP8_OUT, NONE, RING, SILU, SP8, TOL, ConvCase, conv_ex, forced_cfg, output,
                               sp8_input, weights)

pytestmark = pytest.mark.gpu

CFG_N160 = 7
CFG_192 = 1  # the 128 x 192 tile
MAPS = [(1, 7, 7), (2, 12, 20), (3, 28, 28)]


@pytest.fixture(autouse=True)
def _f16x3():
    from mtgv import native

    before = native.get_gemm_precision()
    native.set_gemm_precision("f16x3")
    yield
    native.set_gemm_precision(before)


def _case(seed, n, h, w, cin, cout=160):
    # input: channels 8.. of a pixel 16 floats wider; output: columns 8.. of 176
    return ConvCase(seed, (n, h, w, cin, cout), 3, 1, SILU, SP8, x_view=(cin + 16, 8), out_view=(cout + 16, 8))


@pytest.mark.parametrize("n,h,w", MAPS)
@pytest.mark.parametrize("cin", [64, 128, 256])
def test_tile160_window_conv(n, h, w, cin):
    c = _case(30, n, h, w, cin)
    with forced_cfg(CFG_N160):
        path, err, bits = c.run()
    print(f"tile160 {(n, h, w, cin)}: path={path} max_err={err:.3g}")
    assert path == (CFG_N160, A_WINDOW, EPI_SP8_OUT, RING), path
    assert err < TOL, err
    with forced_cfg(CFG_96):
        path2, err2, bits2 = c.run()
    assert path2[:3] == (CFG_96, A_WINDOW, EPI_SP8_OUT), path2
    assert err2 < TOL, err2
    assert (bits == bits2).all(), "the 128 x 160 tile and the 128 x 96 tile must give the same bits"


@pytest.mark.parametrize("h,want,amode", [(91, CFG_N160, A_WINDOW), (90, CFG_192, A_CONV)])
def test_tile160_named_beyond_one_round(h, want, amode):
    """8 x 91 x 91 = 66248 rows are 518 tiles of 128 x 160, more than one round of 512: the planner names tile 7.
    8 x 90 x 91 = 65520 rows are 512, one round: the search's choice stays.  By its cost model (rounds x tile area /
    efficiency, gemm_sp.hip) that is the 128 x 192 tile - one round of 512 tiles at 1.00 against two rounds of the 128 x 96
    tile at 0.88 - and a 91-pixel-wide window (312 pixels x 128 B = 39.0 KB) beside that tile's 48 KB weight ring does not
    fit twice per CU, so it gathers its taps (SP_A_CONV).  Forced, either map runs the window conv on the other tile."""
    c = _case(36, 8, h, 91, 32)
    path, err, bits = c.run()
    print(f"tile160 unforced {(8, h, 91, 32)}: path={path} max_err={err:.3g}")
    assert path == (want, amode, EPI_SP8_OUT, RING), path
    assert err < TOL, err
    with forced_cfg(CFG_96 if want == CFG_N160 else CFG_N160):
        path2, err2, bits2 = c.run()
    assert path2[0] != want and path2[1] == A_WINDOW and err2 < TOL, (path2, err2)
    assert (bits == bits2).all()


def test_tile160_forced_where_its_instance_exists():
    """MTGV_SP_CFG=7 on a SiLU window conv with SP8 output and 96 columns: the tile runs with 64 of its columns masked"""
    c = _case(31, 2, 12, 20, 64, cout=96)
    path0, err0, bits0 = c.run()
    assert path0[0] != CFG_N160 and path0[1] == A_WINDOW and err0 < TOL, (path0, err0)
    with forced_cfg(CFG_N160):
        path, err, bits = c.run()
    assert path == (CFG_N160, A_WINDOW, EPI_SP8_OUT, RING), path
    assert err < TOL and (bits == bits0).all()


def test_tile160_not_forced_without_an_instance():
    """no instance for a conv without activation and f32 output: forcing tile 7 is refused like an unknown id"""
    from test_gpu_sp8_conv import F32

    c = ConvCase(32, (2, 12, 20, 64, 160), 3, 1, NONE, F32)
    with forced_cfg(CFG_N160):
        path, err, _ = c.run()
    assert path[0] != CFG_N160 and err < TOL, (path, err)


def test_tile160_not_for_1x1():
    c = ConvCase(33, (2, 12, 20, 64, 160), 1, 1, SILU, SP8)
    path, err, _ = c.run()
    assert path[0] != CFG_N160 and path[1] == A_SP8 and err < TOL, (path, err)
    with forced_cfg(CFG_N160):
        path, err, _ = c.run()
    assert path[0] != CFG_N160 and err < TOL, (path, err)


def test_tile160_not_for_stride2():
    c = ConvCase(34, (2, 12, 20, 64, 160), 3, 2, SILU, SP8)
    path, err, _ = c.run()
    assert path[0] != CFG_N160 and path[1] == A_CONV and err < TOL, (path, err)


def test_tile160_does_not_chain():
    """a 3x3 with 160 columns and a chained second layer: no chain tile is that wide, so the pair is refused (status 1)
    and never reaches tile 7"""
    rng = np.random.default_rng(35)
    x, _ = sp8_input(rng, 1, 7, 7, 64)
    w1, b1 = weights(rng, 160, 3, 64)
    w2, b2 = weights(rng, 32, 1, 160)
    out2 = output(49, 32, SP8)
    with pytest.raises(AssertionError, match="chain"):
        conv_ex(x, 1, 7, 7, w1, b1, 1, 1, SILU, None, w2=w2.reshape(32, 160), bias2=b2, act2=NONE, out2=out2)
