"""The fused ConvNeXt-V2 MLP kernel (mlp_fused_kernel.h: pwconv1 + activation + GRN + pwconv2 + residual, hidden tensor in
registers) against the fp64 oracle, at the smallest shapes that reach each of its paths: ragged last tiles of 32 / 64 / 96
rows, image boundaries at every wave of a tile, the C = 80 tail, and the LayerNorm epilogue on ragged tiles.

The route is witnessed by the launch profiler's CSV: the two fused launches are recorded with sp == 2 (mlp_fused.hip).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_BLOCK = 2e-5  # the bound test_block_vs_oracle (test_gpu_ops.py) sets for this op
TOL = 1e-4  # BASELINE.json north_star: fp32 embeddings within 1e-4 of the PyTorch CPU path
SENTINEL = 12345.678  # finite fill of everything a launch must leave alone
OUT_TAIL_ROWS, WS_TAIL_FLOATS = 128, 4096


def _lib():
    from mtgv import native

    return native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _restore_precision():
    from mtgv import native

    before = native.get_gemm_precision()
    yield
    native.set_gemm_precision(before)


# ---------------------------------------------------------------------------
# one block: inputs, fp64 reference, launch
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(n, h, w, c, act):
    """parameters drawn as in test_block_vs_oracle; images that differ in noise level and carry their own channel
    pattern, so that neighbouring images' GRN multipliers are far apart (after the block's LayerNorm plain iid noise
    gives every image nearly the same statistics, and reading the neighbour's multipliers would go unnoticed).
    -> (params f32, x f32 NCHW, ref fp64 NHWC, GRN multipliers Gx / mean(Gx) fp64 [n][4c]); computed once per case"""
    import torch.nn.functional as F

    from oracle import encoder_ref as R

    rng = np.random.default_rng(c + h)
    p = {
        "b.dwconv.weight": rng.standard_normal((c, 1, 7, 7)) / 7,
        "b.dwconv.bias": 0.1 * rng.standard_normal(c),
        "b.norm.weight": 1 + 0.1 * rng.standard_normal(c),
        "b.norm.bias": 0.1 * rng.standard_normal(c),
        "b.pwconv1.weight": rng.standard_normal((4 * c, c)) / np.sqrt(c),
        "b.pwconv1.bias": 0.1 * rng.standard_normal(4 * c),
        "b.grn.gamma": 0.3 * rng.standard_normal((1, 1, 1, 4 * c)),
        "b.grn.beta": 0.1 * rng.standard_normal((1, 1, 1, 4 * c)),
        "b.pwconv2.weight": rng.standard_normal((c, 4 * c)) / np.sqrt(4 * c),
        "b.pwconv2.bias": 0.1 * rng.standard_normal(c),
    }
    p = {k: v.astype(np.float32) for k, v in p.items()}
    noise = rng.standard_normal((n, c, h, w))
    pattern = rng.standard_normal((n, c))
    level = 0.5 + 0.5 * np.arange(n)
    x = (noise * level[:, None, None, None] + 2.0 * pattern[:, :, None, None]).astype(np.float32)
    p64 = {k: torch.from_numpy(v).double() for k, v in p.items()}
    x64 = torch.from_numpy(x).double()
    ref = R.block(x64, p64, "b", act).permute(0, 2, 3, 1).contiguous()
    # the multipliers of convnextv2.py:171-174, restated up to GRN for the check that the images are told apart
    t = F.conv2d(x64, p64["b.dwconv.weight"], p64["b.dwconv.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
    t = R.layernorm_channels_last(t, p64["b.norm.weight"], p64["b.norm.bias"])
    t = R.activation(F.linear(t, p64["b.pwconv1.weight"], p64["b.pwconv1.bias"]), act)
    gx = torch.norm(t, p=2, dim=(1, 2))
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    return p, x, ref, nx


def _neighbour_distance(nx):
    """smallest relative L2 distance between the multiplier vectors of two neighbouring images"""
    d = [(nx[i] - nx[i + 1]).norm() / torch.maximum(nx[i].norm(), nx[i + 1].norm()) for i in range(nx.shape[0] - 1)]
    return min(d).item() if d else float("inf")


def _run_block(tmp_path, p, x, act):
    """one mtgv_op_block launch under the launch profiler -> (out NHWC on the CPU, the CSV's records as dicts).
    Asserts what holds for every launch: the 128 rows behind `out`, the 4096 floats behind the workspace and the input
    are bit-unchanged."""
    nv = _lib()
    L = nv.lib()
    n, c, h, w = x.shape
    m = n * h * w
    X = _dev(x.transpose(0, 2, 3, 1))
    x_before = X.clone()
    out = torch.full((m + OUT_TAIL_ROWS, c), float("nan"), device="cuda")
    out[m:] = SENTINEL
    ws_floats = int(L.mtgv_op_block_workspace_floats(n, h, w, c))
    ws = torch.zeros(ws_floats + WS_TAIL_FLOATS, device="cuda")
    ws[ws_floats:] = SENTINEL
    d = {k: _dev(v) for k, v in p.items()}
    d["b.dwconv.weight"] = _dev(p["b.dwconv.weight"].reshape(c, 49).T)
    csv = str(tmp_path / "gemm.csv")
    nv.check(L.mtgv_profile_gemm(1))
    try:
        nv.check(
            L.mtgv_op_block(
                nv.ptr(X), nv.ptr(out), n, h, w, c, 1 if act == "gelu" else 2,
                nv.ptr(d["b.dwconv.weight"]), nv.ptr(d["b.dwconv.bias"]), nv.ptr(d["b.norm.weight"]), nv.ptr(d["b.norm.bias"]),
                nv.ptr(d["b.pwconv1.weight"]), nv.ptr(d["b.pwconv1.bias"]), nv.ptr(d["b.grn.gamma"]), nv.ptr(d["b.grn.beta"]),
                nv.ptr(d["b.pwconv2.weight"]), nv.ptr(d["b.pwconv2.bias"]), nv.ptr(ws), nv.stream(),
            )
        )
        torch.cuda.synchronize()
        nv.check(L.mtgv_profile_gemm_dump(csv.encode()))
    finally:
        nv.check(L.mtgv_profile_gemm(0))
    sentinel = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    assert (out[m:].view(torch.int32) == sentinel).all(), "rows behind the output were written"
    assert (ws[ws_floats:].view(torch.int32) == sentinel).all(), "floats behind the workspace were written"
    assert torch.equal(X.view(torch.int32), x_before.view(torch.int32)), "the input was written"
    return out[:m].view(n, h, w, c).cpu(), _records(csv)


def _records(csv):
    lines = open(csv).read().split()
    names = lines[0].split(",")
    return [dict(zip(names, ln.split(","))) for ln in lines[1:]]


def _fused_shapes(rows):
    return [(int(r["M"]), int(r["N"]), int(r["K"])) for r in rows if r["sp"] == "2"]


def _where(err):
    """where the largest error sits: an error concentrated in a tile, a wave's rows or a column points at the kernel"""
    n, h, w, c = err.shape
    i = int(err.argmax())
    img, rem = divmod(i, h * w * c)
    return f"max at image {img}, row {rem // c} (tile row {(img * h * w + rem // c) % 128}), channel {rem % c}"


# (n, h, w, C, act): the smallest instance of ...
FUSED = [
    (1, 8, 16, 96, "mish"),  # M = 128: one full tile, one image
    (1, 8, 20, 96, "gelu"),  # M = 160: last tile of 32 rows, three inactive waves
    (3, 8, 20, 96, "mish"),  # M = 480: last tile of 96 rows; image boundaries at rows 160 / 320 = wave 1 of tile 1, wave 2 of tile 2
    (2, 8, 28, 80, "mish"),  # M = 448: C = 80 tail (k beyond C in the last W1 sub-block, masked columns), last tile of 64 rows, boundary at 224
    (3, 8, 20, 80, "gelu"),  # M = 480: C = 80 with gelu, ragged like the third case
    (5, 4, 40, 96, "gelu"),  # M = 800: five images, a boundary in every other tile, last tile of 32 rows
]


@pytest.mark.parametrize("n,h,w,c,act", FUSED)
def test_fused_block_vs_fp64(tmp_path, n, h, w, c, act):
    """mtgv_op_block on the fused kernel (f16x3 mode, hw >= 128, hw % 32 == 0, C = 96 / 80) against the fp64 block.
    Route: exactly two profiler records, both sp == 2, shaped (M, 4C, C) and (M, C, 4C).  Accuracy: < 2e-5.
    Measured max |out - ref64| on MI355X, in the order of FUSED (max |ref| 6.5 to 13.5; the fp32 PyTorch block: 1.8e-6 to
    3.2e-6): 1.45e-6, 1.38e-6, 1.97e-6, 1.55e-6, 1.99e-6, 1.89e-6 - spread over rows, tiles and images."""
    nv = _lib()
    nv.set_gemm_precision("f16x3")
    p, x, ref, nx = _case(n, h, w, c, act)
    if n > 1:
        dist = _neighbour_distance(nx)
        assert dist > 0.25, f"neighbouring images' GRN multipliers differ by only {dist:.2f} (relative L2)"
    out, rows = _run_block(tmp_path, p, x, act)
    m = n * h * w
    assert len(rows) == 2 and _fused_shapes(rows) == [(m, 4 * c, c), (m, c, 4 * c)], rows
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs()
    print(f"fused ({n}, {h}, {w}, {c}, {act}): max|out - ref64| = {err.max().item():.3e}, max|ref| = {ref.abs().max().item():.2f}; {_where(err)}")
    assert err.max().item() < TOL_BLOCK, _where(err)


# hw = 144 is no multiple of 32; hw = 96 is below 128; C = 64 has no instance
UNFUSED = [(2, 9, 16, 96, "mish"), (2, 8, 12, 96, "mish"), (1, 8, 20, 64, "mish")]


@pytest.mark.parametrize("n,h,w,c,act", UNFUSED)
def test_dispatch_boundary_stays_unfused(tmp_path, n, h, w, c, act):
    """just outside mlp_fused_supported the block runs as separate launches (no sp == 2 record) and is as accurate.
    Measured max |out - ref64| on MI355X, in the order of UNFUSED: 2.16e-6, 1.82e-6, 1.05e-6."""
    nv = _lib()
    nv.set_gemm_precision("f16x3")
    p, x, ref, _ = _case(n, h, w, c, act)
    out, rows = _run_block(tmp_path, p, x, act)
    assert len(rows) >= 2 and _fused_shapes(rows) == [], rows
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs()
    print(f"unfused ({n}, {h}, {w}, {c}, {act}): max|out - ref64| = {err.max().item():.3e}; {_where(err)}")
    assert err.max().item() < TOL_BLOCK, _where(err)


def test_f32_mode_stays_unfused_on_the_same_inputs(tmp_path):
    """(3, 8, 20, 96, mish) in the f32 operand mode: no fused launch, and an independent measurement on the very inputs of
    the fused case.  Measured max |out - ref64| on MI355X: f32 unfused 2.86e-6, f16x3 fused 1.97e-6."""
    nv = _lib()
    n, h, w, c, act = 3, 8, 20, 96, "mish"
    p, x, ref, _ = _case(n, h, w, c, act)
    nv.set_gemm_precision("f32")
    out32, rows32 = _run_block(tmp_path, p, x, act)
    nv.set_gemm_precision("f16x3")
    out16, rows16 = _run_block(tmp_path, p, x, act)
    e32 = (out32.double() - ref).abs().max().item()
    e16 = (out16.double() - ref).abs().max().item()
    print(f"(3, 8, 20, 96, mish): f32 unfused max|out - ref64| = {e32:.3e}, f16x3 fused = {e16:.3e}")
    assert len(rows32) >= 2 and _fused_shapes(rows32) == [], rows32
    assert len(_fused_shapes(rows16)) == 2, rows16
    assert torch.isfinite(out32).all() and e32 < TOL_BLOCK
    assert torch.isfinite(out16).all() and e16 < TOL_BLOCK


@pytest.mark.parametrize("n,h,w,c,act", [(3, 8, 20, 96, "mish"), (2, 8, 28, 80, "gelu")])
def test_batch_and_tile_invariance(tmp_path, n, h, w, c, act):
    """"results do not depend on the batch or the tile" (mlp_fused_kernel.h): image i of a batch equals, bit for bit, the
    same image run alone with the same weights.  In the batch image 1 starts at wave 1 (hw = 160) or wave 3 (hw = 224) of
    a tile and reads the second staged row of GRN multipliers; alone it starts at row 0 of tile 0 and reads the first."""
    nv = _lib()
    nv.set_gemm_precision("f16x3")
    p, x, ref, _ = _case(n, h, w, c, act)
    out, rows = _run_block(tmp_path, p, x, act)
    assert len(_fused_shapes(rows)) == 2, rows
    assert (out.double() - ref).abs().max().item() < TOL_BLOCK
    for i in range(n):
        solo, rows = _run_block(tmp_path, p, x[i : i + 1], act)
        assert _fused_shapes(rows) == [(h * w, 4 * c, c), (h * w, c, 4 * c)], rows
        same = torch.equal(out[i].view(torch.int32), solo[0].view(torch.int32))
        assert same, f"image {i}: {(out[i] != solo[0]).sum().item()} values differ, max {(out[i] - solo[0]).abs().max().item():.3e}"


# ---------------------------------------------------------------------------
# the LayerNorm epilogue (last block of stage 0, reachable from the encoder only) on ragged tiles
# ---------------------------------------------------------------------------
# (kind, image (H, W), dims[0], z, n): stage-0 hw, M, tiles of 128 rows
ENCODERS = [
    ("ae", (96, 96), 96, 36, 3),  # hw 576, M 1728: 13.5 tiles, image boundaries inside tiles
    ("ae", (32, 96), 80, 12, 1),  # hw 192, M 192: 1.5 tiles
    ("plain", (32, 160), 96, 20, 2),  # hw 320, M 640: 5 tiles, boundary at 2.5
    ("plain", (96, 96), 80, 20, 3),  # hw 576, M 1728: 13.5 tiles
]


@pytest.mark.parametrize("kind,hw,c0,z,n", ENCODERS)
def test_layernorm_epilogue_on_ragged_tiles(tmp_path, monkeypatch, kind, hw, c0, z, n):
    """Small encoders whose stage 0 (two blocks, C = 96 / 80) runs on the fused kernel with a last tile of 64 rows - the only
    ragged tail a stage 0 can have (its hw is a multiple of 64); the second block normalises its rows for the downsample
    in its epilogue (MTGV_LN_FUSE, default on) and overwrites its residual with them in SP8 form.
    Both forms are within 1e-4 of the fp64 embedding and within 1e-5 of each other; they sum a row in different orders,
    so bit-equal embeddings would mean the epilogue never ran - and a forward with stage capture, which switches the
    epilogue off, must give the bits of MTGV_LN_FUSE=0.  The captured stages are within 1e-4 of the fp64 stages.
    Measured on MI355X, in the order of ENCODERS (max |z64| 2.1 to 2.8): max|z1 - z64|, max|z0 - z64|, max|z1 - z0|; largest stage error
    2.76e-6, 2.52e-6, 1.43e-6; 2.21e-6 (stage 0)
    7.33e-7, 3.23e-7, 4.77e-7; 1.57e-6 (stage 0)
    8.45e-7, 7.26e-7, 7.15e-7; 3.06e-6 (stage 2)
    8.44e-7, 7.24e-7, 8.94e-7; 2.29e-6 (stage 0)
    The 1-row-high deep stages of the 32-pixel-high configurations trip nothing."""
    from mtgv import native, spec
    from mtgv.encoder import Encoder
    from oracle import encoder_ref as R

    try:
        native.set_gemm_precision("f16x3")
    except (AssertionError, RuntimeError):
        pass
    if native.get_gemm_precision() != "f16x3":
        pytest.skip("the fused MLP kernel belongs to the f16x3 operand mode, which this library cannot be set to")
    cfg = spec.EncoderConfig(kind, hw, 3, z, (2, 1, 1, 1), (c0, 16, 16, 16), "conv+linear" if kind == "ae" else "plain", kind == "ae")
    sd = spec.random_encoder_state(cfg, 1)
    x = np.random.default_rng(0).random((n, 3, *hw)).astype(np.float32)
    z64, stages64 = R.encoder_forward(sd, cfg, torch.from_numpy(x).double(), dtype=torch.float64, return_stages=True)
    z64 = z64.numpy()
    enc = Encoder(cfg, sd, max_batch=n)
    X = torch.from_numpy(x)
    L = native.lib()

    monkeypatch.setenv("MTGV_LN_FUSE", "1")
    csv = str(tmp_path / "gemm.csv")
    native.check(L.mtgv_profile_gemm(1))
    try:
        z1 = enc.encode(X).cpu().numpy()
        native.check(L.mtgv_profile_gemm_dump(csv.encode()))
    finally:
        native.check(L.mtgv_profile_gemm(0))
    m = n * (hw[0] // 4) * (hw[1] // 4)
    assert _fused_shapes(_records(csv)) == [(m, 4 * c0, c0), (m, c0, 4 * c0)] * 2  # both blocks of stage 0, nothing else
    np.testing.assert_array_equal(z1, enc.encode(X).cpu().numpy())  # the profiler changes no value

    monkeypatch.setenv("MTGV_LN_FUSE", "0")
    z0 = enc.encode(X).cpu().numpy()
    monkeypatch.setenv("MTGV_LN_FUSE", "1")
    enc.set_capture(True)
    zc = enc.encode(X).cpu().numpy()
    errs = []
    for s in range(4):
        got = enc.stage_output(s, n).cpu().double().permute(0, 3, 1, 2)
        errs.append((got - stages64[s]).abs().max().item())
    enc.set_capture(False)

    e1, e0, e10 = np.abs(z1 - z64).max(), np.abs(z0 - z64).max(), np.abs(z1 - z0).max()
    print(f"{kind} {hw} C={c0} n={n}: max|z1 - z64| = {e1:.3e}, max|z0 - z64| = {e0:.3e}, max|z1 - z0| = {e10:.3e}, "
          f"max|z64| = {np.abs(z64).max():.2f}, stages " + " ".join(f"{e:.3e}" for e in errs))
    assert np.isfinite(z1).all() and e1 < TOL
    assert np.isfinite(z0).all() and e0 < TOL
    assert e10 < 1e-5
    assert not np.array_equal(z1, z0), "bit-equal embeddings: the LayerNorm epilogue was not taken"
    assert np.array_equal(zc, z0), "stage capture switches the epilogue off: the bits of MTGV_LN_FUSE=0"
    for s in range(4):
        assert errs[s] < TOL, f"stage {s}: {errs[s]}"
