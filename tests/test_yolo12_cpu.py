"""CPU-only: YOLO12 (spec arch "12": A2C2f, ABlock, area attention) in the spec, the export mirror and the reference
tests/yolo12_ref.py.  The GPU side is tests/test_gpu_yolo12.py and tests/test_gpu_area_attn.py; the cases are
tests/yolo12_common.py's."""
import hashlib

import numpy as np
import pytest
import torch

import yolo12_common as Y
import yolo12_ref as R

SCALES, TASKS = "nsmlx", ("seg", "obb")

# state_dict keys and elements (BatchNorm running statistics included) at nc = 3, from the shapes of the recalled definition
COUNTS = {
    ("n", "seg"): (631, 2_844_745), ("n", "obb"): (614, 2_663_132),
    ("s", "seg"): (631, 9_954_265), ("s", "obb"): (614, 9_585_372),
    ("m", "seg"): (681, 22_513_017), ("m", "obb"): (664, 21_054_556),
}


@pytest.mark.parametrize("scale,task", list(COUNTS))
def test_key_and_element_counts(scale, task):
    from mtgv import spec

    shapes = spec.detector_param_shapes(spec.detector_scale_config("12", scale, task=task))
    assert (len(shapes), sum(int(np.prod(v)) for v in shapes.values())) == COUNTS[(scale, task)]


@pytest.mark.parametrize("scale", SCALES)
def test_scale_config_is_yolo12(scale):
    from mtgv import spec

    for name in ("12", "v12", 12):
        cfg = spec.detector_scale_config(name, scale)
        assert cfg.arch == "12" and cfg.head_index == 21 and cfg.scale == scale
        assert (cfg.depth, cfg.width, cfg.max_ch) == spec.DETECTOR_SCALES["11"][scale]
    graph, feats = spec.detector_graph(cfg)
    assert feats == (14, 17, 20) and len(graph) == 21
    assert not any(kind in ("SPPF", "C2PSA", "C2f") for _, kind, _ in graph)
    a2 = {i: a for i, kind, a in graph if kind == "A2C2f"}
    assert sorted(a2) == [6, 8, 11, 14, 17]
    assert [a2[i][2] for i in sorted(a2)] == [True, True, False, False, False] and (a2[6][3], a2[8][3]) == (4, 1)
    big = scale in "lx"
    assert a2[6][1] == (4 if big else 2) and a2[6][4] == big and a2[6][5] == (1.2 if big else 2.0)
    assert all(a[2] == (scale in "mlx") for i, kind, a in graph if kind == "C3k2" and i != 20)


def test_widths_at_n():
    from mtgv import spec

    s = spec.detector_param_shapes(spec.detector_scale_config("12", "n"))
    assert s["model.6.m.0.0.attn.qkv.conv.weight"] == (192, 64, 1, 1) and s["model.6.m.1.1.mlp.0.conv.weight"] == (128, 64, 1, 1)
    assert s["model.8.m.1.1.attn.pe.conv.weight"] == (128, 1, 7, 7) and s["model.8.m.0.0.mlp.1.conv.weight"] == (128, 256, 1, 1)
    assert s["model.11.m.0.cv3.conv.weight"] == (64, 64, 1, 1) and s["model.11.cv2.conv.weight"] == (128, 128, 1, 1)
    assert "model.6.gamma" not in s
    assert spec.detector_param_shapes(spec.detector_scale_config("12", "l"))["model.6.gamma"] == (512,)


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("scale", SCALES)
def test_config_for_state_finds_yolo12(scale, task):
    """a head at model.21 with no model.22 / model.23 keys is YOLO12; m and l share the stem width and differ by model.2.m.1"""
    from mtgv import spec

    cfg = spec.detector_scale_config("12", scale, task=task, input_hw=(64, 96), nc=2)
    sd = spec.random_detector_state(cfg, Y.WEIGHT_SEED)
    got = spec.detector_config_for_state(sd, input_hw=(64, 96))
    assert (got.arch, got.scale, got.task, got.nc) == ("12", scale, task, 2)
    assert got == cfg


# sha256 over the float32 bytes of every array of random_detector_state(detector_scale_config(arch, scale), 4), in key order,
# arch v8 then 11, scales n, s, m - computed with the spec of the commit before YOLO12 was added
PARENT_STATES_SHA256 = "39a812d2e8fda1acc3b008fc434d990bce66bb26e03db1b8ede29281a8456a70"


def test_other_families_states_are_unchanged():
    from mtgv import spec

    h = hashlib.sha256()
    for arch in ("v8", "11"):
        for scale in "nsm":
            for v in spec.random_detector_state(spec.detector_scale_config(arch, scale), 4).values():
                h.update(v.tobytes())
    assert h.hexdigest() == PARENT_STATES_SHA256


def test_ablock_gains():
    """the non-activated convs of an ABlock are drawn smaller (std gain / sqrt(fan_in)); everything else keeps 1.6"""
    from mtgv import spec

    sd = spec.random_detector_state(spec.detector_scale_config("12", "s"), Y.WEIGHT_SEED)
    for frag, gain in ((".attn.qkv.", 1.0), (".attn.pe.", 1.0), (".attn.proj.", 0.5), (".mlp.1.", 0.5), (".mlp.0.", 1.6), (".cv2.conv", 1.6)):
        ws = [v for k, v in sd.items() if frag in k and k.endswith("conv.weight") and k.startswith("model.6.")]
        assert ws
        for w in ws:
            assert abs(w.std() * np.sqrt(np.prod(w.shape[1:])) / gain - 1) < 0.1, frag


@pytest.mark.parametrize("task", TASKS)
def test_export_module_equals_the_reference(task):
    """strict load of the random state; float32 output within 1e-5 of yolo12_ref.forward(float32) at 64 x 96"""
    from mtgv.export_detector import DetectorModule

    cfg, sd, frames = Y.inputs("n", task, Y.SMALL_HW, Y.SMALL_N)
    m = DetectorModule(cfg).eval()
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    full.update({k: v for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")})
    m.load_state_dict(full, strict=True)
    with torch.no_grad():
        out = m(R.D.preprocess(frames))
    ref = R.forward(sd, cfg, frames, dtype=torch.float32)
    out, ref = (out, ref) if task == "seg" else ((out,), (ref,))
    for a, b in zip(out, ref):
        err = float((a - b).abs().max())
        print(f"export {task}: {tuple(a.shape)} err {err:.2e}")
        assert a.shape == b.shape and err < 1e-5


def test_other_families_exports_keep_the_conv_dfl():
    """only YOLO12's Segment head writes the DFL as the reference's expectation sum; YOLOv8 / YOLO11 (and every OBB head) keep
    the 1x1 conv, so their export mirrors compute what they computed before YOLO12 was added"""
    from mtgv import spec
    from mtgv.export_detector import DetectorModule

    for arch in ("v8", "11", "12"):
        for task in TASKS:
            with torch.device("meta"):
                head = DetectorModule(spec.detector_scale_config(arch, "n", task=task, input_hw=(64, 96))).model[-1]
            assert head.dfl.as_sum == (arch == "12" and task == "seg"), (arch, task)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((2, 64, 50))).float()
    from mtgv.export_detector import _DFL

    conv, as_sum = _DFL(16), _DFL(16, as_sum=True)
    for m in (conv, as_sum):
        m.conv.weight.data[:] = torch.arange(16.0).view(1, 16, 1, 1)
    want = conv.conv(x.view(2, 4, 16, 50).transpose(2, 1).softmax(1)).view(2, 4, 50)
    assert torch.equal(conv(x), want) and float((as_sum(x) - want).abs().max()) < 1e-5


@pytest.mark.parametrize("scale,task", list(COUNTS) + [("l", "seg"), ("x", "obb")])
def test_export_module_keys(scale, task):
    from mtgv import spec
    from mtgv.export_detector import DetectorModule

    cfg = spec.detector_scale_config("12", scale, task=task, input_hw=(64, 96))
    want = spec.detector_param_shapes(cfg)
    with torch.device("meta"):
        module = DetectorModule(cfg)
    got = {k: tuple(v.shape) for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert list(got) == list(want) and got == {k: tuple(v) for k, v in want.items()}


def test_reference_runs_l_with_gamma():
    """scale l (residual gamma, MLP ratio 1.2, four modules per attention block) through reference and export mirror"""
    from mtgv import spec
    from mtgv.export_detector import to_torch_module

    cfg = spec.detector_scale_config("12", "l", input_hw=(32, 32))
    sd = spec.random_detector_state(cfg, Y.WEIGHT_SEED)
    frames = np.random.default_rng(5).integers(0, 256, (1, 32, 32, 3), dtype=np.uint8)
    pred, protos = R.forward(sd, cfg, frames)
    with torch.no_grad():
        p2, q2 = to_torch_module(cfg, sd)(R.D.preprocess(frames))
    assert torch.isfinite(pred).all() and float((pred - p2).abs().max()) < 1e-4 and float((protos - q2).abs().max()) < 1e-4


@pytest.mark.parametrize("area", [4, 1])
def test_area_semantics_of_the_reference(area):
    """changing one token's q / k / v in area 0 changes area 0's attention output (before pe) and, with area 4, leaves every
    token of areas 1..3 bit-identical; with area 1 it changes every token's.  6 x 10: areas of 15 tokens, 1.5 rows each."""
    h, w, heads = 6, 10, 2
    qkv = torch.from_numpy(np.random.default_rng(7).standard_normal((1, heads * 96, h, w))).float()
    y0, _ = R.area_attention(qkv, heads, area)
    q2 = qkv.clone()
    q2[0, :, 0, 3] += 1.0  # token 3
    y1, _ = R.area_attention(q2, heads, area)
    changed = (y0 != y1).flatten(2).any(1)[0]  # per token
    na = h * w // area
    assert changed[:na].all()
    if area > 1:
        assert not changed[na:].any()
    else:
        assert changed.all()


def test_area_attention_equals_per_chunk_softmax():
    """the reshapes of area_attention against a loop over images, areas and heads"""
    h, w, heads, area = 4, 6, 2, 4
    qkv = torch.from_numpy(np.random.default_rng(8).standard_normal((2, heads * 96, h, w)))
    y, v = R.area_attention(qkv, heads, area)
    t = qkv.flatten(2).transpose(1, 2)  # (B, N, 3c)
    na = h * w // area
    for b in range(2):
        for a in range(area):
            for hd in range(heads):
                blk = t[b, a * na : (a + 1) * na, hd * 96 : (hd + 1) * 96]
                q, k, vv = blk[:, :32], blk[:, 32:64], blk[:, 64:]
                want = ((q @ k.T) * 32**-0.5).softmax(-1) @ vv
                got = y.flatten(2).transpose(1, 2)[b, a * na : (a + 1) * na, hd * 32 : (hd + 1) * 32]
                assert float((want - got).abs().max()) < 1e-12
                assert torch.equal(v.flatten(2).transpose(1, 2)[b, a * na : (a + 1) * na, hd * 32 : (hd + 1) * 32], vv)


@pytest.mark.parametrize("case", Y.ALL_CASES, ids=Y.case_id)
def test_reference_float32_is_well_inside_the_gpu_tolerance(case):
    """the float32 reference within a third of what tests/test_gpu_yolo12.py allows the GPU against the float64 reference
    (1e-4; boxes max(in_h, in_w) * 1e-4 px).  Measured: at most 4.3e-6, and 1.2e-4 px on boxes (640 x 640)."""
    cfg = Y.inputs(*case)[0]
    _, p64, q64 = Y.reference(*case)
    _, p32, q32 = Y.reference(*case, f32=True)
    nc = cfg.nc

    def err(a, b):
        return float(np.abs(a.astype(np.float64) - b).max())

    box, cls, rest = err(p32[:, :4], p64[:, :4]), err(p32[:, 4 : 4 + nc], p64[:, 4 : 4 + nc]), err(p32[:, 4 + nc :], p64[:, 4 + nc :])
    protos = 0.0 if q64 is None else err(q32, q64)
    print(f"{Y.case_id(case)}: box {box:.2e}px cls {cls:.2e} coef/angle {rest:.2e} protos {protos:.2e}")
    assert cls < 1e-4 / 3 and rest < 1e-4 / 3 and protos < 1e-4 / 3
    assert box < max(cfg.in_h, cfg.in_w) * 1e-4 / 3


@pytest.mark.parametrize("key", list(Y.E2E_CASES), ids=lambda k: f"12{k[0]}-{k[1]}")
def test_end_to_end_cases_are_decided(key):
    """what yolo12_common.E2E_CASES was chosen for"""
    case = (*key, Y.SMALL_HW, Y.SMALL_N)
    kw = Y.E2E_CASES[key]
    cfg = Y.inputs(*case, **kw)[0]
    d64, p64, _ = Y.reference(*case, **kw)
    d32, _, _ = Y.reference(*case, **kw, f32=True)
    for a, b in zip(d32, d64):
        assert 10 < len(b["keep_idx"]) < cfg.max_det
        np.testing.assert_array_equal(a["keep_idx"], b["keep_idx"])
    assert np.abs(p64[:, 4 : 4 + cfg.nc] - cfg.conf).min() > 1e-2


def test_flops_count_of_the_reference():
    """the independent count at 640 x 640, nc = 3, beside ultralytics' published figure for yolo12n-seg at 80 classes [recalled]"""
    from mtgv import spec

    n = R.flops_per_frame(spec.detector_scale_config("12", "n"))
    print(f"yolo12n-seg, nc = 3: {n / 1e9:.2f} GFLOP per 640 x 640 frame (published, 80 classes, recalled: 9.9)")
    att = sum(2.0 * (c // 32) * px * (px // area) * 64 * 4 for c, px, area in ((64, 1600, 4), (128, 400, 1)))
    assert abs(att - 0.98e9) < 0.01e9  # 8 blocks: 4 at P4 (4 areas x 2 heads), 4 at P5 (4 heads), each 400^2 x 64 x 2
