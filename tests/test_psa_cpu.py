"""CPU-only companion of test_gpu_psa_direct.py (cases, draws, references: psa_common.py).
  - The cases can tell the likely mistakes of an online-softmax attention kernel and of a depthwise 3x3 with a channel
    gather apart, shown on the fp64 references alone: for every case each mistake that can show there moves the
    reference by at least 100 x the bound the GPU test holds the kernel to on that case (4 x the float32 torch error).
    Every mistake applies to at least one case.
  - The fp64 attention reference is oracle/detector_ref._attention's own code fed the same q, k and v (its two 1x1 convs
    replaced by the identity, its depthwise conv and BatchNorm given the folded pe taps), to 1e-12: the operation the
    detector is held to, not a second opinion of it.
  - The draws: logits of the size the table claims, the ramp moving the maximum to the late keys, scaled borders.
  - The ctypes descriptor matches the header's struct; bad arguments are status 1 with a message naming the op from both
    entry points without a GPU, every refusal of psa_common's tables included; a valid call reports the HIP failure
    (status 3) where there is no device, never a result."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import psa_common as pc
from conftest import ROOT

FACTOR = 100.0
EPS = 1e-3


# ---- attention ----
@pytest.mark.parametrize("kind", pc.ATTN_DRAWS)
@pytest.mark.parametrize("case", pc.ATTN_CASES, ids=pc.attn_id)
def test_attention_cases_separate_the_mutations(case, kind):
    d = pc.attn_draw(case, kind)
    ref, bound, err32 = pc.attn_expected(case, kind, False)  # the mistakes are the attention's: the bound of the attention-only call
    assert np.isfinite(ref).all() and ref.shape == (case[0], case[1] * case[2], case[3] * pc.HD) and bound > 0
    for m in pc.ATTN_MUTATIONS:
        if not pc.attn_applies(m, case):
            continue
        diff = float(np.abs(pc.attn_reference(case, d, False, m) - ref).max())
        print(f"psa_attn {pc.attn_id(case)} {kind} {m}: max |mutated - reference| = {diff:.3g} = {diff / bound:.0f} x bound {bound:.3g}")
        assert diff >= FACTOR * bound, (case, kind, m, diff, bound)


def test_every_attention_mutation_is_exercised():
    for m in pc.ATTN_MUTATIONS:
        assert sum(pc.attn_applies(m, c) for c in pc.ATTN_CASES) >= 4, m
    # the edges the table names
    N = [c[1] * c[2] for c in pc.ATTN_CASES]
    assert N == [6, 16, 21, 256, 257, 300, 400]
    assert {c[3] for c in pc.ATTN_CASES} == {1, 2, 4} and {c[0] for c in pc.ATTN_CASES} == {1, 2, 3}


def test_attention_draws():
    case = (2, 15, 20, 2)
    flat, ramp = pc.attn_draw(case, "flat"), pc.attn_draw(case, "ramp")
    assert 15.0 < pc.max_logit(case, "flat") < 25.0 and 15.0 < pc.max_logit(case, "ramp") < 30.0
    q = flat.qkv.reshape(2, 300, 2, 128)
    assert 1.7 < q[..., :64].std() < 1.9 and 0.95 < q[..., 64:].std() < 1.05
    assert np.array_equal(flat.qkv.reshape(2, 300, 2, 128)[..., 64:], ramp.qkv.reshape(2, 300, 2, 128)[..., 64:])
    # ramp: the key with the largest logit sits in the last quarter for most queries, in the first for almost none
    t = torch.tensor(ramp.qkv).double().view(2, 300, 2, 128).permute(0, 2, 1, 3)
    best = (t[..., :32] @ t[..., 32:64].transpose(-1, -2)).argmax(-1)
    assert (best >= 225).double().mean() > 0.5 and (best < 75).double().mean() < 0.05
    for a in (*flat, pc.attn_expected(case, "flat", True)[0]):
        assert not a.flags.writeable


def test_reference_is_the_oracles_attention(monkeypatch):
    from oracle import detector_ref as R

    case, kind = (3, 3, 7, 1), "ramp"
    n, h, w, heads = case
    d = pc.attn_draw(case, kind)
    c = heads * pc.HD
    qkv_map = torch.tensor(d.qkv).double().transpose(1, 2).reshape(n, heads * 128, h, w)
    monkeypatch.setattr(R, "_conv", lambda x, p, prefix, k, s=1, eps=1e-3, act=True: qkv_map if prefix.endswith(".qkv") else x)
    p = {
        "a.pe.conv.weight": torch.tensor(d.pe_w9).double().T.reshape(c, 1, 3, 3),
        "a.pe.bn.running_mean": torch.zeros(c, dtype=torch.float64),
        "a.pe.bn.running_var": torch.full((c,), 1.0 - EPS, dtype=torch.float64),  # BatchNorm as the identity + bias
        "a.pe.bn.weight": torch.ones(c, dtype=torch.float64),
        "a.pe.bn.bias": torch.tensor(d.pe_bias).double(),
    }
    y = R._attention(torch.zeros(n, c, h, w, dtype=torch.float64), p, "a", heads, EPS)
    got = y.flatten(2).transpose(1, 2).numpy()
    assert np.abs(got - pc.attn_expected(case, kind, True)[0]).max() < 1e-12
    p["a.pe.conv.weight"] = torch.zeros_like(p["a.pe.conv.weight"])
    p["a.pe.bn.bias"] = torch.zeros(c, dtype=torch.float64)
    y = R._attention(torch.zeros(n, c, h, w, dtype=torch.float64), p, "a", heads, EPS)
    assert np.abs(y.flatten(2).transpose(1, 2).numpy() - pc.attn_expected(case, kind, False)[0]).max() < 1e-12


# ---- depthwise 3x3 ----
@pytest.mark.parametrize("index", range(len(pc.DW_CASES)), ids=[pc.dw_id(c) for c in pc.DW_CASES])
def test_dwconv3_cases_separate_the_mutations(index):
    case = pc.DW_CASES[index]
    d = pc.dw_draw(index)
    ref, bound, err32 = pc.dw_expected(index)
    assert np.isfinite(ref).all() and ref.shape == (case.n, case.h, case.w, case.c) and bound > 0
    for m in pc.DW_MUTATIONS:
        if not pc.dw_applies(m, case):
            continue
        diff = np.abs(pc.dw_reference(case, d, mutation=m) - ref)
        print(f"dwconv3 {pc.dw_id(case)} {m}: max |mutated - reference| = {diff.max():.3g} = {diff.max() / bound:.0f} x bound {bound:.3g}")
        assert diff.max() >= FACTOR * bound, (index, m, float(diff.max()), bound)
        if m in ("hpad_adjacent_row", "vpad_neighbour_image") and min(case.h, case.w) > 2:  # these show at a border only
            inner = diff[:, 1:-1] if m == "vpad_neighbour_image" else diff[:, :, 1:-1]
            assert inner.max() < 1e-9, (index, m)


def test_every_dwconv3_mutation_is_exercised():
    for m in pc.DW_MUTATIONS:
        assert sum(pc.dw_applies(m, c) for c in pc.DW_CASES) >= 1, m
    pe, cls, both = pc.DW_CASES[5], pc.DW_CASES[6], pc.DW_CASES[7]
    # the positional-encoding form reads the v rows of a two-head qkv pixel
    assert list(pc.cin(pe)) == list(range(64, 128)) + list(range(192, 256)) and pe.add and pe.act == pc.NONE
    assert list(pc.cin(cls)) == list(range(8, 48)) and cls.act == pc.SILU and not cls.add and (pc.out_ct_of(cls), cls.out_co) == (64, 16)
    assert list(pc.cin(both)) == list(range(16)) + list(range(48, 64)) and both.add and both.act == pc.SILU
    assert -(-(2 * 7 * 9 * 72 // 8) // 256) == 5 and (2 * 7 * 9 * 72 // 8) % 256 != 0  # five blocks, the last ragged
    for c in pc.DW_CASES + [pc.DW_CASE_QUADS]:
        assert pc.cin(c).max() < pc.x_ct_of(c) and c.out_co + c.c <= pc.out_ct_of(c), c


def test_dwconv3_draw():
    d = pc.dw_draw(4)
    x = d.full
    border = np.concatenate([x[:, 0].ravel(), x[:, -1].ravel(), x[:, :, 0].ravel(), x[:, :, -1].ravel()])
    assert 7.0 < border.std() < 9.0 and 0.9 < x[:, 1:-1, 1:-1].std() < 1.1 and 0.28 < d.w9.std() < 0.39
    assert not x.flags.writeable and pc.dw_draw(4) is d


# ---- the entry points without a GPU ----
def test_descriptor_matches_header():
    from mtgv import native

    src = open(os.path.join(ROOT, "include", "mtgv.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mtgv_dwconv3;", src).group(1)
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
    assert [(n, t) for n, t in native.Dwconv3._fields_] == list(zip(names, kinds))
    assert names == "x n h w x_ct x_co x_fmt c g_size g_stride w9 bias act add add_ld out out_ct out_co out_fmt".split()
    assert native.lib().mtgv_version() >= 114


class _Host:
    """host memory standing in for device tensors: 16-byte aligned addresses, never read by a refused call"""

    def __init__(self, names):
        self.buf = np.zeros(16 * (len(names) + 1), np.float32)
        a0 = -(-self.buf.ctypes.data // 16) * 16
        self.ptr = {k: a0 + 64 * i for i, k in enumerate(names)}


def psa_call(L, a, stream=None):
    return L.mtgv_op_psa_attn(a["qkv"], a["pe_w9"], a["pe_bias"], a["n"], a["h"], a["w"], a["heads"], a["out"], stream)


def dw_call(L, a, stream=None):
    from mtgv import native

    d = native.Dwconv3()
    for k, _ in native.Dwconv3._fields_:
        setattr(d, k, a[k])
    return L.mtgv_op_dwconv3(C.byref(d), stream)


def test_status_convention_without_gpu():
    from mtgv import native

    L = native.lib()
    host = _Host(("qkv", "pe_w9", "pe_bias", "out"))
    for what, change in pc.ATTN_REFUSALS:
        rc = psa_call(L, pc.refusal_args(pc.ATTN_REFUSAL_BASE, change, host.ptr))
        assert rc == 1 and b"psa_attn" in L.mtgv_last_error(), (what, rc, L.mtgv_last_error())
    host = _Host(("x", "w9", "bias", "add", "out"))
    assert L.mtgv_op_dwconv3(None, None) == 1 and b"dwconv3" in L.mtgv_last_error()
    for what, change in pc.DW_REFUSALS:
        rc = dw_call(L, pc.refusal_args(pc.DW_REFUSAL_BASE, change, host.ptr))
        assert rc == 1 and b"dwconv3" in L.mtgv_last_error(), (what, rc, L.mtgv_last_error())
    if L.mtgv_device_count() == 0:  # a valid call: the launch itself fails, and says so
        rc = psa_call(L, {**pc.ATTN_REFUSAL_BASE, **host.ptr, "qkv": host.ptr["x"], "pe_w9": None, "pe_bias": None})
        assert rc == 3 and b"hip" in L.mtgv_last_error().lower(), (rc, L.mtgv_last_error())
        rc = dw_call(L, {**pc.DW_REFUSAL_BASE, **host.ptr})
        assert rc == 3 and b"hip" in L.mtgv_last_error().lower(), (rc, L.mtgv_last_error())
