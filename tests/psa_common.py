"""Shared by test_psa_cpu.py and test_gpu_psa_direct.py: the cases of the direct tests of YOLO11's two own kernels
(detector_v11.hip) - attn_kernel<32, 64, 16>, the C2PSA attention core (mtgv_op_psa_attn), and dwconv3_kernel<IN_SP8, OUT_SP8>,
the depthwise 3x3 (mtgv_op_dwconv3) - with their seeded draws and the fp64 references of the two operations, the mistakes
such kernels are likely to make as switches of those references.  No GPU needed here.

Attention.  qkv (n, N = h w, heads * 128) f32, per head [q 32 | k 32 | v 64]:
  out[b, i, head * 64 + d] = sum_j softmax_j(q_i . k_j / sqrt(32)) v_j[d]          per image b and head
  (+ the depthwise 3x3 of the v channels over the h x w map, taps pe_w9 [9][heads * 64], bias pe_bias)
Draws: qkv N(0, 1) with the q and k channels times QK_SCALE = 1.8 (test_gpu_area_attn.py's: logits up to about 19, a
softmax with a few keys carrying the weight) - "flat" - and the same with key row j times 0.3 + 1.2 j / (N - 1) - "ramp":
the largest logit then sits in a late 16-key chunk for most queries, so the running maximum of an online softmax rises
chunk after chunk and its rescale runs every time.  pe taps N(0, 1) / 3, pe bias 0.1 N(0, 1).

Depthwise 3x3, stride 1, zero padding 1:
  out[.., k] = act(bias[k] + sum_taps w9[tap][k] x[.., cin(k)]) (+ add[.., k]),   cin(k) = x_co + (k / g_size) g_stride + k % g_size
Draw (dwconv_ln_common's): the whole input pixel N(0, 1) with the outermost row and column of every image times 8 - a halo
read without its mask lands on a large value - taps N(0, 1) / 3, bias N(0, 1), addend N(0, 1).  The channels of the pixel
the kernel must not read are drawn too: the mistaken gathers read them (the GPU test puts NaNs there).

The bound of either test is the project's rule (test_gpu_area_attn.py): four times the largest error of the same
expression evaluated by torch in float32 on the CPU on the same inputs, both errors against the fp64 reference - never a
figure taken from the kernel.  attn_expected() / dw_expected() compute it per case.

Separation, max |mistaken reference - reference| / bound, the smallest over the cases (and draws) a mistake applies to
(test_psa_cpu.py requires 100 on every case; `pytest -s` prints every figure):
  attention                          at                     depthwise 3x3                      at
  qk_swapped             196649   N = 400 ramp              taps_transposed        2103519   (2, 5, 7, 40) SiLU
  scale_dropped          108983   N = 400 ramp              kernel_flipped         2594008   (2, 5, 7, 40) SiLU
  scale_hd                54051   N = 400 ramp              hpad_adjacent_row      1419211   (2, 6, 5, 128) pe form
  pad_zero                  142   N = 300 flat              vpad_neighbour_image   1626306   (2, 6, 5, 128) pe form
  no_rescale             151271   N = 400 ramp              bias_dropped            201486   (2, 6, 5, 128) pe form
  softmax_over_queries   171205   N = 400 ramp              gather_ignored         3055907   (2, 5, 7, 40) SiLU
  cross_image            287519   N = 300 ramp              stride_as_size         2247202   (2, 6, 5, 128) pe form
  head_mix               237128   N = 400 ramp              add_dropped             268585   (2, 6, 5, 128) pe form
  v_is_k                 411075   N = 400 ramp              act_after_add           324902   (2, 3, 4, 32) SiLU + add
                                                            act_dropped            2624463   (2, 5, 7, 40) SiLU
The 3x3 draw needed no change.  pad_zero is the one mistake near the limit, and only at N = 300 (422 at N = 257, 4e4 and
more at N = 6 and 21): four padding keys of score 0 beside 300 keys whose best logit is about 9 for the least peaked
query move that query's output by 2e-3.  How far depends on the least peaked query of the draw: over the seeds
11400 .. 11463 the figure is 52 .. 142, median 94, past 100 on 28 of the 64.  ATTN_SEED is the one with the most room, so
that the float32 torch error of another CPU does not decide the CPU test; every other attention mistake is past 2e4 on
each of the first eight of those seeds."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

KD, HD = 32, 64          # key and value width of a head: attn_kernel<32, 64, 16>
KC = 16                  # keys per LDS chunk
QK_SCALE = 1.8
NONE, SILU = 0, 3        # common.h: Act
ATTN_SEED = 11439       # (why this one: the docstring's last paragraph)


def _t(a, dtype):
    """a (read-only) numpy array as a torch tensor of `dtype`: a copy"""
    return torch.tensor(np.asarray(a)).to(dtype)

# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
# (n, h, w, heads): the smallest shapes that reach each edge of the kernel
ATTN_CASES = [
    (1, 2, 3, 2),     # N = 6: one ragged key chunk
    (2, 4, 4, 2),     # N = 16: exactly one chunk
    (3, 3, 7, 1),     # N = 21: one head, three images, ragged second chunk
    (2, 16, 16, 2),   # N = 256: exactly one query tile
    (1, 1, 257, 2),   # N = 257: one live thread in the second query tile, ragged last chunk; H = 1 for the positional encoding
    (2, 15, 20, 2),   # N = 300: the 480 x 640 map; two query tiles, last chunk 12 keys
    (1, 20, 20, 4),   # N = 400: the 640 x 640 map at scales s and m
]
ATTN_DRAWS = ("flat", "ramp")
ATTN_MUTATIONS = ("qk_swapped", "scale_dropped", "scale_hd", "pad_zero", "no_rescale", "softmax_over_queries", "cross_image", "head_mix",
                  "v_is_k")


def attn_id(case):
    return "n%d-%dx%d-h%d" % case


def attn_applies(mutation, case):
    """whether the mistake can show at this case at all"""
    n, h, w, heads = case
    if mutation == "pad_zero":
        return h * w % KC != 0
    if mutation == "no_rescale":
        return h * w > KC
    if mutation == "cross_image":
        return n > 1
    if mutation == "head_mix":
        return heads > 1
    return True


AttnDraw = namedtuple("AttnDraw", "qkv pe_w9 pe_bias")


@functools.lru_cache(maxsize=None)
def attn_draw(case, kind):
    """qkv (n, N, heads * 128), pe_w9 [9][heads * 64], pe_bias [heads * 64]; all f32, read-only.  Both kinds of a case share
    the normal draws"""
    n, h, w, heads = case
    N = h * w
    rng = np.random.default_rng([ATTN_SEED, *case])
    qkv = rng.standard_normal((n, N, heads, 2 * KD + HD)).astype(np.float32)
    qkv[..., : 2 * KD] *= np.float32(QK_SCALE)
    if kind == "ramp":
        ramp = 0.3 + 1.2 * np.arange(N) / max(N - 1, 1)
        qkv[..., KD : 2 * KD] *= ramp.astype(np.float32)[None, :, None, None]
    else:
        assert kind == "flat", kind
    c = heads * HD
    d = AttnDraw(qkv.reshape(n, N, heads * (2 * KD + HD)), (rng.standard_normal((9, c)) / 3.0).astype(np.float32),
                 (0.1 * rng.standard_normal(c)).astype(np.float32))
    for a in d:
        a.setflags(write=False)
    return d


def _online(s, v):
    """softmax(s) v by chunks of KC keys with a running maximum, the accumulator and the sum NOT rescaled when it rises"""
    m = torch.full(s.shape[:-1], -float("inf"), dtype=s.dtype)
    l = torch.zeros(s.shape[:-1], dtype=s.dtype)
    acc = torch.zeros(s.shape[:-1] + (v.shape[-1],), dtype=s.dtype)
    for k0 in range(0, s.shape[-1], KC):
        sc = s[..., k0 : k0 + KC]
        m = torch.maximum(m, sc.amax(-1))
        p = (sc - m[..., None]).exp()
        l = l + p.sum(-1)
        acc = acc + p @ v[..., k0 : k0 + KC, :]
    return acc / l[..., None]


def attn_reference(case, d, pe, mutation=None, dtype=torch.float64):
    """the operation in torch at `dtype` from the exact f32 inputs: (n, N, heads * 64) as float64 numpy.  `mutation`: one of
    ATTN_MUTATIONS (they change the attention, not the positional encoding)"""
    assert mutation is None or (mutation in ATTN_MUTATIONS and attn_applies(mutation, case)), mutation
    n, h, w, heads = case
    N = h * w
    t = _t(d.qkv, dtype).view(n, N, heads, 2 * KD + HD).permute(0, 2, 1, 3)  # (n, heads, N, 128)
    q, k, v = t[..., :KD], t[..., KD : 2 * KD], t[..., 2 * KD :]
    v_pe = v
    if mutation == "qk_swapped":
        q, k = k, q
    if mutation == "v_is_k":  # the 64 values read from the key offset on
        v = t[..., KD : KD + HD]
    if mutation == "head_mix":
        v = v.roll(1, dims=1)
    if mutation == "cross_image":  # every query sees the keys of all images
        k = k.permute(1, 0, 2, 3).reshape(1, heads, n * N, KD).expand(n, -1, -1, -1)
        v = v.permute(1, 0, 2, 3).reshape(1, heads, n * N, HD).expand(n, -1, -1, -1)
    scale = 1.0 if mutation == "scale_dropped" else (HD if mutation == "scale_hd" else KD) ** -0.5
    s = (q @ k.transpose(-1, -2)) * scale  # (n, heads, queries, keys)
    if mutation == "pad_zero":  # the keys that fill the last chunk count, with score 0 and value 0
        s = torch.cat([s, s.new_zeros(s.shape[:-1] + (-N % KC,))], -1)
        y = s.softmax(-1)[..., :N] @ v
    elif mutation == "no_rescale":
        y = _online(s, v)
    elif mutation == "softmax_over_queries":
        y = s.softmax(-2) @ v
    else:
        y = s.softmax(-1) @ v
    y = y.permute(0, 2, 1, 3).reshape(n, N, heads * HD)
    if pe:
        c = heads * HD
        vmap = v_pe.permute(0, 1, 3, 2).reshape(n, c, h, w)
        wt = _t(d.pe_w9, dtype).T.reshape(c, 1, 3, 3)
        y = y + F.conv2d(vmap, wt, _t(d.pe_bias, dtype), padding=1, groups=c).flatten(2).transpose(1, 2)
    return y.double().numpy()


@functools.lru_cache(maxsize=None)
def attn_expected(case, kind, pe):
    """(fp64 reference, bound = 4 x max error of the float32 torch evaluation, that error): computed once, read-only"""
    d = attn_draw(case, kind)
    r64 = attn_reference(case, d, pe)
    err32 = float(np.abs(attn_reference(case, d, pe, dtype=torch.float32) - r64).max())
    r64.setflags(write=False)
    return r64, 4.0 * err32, err32


def max_logit(case, kind):
    d = attn_draw(case, kind)
    n, h, w, heads = case
    t = _t(d.qkv, torch.float64).view(n, h * w, heads, 2 * KD + HD).permute(0, 2, 1, 3)
    return float(((t[..., :KD] @ t[..., KD : 2 * KD].transpose(-1, -2)) * KD**-0.5).abs().max())


# ---------------------------------------------------------------------------
# depthwise 3x3
# ---------------------------------------------------------------------------
# x_ct = 0: a pixel of exactly the channels read; out_ct = 0: of c channels
DwCase = namedtuple("DwCase", "n h w c act add x_ct x_co g_size g_stride out_ct out_co", defaults=(NONE, False, 0, 0, 0, 0, 0, 0))
DW_CASES = [
    DwCase(1, 1, 1, 8),      # centre tap only
    DwCase(2, 1, 5, 16),     # H = 1
    DwCase(2, 5, 1, 16),     # W = 1
    DwCase(3, 4, 6, 24),     # halos of two neighbouring images
    DwCase(2, 7, 9, 72),     # 1134 threads: five blocks, the last ragged
    DwCase(2, 6, 5, 128, NONE, True, 256, 64, 64, 128),            # the positional-encoding form: the v rows of a two-head qkv
    DwCase(2, 5, 7, 40, SILU, False, 40 + 16, 8, 0, 0, 40 + 24, 16),  # the class-branch form, as channel slices of wider pixels
    DwCase(2, 3, 4, 32, SILU, True, 64, 0, 16, 48),                # SiLU and addend together, two groups of 16 at stride 48
]
FORMAT_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (x_fmt, out_fmt): 0 f32, 1 SP8
DW_MUTATIONS = ("taps_transposed", "kernel_flipped", "hpad_adjacent_row", "vpad_neighbour_image", "bias_dropped", "gather_ignored",
                "stride_as_size", "add_dropped", "act_after_add", "act_dropped")
BORDER_SCALE = 8.0


def dw_id(case):
    return "n%d-%dx%d-c%d" % case[:4] + ("-silu" if case.act == SILU else "") + ("-add" if case.add else "") + ("-g%d" % case.g_size if case.g_size else "")


def x_ct_of(case):
    return case.x_ct or case.c


def out_ct_of(case):
    return case.out_ct or case.c


def cin(case, mutation=None):
    """input channel of every output channel, counted from channel 0 of the pixel.  gather_ignored: the whole expression
    taken for k (no groups, no view offset); stride_as_size: the groups taken for adjacent (g_stride = g_size)"""
    k = np.arange(case.c)
    gs = case.g_size or case.c
    if mutation == "gather_ignored":
        return k
    if mutation == "stride_as_size":
        return k + case.x_co
    return (k // gs) * case.g_stride + k % gs + case.x_co


def dw_applies(mutation, case):
    """whether the mistake can show at this case at all"""
    n, h, w = case.n, case.h, case.w
    if mutation in ("taps_transposed", "kernel_flipped"):
        return h * w > 1  # a 1 x 1 image sees the centre tap alone
    if mutation == "hpad_adjacent_row":
        return n * h > 1  # the pixel before and after a row: the adjacent row's, at the first and last row the neighbouring image's
    if mutation == "vpad_neighbour_image":
        return n > 1
    if mutation in ("gather_ignored", "stride_as_size"):
        return not np.array_equal(cin(case, mutation), cin(case))
    if mutation == "add_dropped":
        return case.add
    if mutation == "act_dropped":
        return case.act == SILU
    if mutation == "act_after_add":
        return case.add and case.act == SILU
    return True


DwDraw = namedtuple("DwDraw", "full w9 bias add")


@functools.lru_cache(maxsize=None)
def dw_draw(index):
    return dw_draw_of(DW_CASES[index], 11450 + index)


def dw_draw_of(case, seed):
    """full [n][h][w][x_ct] (the whole input pixel), w9 [9 (kh 3 + kw)][c], bias [c], add [n][h][w][c] or None; f32, read-only"""
    n, h, w, c = case[:4]
    rng = np.random.default_rng(seed)
    full = rng.standard_normal((n, h, w, x_ct_of(case))).astype(np.float32)
    scale = np.ones((h, w), np.float32)
    scale[0] = scale[-1] = scale[:, 0] = scale[:, -1] = BORDER_SCALE
    full *= scale[None, :, :, None]
    w9 = (rng.standard_normal((9, c)) / 3.0).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    add = rng.standard_normal((n, h, w, c)).astype(np.float32) if case.add else None
    d = DwDraw(full, w9, bias, add)
    for a in d:
        if a is not None:
            a.setflags(write=False)
    return d


def _padded(x, mutation):
    """(n, h, w, c) -> the (n, c, h + 2, w + 2) map the 9 taps read: zeros around every image, or what a kernel that
    forgets one of the two masks reads there"""
    n, h, w, c = x.shape
    if mutation == "hpad_adjacent_row":  # no column mask: the pixel before and after a row in memory
        flat = torch.cat([x.new_zeros(1, c), x.reshape(n * h * w, c), x.new_zeros(1, c)])
        rows = flat.unfold(0, w + 2, w)  # [n h][c][w + 2]
        return F.pad(rows.reshape(n, h, c, w + 2).permute(0, 2, 1, 3), (0, 0, 1, 1))
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 0, 0))  # columns
    if mutation == "vpad_neighbour_image":  # no row mask: the images one below the other as one map
        tall = F.pad(xp.permute(1, 0, 2, 3).reshape(c, n * h, w + 2), (0, 0, 1, 1))
        return tall.unfold(1, h + 2, h).permute(1, 0, 3, 2)  # [n][c][h + 2][w + 2]
    return F.pad(xp, (0, 0, 1, 1))


def dw_reference(case, d, full=None, mutation=None, dtype=torch.float64):
    """the operation in torch at `dtype`: [n][h][w][c] as float64 numpy.  `full`: the values the kernel reads in place of
    d.full (an SP8 input: sp8_util.unpack of its bytes), any float type; `mutation`: one of DW_MUTATIONS"""
    assert mutation is None or (mutation in DW_MUTATIONS and dw_applies(mutation, case)), mutation
    c = case.c
    full = d.full if full is None else full
    x = _t(full[..., cin(case, mutation if mutation in ("gather_ignored", "stride_as_size") else None)], dtype)
    k = _t(d.w9, dtype).reshape(3, 3, c)
    if mutation == "taps_transposed":
        k = k.permute(1, 0, 2)
    if mutation == "kernel_flipped":
        k = k.flip(0, 1)
    bias = None if mutation == "bias_dropped" else _t(d.bias, dtype)
    y = F.conv2d(_padded(x, mutation), k.permute(2, 0, 1)[:, None].contiguous(), bias, groups=c).permute(0, 2, 3, 1)
    add = _t(d.add, dtype) if case.add and mutation != "add_dropped" else None
    if mutation == "act_after_add":
        y = F.silu(y + add)
    else:
        if case.act == SILU and mutation != "act_dropped":
            y = F.silu(y)
        if add is not None:
            y = y + add
    return y.double().numpy()


# f32 views at multiples of 4 floats that are no multiples of 8: what the f32 instantiation takes and an SP8 side does not
DW_CASE_QUADS = DwCase(2, 3, 4, 32, SILU, True, 72, 4, 16, 48, 40, 4)
DW_QUADS_SEED = 11449

# What the launches refuse, as changes of one valid call each (status 1, nothing launched, the output untouched).
# "+4": the pointer moved by four bytes.  Attention: the call (n, h, w, heads) = (2, 3, 4, 2) with its positional encoding.
ATTN_REFUSAL_BASE = dict(n=2, h=3, w=4, heads=2)
ATTN_REFUSALS = [
    ("null qkv", dict(qkv=None)), ("null out", dict(out=None)), ("n = 0", dict(n=0)), ("h = 0", dict(h=0)), ("w = -3", dict(w=-3)),
    ("heads = 0", dict(heads=0)), ("n = 65536", dict(n=65536)), ("heads = 65536", dict(heads=65536)),
    ("pe weights without bias", dict(pe_bias=None)), ("pe bias without weights", dict(pe_w9=None)),
    ("qkv misaligned", dict(qkv="+4")), ("out misaligned", dict(out="+4")), ("pe weights misaligned", dict(pe_w9="+4")),
    ("pe bias misaligned", dict(pe_bias="+4")),
]
# 3x3: two groups of 16 channels at stride 48 in a pixel of 72 floats (8 to spare), SiLU, addend, f32 both sides
DW_REFUSAL_BASE = dict(n=2, h=3, w=4, x_ct=72, x_co=0, x_fmt=0, c=32, g_size=16, g_stride=48, act=SILU, add_ld=32, out_ct=40, out_co=0, out_fmt=0)
DW_REFUSALS = [
    ("null x", dict(x=None)), ("null w9", dict(w9=None)), ("null bias", dict(bias=None)), ("null out", dict(out=None)),
    ("n = 0", dict(n=0)), ("h = 0", dict(h=0)), ("w = -1", dict(w=-1)), ("c = 0", dict(c=0)),
    ("c % 8 != 0", dict(c=28)), ("g_size = 12", dict(g_size=12)), ("g_size = -8", dict(g_size=-8)),
    ("x_ct % 4 != 0", dict(x_ct=70)), ("x_co % 4 != 0", dict(x_co=2)), ("g_stride % 4 != 0", dict(g_stride=50)),
    ("SP8 x_co = 4", dict(x_fmt=1, x_co=4)), ("SP8 g_stride = 52", dict(x_fmt=1, g_stride=52)),
    ("add_ld % 4 != 0", dict(add_ld=34)), ("add_ld < c", dict(add_ld=24)),
    ("out_ct % 4 != 0", dict(out_ct=38)), ("out_co % 4 != 0", dict(out_co=2)), ("SP8 out_co = 4", dict(out_fmt=1, out_co=4)),
    ("x misaligned", dict(x="+4")), ("w9 misaligned", dict(w9="+4")), ("bias misaligned", dict(bias="+4")), ("add misaligned", dict(add="+4")),
    ("out misaligned", dict(out="+4")),
    ("input channels past the pixel", dict(x_co=16)), ("output channels past the pixel", dict(out_co=12)),
    ("act = 2", dict(act=2)), ("x_fmt = 2", dict(x_fmt=2)), ("out_fmt = -1", dict(out_fmt=-1)),
]


def refusal_args(base, change, pointers):
    """base with `change` applied; pointers {name: address}: None stays None, "+4" is the address plus four bytes"""
    a = {**base, **pointers}
    for k, v in change.items():
        a[k] = a[k] + 4 if v == "+4" else v
    return a


def dw_expected_of(case, d, full=None):
    """(fp64 reference, bound = 4 x max error of the float32 torch evaluation, that error) on the values `full`"""
    r64 = dw_reference(case, d, full)
    err32 = float(np.abs(dw_reference(case, d, None if full is None else np.asarray(full, np.float32), dtype=torch.float32) - r64).max())
    return r64, 4.0 * err32, err32


@functools.lru_cache(maxsize=None)
def dw_expected(index):
    """dw_expected_of the case's own f32 draw: computed once, read-only"""
    r64, bound, err32 = dw_expected_of(DW_CASES[index], dw_draw(index))
    r64.setflags(write=False)
    return r64, bound, err32

