#!/usr/bin/env python3
"""Labelled bank match timing against the unlabelled one-pass kernel: python tools/match_labels_probe.py [rows] [rounds]

100 000 x 768 bank, every row tagged (random 64-bit words) and grouped (about 30 000 groups, like printings per card).
Shapes: b = 8, k = 3 (the server's) and b = 256, k = 3.  Variants, timed with HIP events after warm-up, in one process and
alternating within every round:
    plain     match(q, k) with MTGV_MATCH_PREPASS=0 - measured twice per round (plain, plain'), so the spread of the
              unlabelled call is measured the same way as the differences
    filter    one required tag bit per query (half of the rows eligible)
    distinct  one hit per group
    both      filter + distinct
Per variant: median over the rounds of the per-call time, min..max, and the share the GEMM launch (scores + fused top-k
epilogue; the launch profiler's events) has in a separate pass - the rest is the query normalisation and the merge."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]
import numpy as np
import torch

from mtgv import native
from mtgv.matcher import Matcher

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
CALLS = 20  # calls per timed burst
os.environ["MTGV_MATCH_PREPASS"] = "0"

g = torch.Generator(device="cuda").manual_seed(2)
rng = np.random.default_rng(2)
m = Matcher(768, capacity=rows)
m.add(torch.randn((rows, 768), generator=g, device="cuda"))
m.set_labels(0, rng.integers(0, 2**64, rows, dtype=np.uint64), rng.integers(0, max(1, rows * 3 // 10), rows).astype(np.int32))


def burst(fn):
    """ms per call of CALLS back-to-back calls, HIP events around the burst"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


def gemm_ms(fn):
    """ms per call inside the GEMM launch (launch profiler: events around every launch)"""
    lib = native.lib()
    native.check(lib.mtgv_profile_gemm(1))
    try:
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        native.check(lib.mtgv_profile_gemm_read(C.byref(ms), C.byref(fl), C.byref(n)))
    finally:
        native.check(lib.mtgv_profile_gemm(0))
    return ms.value / CALLS


print(f"bank {rows} x 768, {rounds} rounds of {CALLS} calls per variant, alternating; precision {native.get_gemm_precision()}")
for b, k in ((8, 3), (256, 3)):
    q = torch.randn((b, 768), generator=g, device="cuda")
    masks = np.zeros((b, 3), np.uint64)
    masks[:, 0] = np.uint64(1) << rng.integers(0, 64, b).astype(np.uint64)
    masks_dev = torch.from_numpy(masks.view(np.int64)).cuda()
    variants = {
        "plain": lambda: m.match(q, k),
        "filter": lambda: m.match(q, k, filter=masks_dev),
        "distinct": lambda: m.match(q, k, distinct=True),
        "both": lambda: m.match(q, k, filter=masks_dev, distinct=True),
        "plain'": lambda: m.match(q, k),
    }
    for fn in variants.values():  # warm-up: workspace growth, code objects
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t[name].append(burst(fn))
    gm = {name: gemm_ms(fn) for name, fn in variants.items()}
    base = statistics.median(t["plain"] + t["plain'"])
    spread = max(abs(statistics.median(t["plain"]) - statistics.median(t["plain'"])), statistics.pstdev(t["plain"] + t["plain'"]))
    print(f"b = {b}, k = {k}: unlabelled median {base:.4f} ms, run-to-run spread {spread:.4f} ms")
    for name in variants:
        med = statistics.median(t[name])
        print(f"  {name:9s} median {med:.4f} ms  (min {min(t[name]):.4f}, max {max(t[name]):.4f})  vs unlabelled {med - base:+.4f} ms"
              f"  GEMM launch {gm[name]:.4f} ms, rest {med - gm[name]:+.4f} ms")
