#!/usr/bin/env python3
"""Labelled sharded match timing: python tools/dist_labels_probe.py [rows] [rounds]

The bench's match shape - 256 queries, a 100 000 x 768 bank, k = 3 - at world size 1 through RCCL (backend nccl,
MTGV_FORCE_COLLECTIVE=1, as tests/test_gpu_rccl.py runs it), every row tagged and grouped like tools/match_labels_probe.py's
bank.  Variants, timed with HIP events after the settle calls, in one process and alternating within every round:
    exchange            ShardedMatcher.match(q, k): the calls of the unlabelled lean exchange (two all-gathers, pre-pass)
    exchange distinct   ... distinct=True (two all-gathers, the labelled one-pass kernel, the merge that dedupes)
    exchange both       ... filter + distinct (a third all-gather for the masks)
    packed_ex d / b     mtgv_bank_topk_packed_ex alone (distinct / filter + distinct)
    merge_ex            mtgv_topk_merge_gathered_ex alone, distinct, on the gathered (1, 256, 3, 2) buffer
    single / d / b      the single-bank calls at the same shape: mtgv_bank_topk, mtgv_bank_topk_ex (distinct / both) - the yardstick
Per variant: median over the rounds of the per-call time, min..max.  Expectation: exchange distinct / both = the single-bank
labelled call plus the collectives' latency (exchange minus single, unlabelled)."""
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]
import numpy as np
import torch
import torch.distributed as dist

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 60
B, K, CALLS, SETTLE = 256, 3, 10, 20

s = socket.socket()
s.bind(("127.0.0.1", 0))
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]), MTGV_FORCE_COLLECTIVE="1")
s.close()
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))

from mtgv import ShardedMatcher, native
from mtgv.matcher import merge_gathered

g = torch.Generator(device="cuda").manual_seed(2)
rng = np.random.default_rng(2)
sm = ShardedMatcher(768, rows)
sm.add_local(torch.randn((rows, 768), generator=g, device="cuda"))
sm.set_labels(0, rng.integers(0, 2**64, rows, dtype=np.uint64), rng.integers(0, max(1, rows * 3 // 10), rows).astype(np.int32))
m = sm.local
q = torch.randn((B, 768), generator=g, device="cuda")
masks = np.zeros((B, 3), np.uint64)
masks[:, 0] = np.uint64(1) << rng.integers(0, 64, B).astype(np.uint64)
masks_dev = torch.from_numpy(masks.view(np.int64)).cuda()
gathered = m.match_packed(q, K, distinct=True)[None].contiguous()

variants = {
    "exchange": lambda: sm.match(q, K),
    "exchange distinct": lambda: sm.match(q, K, distinct=True),
    "exchange both": lambda: sm.match(q, K, filter=masks_dev, distinct=True),
    "packed_ex d": lambda: m.match_packed(q, K, distinct=True),
    "packed_ex b": lambda: m.match_packed(q, K, filter=masks_dev, distinct=True),
    "merge_ex": lambda: merge_gathered(gathered, 0, B, K, distinct=True),
    "single": lambda: m.match(q, K),
    "single d": lambda: m.match(q, K, distinct=True),
    "single b": lambda: m.match(q, K, filter=masks_dev, distinct=True),
}


def burst(fn):
    """ms per call of CALLS back-to-back calls, HIP events around the burst"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


ref = m.match(q, K, filter=masks_dev, distinct=True)
got = sm.match(q, K, filter=masks_dev, distinct=True)
assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), "the exchange differs from the single-bank call"
for fn in variants.values():  # settle: workspace growth, code objects, RCCL's first collectives
    for _ in range(SETTLE):
        fn()
torch.cuda.synchronize()
t = {name: [] for name in variants}
for _ in range(rounds):
    for name, fn in variants.items():
        t[name].append(burst(fn))
print(f"bank {rows} x 768, b = {B}, k = {K}, world size 1 (nccl, forced collective); {rounds} rounds of {CALLS} calls per variant, alternating; "
      f"precision {native.get_gemm_precision()}")
med = {name: statistics.median(v) for name, v in t.items()}
for name in variants:
    print(f"  {name:18s} median {med[name]:.4f} ms  (min {min(t[name]):.4f}, max {max(t[name]):.4f})")
coll = med["exchange"] - med["single"]
print(f"collectives and exchange overhead, unlabelled (exchange - single): {coll:+.4f} ms")
for a, b in (("exchange distinct", "single d"), ("exchange both", "single b")):
    print(f"{a} - {b}: {med[a] - med[b]:+.4f} ms  (expected about {coll:+.4f})")
dist.barrier()
dist.destroy_process_group()
