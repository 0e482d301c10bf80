"""Multi-GPU layout: one process per GPU, frames data-parallel, bank sharded by rows.

The only exchange step of the path is the match: every query must see every bank row.
With the bank split by rows over R ranks (rank r holds rows [r*N/R, (r+1)*N/R), global id =
local row + offset), top-k of the union = merge of per-shard top-k:

    1. all_gather the local query embeddings        (B_local x D fp32 each)
    2. every rank scores ALL queries against its shard, local top-k (ids already global)
    3. all_gather the (id, score) candidates, packed into ONE int64 buffer (B_total x k x 2 per rank)
    4. every rank merges the R*k candidates of its OWN queries (score desc, id asc)

Both messages are KB-scale: latency-bound, xGMI bandwidth is irrelevant, so the step has exactly two
collectives (RCCL `all_gather_into_tensor`, backend "nccl" on ROCm).  With `local_topk_packed` / `merge_gathered`
(`Matcher.match_packed`, `matcher.merge_gathered`) step 2 writes the exchange format itself and step 4 reads the
gathered buffer in place: the exchange then launches NOTHING but two library kernels and RCCL's two all-gathers - no
PyTorch arithmetic - which is what lets it run on one of the two streams of `Pipeline.run_many` (include/mtgv.h,
concurrency contract).  MTGV_FORCE_COLLECTIVE=1 runs them at
world size 1 too (a one-GPU box can then exercise the RCCL path: tests/test_gpu_dist.py).  The local top-k and the merge
are pluggable so the collective logic is exercised on CPU with gloo (tests/test_dist_cpu.py).

Row labels (filter / distinct, `Matcher.match`) cross the exchange too: step 2 is then the labelled match of the shard,
each candidate carries its row's group in the high half of its score word (same message size), and with distinct step 4
retires a picked group's other candidates, since two shards may each report a row of one card.  Per-query filters are
all-gathered beside the queries (a third KB-scale collective, only then).  `ShardedMatcher` is the whole of it as an
object with `Matcher`'s surface.
"""

from __future__ import annotations

import os
from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist


def shard_rows(n_rows: int, rank: int, world: int) -> Tuple[int, int]:
    """contiguous row range [start, stop) of `rank`; remainders go to the first ranks"""
    base, rem = divmod(n_rows, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def shard_frames(n_frames: int, rank: int, world: int) -> Tuple[int, int]:
    return shard_rows(n_frames, rank, world)


def _all_gather_cat(x: torch.Tensor, group=None) -> torch.Tensor:
    world = dist.get_world_size(group)
    out = torch.empty((world, *x.shape), dtype=x.dtype, device=x.device)
    try:
        dist.all_gather_into_tensor(out, x.contiguous(), group=group)
    except (RuntimeError, NotImplementedError):  # backends without the fused form
        parts = [torch.empty_like(x) for _ in range(world)]
        dist.all_gather(parts, x.contiguous(), group=group)
        out = torch.stack(parts)
    return out


def sharded_topk(q_local: torch.Tensor, k: int, local_topk: Callable, merge: Callable, group=None, *,
                 local_topk_packed: Optional[Callable] = None, merge_gathered: Optional[Callable] = None,
                 masks_local: Optional[torch.Tensor] = None, distinct: bool = False):
    """q_local (B_local, D) -> global (ids (B_local, k) int64, scores (B_local, k)) for this rank's queries.

    local_topk(q (B,D), k) -> (ids int64 (B,k) GLOBAL ids, scores (B,k)) over this rank's bank shard.
    merge(cand_scores (B, R*k), cand_ids (B, R*k), k) -> (ids, scores).
    Lean form (both given): local_topk_packed(q (B,D), k) -> (B, k, 2) int64 (id, float32 score bits);
    merge_gathered(gathered (R, B_total, k, 2), row0, b, k) -> (ids, scores) - no tensor arithmetic in between.
    Every rank must pass the same B_local.

    Labelled form (row labels, `Matcher.match`'s filter / distinct over the sharded bank; lean callables required):
    masks_local (B_local, 3) int64 = this rank's queries' (all_of, any_of, none_of) bit patterns, and / or distinct.  The
    masks are all-gathered beside the queries - a third KB-scale collective, made only when masks are given - and the
    callables are called as local_topk_packed(q, k, filter=masks_all or None, distinct=distinct) -> (B, k, 2) with the row's
    group in the high half of word 1, and merge_gathered(gathered, row0, b, k, distinct=distinct); every shard removes its
    own duplicate groups and the merge removes them across shards (exact).  Like B_local, the choice
    of masks-or-not and of distinct must be the same on every rank: they decide which collectives are made and how the
    message is read.  Without a process group local_topk is called with the same keywords."""
    labelled = masks_local is not None or distinct
    force = os.environ.get("MTGV_FORCE_COLLECTIVE") == "1"
    if not dist.is_initialized() or (dist.get_world_size(group) == 1 and not force):
        return local_topk(q_local, k, filter=masks_local, distinct=distinct) if labelled else local_topk(q_local, k)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    b_local = q_local.shape[0]
    assert not labelled or (local_topk_packed is not None and merge_gathered is not None), "the labelled exchange needs local_topk_packed and merge_gathered"
    if local_topk_packed is not None and merge_gathered is not None:
        q_all = _all_gather_cat(q_local, group).view(world * b_local, -1)  # a view of the collective's output
        local_kw, merge_kw = {}, {}  # the label keywords are passed only when labelled: the unlabelled calls stay as they were
        if labelled:
            local_kw, merge_kw = {"filter": None, "distinct": distinct}, {"distinct": distinct}
            if masks_local is not None:
                assert masks_local.dtype == torch.int64 and tuple(masks_local.shape) == (b_local, 3), f"masks_local: {tuple(masks_local.shape)} {masks_local.dtype}"
                local_kw["filter"] = _all_gather_cat(masks_local, group).view(world * b_local, 3)
        packed = local_topk_packed(q_all, k, **local_kw)
        return merge_gathered(_all_gather_cat(packed, group), rank * b_local, b_local, k, **merge_kw)
    q_all = _all_gather_cat(q_local, group).reshape(world * b_local, -1)
    ids, scores = local_topk(q_all, k)
    # one message: [..., 0] = id, [..., 1] = the score's float32 bit pattern
    packed = torch.stack((ids.to(torch.int64), scores.to(torch.float32).contiguous().view(torch.int32).to(torch.int64)), dim=-1)
    allp = _all_gather_cat(packed.contiguous(), group)  # (R, B_total, k, 2)
    mine = allp[:, rank * b_local : (rank + 1) * b_local].permute(1, 0, 2, 3).reshape(b_local, world * k, 2)
    cand_i = mine[..., 0].contiguous()
    cand_s = mine[..., 1].to(torch.int32).contiguous().view(torch.float32)
    return merge(cand_s, cand_i, k)


class ShardedMatcher:
    """The row-sharded bank as one object with `Matcher`'s surface: every rank holds the rows
    shard_rows(n_rows_total, rank, world) in a local `Matcher` whose id_base is the shard's first row, and `match` is the
    exchange above - ids are global rows, the contract is `Matcher.match`'s, filter and distinct included.

        m = ShardedMatcher(768, n_rows_total)          # after init_process_group; one per rank
        m.add_local(bank[m.rows.start:m.rows.stop])    # this rank's rows, in order
        m.set_labels(0, tags, groups)                  # GLOBAL rows: the part inside the shard is applied
        ids, scores = m.match(z, 3, filter=(all_of, 0, 0), distinct=True)

    Without a process group, or at world size 1 without MTGV_FORCE_COLLECTIVE=1, it is the local Matcher.  On an "nccl"
    group nothing leaves the device and the exchange launches only the two library kernels and RCCL's all-gathers (no
    PyTorch arithmetic on the stream: include/mtgv.h, concurrency contract); an unlabelled match makes the calls of
    sharded_topk's lean form, two-pass pre-pass included.  On a "gloo" group the messages are staged through host memory
    (memcpys, no kernels) - the rehearsal of several ranks on one GPU.  Every rank must call `match` with the same
    B_local, k, distinct and filter-or-not; the filters themselves may differ per rank and per query.
    Not supported on a sharded bank: `TrackedPipeline` (each rank has its own number of due tracks, the exchange needs
    equal B_local) and `adapters.VectorStoreQdrant` (single-bank)."""

    issues_collectives = True  # Pipeline.run_many: normal stream priorities, as for a caller-supplied collective match

    def __init__(self, dim: int = 768, n_rows_total: int = 131072, group=None, device=None):
        from .matcher import Matcher

        self.group = group
        self.n_rows_total = int(n_rows_total)
        on = dist.is_initialized()
        self.world, self.rank = (dist.get_world_size(group), dist.get_rank(group)) if on else (1, 0)
        lo, hi = shard_rows(self.n_rows_total, self.rank, self.world)
        self.rows = range(lo, hi)
        # (a bank needs a capacity of at least one row; a rank whose shard is empty keeps an empty bank)
        self.local = Matcher(dim, capacity=max(1, hi - lo), id_base=lo, device=device)
        self.dim, self.device = self.local.dim, self.local.device

    def __len__(self) -> int:
        return self.n_rows_total

    def add_local(self, vectors) -> range:
        """Append rows of this rank's shard, in order; returns the GLOBAL row range they occupy."""
        r = self.local.add(vectors)
        assert r.stop <= len(self.rows), f"{r.stop} rows in a shard of {len(self.rows)}"
        return range(self.rows.start + r.start, self.rows.start + r.stop)

    def set_labels(self, start: int, tags=None, groups=None):
        """`Matcher.set_labels` by GLOBAL row: of the rows from `start` on, the part inside this rank's shard is labelled
        (those rows must have been added); group numbers mean the same on every rank."""
        import numpy as np

        t = None if tags is None else np.asarray(tags).reshape(-1)
        g = None if groups is None else np.asarray(groups).reshape(-1)
        if t is None and g is None:
            return
        n = t.size if t is not None else g.size
        assert g is None or t is None or g.size == t.size, f"{t.size} tags for {g.size} groups"
        a, b = max(int(start), self.rows.start), min(int(start) + n, self.rows.stop)
        if a < b:
            part = slice(a - int(start), b - int(start))
            self.local.set_labels(a - self.rows.start, None if t is None else t[part], None if g is None else g[part])

    def _collective(self) -> bool:
        return dist.is_initialized() and (self.world > 1 or os.environ.get("MTGV_FORCE_COLLECTIVE") == "1")

    def match(self, embedding, k: int = 1, threshold: Optional[float] = None, *, filter=None, distinct: bool = False):
        """`Matcher.match` over the whole sharded bank for this rank's queries: (ids (B, k) int64 global rows, scores (B, k)
        float32) on the GPU."""
        from .matcher import merge_gathered, merge_topk

        m = self.local
        if not self._collective():
            return m.match(embedding, k, threshold, filter=filter, distinct=distinct)
        if not isinstance(embedding, torch.Tensor):
            embedding = torch.as_tensor(embedding, dtype=torch.float32)
        q = embedding.to(m.device, torch.float32)
        if q.ndim == 1:
            q = q[None]
        assert q.ndim == 2 and q.shape[1] == m.dim, f"{tuple(q.shape)}"
        q = q.contiguous()
        masks = None if filter is None else m._masks(filter, q.shape[0])
        if q.shape[0] == 0:  # (every rank passes the same B_local: none of them enters a collective)
            return m.match(q, k, threshold, filter=masks, distinct=distinct)
        labels = {} if masks is None and not distinct else {"masks_local": masks, "distinct": distinct}
        if dist.get_backend(self.group) != "gloo":
            return sharded_topk(q, k, m.match, merge_topk, self.group, local_topk_packed=m.match_packed,
                                merge_gathered=lambda gth, row0, b, kk, **kw: merge_gathered(gth, row0, b, kk, threshold, **kw), **labels)

        # gloo: the same library calls, the collectives on host copies
        def loc(x, kk, filter=None, **kw):
            return m.match_packed(x.to(m.device), kk, filter=None if filter is None else filter.to(m.device), **kw).cpu()

        def mrg(gth, row0, b, kk, **kw):
            return merge_gathered(gth.to(m.device), row0, b, kk, threshold, **kw)

        if masks is not None:
            labels["masks_local"] = masks.cpu()
        return sharded_topk(q.cpu(), k, None, None, self.group, local_topk_packed=loc, merge_gathered=mrg, **labels)
