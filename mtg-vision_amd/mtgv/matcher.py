"""Host side of the match stage: exact cosine top-k over the whole card bank.

`Matcher.match(embedding, k)` is the north-star name.  The reference goes through
`VectorStoreQdrant.query_nearby` (mtgvision/qdrant.py:76-95; collection of 768-d
vectors with Distance.COSINE) - see `mtgv.adapters.VectorStoreQdrant` for that
signature.  All arithmetic is in libmtgv.so (match.hip / gemm_f32.hip).
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import native


class Matcher:
    """Device-resident bank of L2-normalised vectors (rows = local ids 0..size-1).

    `id_base` is added to every returned id: with the bank sharded by rows over
    ranks, rank r passes the global index of its first row (mtgv.dist).
    """

    def __init__(self, dim: int = 768, capacity: int = 131072, id_base: int = 0, device=None):
        native.require_gpu()
        self.dim = int(dim)
        self.capacity = int(capacity)
        self.id_base = int(id_base)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = native.c_vp(0)
        self.labelled = False  # set_labels was called since the last clear (bank.save_store writes labels only then)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_bank_create(self.dim, self.capacity, C.byref(self._h)))

    def __len__(self) -> int:
        return int(native.lib().mtgv_bank_size(self._h))

    def add(self, vectors: Union[np.ndarray, torch.Tensor]) -> range:
        """Append rows; returns the local row range they occupy.  Vectors are normalised on the GPU."""
        start = len(self)
        if isinstance(vectors, np.ndarray):
            vectors = torch.from_numpy(np.ascontiguousarray(vectors, dtype=np.float32))
        vectors = vectors.to(torch.float32)
        if vectors.ndim == 1:
            vectors = vectors[None]
        assert vectors.ndim == 2 and vectors.shape[1] == self.dim, f"{tuple(vectors.shape)}"
        vectors = vectors.contiguous()
        with torch.cuda.device(self.device):
            native.check(
                native.lib().mtgv_bank_append(
                    self._h, native.ptr(vectors), vectors.shape[0], 1 if vectors.is_cuda else 0, native.stream()
                )
            )
            if vectors.is_cuda:
                torch.cuda.current_stream().synchronize()
        return range(start, start + vectors.shape[0])

    def set_row(self, row: int, vector):
        v = np.ascontiguousarray(np.asarray(vector, dtype=np.float32).reshape(-1))
        assert v.size == self.dim
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_bank_set_row(self._h, int(row), v.ctypes.data_as(native.c_vp), native.stream()))

    def rows(self, start: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), np.float32)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_bank_get_rows(self._h, int(start), int(n), out.ctypes.data_as(native.c_vp)))
        return out

    def clear(self):
        with torch.cuda.device(self.device):  # (a labelled bank waits for its device's matches in flight before it resets the labels)
            native.check(native.lib().mtgv_bank_clear(self._h))
        self.labelled = False

    def set_labels(self, start: int, tags=None, groups=None):
        """Label the rows from local row `start` on: `tags` uint64 bit sets (the bits' meaning is the caller's), `groups`
        int32 group numbers >= 0, or -1 for "its own group".  Either may be None: that label stays as it is.  New rows
        start with tag 0 / group -1; `set_row` keeps a row's labels, `clear` resets them."""
        t = None if tags is None else np.ascontiguousarray(np.asarray(tags).reshape(-1).astype(np.uint64, copy=False))
        g = None if groups is None else np.asarray(groups).reshape(-1)
        if g is not None:
            assert g.size == 0 or (g.min() >= -(2**31) and g.max() < 2**31), "groups must fit int32"
            g = np.ascontiguousarray(g.astype(np.int32))
        if t is None and g is None:
            return
        n = t.size if t is not None else g.size
        assert g is None or t is None or g.size == t.size, f"{t.size} tags for {g.size} groups"
        with torch.cuda.device(self.device):
            native.check(
                native.lib().mtgv_bank_set_labels(
                    self._h, int(start), int(n), None if t is None else t.ctypes.data_as(native.c_vp),
                    None if g is None else g.ctypes.data_as(native.c_vp), native.stream()
                )
            )
        self.labelled = True

    def labels(self, start: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """(tags uint64 (n,), groups int32 (n,)) of the local rows [start, start + n)."""
        t = np.empty(int(n), np.uint64)
        g = np.empty(int(n), np.int32)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_bank_get_labels(self._h, int(start), int(n), t.ctypes.data_as(native.c_vp), g.ctypes.data_as(native.c_vp)))
        return t, g

    def _masks(self, filter, b: int) -> torch.Tensor:
        """`filter` of match() -> (b, 3) int64 bit patterns on the device"""
        if isinstance(filter, torch.Tensor):
            assert filter.dtype == torch.int64 and tuple(filter.shape) == (b, 3), f"filter: {tuple(filter.shape)} {filter.dtype}, expected ({b}, 3) int64"
            return filter.to(self.device).contiguous()
        if isinstance(filter, np.ndarray):
            assert filter.dtype == np.uint64 and filter.shape == (b, 3), f"filter: {filter.shape} {filter.dtype}, expected ({b}, 3) uint64"
            return torch.from_numpy(np.ascontiguousarray(filter).view(np.int64)).to(self.device)
        assert len(filter) == 3 and all(isinstance(v, (int, np.integer)) and 0 <= int(v) < 2**64 for v in filter), (
            "filter: one (all_of, any_of, none_of) triple of 64-bit masks, or a (B, 3) array"
        )
        row = np.array([int(v) for v in filter], np.uint64).view(np.int64)
        return torch.from_numpy(np.broadcast_to(row, (b, 3)).copy()).to(self.device)

    def match(self, embedding, k: int = 1, threshold: Optional[float] = None, *, filter=None, distinct: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(D,) or (B,D) raw embeddings -> (ids int64 (B,k), scores float32 (B,k)) on the GPU.

        Sorted by cosine score descending, ties by ascending id; id -1 / score -inf pads
        when the bank holds fewer than k rows.  `threshold` is `score_threshold` of
        `query_nearby` (mtgvision/qdrant.py:83,93): hits scoring below it are dropped on the
        device (they become pads).

        `filter`: only rows whose tags pass (all_of, any_of, none_of) take part - one triple of ints for all queries, or
        a (B, 3) array (numpy uint64, or a torch int64 bit pattern).  `distinct`: a group >= 0 is represented by its
        best row only, so the k hits are k different cards.  Both are exact (include/mtgv.h, mtgv_bank_topk_ex); the
        defaults make the same call as before."""
        if isinstance(embedding, np.ndarray) or isinstance(embedding, (list, tuple)):
            embedding = torch.from_numpy(np.ascontiguousarray(np.asarray(embedding, dtype=np.float32)))
        q = embedding.to(self.device, torch.float32)
        if q.ndim == 1:
            q = q[None]
        assert q.ndim == 2 and q.shape[1] == self.dim, f"{tuple(q.shape)}"
        q = q.contiguous()
        b = q.shape[0]
        ids = torch.empty((b, k), dtype=torch.int64, device=self.device)
        scores = torch.empty((b, k), dtype=torch.float32, device=self.device)
        masks = None if filter is None else self._masks(filter, b)
        if b == 0:
            return ids, scores
        with torch.cuda.device(self.device):
            if masks is None and not distinct:
                native.check(
                    native.lib().mtgv_bank_topk(self._h, native.ptr(q), b, int(k), self.id_base, _thr(threshold), native.ptr(ids), native.ptr(scores),
                                                native.stream())
                )
            else:
                native.check(
                    native.lib().mtgv_bank_topk_ex(self._h, native.ptr(q), b, int(k), self.id_base, _thr(threshold), native.ptr(masks),
                                                   1 if distinct else 0, native.ptr(ids), native.ptr(scores), native.stream())
                )
        return ids, scores

    def match_packed(self, q: torch.Tensor, k: int = 1, *, filter=None, distinct: bool = False) -> torch.Tensor:
        """The local top-k in the sharded match's exchange format (mtgv.dist, include/mtgv.h): q (B, D) float32 on the
        device, contiguous -> (B, k, 2) int64 = (global id or -1, float32 bit pattern of the score).  One library call,
        no other kernel: what one all-gather then carries to every rank.

        `filter` (the forms `match` takes; a (B, 3) int64 tensor on the device is used as it is) / `distinct`: the
        labelled match of this shard (mtgv_bank_topk_packed_ex) - the high half of word 1 then carries the row's group,
        which `merge_gathered(..., distinct=True)` needs, and an empty shard answers with pads.  The defaults make the
        same call as before."""
        assert q.is_cuda and q.dtype == torch.float32 and q.ndim == 2 and q.shape[1] == self.dim and q.is_contiguous(), f"{tuple(q.shape)} {q.dtype}"
        b = q.shape[0]
        packed = torch.empty((b, k, 2), dtype=torch.int64, device=self.device)
        masks = None if filter is None else self._masks(filter, b)
        if b:
            with torch.cuda.device(self.device):
                if masks is None and not distinct:
                    native.check(native.lib().mtgv_bank_topk_packed(self._h, native.ptr(q), b, int(k), self.id_base, native.ptr(packed), native.stream()))
                else:
                    native.check(native.lib().mtgv_bank_topk_packed_ex(self._h, native.ptr(q), b, int(k), self.id_base, native.ptr(masks),
                                                                       1 if distinct else 0, native.ptr(packed), native.stream()))
        return packed

    def prepass_fallbacks(self) -> int:
        """Queries of two-pass matches (>= 128 queries per call) that had to be scanned exactly so far (include/mtgv.h).
        An all-zero query is not among them: its answer (the k first rows at score 0) needs no scan and is given directly."""
        v = native.c_i64(0)
        native.check(native.lib().mtgv_bank_prepass_fallbacks(self._h, C.byref(v)))
        return int(v.value)

    def prepass_candidates(self, q: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """TEST SURFACE, not part of the match API: the first pass of the two-pass match on its own
        (mtgv_bank_prepass_candidates).  q (B, D) float32 on the device -> (scores float32 (B, slots, per_range), rows int32
        of the same shape, range_cols): per 96-row range of the bank its best approximate (fp16 x fp16) scores, pads
        (-inf, -1).  `out`: flat buffers to write into instead of fresh ones (at least B * slots * per_range elements);
        a refused call (AssertionError: the bank or batch never takes the first pass) leaves them untouched."""
        assert q.is_cuda and q.dtype == torch.float32 and q.ndim == 2 and q.shape[1] == self.dim and q.is_contiguous(), f"{tuple(q.shape)} {q.dtype}"
        b = q.shape[0]
        slots, cols, kp = native.c_i32(0), native.c_i32(0), native.c_i32(0)
        native.check(native.lib().mtgv_bank_prepass_layout(self._h, C.byref(slots), C.byref(cols), C.byref(kp)))
        n = b * slots.value * kp.value
        if out is None:
            out = (torch.empty(n, dtype=torch.float32, device=self.device), torch.empty(n, dtype=torch.int32, device=self.device))
        cs, ci = out
        assert cs.dtype == torch.float32 and ci.dtype == torch.int32 and cs.numel() >= n and ci.numel() >= n
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_bank_prepass_candidates(self._h, native.ptr(q), b, native.ptr(cs), native.ptr(ci), C.byref(slots),
                                                                   C.byref(cols), native.stream()))
        shape = (b, slots.value, kp.value)
        return cs[:n].view(shape), ci[:n].view(shape), cols.value

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                native.lib().mtgv_bank_destroy(self._h)
                self._h = native.c_vp(0)
        except Exception:
            pass


def _thr(threshold: Optional[float]) -> float:
    return float("-inf") if threshold is None else float(threshold)


def merge_topk(cand_scores: torch.Tensor, cand_ids: torch.Tensor, k: int, threshold: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge (B, ncand) candidate (score, id) pairs - e.g. the all-gathered per-shard top-k -
    into the global top-k with the same (score desc, id asc) order.  Consumes cand_scores."""
    assert cand_scores.is_cuda and cand_ids.is_cuda and cand_scores.shape == cand_ids.shape and cand_scores.ndim == 2
    cs = cand_scores.to(torch.float32).contiguous().clone()
    ci = cand_ids.to(torch.int64).contiguous()
    b, n = cs.shape
    ids = torch.empty((b, k), dtype=torch.int64, device=cs.device)
    scores = torch.empty((b, k), dtype=torch.float32, device=cs.device)
    with torch.cuda.device(cs.device):
        native.check(native.lib().mtgv_topk_merge(native.ptr(cs), native.ptr(ci), b, n, int(k), _thr(threshold), native.ptr(ids), native.ptr(scores), native.stream()))
    return ids, scores


def merge_gathered(gathered: torch.Tensor, row0: int, b: int, k: int, threshold: Optional[float] = None, *,
                   distinct: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge the all-gathered per-shard candidates (R, B_total, k, 2) int64 in the exchange format of
    `Matcher.match_packed` for the queries [row0, row0 + b): global (ids (b, k) int64, scores (b, k) float32), score desc
    then id asc.  One library kernel reads the collective's output buffer in place.

    `distinct`: the candidates come from `match_packed(..., distinct=True)` on every shard; a picked candidate retires the
    other candidates of its group (mtgv_topk_merge_gathered_ex), so the result is `Matcher.match(..., distinct=True)` over
    the whole bank.  Filter-only exchanges merge with the default."""
    assert gathered.is_cuda and gathered.dtype == torch.int64 and gathered.ndim == 4 and gathered.shape[2] == k and gathered.shape[3] == 2
    assert gathered.is_contiguous()
    R, b_total = gathered.shape[0], gathered.shape[1]
    ids = torch.empty((b, k), dtype=torch.int64, device=gathered.device)
    scores = torch.empty((b, k), dtype=torch.float32, device=gathered.device)
    if b:
        with torch.cuda.device(gathered.device):
            if not distinct:
                native.check(native.lib().mtgv_topk_merge_gathered(native.ptr(gathered), R, b_total, int(k), int(row0), int(b), _thr(threshold),
                                                                   native.ptr(ids), native.ptr(scores), native.stream()))
            else:
                native.check(native.lib().mtgv_topk_merge_gathered_ex(native.ptr(gathered), R, b_total, int(k), int(row0), int(b), _thr(threshold),
                                                                      1, native.ptr(ids), native.ptr(scores), native.stream()))
    return ids, scores
