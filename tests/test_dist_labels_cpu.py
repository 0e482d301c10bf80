"""CPU: row labels across the sharded exchange (mtgv.dist; mtgv_bank_topk_packed_ex / mtgv_topk_merge_gathered_ex).  The
scheme restated in numpy (dist_labels_common.py) against the brute-force oracle of match_labels_common.py, the two wrong
variants as negative controls, the exchange words' bit layout, and dist.sharded_topk's labelled form on two gloo ranks."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dist_labels_common as D
import match_labels_common as L

RS = [1, 2, 3, 5, 7]
VARIANTS = ["filter", "distinct", "both"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scores fp64 (B, N), tags, groups, masks, designed) of a named input, computed once and left unchanged"""
    from oracle import match_ref as M

    if name.startswith("random"):
        bank, q, tags, groups, masks = L.random_case(int(name[6:]))
        return M.scores(q, bank), tags, groups, masks, False
    bank, q1, groups = {"hiding": L.hiding_case, "ties": L.ties_case, "cross": D.cross_shard_case}[name](64)
    return M.scores(q1[None], bank), np.zeros(L.N, np.uint64), groups, None, True


def _labels(name, variant):
    s, tags, groups, masks, designed = _case(name)
    if designed:  # no tags: the filter variants run with the mask that admits every row
        return L.NO_FILTER, variant != "filter"
    return L.variant_labels((None, None, tags, groups, masks), variant)


@functools.lru_cache(maxsize=None)
def _oracle(name, variant, k):
    s, tags, groups, _, _ = _case(name)
    masks, distinct = _labels(name, variant)
    return L.labelled_topk(s, tags, groups, masks, distinct, k)[0]


def _scheme(name, variant, k, R, **kw):
    s, tags, groups, _, _ = _case(name)
    masks, distinct = _labels(name, variant)
    return D.sharded_labelled_topk(s, tags, groups, masks, distinct, k, R, **kw)


# ---- 1. the scheme is exact ----
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("name", ["random64", "random36", "hiding", "ties"])
def test_scheme_equals_oracle(name, R):
    ks = [1, 3, 8] + ([100] if _case(name)[4] else [])
    for variant in VARIANTS:
        for k in ks:
            ids, sc = _scheme(name, variant, k, R)
            want = _oracle(name, variant, k)
            assert (ids == want).all(), f"{name} {variant} k={k} R={R}: queries {np.nonzero((ids != want).any(1))[0][:8].tolist()} differ"
            assert np.isneginf(sc[ids < 0]).all() and np.isfinite(sc[ids >= 0]).all()


# ---- 2. negative controls: each wrong variant is caught on a named input ----
def test_merge_without_dedupe_is_wrong():
    ids, _ = _scheme("ties", "distinct", 100, 3, merge_dedupe=False)
    assert (ids != _oracle("ties", "distinct", 100)).any()
    ids, _ = _scheme("random36", "distinct", 3, 3, merge_dedupe=False)
    bad = (ids != _oracle("random36", "distinct", 3)).any(1)
    print(f"merge without dedupe: {int(bad.sum())} of {len(bad)} queries of random_case(36) wrong at k = 3, R = 3")
    assert bad.any()


def test_local_without_dedupe_is_wrong():
    ids, _ = _scheme("hiding", "distinct", 3, 3, local_dedupe=False)
    assert ids[0].tolist() != _oracle("hiding", "distinct", 3)[0].tolist() == [204, 210, 30]


# ---- 3. the designed cross-shard case ----
def test_cross_shard_case():
    assert D.shards(L.N, D.CROSS_R) == [(0, 141), (141, 281), (281, 421)]
    k, R = D.CROSS_K, D.CROSS_R
    assert _oracle("cross", "distinct", k)[0].tolist() == D.CROSS_WANT
    assert _scheme("cross", "distinct", k, R)[0][0].tolist() == D.CROSS_WANT
    assert _scheme("cross", "distinct", k, R, merge_dedupe=False)[0][0].tolist() == D.CROSS_WANT_NO_MERGE_DEDUPE
    ids, sc = _scheme("cross", "distinct", k, R, threshold=D.CROSS_THR)
    assert ids[0].tolist() == D.CROSS_WANT_THR and np.isneginf(sc[0, 2:]).all()
    s, tags, groups, _, _ = _case("cross")
    assert L.labelled_topk(s, tags, groups, L.NO_FILTER, True, k, D.CROSS_THR)[0][0].tolist() == D.CROSS_WANT_THR


# ---- 4. bit layout of the exchange words ----
def test_exchange_word_layout():
    ids = np.array([[7, 421, -1]], np.int64)
    sc = np.array([[0.75, -0.5, 123.0]], np.float32)
    p = D.pack(ids, sc, np.array([[-1, 2**31 - 1, 5]]))
    assert p.dtype == np.int64 and p.shape == (1, 3, 2)
    w = p[0, :, 1].view(np.uint64)
    assert int(w[0]) >> 32 == 0xFFFFFFFF and int(w[0]) & 0xFFFFFFFF == int(np.float32(0.75).view(np.uint32))  # group -1
    assert int(w[1]) >> 32 == 2**31 - 1
    assert p[0, 2].tolist() == [-1, np.uint64((0xFFFFFFFF << 32) | 0xFF800000).view(np.int64)]  # the pad: id -1, -inf, group -1
    # the low half, read as the unlabelled merge reads it (test_dist_cpu.py: astype(uint32).view(float32)), is the score
    low = p[..., 1].astype(np.uint32).view(np.float32)
    assert low[0, :2].tolist() == [0.75, -0.5] and np.isneginf(low[0, 2])
    i2, s2, g2 = D.unpack(p)
    assert i2.tolist() == [[7, 421, -1]] and g2.tolist() == [[-1, 2**31 - 1, -1]] and s2[0, :2].tolist() == [0.75, -0.5]


def test_new_entry_points_status_without_gpu():
    """version 108 exports the two calls; null arguments are status 1 before any device is touched"""
    from mtgv import native

    lib = native.lib()
    assert lib.mtgv_version() >= 108
    for rc in (
        lib.mtgv_bank_topk_packed_ex(None, None, 1, 1, 0, None, 1, None, None),
        lib.mtgv_topk_merge_gathered_ex(None, 1, 1, 1, 0, 1, 0.0, 1, None, None, None),
    ):
        assert rc == 1 and b"null" in lib.mtgv_last_error()
        with pytest.raises(AssertionError):
            native.check(rc)


# ---- 5. dist.sharded_topk's labelled form on two gloo ranks ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, ret):
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path[:0] = [root, os.path.join(root, "mtg-vision_amd"), here]
    from mtgv import dist as mdist
    from oracle import match_ref as M

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bank, q, tags, groups, masks = L.random_case(64)
        b_local, k = L.B_MAX // world, 3
        lo, hi = mdist.shard_rows(L.N, rank, world)
        mine = slice(rank * b_local, (rank + 1) * b_local)
        calls = []
        orig = mdist._all_gather_cat

        def spy(x, group=None):
            calls.append(tuple(x.shape))
            return orig(x, group)

        mdist._all_gather_cat = spy

        def local_topk_packed(qa, kk, filter=None, distinct=False):
            m = L.NO_FILTER if filter is None else filter.numpy().view(np.uint64)
            return torch.from_numpy(D.local_packed(M.scores(qa.numpy(), bank[lo:hi]), lo, tags[lo:hi], groups[lo:hi], m, distinct, kk))

        def merge_gathered(g, row0, b, kk, distinct=False):
            ids, sc = D.merge(g.numpy(), row0, b, kk, distinct)
            return torch.from_numpy(ids), torch.from_numpy(sc)

        s = M.scores(q[mine], bank)
        q_local = torch.from_numpy(q[mine])
        m_local = torch.from_numpy(np.ascontiguousarray(masks[mine]).view(np.int64))  # differ per query and per rank
        kw = dict(local_topk_packed=local_topk_packed, merge_gathered=merge_gathered)
        ok = True
        ids, _ = mdist.sharded_topk(q_local, k, None, None, distinct=True, **kw)
        ok &= calls == [(b_local, 64), (world * b_local, k, 2)]
        ok &= bool((ids.numpy() == L.labelled_topk(s, tags, groups, L.NO_FILTER, True, k)[0]).all())
        for distinct in (True, False):
            del calls[:]
            ids, _ = mdist.sharded_topk(q_local, k, None, None, masks_local=m_local, distinct=distinct, **kw)
            ok &= calls == [(b_local, 64), (b_local, 3), (world * b_local, k, 2)]
            ok &= bool((ids.numpy() == L.labelled_topk(s, tags, groups, masks[mine], distinct, k)[0]).all())
        ret[rank] = ok
    finally:
        dist.destroy_process_group()


def test_sharded_topk_labelled_gloo():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert all(ret.get(r) for r in range(world))
