"""Bank build + persistence.

Reference dataflow (mtgvision/qdrant_populate.py:70-90, four worker processes, encoder batch = 1):
    retrieve existing ids -> for each missing card: download -> imread -> make_cropped(size_hw=encoder.input_hwc)
    -> encoder.predict -> QdrantPoint(id, vector) -> save_points.
Here the same steps run per batch on the GPU: one ragged `make_cropped` launch, one batched encoder forward,
one append to the device-resident bank.  Downloading stays with the caller; images arrive as arrays (`make_cropped`,
`build_bank`) or as JPEG files decoded on the GPU (`make_cropped_jpeg`, `build_bank_jpeg`, mtgv.jpeg).
"""

from __future__ import annotations

import json
import os
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import native
from .adapters import QdrantPoint, VectorStoreQdrant
from .encoder import Encoder


def make_cropped(images: Sequence[np.ndarray], size_hw=(192, 128), device=None) -> torch.Tensor:
    """list of uint8 HWC card images (any sizes) -> (n, h, w, 3) float32 in [0,1] on the GPU
    (SyntheticBgFgMtgImages.make_cropped, encoder_datasets.py:733-753)."""
    native.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = len(images)
    oh, ow = size_hw
    out = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    flat, offs, hw, pos = [], [], [], 0
    for im in images:
        im = np.asarray(im)
        assert im.ndim == 3 and im.shape[-1] == 3 and im.dtype == np.uint8, f"{im.shape} {im.dtype}"
        flat.append(np.ascontiguousarray(im).reshape(-1))
        offs.append(pos)
        hw.append(im.shape[:2])
        pos += im.size
    buf = torch.from_numpy(np.concatenate(flat)).to(dev)
    offs_t = torch.tensor(offs, dtype=torch.int64, device=dev)
    hw_t = torch.tensor(hw, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        native.check(native.lib().mtgv_make_cropped(native.ptr(buf), native.ptr(offs_t), native.ptr(hw_t), n, oh, ow, native.ptr(out), native.stream()))
    return out


def make_cropped_jpeg(datas: Sequence[bytes], size_hw=(192, 128), device=None, decoder=None) -> torch.Tensor:
    """list of JPEG card scans -> (n, h, w, 3) float32 in [0,1] on the GPU: one batched GPU decode into the ragged layout,
    then the same make_cropped launch.  Baseline and progressive files, in any mix (a `decoder` passed in is used as
    given).  Unsupported or corrupt files raise (mtgv.jpeg.JpegDecoder)."""
    from .jpeg import JpegDecoder, _padded_pixels, jpeg_info

    native.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = len(datas)
    oh, ow = size_hw
    out = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if decoder is None:
        infos = [jpeg_info(d, progressive=True) for d in datas]
        decoder = JpegDecoder(n, sum(len(d) for d in datas), sum(_padded_pixels(f) for f in infos), dev, progressive=True,
                              max_scans=max(1, sum(f.scans for f in infos if f.progressive)))
    buf, offs_t, hw_t, _ = decoder.decode(datas)
    with torch.cuda.device(dev):
        native.check(native.lib().mtgv_make_cropped(native.ptr(buf), native.ptr(offs_t), native.ptr(hw_t), n, oh, ow, native.ptr(out), native.stream()))
    return out


def build_bank_jpeg(cards: Iterable[Tuple[str, bytes]], encoder: Encoder, store: VectorStoreQdrant, batch_size: int = 256) -> int:
    """build_bank over (id, JPEG bytes) pairs: each batch is decoded on the GPU (make_cropped_jpeg), baseline and progressive
    files alike - downloaded card scans are routinely progressive.  Returns the number of cards added."""
    from .jpeg import JpegDecoder, _padded_pixels, jpeg_info

    h, w, _ = encoder.input_hwc
    added = 0
    batch: List[Tuple[str, bytes]] = []
    dec = None

    def flush():
        nonlocal added, batch, dec
        if not batch:
            return
        existing = {p.id for p in store.retrieve((cid for cid, _ in batch), with_payload=False)}
        todo = [(cid, d) for cid, d in batch if str(cid) not in existing]
        batch = []
        if not todo:
            return
        datas = [d for _, d in todo]
        infos = [jpeg_info(d, progressive=True) for d in datas]
        nb, pix = sum(len(d) for d in datas), sum(_padded_pixels(f) for f in infos)
        scans = sum(f.scans for f in infos if f.progressive)
        if dec is None or dec.max_images < len(datas) or dec.max_bytes < nb or dec.max_pixels < pix or dec.max_scans < scans:
            dec = JpegDecoder(batch_size, max(nb, dec.max_bytes if dec else 0), max(pix, dec.max_pixels if dec else 0), encoder.device,
                              progressive=True, max_scans=max(scans, 16 * batch_size, dec.max_scans if dec else 0))
        x = make_cropped_jpeg(datas, (h, w), encoder.device, dec)
        z = encoder.encode(x).cpu().numpy()
        store.save_points(QdrantPoint(id=str(cid), vector=zi, payload=None) for (cid, _), zi in zip(todo, z))
        added += len(todo)

    for item in cards:
        batch.append(item)
        if len(batch) >= batch_size:
            flush()
    flush()
    return added


def build_bank(cards: Iterable[Tuple[str, np.ndarray]], encoder: Encoder, store: VectorStoreQdrant, batch_size: int = 256) -> int:
    """cards: (id, uint8 HWC image) pairs.  Embeds every card whose id is not in the store yet and upserts it.
    Returns the number of cards added (CardProcessor.process_batch returns the same count)."""
    h, w, _ = encoder.input_hwc
    added = 0
    batch: List[Tuple[str, np.ndarray]] = []

    def flush():
        nonlocal added, batch
        if not batch:
            return
        existing = {p.id for p in store.retrieve((cid for cid, _ in batch), with_payload=False)}
        todo = [(cid, im) for cid, im in batch if str(cid) not in existing]
        batch = []
        if not todo:
            return
        x = make_cropped([im for _, im in todo], (h, w), encoder.device)
        z = encoder.encode(x).cpu().numpy()
        store.save_points(QdrantPoint(id=str(cid), vector=zi, payload=None) for (cid, _), zi in zip(todo, z))
        added += len(todo)

    for item in cards:
        batch.append(item)
        if len(batch) >= batch_size:
            flush()
    flush()
    return added


def save_store(store: VectorStoreQdrant, path: str) -> None:
    """On-disk bank: <path>.npz (ids as fixed-width strings + float32 matrix of the stored, normalised vectors)
    and <path>.payload.json.  A store whose rows were labelled (`set_labels` / `group_by_payload`) also writes their
    `tags` (uint64) and `groups` (int32) arrays; an unlabelled store writes the same file as before."""
    n = len(store._ids)
    vecs = store._bank.rows(0, n) if n else np.zeros((0, store._VECTOR_SIZE), np.float32)
    arrays = dict(ids=np.asarray(store._ids, dtype=np.str_), vectors=vecs)
    if n and store._bank.labelled:
        arrays["tags"], arrays["groups"] = store._bank.labels(0, n)
    np.savez(path + ".npz", **arrays)
    with open(path + ".payload.json", "w") as f:
        json.dump({k: v for k, v in store._payload.items()}, f)


def load_store(path: str, capacity: int = 131072) -> VectorStoreQdrant:
    d = np.load(path + ".npz", allow_pickle=False)
    ids, vecs = [str(i) for i in d["ids"]], d["vectors"]
    store = VectorStoreQdrant(capacity=max(capacity, len(ids)))
    payload = {}
    if os.path.exists(path + ".payload.json"):
        payload = json.load(open(path + ".payload.json"))
    for s in range(0, len(ids), 4096):
        store.save_points(QdrantPoint(id=i, vector=v, payload=payload.get(i)) for i, v in zip(ids[s : s + 4096], vecs[s : s + 4096]))
    if "tags" in d.files and len(ids):  # ids are unique in a saved store: row r holds ids[r]
        store._bank.set_labels(0, d["tags"], d["groups"])
    return store
