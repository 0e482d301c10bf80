"""JPEG decode on the GPU: baseline, and progressive on request (csrc/jpeg.hip, csrc/jpeg_prog.hip).

The reference decodes every frame on the host (mtgvision/server.py:272-280: cv2.imdecode(..., IMREAD_COLOR_RGB)) and
reads card scans from JPEG files for the bank build (qdrant_populate.py:70-90).  Here the compressed bytes go to the
device in one copy per batch and are decoded there:

    dec = JpegDecoder(max_images=32, max_bytes=4 << 20, max_pixels=32 * 640 * 480)
    frames = dec.decode_frames(list_of_jpeg_bytes)          # (n, 640, 640, 3) uint8, letterboxed, on the GPU; input_hw=(480, 640): (n, 480, 640, 3)
    buf, offsets, hw, status = dec.decode(list_of_jpeg_bytes)  # ragged RGB, the layout mtgv_make_cropped takes
    src = dec.decode_sources(list_of_jpeg_bytes)            # both: mtgv.pipeline.SourceFrames - Pipeline.run(src) crops the cards from the camera's pixels

Supported: baseline / extended sequential Huffman 8-bit (SOF0 / SOF1), greyscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0,
restart intervals.  The output equals libjpeg-turbo's default decode (Pillow's `Image.open(f).convert("RGB")`).
Anything else raises before a launch; there is no host fallback inside the library - a caller that wants one checks
`jpeg_info(data).supported` itself.

Progressive files (SOF2, Huffman, 8-bit, the same component layouts; what optimising encoders such as mozjpeg write by
default) are opt-in: `jpeg_info(data, progressive=True)`, `JpegDecoder(..., progressive=True)`,
`JpegFrames(..., progressive=True)`.  Such a decoder takes batches that mix baseline and progressive files, with the same
exact output; the bank-build helpers (mtgv.bank.make_cropped_jpeg / build_bank_jpeg) create theirs that way.  Refused:
an illegal scan script, arithmetic coding, more scans per batch than `max_scans`, and an incomplete progression (some
coefficient never reaches Al = 0: libjpeg would smooth such a file).  Without the option everything behaves as before.
"""

from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from . import native
from .detector import fit_geometry, letterbox_geometry


class JpegInfo(NamedTuple):
    h: int
    w: int
    components: int
    sampling: int  # 444 / 422 / 420 / 400 (greyscale), 0 other
    restart_interval: int  # MCUs per restart segment, 0 none
    supported: bool
    reason: str  # first unsupported feature ("" when supported)
    progressive: bool = False  # SOF2 (only reported by jpeg_info(..., progressive=True))
    scans: int = 1


def jpeg_info(data: bytes, progressive: bool = False) -> JpegInfo:
    """Header probe on the host (no device needed).  Raises AssertionError for malformed input.  progressive=True: what a
    JpegDecoder(progressive=True) takes - a progressive file inside the subset is supported, with its number of scans."""
    L = native.lib()
    info = (C.c_int32 * 8)()
    buf = C.create_string_buffer(bytes(data), len(data)) if len(data) else None
    if progressive:
        native.check(L.mtgv_jpeg_info_ex(buf, len(data), native.JPEG_PROGRESSIVE, info))
    else:
        native.check(L.mtgv_jpeg_info(buf, len(data), info))
        info[6], info[7] = 0, 1
    sup = bool(info[5])
    reason = "" if sup else (L.mtgv_last_error() or b"").decode("utf-8", "replace")
    return JpegInfo(info[0], info[1], info[2], info[3], info[4], sup, reason, bool(info[6]), info[7])


def _pack(datas: Sequence[bytes]):
    datas = [bytes(d) for d in datas]
    sizes = np.array([len(d) for d in datas], np.int64)
    offs = np.zeros(len(datas), np.int64)
    if len(datas) > 1:
        offs[1:] = np.cumsum(sizes)[:-1]
    blob = np.frombuffer(b"".join(datas), np.uint8) if sizes.sum() else np.zeros(1, np.uint8)
    return np.ascontiguousarray(blob), offs, sizes


def _p(a: np.ndarray):
    return C.c_void_p(a.ctypes.data)


class JpegDecoder:
    """Batched GPU JPEG decoder.  Limits (fixed here, workspace allocated once): max_images per call, max_bytes of
    compressed data per call, max_pixels per call counted after padding each image to whole MCUs (8 or 16 pixels).
    progressive=True: the decoder also takes progressive files, mixed with baseline ones in any batch; max_scans bounds
    the scans of all progressive files of one batch (None: 16 * max_images; Pillow writes 10 per colour file).
    Not thread-safe; calls run on the current stream of `device`."""

    def __init__(self, max_images: int, max_bytes: int, max_pixels: int, device=None, progressive: bool = False, max_scans: int = None):
        native.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_images, self.max_bytes, self.max_pixels = int(max_images), int(max_bytes), int(max_pixels)
        self.progressive = bool(progressive)
        assert max_scans is None or self.progressive, "max_scans needs progressive=True"
        self.max_scans = 0 if max_scans is None else int(max_scans)
        self._h = native.c_vp(0)
        with torch.cuda.device(self.device):
            if self.progressive:
                native.check(native.lib().mtgv_jpeg_decoder_create_ex(self.max_images, self.max_bytes, self.max_pixels, native.JPEG_PROGRESSIVE,
                                                                      self.max_scans, C.byref(self._h)))
            else:
                native.check(native.lib().mtgv_jpeg_decoder_create(self.max_images, self.max_bytes, self.max_pixels, C.byref(self._h)))

    def _infos(self, datas: Sequence[bytes]) -> List[JpegInfo]:
        infos = [jpeg_info(d, self.progressive) for d in datas]
        bad = [(i, f.reason) for i, f in enumerate(infos) if not f.supported]
        if bad:
            raise AssertionError(f"jpeg: unsupported input (no GPU decode; decode these on the host): {bad}")
        return infos

    def _launch(self, datas, dst: torch.Tensor, dst_off: np.ndarray, pitch: np.ndarray) -> torch.Tensor:
        """decode into dst (uint8 device tensor), synchronise, raise on a non-zero status"""
        n = len(datas)
        blob, offs, sizes = _pack(datas)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        dst_off = np.ascontiguousarray(dst_off, np.int64)
        pitch = np.ascontiguousarray(pitch, np.int64)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_jpeg_decode(self._h, _p(blob), _p(offs), _p(sizes), n, native.ptr(dst), _p(dst_off), _p(pitch),
                                                       native.ptr(status), native.stream()))
        return status

    @staticmethod
    def _raise_on_status(status: torch.Tensor) -> None:
        st = status.cpu().numpy()  # synchronises
        failed = np.nonzero(st)[0].tolist()
        if failed:
            raise RuntimeError(f"jpeg: corrupt entropy-coded data in image(s) {failed} of the batch")

    def decode(self, datas: Sequence[bytes], check: bool = True):
        """JPEG files -> (buf (sum h*w*3,) uint8, offsets (n,) int64, hw (n, 2) int32, status (n,) int32), all on the
        device: images back to back in HWC RGB, the ragged layout mtgv_make_cropped takes.  With check (default) the
        call synchronises and raises RuntimeError naming the images whose stream did not decode."""
        infos = self._infos(datas)
        n = len(datas)
        hw = np.array([(f.h, f.w) for f in infos], np.int64).reshape(n, 2)
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offs = np.zeros(n, np.int64)
        if n > 1:
            offs[1:] = np.cumsum(nbytes)[:-1]
        buf = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device=self.device)
        if n == 0:
            z = torch.zeros(0, dtype=torch.int64, device=self.device)
            return buf, z, z.view(0, 2).int(), z.int()
        status = self._launch(datas, buf, offs, hw[:, 1] * 3)
        if check:
            self._raise_on_status(status)
        return buf, torch.from_numpy(offs).to(self.device), torch.from_numpy(hw.astype(np.int32)).to(self.device), status

    @staticmethod
    def images(buf: torch.Tensor, offsets, hw) -> List[torch.Tensor]:
        """per-image (h, w, 3) views of decode()'s buffer"""
        offsets = offsets.cpu().tolist() if torch.is_tensor(offsets) else list(offsets)
        hw = hw.cpu().tolist() if torch.is_tensor(hw) else list(hw)
        return [buf[o : o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offsets, hw)]

    def decode_frames(self, datas: Sequence[bytes], size: int = 640, pad_value: int = 114, out: torch.Tensor = None, check: bool = True,
                      input_hw=None):
        """JPEG frames -> (n, size, size, 3) - with input_hw (n, in_h, in_w, 3) - uint8 letterboxed frames on the GPU
        (mtgv.detector.letterbox_geometry / fit_geometry).  A frame
        that already fits (640x480 webcam frames) is decoded straight into its padded frame through offset and pitch and only
        the pad is filled; any other is decoded to scratch and resampled by mtgv_letterbox_rect_u8.
        input_hw = (in_h, in_w): the input of a rectangular detector (spec.DetectorConfig(input_hw=...)) instead, every frame
        scaled to fit and centred in it (mtgv.detector.fit_geometry) -> (n, in_h, in_w, 3).  A frame of exactly that size (a
        640x480 JPEG into (480, 640)) is decoded straight into the detector's input: no pad pass, no resample."""
        infos = self._infos(datas)
        n = len(datas)
        oh, ow = (size, size) if input_hw is None else (int(input_hw[0]), int(input_hw[1]))
        if out is None:
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=self.device)
        assert out.shape == (n, oh, ow, 3) and out.dtype == torch.uint8 and out.is_contiguous()
        if n == 0:
            return out
        L = native.lib()
        fsz = oh * ow * 3
        geo = [letterbox_geometry(f.h, f.w, size) if input_hw is None else fit_geometry(f.h, f.w, oh, ow) for f in infos]
        direct = [i for i, f in enumerate(infos) if (geo[i][1], geo[i][2]) == (f.h, f.w)]
        other = [i for i in range(n) if (geo[i][1], geo[i][2]) != (infos[i].h, infos[i].w)]
        dst_off = np.zeros(n, np.int64)
        pitch = np.zeros(n, np.int64)
        scratch = None
        if other:
            sz = np.array([infos[i].h * infos[i].w * 3 for i in other], np.int64)
            soff = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
            scratch = torch.empty(int(sz.sum()), dtype=torch.uint8, device=self.device)
        # one decode writes into the frames and the scratch: two destinations, one base pointer -> offsets relative to
        # the lower of the two allocations
        base = out if scratch is None else (out if out.data_ptr() <= scratch.data_ptr() else scratch)
        b0 = base.data_ptr()
        for i in direct:
            _, nh, nw, top, left = geo[i]
            dst_off[i] = out.data_ptr() - b0 + i * fsz + (top * ow + left) * 3
            pitch[i] = ow * 3
        for j, i in enumerate(other):
            dst_off[i] = scratch.data_ptr() - b0 + int(soff[j])
            pitch[i] = infos[i].w * 3
        status = self._launch(datas, base, dst_off, pitch)
        with torch.cuda.device(self.device):
            groups = {}
            for i in direct:
                groups.setdefault(geo[i][1:], []).append(i)
            for (nh, nw, top, left), idx in groups.items():
                if (nh, nw) == (oh, ow):
                    continue  # the frame fills its input: there is no pad
                runs = _runs(idx)
                for a, b in runs:  # consecutive frames of one geometry: one launch
                    native.check(L.mtgv_letterbox_pad_rect_u8(C.c_void_p(out.data_ptr() + a * fsz), b - a, oh, ow, nh, nw, top, left, pad_value,
                                                              native.stream()))
            for j, i in enumerate(other):
                f = infos[i]
                _, nh, nw, top, left = geo[i]
                native.check(L.mtgv_letterbox_rect_u8(C.c_void_p(scratch.data_ptr() + int(soff[j])), 1, f.h, f.w, C.c_void_p(out.data_ptr() + i * fsz),
                                                      oh, ow, nh, nw, top, left, pad_value, native.stream()))
        if scratch is not None:
            scratch.record_stream(torch.cuda.current_stream(self.device))
        if check:
            self._raise_on_status(status)
        self.last_status = status
        return out

    def decode_sources(self, datas: Sequence[bytes], size: int = 640, input_hw=None, pad_value: int = 114, out: torch.Tensor = None,
                       buf: torch.Tensor = None, check: bool = True):
        """JPEG frames -> `mtgv.pipeline.SourceFrames`: the frames at the camera's resolution (`buf`, `offsets`, `hw`: what
        `decode` returns) beside the detector input made from them (`frames`: what `decode_frames` returns, byte for byte).
        One decode into the ragged layout, one letterbox launch for the whole batch whatever the frames' sizes
        (mtgv_letterbox_ragged_u8).  Hand the result to `Pipeline.run` and the cards are cropped from the camera's pixels.
        out: the (n, size, size, 3) / (n, in_h, in_w, 3) tensor for the frames; buf: a uint8 tensor of at least sum h * w * 3
        bytes for the sources (JpegFrames keeps both in its ring)."""
        from .pipeline import SourceFrames

        infos = self._infos(datas)
        n = len(datas)
        hw = np.array([(f.h, f.w) for f in infos], np.int64).reshape(n, 2)
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offs = np.zeros(n, np.int64)
        if n > 1:
            offs[1:] = np.cumsum(nbytes)[:-1]
        total = int(nbytes.sum())
        if buf is None:
            buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        assert buf.dtype == torch.uint8 and buf.ndim == 1 and buf.is_contiguous() and buf.numel() >= total and buf.is_cuda, \
            f"source buffer {tuple(buf.shape)} {buf.dtype} for {total} bytes"
        buf = buf[:total]
        status = self._launch(datas, buf, offs, hw[:, 1] * 3) if n else torch.zeros(0, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            sf = SourceFrames.from_ragged(buf, offs, hw, size, input_hw, pad_value, out)
        if check:
            self._raise_on_status(status)
        self.last_status = status
        return sf

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                native.lib().mtgv_jpeg_decoder_destroy(self._h)
                self._h = native.c_vp(0)
        except Exception:
            pass


def _runs(idx: List[int]):
    """[(start, end)) runs of consecutive integers"""
    out, s = [], None
    for k, i in enumerate(idx):
        if s is None:
            s = i
        if k + 1 == len(idx) or idx[k + 1] != i + 1:
            out.append((s, i + 1))
            s = None
    return out


class JpegFrames:
    """Frame batches that arrive as JPEG bytes (one file per websocket message, mtgvision/server.py:272-280), decoded on
    the GPU into a small ring of letterboxed frame buffers on a stream of their own; the same lease interface as
    mtgv.pipeline.HostFrames, so `Pipeline.run_many(src.leases(n))` consumes them unchanged.

    A lease's `tensor()` makes the consuming stream wait for its decode; `done()` (called by the pipeline after the de-warp)
    lets the buffer be overwritten by the decode `depth` batches later.  The host parse and the staging copy happen when a
    lease is issued (unsupported input raises there); a lease's `status` is its batch's (n,) int32 device status word,
    which the caller reads once the pipeline's outputs are synchronised (reading it earlier would stall the overlap)."""

    def __init__(self, jpeg_batches: Sequence[Sequence[bytes]], device, size: int = 640, pad_value: int = 114, depth: int = 3,
                 decoder: JpegDecoder = None, input_hw=None, progressive: bool = False, keep_source: bool = False):
        """input_hw = (in_h, in_w): buffers of a rectangular detector's input (JpegDecoder.decode_frames);
        progressive: the decoder created here also takes progressive frames (a `decoder` passed in is used as given);
        keep_source: the ring also holds every batch's frames at the camera's resolution (JpegDecoder.decode_sources; the
        buffers are sized here from the largest batch, like the decoder) and a lease has `sources()`, which Pipeline.run /
        run_many pick up: the cards are cropped from the camera's pixels.  `tensor()` still returns the frames."""
        assert depth >= 2 and len(jpeg_batches) > 0
        self.batches = [list(b) for b in jpeg_batches]
        self.device = torch.device(device)
        self.size, self.pad_value, self.depth = size, pad_value, depth
        self.input_hw = None if input_hw is None else (int(input_hw[0]), int(input_hw[1]))
        oh, ow = (size, size) if self.input_hw is None else self.input_hw
        n = max(len(b) for b in self.batches)
        self.keep_source = bool(keep_source)
        infos = None
        if decoder is None or self.keep_source:
            infos = [[jpeg_info(d, progressive or getattr(decoder, "progressive", False)) for d in b] for b in self.batches]
        if decoder is None:
            nbytes = max(sum(len(d) for d in b) for b in self.batches)
            pix = max(sum(_padded_pixels(f) for f in b) for b in infos)
            scans = max(sum(f.scans for f in b if f.progressive) for b in infos) if progressive else None
            decoder = JpegDecoder(n, nbytes, pix, self.device, progressive=progressive, max_scans=max(scans, 1) if progressive else None)
        self.dec = decoder
        self.s_dec = torch.cuda.Stream(self.device)
        self.bufs = [torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=self.device) for _ in range(depth)]
        self.src_bufs = None
        if self.keep_source:
            src_bytes = max(sum(f.h * f.w * 3 for f in b) for b in infos)
            self.src_bufs = [torch.empty(max(src_bytes, 1), dtype=torch.uint8, device=self.device) for _ in range(depth)]
        self.decoded = [torch.cuda.Event() for _ in range(depth)]
        self.released = [None] * depth
        self._issued = 0

    class _Lease:
        def __init__(self, src, slot, n, status):
            self.src, self.slot, self.n, self.status = src, slot, n, status

        def tensor(self) -> torch.Tensor:
            torch.cuda.current_stream(self.src.device).wait_event(self.src.decoded[self.slot])
            return self.src.bufs[self.slot][: self.n]

        def done(self) -> None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.src.device))
            self.src.released[self.slot] = ev

    class _SourceLease(_Lease):
        """a lease of JpegFrames(keep_source=True): `sources()` is the batch's SourceFrames (its `frames` are `tensor()`),
        `done()` releases the frame buffer and the source buffer together"""

        def __init__(self, src, slot, n, status, sf):
            super().__init__(src, slot, n, status)
            self._sf = sf

        def sources(self):
            cur = torch.cuda.current_stream(self.src.device)
            cur.wait_event(self.src.decoded[self.slot])
            for t in (self._sf.offsets, self._sf.hw, self._sf.geo, self._sf.ratio):  # allocated on the decode stream
                t.record_stream(cur)
            return self._sf

    def _issue(self, batch_index: int):
        j = self._issued % self.depth
        datas = self.batches[batch_index % len(self.batches)]
        self._issued += 1
        with torch.cuda.stream(self.s_dec):
            if self.released[j] is not None:
                self.s_dec.wait_event(self.released[j])  # the batch that used this buffer has been de-warped
            n = len(datas)
            sf = None
            if self.keep_source:
                sf = self.dec.decode_sources(datas, self.size, self.input_hw, self.pad_value, out=self.bufs[j][:n], buf=self.src_bufs[j], check=False)
            else:
                self.dec.decode_frames(datas, self.size, self.pad_value, out=self.bufs[j][:n], check=False, input_hw=self.input_hw)
            status = self.dec.last_status
            self.decoded[j].record(self.s_dec)
        return JpegFrames._SourceLease(self, j, n, status, sf) if self.keep_source else JpegFrames._Lease(self, j, n, status)

    def leases(self, n: int):
        """n leases of batches 0, 1, ... (cyclically), decodes one to two batches ahead of their consumer (HostFrames.leases)"""
        ahead = [self._issue(b) for b in range(min(n, self.depth - 1))]
        issued = len(ahead)
        for i in range(n):
            if i > 0 and issued < n:
                ahead.append(self._issue(issued))
                issued += 1
            yield ahead.pop(0)


def _padded_pixels(f: JpegInfo) -> int:
    m = 16 if f.sampling == 420 else 8
    mx = 16 if f.sampling in (420, 422) else 8
    return -(-f.h // m) * m * (-(-f.w // mx) * mx)


# ---------------------------------------------------------------------------------------------------------------------
# encode (csrc/jpeg_enc.hip)

SAMPLINGS = (420, 444)


def jpeg_encode_bound(h: int, w: int, sampling: int = 420) -> int:
    """worst-case file size in bytes of one h x w image (host only, no device needed)"""
    n = C.c_int64(0)
    native.check(native.lib().mtgv_jpeg_encode_bound(int(h), int(w), int(sampling), C.byref(n)))
    return n.value


def jpeg_header(h: int, w: int, quality: int = 50, sampling: int = 420) -> bytes:
    """the bytes from SOI through SOS exactly as the encoder writes them (host only)"""
    buf = (C.c_uint8 * 1024)()
    n = C.c_int64(0)
    native.check(native.lib().mtgv_jpeg_encode_header(int(h), int(w), int(quality), int(sampling), buf, len(buf), C.byref(n)))
    return bytes(buf[: n.value])


class JpegEncoder:
    """Batched GPU JPEG encoder: (N, H, W, 3) RGB uint8 -> N baseline JPEG files, byte for byte what Pillow (libjpeg-turbo)
    writes with `Image.save(f, "JPEG", quality=q, subsampling=2 / 0)` for sampling 420 / 444.

        enc = JpegEncoder(max_images=256, max_pixels=256 * 192 * 128)
        buf, offsets = enc.encode_device(crops)       # packed files + (N + 1,) int64 offsets, on the device, no sync
        files = enc.encode(crops)                     # list of bytes: one synchronisation, two copies

    Limits (fixed here, workspace allocated once): max_images per call, max_pixels per call counted after padding each
    image to whole MCUs (multiples of 16 for 4:2:0, 8 for 4:4:4).  Not thread-safe; calls run on the current stream of
    `device` and launch library kernels only."""

    def __init__(self, max_images: int, max_pixels: int, device=None):
        native.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_images, self.max_pixels = int(max_images), int(max_pixels)
        self._h = native.c_vp(0)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_jpeg_encoder_create(self.max_images, self.max_pixels, C.byref(self._h)))

    def encode_device(self, images: torch.Tensor, quality: int = 50, sampling: int = 420, out: torch.Tensor = None):
        """(N, H, W, 3) uint8 device tensor -> (buf, offsets): file i is buf[offsets[i]:offsets[i + 1]].  buf holds
        N * jpeg_encode_bound(H, W, sampling) bytes (or is `out`, at least that large); both stay on the device and
        the call does not synchronise."""
        assert images.dim() == 4 and images.shape[-1] == 3 and images.dtype == torch.uint8, (tuple(images.shape), images.dtype)
        assert images.device == self.device, (images.device, self.device)
        images = images.contiguous()
        n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
        cap = n * jpeg_encode_bound(h, w, sampling) if n else 0
        if out is None:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.device == self.device and out.is_contiguous()
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().mtgv_jpeg_encode(self._h, native.ptr(images), n, h, w, int(quality), int(sampling), native.ptr(out),
                                                       out.numel(), native.ptr(offsets), native.stream()))
        return out, offsets

    def encode(self, images: torch.Tensor, quality: int = 50, sampling: int = 420) -> List[bytes]:
        """(N, H, W, 3) uint8 device tensor -> N JPEG files on the host"""
        buf, offsets = self.encode_device(images, quality, sampling)
        return split_files(buf, offsets)

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                native.lib().mtgv_jpeg_encoder_destroy(self._h)
                self._h = native.c_vp(0)
        except Exception:
            pass


def split_files(buf: torch.Tensor, offsets: torch.Tensor) -> List[bytes]:
    """encode_device's (buf, offsets) -> list of bytes: the offsets first (this synchronises), then the used part of buf"""
    off = offsets.cpu().numpy()
    data = buf[: int(off[-1])].cpu().numpy().tobytes()
    return [data[int(off[i]) : int(off[i + 1])] for i in range(len(off) - 1)]
