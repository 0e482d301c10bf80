"""Shared by test_source_frames_cpu.py and test_gpu_source_frames.py: numpy restatements of what the source-frame path
computes (the quad mapping of mtgv_warp_quads_src, the ragged layout) and the frames the tests use.  No GPU needed here."""
import re

import numpy as np

from mtgv.detector import fit_geometry


def declared(header_path):
    """the symbols include/mtgv.h declares (test_abi_cpu.py's rule)"""
    src = open(header_path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"MTGV_API\s+[\w\s\*]+?\b(mtgv_\w+)\s*\(", src)))


def map_quads(quads, frame_idx, hw, input_hw):
    """(nq, 4, 2) float32 corners in the pixels of the detector's (in_h, in_w) input -> float32 corners in the pixels of each
    quad's own (h, w) frame: one Python float (float64) operation after the other, x = (x_det - left) / ratio clipped to
    [0, w], y = (y_det - top) / ratio clipped to [0, h], then rounded to float32"""
    quads = np.asarray(quads, np.float32)
    out = np.empty(quads.shape, np.float32)
    for q in range(quads.shape[0]):
        h, w = (int(v) for v in hw[int(frame_idx[q])])
        ratio, _, _, top, left = fit_geometry(h, w, int(input_hw[0]), int(input_hw[1]))
        for i in range(4):
            x = (float(quads[q, i, 0]) - float(left)) / float(ratio)
            y = (float(quads[q, i, 1]) - float(top)) / float(ratio)
            x = 0.0 if x < 0.0 else (float(w) if x > float(w) else x)
            y = 0.0 if y < 0.0 else (float(h) if y > float(h) else y)
            out[q, i, 0], out[q, i, 1] = np.float32(x), np.float32(y)
    return out


def ragged(frames):
    """list of (h, w, 3) uint8 arrays -> (bytes back to back, offsets (n,) int64, hw (n, 2) int64)"""
    hw = np.array([f.shape[:2] for f in frames], np.int64).reshape(len(frames), 2)
    nbytes = hw[:, 0] * hw[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in frames]), offsets, hw


def noise_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def bits(a):
    """float32 array -> its bit patterns (bit-for-bit comparisons: -0.0 != 0.0, NaN == the same NaN)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
