#!/usr/bin/env python3
"""Headline benchmark: cards/sec end to end (detect + crop + embed + top-1 over a 100k x 768 bank).

    python bench.py [--gpus N --steps K --warmup W]      (N > 1 from a plain shell: starts the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --full                               (also the unsettled, sustained, one-stream and host-to-device
                                                          figures, the roofline passes and the CPU baseline)
    python bench.py --dump-outputs DIR                   (rank 0's last timed step as DIR/<name>.npy)

A plain run sets up, settles and warms up, times K steps and prints the headline figure; everything else it can measure
sits behind --full.

One "step" = one pass of the whole hot path over one batch of synthetic frames resident in HBM:
per GPU 32 frames (640x640x3 uint8) -> YOLOv8n-seg detect + NMS + mask logits -> for the 8 best detections
per frame the oriented quadrilateral fitted to the detection's mask (--quads mask, the default: the
reference's dataflow, od_export.py:52-111; --quads box crops the boxes) de-warped to 192x128 crops ->
ConvNeXt-V2 (AE-tiny, z=768) embeddings -> cosine top-1 over the bank.  Weak scaling: per-GPU frames are fixed, the bank is sharded by rows over the ranks and the
per-shard top-k are all-gathered over RCCL/xGMI and merged.  Rank 0 prints ONE JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mtg-vision_amd")]

import numpy as np
import torch
import torch.distributed as dist

# /opt/skills/guides/MI355X_MICROARCH.md: dense MFMA peaks (f32-input; f16-input) and the HBM3E rate
PEAK_MFMA_TFLOPS = {"f32": 157.3, "f16x3": 2500.0}
MFMA_FLOPS_PER_FLOP = {"f32": 1, "f16x3": 3}  # f16x3 issues three fp16 MFMAs per algorithmic product
PEAK_HBM_GBS = 8000.0


def group_launches(recs, nprof, precision):
    """Per-group roofline view of the GEMM launches of one step (records of mtgv_profile_gemm_dump over nprof passes).
    Groups: pwconv1 (1x1 + activation + GRN partials), pwconv2 (GRN-scaled 1x1 + residual), bank (scores + top-k),
    det3x3 / det1x1 (detector convolutions), enc_other (stem, downsample, head)."""
    peak = PEAK_MFMA_TFLOPS[precision]
    mult = MFMA_FLOPS_PER_FLOP[precision]
    per = max(1, len(recs) // nprof)
    # launch order inside one pass: detector, then the encoder (whose first launch is the 4x4 stem), then the bank
    enc_start = min((i for i, r in enumerate(recs[:per]) if int(r["KH"]) == 4 or int(r["grn"])), default=per)
    out = {}
    for i, r in enumerate(recs):
        j = i % per
        if int(r["topk"]) > 0:
            g = "bank"
        elif int(r["grn"]):
            g = "pwconv1"
        elif int(r["apro"]):
            g = "pwconv2"
        elif j < enc_start:
            g = "det3x3" if int(r["KH"]) == 3 else "det1x1"
        else:
            g = "enc_other"
        d = out.setdefault(g, {"launches": 0, "ms": 0.0, "flop": 0.0, "issued": 0.0, "bytes": 0.0, "fill": 0.0})
        d["launches"] += 1
        d["ms"] += float(r["ms"])
        fl = 2.0 * int(r["M"]) * int(r["N"]) * int(r["K"]) * int(r["batch"]) + float(r.get("xflops", 0) or 0)  # (+ a chained second layer)
        d["flop"] += fl
        # MFMA FLOPs issued per algorithmic FLOP: 3 for the split products, 1 for f32 operands and for the fp16 first
        # pass of the two-pass bank match (sp = 3), 6 for the fused MLP's output pass (sp = 2 with a GRN-scaled A:
        # GEMM1 is computed again, so 2 x 3 products for the pwconv2 FLOPs it is credited with)
        sp = int(r.get("sp", 0) or 0)
        d["issued"] += fl * (1 if sp == 3 else (2 * mult if sp == 2 and int(r["apro"]) else mult))
        d["bytes"] += float(r.get("bytes", 0) or 0)
        d["fill"] += float(r.get("fill", 0) or 0)
    res = {}
    for g, d in out.items():
        sec = d["ms"] * 1e-3
        tf = d["flop"] / sec / 1e12 if sec > 0 else 0.0
        res[g] = {
            "launches_per_step": d["launches"] // nprof,
            "ms_per_step": round(d["ms"] / nprof, 3),
            "algorithmic_tflops": round(tf, 1),
            "issued_mfma_frac": round(d["issued"] / sec / 1e12 / peak, 4) if sec > 0 else 0.0,
            "issued_gflop_per_step": round(d["issued"] / nprof / 1e9, 2),
            "compulsory_gbs": round(d["bytes"] / sec / 1e9, 1) if sec > 0 else 0.0,
            "hbm_frac": round(d["bytes"] / sec / 1e9 / PEAK_HBM_GBS, 4) if sec > 0 else 0.0,
            # what the tiles of the group pull through L2 into LDS (every tile its A and B panels), per second
            "lds_fill_tbs": round(d["fill"] / sec / 1e12, 2) if sec > 0 else 0.0,
        }
    return res


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(step_out, out_dir, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: what one step hands a caller of Pipeline.run (ids, scores, n_det, boxes, crops, z and the detector's
    tensors as det_<name>) written as out_dir/<name>.npy, floating point as float32 (float64 kept), integers as float64
    (exact).  Every array gets an equal share of what the smaller ones leave of `limit`; one larger than its share keeps a
    fixed, seeded sample of its rows (sorted), listed in out_dir/<name>_rows.npy.  Returns {name: shape written}."""
    flat = {}
    for k, v in step_out.items():
        if isinstance(v, dict):
            flat.update({f"{k}_{kk}": vv for kk, vv in v.items() if vv is not None})
        elif v is not None:
            flat[k] = v
    host = {}
    for k, t in flat.items():
        x = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        host[k] = x.astype(np.float64 if x.dtype == np.float64 or (x.dtype.kind in "iu" and x.dtype.itemsize > 2) else np.float32)
    os.makedirs(out_dir, exist_ok=True)
    left, written = limit - 2 * 128 * len(host), {}  # (an .npy header is 128 bytes)
    order = sorted(host, key=lambda k: (host[k].nbytes, k))
    for i, k in enumerate(order):
        x = host[k]
        share = left // (len(order) - i)
        if x.nbytes > share:
            # rows along the first axis; single elements where even one row would take half the share
            rows = x.reshape(len(x), -1) if x.ndim > 1 and x[0].nbytes * 2 <= share else x.reshape(-1, 1)
            n = min(len(rows), max(1, share // (rows[0].nbytes + 8)))
            sel = np.sort(np.random.default_rng(0).choice(len(rows), n, replace=False))
            x = x[sel] if len(rows) == len(x) else x.reshape(-1)[sel]
            np.save(os.path.join(out_dir, f"{k}_rows.npy"), sel.astype(np.float64))
            left -= sel.size * 8
        np.save(os.path.join(out_dir, f"{k}.npy"), x)
        left -= x.nbytes
        written[k] = tuple(x.shape)
    return written


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32, help="frames per GPU per step")
    ap.add_argument("--cards", type=int, default=8, help="cards per frame (K)")
    ap.add_argument("--encoder", default="cnvnxt2ae_tiny", help="cnvnxt2ae_tiny | cnvnxt2ae_nano | ...")
    ap.add_argument("--detector", default="yolov8n-seg", choices=["yolov8n-seg", "yolo11n-seg"],
                    help="yolov8n-seg (BASELINE.json) or yolo11n-seg (the family the reference trains by default, od_train.py:20)")
    ap.add_argument("--bank", type=int, default=100_000)
    ap.add_argument("--bank-mode", default="sharded", choices=["sharded", "replicated"])
    ap.add_argument("--quads", default="mask", choices=["box", "mask"], help="mask (default): crop the oriented quadrilateral fitted to each "
                    "detection's mask on the GPU, the reference's dataflow (od_export.py:52-111); box: crop the axis-aligned detection "
                    "boxes (SURVEY 8d config 4 permits them)")
    ap.add_argument("--precision", default=None, choices=["f32", "f16x3"], help="GEMM operand precision (default: library default / MTGV_GEMM_PREC)")
    ap.add_argument("--no-overlap", action="store_true", help="one stream: detect(i) -> embed(i) strictly in sequence")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-f32-roofline", action="store_true", help="skip the extra profiled passes in the f32 operand mode")
    ap.add_argument("--no-one-stream", action="store_true", help="skip the second timed region (the same steps on one stream)")
    ap.add_argument("--settle-steps", type=int, default=160, help="untimed steady load before the warm-up steps (a step count, the same on "
                    "every rank: the sharded match is a collective): a freshly leased GPU can run its first few hundred milliseconds of "
                    "work below its sustained clocks (one box of round 3 timed a 0.2 s region 10 %% slower as the first process than "
                    "the same command a minute later)")
    ap.add_argument("--cpu-frames", type=int, default=16, help="frames in the bounded CPU-baseline sample")
    ap.add_argument("--sustained-seconds", type=float, default=2.0, help="config.sustained_value: the same step loop run for at least this "
                    "long after the timed region (0: skip)")
    ap.add_argument("--no-h2d", action="store_true", help="skip config.with_h2d_value (frames arriving in pinned host memory)")
    ap.add_argument("--full", action="store_true", help="besides `value`: config.unsettled_value, the sustained, one-stream and "
                    "host-to-device figures, the roofline passes and the CPU baseline (each still subject to its --no-* switch "
                    "above); a plain run times the K steps of `value` only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what rank 0's last timed "
                    "step returned (ids, scores, boxes, crops, embeddings, detector tensors) as DIR/<name>.npy, float32 / float64, "
                    "at most 64 MB in all (larger arrays as a seeded sample of rows)")
    return ap.parse_args()


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` from a plain shell: start the N ranks as a child `torch.distributed.run`, relay rank 0's
    JSON line and return the child's exit code.  This parent never touches the GPU (no HIP call before or after)."""
    import socket
    import subprocess

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout:
        if ln.startswith("{"):
            line = ln.rstrip("\n")
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    return rc if rc != 0 or line is not None else 1


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(launch_ranks(a.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: the launcher and the flag disagree")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the recognition path has no CPU fallback")
    # rehearsal on a one-GPU box: MTGV_SHARE_GPU=1 maps every rank to device 0 and MTGV_DIST_BACKEND=gloo
    # replaces RCCL (which refuses two ranks on one device); the driver's real runs use neither
    share = os.environ.get("MTGV_SHARE_GPU") == "1"
    backend = os.environ.get("MTGV_DIST_BACKEND", "nccl")
    dev_index = 0 if share else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    # MTGV_FORCE_COLLECTIVE=1 under torch.distributed.run --nproc-per-node 1: the sharded match path with its RCCL
    # all-gathers runs with one rank (rehearsal of the multi-GPU code on a one-GPU box)
    force_coll = os.environ.get("MTGV_FORCE_COLLECTIVE") == "1" and "RANK" in os.environ
    if world > 1 or force_coll:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            try:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            except TypeError:  # older signature without device_id
                dist.init_process_group("nccl", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from mtgv import dist as mdist
    from mtgv import native, spec
    from mtgv.detector import Detector
    from mtgv.encoder import Encoder
    from mtgv.matcher import Matcher, merge_gathered, merge_topk
    from mtgv.pipeline import Pipeline

    if a.precision:
        native.set_gemm_precision(a.precision)
    precision = native.get_gemm_precision()
    F, K = a.frames, a.cards
    det_cfg = spec.yolo11_config() if a.detector == "yolo11n-seg" else spec.DetectorConfig()
    enc_cfg = spec.encoder_config(a.encoder, (192, 128), "conv+linear")
    det_sd = spec.random_detector_state(det_cfg, 3)
    enc_sd = spec.random_encoder_state(enc_cfg, 1)
    detector = Detector(det_cfg, det_sd, max_batch=F)
    encoder = Encoder(enc_cfg, enc_sd, max_batch=F * K)

    # bank: rng(2) standard normal, generated in row blocks so that every rank can build just its shard
    sharded = (world > 1 or force_coll) and a.bank_mode == "sharded"
    lo, hi = mdist.shard_rows(a.bank, rank, world) if sharded else (0, a.bank)
    matcher = Matcher(768, capacity=hi - lo, id_base=lo)
    blk = 12_500
    for b0 in range(0, a.bank, blk):
        b1 = min(a.bank, b0 + blk)
        if b1 <= lo or b0 >= hi:
            continue
        rows = np.random.default_rng([2, b0 // blk]).standard_normal((b1 - b0, 768), dtype=np.float32)
        matcher.add(rows[max(lo, b0) - b0 : min(hi, b1) - b0])
    assert len(matcher) == hi - lo

    if sharded:
        # the exchange in its lean form: the local top-k writes the (id, score bits) message itself and the merge reads the
        # gathered buffer in place, so between them the stream sees only RCCL's two all-gathers (no PyTorch arithmetic:
        # the step may share the GPU with the other stream's f16x3 GEMMs, include/mtgv.h)
        if backend == "nccl":
            match_fn = lambda z, k: mdist.sharded_topk(z, k, matcher.match, merge_topk,  # noqa: E731
                                                       local_topk_packed=matcher.match_packed, merge_gathered=merge_gathered)
        else:  # gloo rehearsal (two ranks on one GPU): the same calls, collectives on host copies (memcpys, no kernels)
            def match_fn(z, k):
                loc = lambda q, kk: matcher.match_packed(q.to(dev), kk).cpu()  # noqa: E731
                mrg = lambda gth, row0, b, kk: merge_gathered(gth.to(dev), row0, b, kk)  # noqa: E731
                return mdist.sharded_topk(z.cpu(), k, None, None, local_topk_packed=loc, merge_gathered=mrg)
    else:
        match_fn = None
    pipe = Pipeline(detector, encoder, matcher, K, 1, match_fn, quad_source=a.quads)

    # NB distinct synthetic batches rotate through the steps (a single 39 MB batch would stay in the Infinity Cache)
    NB = 4
    g = torch.Generator(device=dev).manual_seed(4 + rank)
    batches = [torch.randint(0, 256, (F, 640, 640, 3), generator=g, device=dev, dtype=torch.uint8) for _ in range(NB)]
    frames = batches[0]

    def barrier():
        if world > 1 or force_coll:
            dist.barrier()
        torch.cuda.synchronize()

    # every step is one full pass over one batch; with overlap (default) the detect stage of step i+1 runs on a
    # second HIP stream beside the embed/match stages of step i - all K steps start and finish inside the timed region
    # (opt-in in the library; the bench, which runs only this library's kernels, enables it unless --no-overlap)
    if not a.no_overlap:
        os.environ.setdefault("MTGV_OVERLAP", "on")
    overlap = (not a.no_overlap) and pipe.overlap_enabled()

    def run_steps(k):
        seq = [batches[i % NB] for i in range(k)]
        if not overlap:
            return [pipe.run(fr) for fr in seq]
        return pipe.run_many(seq)

    def timed(fn):
        """barrier + synchronize on both sides, MAX over ranks: seconds"""
        barrier()
        t_ = time.perf_counter()
        r_ = fn()
        barrier()
        d_ = time.perf_counter() - t_
        if world > 1 or force_coll:
            tt = torch.tensor([d_], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            d_ = float(tt.item())
        return d_, r_

    # --full: the contract's measurement exactly as written, first thing in the process - W warm-up steps, then K timed
    # steps - reported as config.unsettled_value; `value` is the same measurement after the settle phase below
    dt_cold = None
    if a.full:
        run_steps(a.warmup)
        dt_cold, _ = timed(lambda: run_steps(a.steps))

    # untimed: bring the freshly leased GPU to its sustained state, then the W warm-up steps the contract asks for
    t_settle = time.perf_counter()
    for _ in range(0, a.settle_steps, 8):
        run_steps(8)
        torch.cuda.synchronize()
    t_settle = time.perf_counter() - t_settle
    run_steps(a.warmup)
    dt, out = timed(lambda: run_steps(a.steps))
    cards = world * F * K * a.steps
    value = cards / dt
    if a.dump_outputs and rank == 0:
        dump_outputs(out[-1], a.dump_outputs)
    import zlib

    # checksum of rank 0's top-1 ids over the timed steps: equal across bank layouts, stream counts and rank counts
    # (rank 0's frames depend on the seed only) - tests/test_gpu_dist.py compares a sharded two-rank run with a replicated one
    ids_crc = zlib.crc32(torch.stack([o["ids"] for o in out]).cpu().numpy().tobytes())

    res = {
        "metric": "cards/sec end-to-end (detect+embed+top-1 over 100k bank), 640x640",
        "value": round(value, 1),
        "unit": "cards/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(dt / a.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        # tensors, accumulation and results are f32 in both modes; f16x3 forms each f32 product from three fp16 MFMAs
        # (error vs fp64 at the f32 level: tests/test_gpu_precision.py) - see config.gemm_operands
        "dtype": "f32" if precision == "f32" else "f32 (products as 3 x f16 MFMA on hi/lo-split operands, f32 accumulate)",
        "data": "synthetic",
        "config": {
            "workload": f"full pipeline per GPU: {F} frames 640x640x3 u8 -> {'YOLO11n-seg' if a.detector == 'yolo11n-seg' else 'YOLOv8n-seg'}(nc=3) detect+NMS+masks -> {K} cards/frame "
            f"-> 192x128 crops -> ConvNeXt-V2 {a.encoder} (z=768) -> cosine top-1 over {a.bank}x768 bank",
            "crop_quads": "detection boxes" if a.quads == "box" else "4-vertex polygons fitted to the detection masks on the GPU (mask_quads_kernel: hull + approxPolyN + orientation)",
            "frames_per_gpu": F,
            "distinct_frame_batches": NB,
            "cards_per_frame": K,
            "bank": [a.bank, 768],
            "bank_layout": ("row-sharded %d-way + RCCL all-gather of per-shard top-1" % world) if sharded else "replicated",
            "weights": "random-init (seeded), no trained weights offline",
            "gemm_precision_mode": precision,
            "gemm_operands": "f32 operands, f32-input MFMA" if precision == "f32" else "f32-grade values kept as fp16 hi+lo pairs (4 B per "
            "element: weights and bank with a power-of-two scale per row, GEMM-bound activations written that way by their producers, the "
            "rest split when a fragment is read), 3 fp16 MFMAs per product, f32 accumulate (error vs fp64 at the f32 level, "
            "tests/test_gpu_precision.py)",
            "streams": ("3 pipeline streams (detect + crop of step i+1 beside embed of step i and, behind it, match of step i, the "
                        "latter two at high priority; the detector's own fork-join off; MTGV_OVERLAP=on set by bench.py, the "
                        "library default is 1; switches MTGV_STREAM_PRIO, MTGV_CROP_STAGE, MTGV_MATCH_STREAM, MTGV_MATCH_PRIO, "
                        "MTGV_OVERLAP_DET_FORK in mtgv/pipeline.py)") if overlap else "1",
            "settle": f"{a.settle_steps} untimed steps ({t_settle:.1f} s of steady load) before the {a.warmup} warm-up steps of `value`"
            + ("; unsettled_value is the same W + K measurement taken BEFORE them, first thing in the process" if a.full else ""),
            "ids_crc32_rank0": ids_crc,
            "rccl_world": dist.get_world_size() if dist.is_initialized() else 1,
            "dist_backend": (dist.get_backend() if dist.is_initialized() else None),
        },
    }
    if dt_cold is not None:
        res["config"]["unsettled_value"] = round(cards / dt_cold, 1)
    if a.full and a.sustained_seconds > 0:
        # the same step loop for seconds instead of K steps (every rank the same step count: the sharded match is a collective)
        n_sus = max(a.steps, int(a.sustained_seconds / (dt / a.steps)) + 1)
        dts, _ = timed(lambda: [run_steps(min(64, n_sus - i0)) and None for i0 in range(0, n_sus, 64)])
        res["config"]["sustained_value"] = round(world * F * K * n_sus / dts, 1)
        res["config"]["sustained_steps"] = n_sus
        res["config"]["sustained_seconds"] = round(dts, 2)
    if a.full and overlap and not a.no_one_stream:
        # the library default (one stream: MTGV_OVERLAP off) on the same K steps, timed the same way; `value` above is the
        # two-stream figure, which needs the opt-in
        pipe.run(batches[0])
        dt1, _ = timed(lambda: [pipe.run(batches[i % NB]) for i in range(a.steps)] and None)
        res["config"]["one_stream_value"] = round(cards / dt1, 1)
        res["config"]["one_stream_ms_per_step"] = round(dt1 / a.steps * 1e3, 3)
    if a.full and not a.no_h2d:
        # frames arriving from the host (the reference's do: server.py:272-280): the NB batches sit in pinned host memory
        # and are copied in on a third stream (copy engine) into a ring of three device buffers, one to two batches ahead
        from mtgv.pipeline import HostFrames

        src = HostFrames([b.cpu() for b in batches], dev)

        def run_h2d(k):
            return pipe.run_many(src.leases(k)) if overlap else [pipe.run(ls) for ls in src.leases(k)]

        run_h2d(a.warmup)
        dth, outh = timed(lambda: run_h2d(a.steps))
        res["config"]["with_h2d_value"] = round(cards / dth, 1)
        res["config"]["with_h2d_ms_per_step"] = round(dth / a.steps * 1e3, 3)
        res["config"]["with_h2d_ids_equal"] = bool(zlib.crc32(torch.stack([o["ids"] for o in outh]).cpu().numpy().tobytes()) == ids_crc)
        del src

    # roofline leg.  Dominant kernel = gemm_f32_kernel (every conv / linear / bank GEMM of the path).  Every rank
    # runs two more passes of the same step, one stream, so that each launch is alone on the GPU and bracketed by HIP
    # events on the stream it is launched on (the sharded match inside the step is a collective: all ranks take part).
    import ctypes as C

    L = native.lib()
    prof = None
    prof_f32 = None

    def profile_pass(prec):
        nprof = 2
        native.check(L.mtgv_profile_gemm(1))
        # every launch alone on the GPU: the detector's internal fork-join (prototype branch and heads on library-owned
        # streams) is switched off for these passes, or concurrent launches would each be charged the other's time
        fork_before = os.environ.get("MTGV_DET_FORK")
        os.environ["MTGV_DET_FORK"] = "0"
        try:
            for i in range(nprof):
                pipe.run(batches[i % NB])
            torch.cuda.synchronize()
        finally:
            if fork_before is None:
                os.environ.pop("MTGV_DET_FORK", None)
            else:
                os.environ["MTGV_DET_FORK"] = fork_before
        ms, fl, nl, by = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_double(0)
        native.check(L.mtgv_profile_gemm_read(C.byref(ms), C.byref(fl), C.byref(nl)))
        native.check(L.mtgv_profile_gemm_bytes(C.byref(by)))
        groups, fill_per_step = None, 0.0
        if rank == 0:
            import csv
            import tempfile

            with tempfile.NamedTemporaryFile(suffix=".csv", delete=False) as tf:
                tmp_csv = tf.name
            native.check(L.mtgv_profile_gemm_dump(tmp_csv.encode()))
            recs = list(csv.DictReader(open(tmp_csv)))
            os.unlink(tmp_csv)
            groups = group_launches(recs, nprof, prec)
            fill_per_step = sum(float(r.get("fill", 0) or 0) for r in recs) / nprof
        native.check(L.mtgv_profile_gemm(0))
        barrier()
        return (ms.value / nprof, fl.value / nprof, int(nl.value // nprof), by.value / nprof, groups, fill_per_step)

    if a.full and not a.no_roofline:
        prof = profile_pass(precision)
        if precision == "f16x3" and not a.no_f32_roofline:
            # the same step with exact f32-input MFMAs (the library's other operand mode): one warm pass, then the same
            # two profiled passes; north_star's ">= 60 % of the MFMA roofline for the 1x1 / bank GEMMs" is stated against
            # this mode's peak (157.3 TFLOP/s)
            native.set_gemm_precision("f32")
            pipe.run(batches[0])
            torch.cuda.synchronize()
            prof_f32 = profile_pass("f32")
            native.set_gemm_precision("f16x3")

    if rank == 0:
        gflops_enc, dw_enc = encoder.flops_per_image()
        det_flops = detector.flops_per_frame()
        res["config"]["algorithmic_gflop_per_card"] = round((gflops_enc + dw_enc + det_flops / K + 2 * a.bank * 768) / 1e9, 3)
        if prof is not None:
            gemm_ms, gemm_fl, launches, gemm_bytes, groups, fill_bytes = prof
            sec = gemm_ms * 1e-3
            tfl = gemm_fl / sec / 1e12 if sec > 0 else 0.0
            gbs = gemm_bytes / sec / 1e9 if sec > 0 else 0.0
            peak_tf = PEAK_MFMA_TFLOPS[precision]
            issued = tfl * MFMA_FLOPS_PER_FLOP[precision]
            if groups:  # exact per launch kind (the fp16 first pass of the bank match issues 1x, the fused MLP's output pass 6x)
                issued = sum(gv["issued_gflop_per_step"] for gv in groups.values()) / 1e3 / sec if sec > 0 else 0.0
            traffic, traffic_src = None, None
            tfile = os.path.join(ROOT, "profiles", "gemm_traffic.json")
            if os.path.exists(tfile):
                try:
                    tj = json.load(open(tfile))
                    traffic = tj.get(precision, {}).get("hbm_bytes_per_step")
                    traffic_src = "static: profiles/gemm_traffic.json, collected at %s (not re-measured by this run)" % tj.get("collected_at", "round 1")
                except Exception:
                    traffic = None
            # which roof binds the kernel: the larger of its two minimum times
            t_mfma = gemm_fl * MFMA_FLOPS_PER_FLOP[precision] / (peak_tf * 1e12)
            t_hbm = gemm_bytes / (PEAK_HBM_GBS * 1e9)
            mfma_view = {"achieved": round(tfl, 2), "peak": peak_tf, "unit": "TFLOP/s", "frac": round(tfl / peak_tf, 4),
                         "issued_mfma_tflops": round(issued, 2), "issued_frac": round(issued / peak_tf, 4)}
            hbm_view = {"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4)}
            bound = "mfma" if t_mfma >= t_hbm else "hbm"
            top = mfma_view if bound == "mfma" else hbm_view
            if bound == "mfma" and precision == "f16x3":
                # against the fp16 MFMA peak the split products count as issued: three (fused output pass: six, fp16
                # first pass of the match: one) MFMA FLOPs per algorithmic FLOP
                top = {"achieved": round(issued, 2), "peak": peak_tf, "unit": "TFLOP/s (MFMA FLOPs issued for the algorithmic work)",
                       "frac": round(issued / peak_tf, 4)}
            res["roofline"] = {
                "bound": bound,
                "kernel": ("gemm_f32_kernel<..., PREC=0> (implicit-GEMM conv/linear/bank kernel; all launches of one step)" if precision == "f32" else
                           "split-precision GEMM launches of one step: gemm_sp_kernel (LDS-DMA, SP8 operands) + gemm_f32_kernel<..., PREC=1> (stem, mask and bank launches)"),
                "achieved": top["achieved"],
                "peak": top["peak"],
                "unit": top["unit"],
                "frac": top["frac"],
                "traffic": traffic,
                "traffic_note": "HBM bytes of these launches per step, rocprofv3 FETCH_SIZE x2 + WRITE_SIZE",
                "traffic_source": traffic_src,
                "groups": groups,
                "launches_per_step": launches,
                "gemm_ms_per_step": round(gemm_ms, 3),
                "algorithmic_gflop_per_step": round(gemm_fl / 1e9, 2),
                "algorithmic_gbyte_per_step": round(gemm_bytes / 1e9, 3),
                "min_ms_at_mfma_peak": round(t_mfma * 1e3, 3),
                "min_ms_at_hbm_peak": round(t_hbm * 1e3, 3),
                "mfma_view": mfma_view,
                "hbm_view": hbm_view,
                # The resource the tiling actually leans on: every tile pulls its A and B panels (4 B per element) through
                # L2 into LDS.  Ceilings: gather-into-LDS rates measured on this part (MI355X_MICROARCH.md, "Indexed rows").
                "lds_fill_view": {"gbyte_per_step": round(fill_bytes / 1e9, 2),
                                  "achieved_tbs": round(fill_bytes / (gemm_ms * 1e-3) / 1e12, 2) if gemm_ms > 0 else None,
                                  "ceiling_tbs": {"infinity_cache_resident": 8.6, "l2_resident": 17.8}, "unit": "TB/s"},
                "measured": "HIP events around every launch on its stream, 2 single-stream passes after the timed region (MTGV_DET_FORK=0 for them: the detector's branches in sequence, every launch alone on the GPU)",
            }
            if prof_f32 is not None:
                ms32, fl32, n32, by32, groups32, _ = prof_f32
                tf32 = fl32 / (ms32 * 1e-3) / 1e12 if ms32 > 0 else 0.0
                res["roofline"]["f32_mode"] = {
                    "what": "the same step after mtgv_set_gemm_precision(f32): every GEMM on v_mfma_f32_32x32x2_f32, same events",
                    "bound": "mfma", "achieved": round(tf32, 2), "peak": PEAK_MFMA_TFLOPS["f32"], "unit": "TFLOP/s",
                    "frac": round(tf32 / PEAK_MFMA_TFLOPS["f32"], 4), "gemm_ms_per_step": round(ms32, 3),
                    "launches_per_step": n32, "groups": groups32,
                }
        if a.full and world == 1 and not a.no_cpu_baseline:
            # bounded CPU sample of the same workload on the host cores: the oracle pipeline
            from oracle import pipeline_ref

            # Thread count: every host core this process may run on is the upper bound, but PyTorch's CPU kernels
            # slow down when oversubscribed (256 threads on this pool's hosts: 15x slower than 16), and the box's
            # CPU share can be a cgroup quota the affinity mask does not show.  Time one frame at a few candidate
            # counts and keep the fastest; "cores" reports the threads actually used.
            try:
                ncpu = len(os.sched_getaffinity(0))
            except AttributeError:
                ncpu = os.cpu_count() or 1
            try:
                q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
                if q != "max":
                    ncpu = max(1, min(ncpu, int(int(q) / int(per))))
            except (OSError, ValueError):
                pass
            cpu_model = "unknown"
            try:
                for ln in open("/proc/cpuinfo"):
                    if ln.startswith("model name"):
                        cpu_model = ln.split(":", 1)[1].strip()
                        break
            except OSError:
                pass
            bank_cpu = matcher.rows(0, len(matcher))
            fr = frames[: min(a.cpu_frames, F)].cpu().numpy()
            tried = {}
            for nt in sorted({ncpu, min(ncpu, 64), min(ncpu, 32), min(ncpu, 16)}, reverse=True):
                torch.set_num_threads(nt)
                pipeline_ref.run(det_sd, det_cfg, enc_sd, enc_cfg, bank_cpu[:1000], fr[:1], K)  # warm the thread pool
                t0 = time.perf_counter()
                pipeline_ref.run(det_sd, det_cfg, enc_sd, enc_cfg, bank_cpu[:1000], fr[:1], K)
                tried[nt] = round(time.perf_counter() - t0, 3)
            nthreads = min(tried, key=tried.get)
            torch.set_num_threads(nthreads)
            cf = min(a.cpu_frames, F)
            pipeline_ref.run(det_sd, det_cfg, enc_sd, enc_cfg, bank_cpu[:1000], fr[:1], K)  # warm the thread pool
            t0 = time.perf_counter()
            pipeline_ref.run(det_sd, det_cfg, enc_sd, enc_cfg, bank_cpu, fr, K, quad_source=a.quads)
            cdt = time.perf_counter() - t0
            # per-stage detail on the same threads (batch 4 and 32; img/s, frames/s, queries/s), each a bounded sample
            from oracle import detector_ref, encoder_ref, match_ref

            stages = {}
            g0 = np.random.default_rng(0)
            h_, w_ = enc_cfg.image_hw
            for nb_ in (4, 32):
                xe = g0.random((nb_, 3, h_, w_), dtype=np.float32)
                encoder_ref.encoder_forward(enc_sd, enc_cfg, xe[:1])
                t0 = time.perf_counter()
                encoder_ref.encoder_forward(enc_sd, enc_cfg, xe)
                stages[f"encoder_img_per_s_batch{nb_}"] = round(nb_ / (time.perf_counter() - t0), 2)
                fd = frames[:nb_].cpu().numpy()
                t0 = time.perf_counter()
                detector_ref.detect(det_sd, det_cfg, fd, True)
                stages[f"detector_frames_per_s_batch{nb_}"] = round(len(fd) / (time.perf_counter() - t0), 2)
                qd = g0.standard_normal((nb_, 768), dtype=np.float32)
                t0 = time.perf_counter()
                match_ref.cosine_topk(qd, bank_cpu, 1, dtype=np.float32)
                stages[f"match_queries_per_s_batch{nb_}"] = round(nb_ / (time.perf_counter() - t0), 2)
            res["cpu_baseline"] = {
                "stages": stages,
                "value": round(cf * K / cdt, 2),
                "unit": "cards/s",
                "cores": nthreads,
                "cpu_model": cpu_model,
                "host_cpu_count": os.cpu_count(),
                "seconds_per_frame_by_threads": tried,
                "kind": "port",
                "sample": f"{cf} frames x {K} cards of the same synthetic workload through oracle/pipeline_ref.py "
                f"(PyTorch CPU fp32 for detector / encoder / match on {nthreads} threads; crops are "
                f"{'the mask quadrilaterals (oracle/quad_ref.py, single-threaded numpy/Python), as on the GPU leg' if a.quads == 'mask' else 'the detection boxes'}), {cdt:.1f} s",
            }
        print(json.dumps(res), flush=True)
    if world > 1 or force_coll:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
