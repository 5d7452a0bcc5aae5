#!/usr/bin/env python3
"""Time the video input stage at the C5 shape (8 clips x 64 frames x 112 x 112) on one MI355X, from a pinned host batch, both ways:

  float32 route  what the reference's loader hands over: float32 [N, 3, T, H, W] -> copy to the device -> (x - 127.5) / 127.5 (stock torch)
                 -> m3t_planes_to_cl4 with the magnitude slot armed (the first convolution's own first step)
  uint8 route    the frames as decoded: uint8 [N, T, H, W, 3] -> copy to the device -> m3t.video.ingest (one kernel; with --crop from
                 128 x 128 frames, with per-clip draws: crop, mirror, cutout; with --input-size 256 from the reference's default
                 256 x 256 face tracks: crop 224, halve to 112 (m3t_video_ingest_half), mirror, cutout -- the float32 route is then fed
                 frames ALREADY cropped and resized, so the comparison leaves out the host's cv2.resize of every frame (and its
                 crop, flip, transpose and cast), which the uint8 route does not need and which cannot be timed without cv2)

and the full C5 training step (bench.py's c5 leg: AffWild2VA audiovisual / attention / v2p_split, training_step + backward + clip) fed
each way, the host-to-device copy of the video included.  The two routes are run alternately in one process; each sample is a host
clock around `--inner` repetitions that end in a device synchronise; medians and the spread (min .. max) are printed as one JSON line.

    python tools/ingest_bench.py [--clips 8] [--frames 64] [--samples 15] [--inner 5] [--step-samples 9] [--crop | --input-size 256]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))


def alternate(fns, samples, inner, warmup=2):
    """ms per call of each function, sampled in turn: [[...], [...]]"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(samples):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) * 1e3 / inner)
    return out


def summary(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--step-samples", type=int, default=9)
    ap.add_argument("--crop", action="store_true", help="uint8 frames of 128 x 128 with per-clip crop / mirror / cutout draws")
    ap.add_argument("--input-size", type=int, default=None, choices=[256],
                    help="uint8 frames of 256 x 256 with per-clip crop (224) / halve (112) / mirror / cutout draws: the halving kernel")
    a = ap.parse_args()
    if a.crop and a.input_size:
        raise SystemExit("--crop and --input-size are two cases: give one")
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import _lib, ops, video
    from m3t.ddp import FlatGradDDP
    from models.model import AffWild2VA
    dev = torch.device("cuda", 0)
    N, T, S = a.clips, a.frames, 112
    rs = np.random.RandomState(0)
    src = a.input_size or (128 if a.crop else S)
    frames = torch.from_numpy(rs.randint(0, 256, (N, T, src, src, 3)).astype(np.uint8)).pin_memory()
    aug = None
    if a.crop:
        random.seed(0)
        np.random.seed(0)
        aug = [video.draw_affwild(128, True, True, True, random.random() > 0.5) for _ in range(N)]
    if a.input_size:
        random.seed(0)
        np.random.seed(0)
        aug = [video.draw_affwild(a.input_size, True, True, True, random.random() > 0.5, resize=True) for _ in range(N)]
    x32_host = torch.from_numpy(rs.randint(0, 256, (N, 3, T, S, S)).astype(np.float32)).pin_memory()
    lib = ops.lib()

    def f32_stage():
        x = (x32_host.to(dev, non_blocking=True) - 127.5) / 127.5
        x_cl = torch.empty(N * T * S * S, 4, dtype=torch.float32, device=dev)
        slot = ops.amax_slots(1, dev)
        ops.amax_out(slot.data_ptr())
        _lib.check(lib.m3t_planes_to_cl4(ops._p(x), ops._p(x_cl), N, 3, T * S * S, ops._stream()), "m3t_planes_to_cl4")
        return x_cl

    def u8_stage():
        return video.ingest(frames, aug, None, "cl", norm="device")

    def f32_copy():
        return x32_host.to(dev, non_blocking=True)

    def u8_copy():
        return frames.to(dev, non_blocking=True)

    stage = alternate([f32_stage, u8_stage, f32_copy, u8_copy], a.samples, a.inner)

    hp = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    hp.modality, hp.fusion_type, hp.loss, hp.window = "audiovisual", "attention", "ccc_mtl", T
    torch.manual_seed(12345)
    m = AffWild2VA(hp).to(dev).train()
    f = lambda arr: torch.from_numpy(arr).to(dev)
    rest = {"se_features": f(rs.standard_normal((N, 512, T)).astype(np.float32)), "audio": f(rs.standard_normal((N, T, 200)).astype(np.float32)),
            "label_valence": f(rs.uniform(-1, 1, (N, T)).astype(np.float32)), "label_arousal": f(rs.uniform(-1, 1, (N, T)).astype(np.float32)),
            "class_expr": f(rs.randint(0, 7, (N, T)).astype(np.int64)), "expr_valid": f(rs.uniform(size=(N, T)) < 0.7)}
    ddp = FlatGradDDP(m, max_norm=1.0)

    def step(batch):
        ddp.zero_grad()
        m.training_step(batch, 0)["loss"].backward()
        ddp.finish()

    def f32_step():
        step(dict(rest, video=x32_host.to(dev, non_blocking=True)))

    def u8_step():
        step(dict(rest, video=frames, video_aug=aug))

    steps = alternate([f32_step, u8_step], a.step_samples, 3)
    px = N * T * S * S
    half = {"halved": True, "left_out": "the float32 route's host work: crop, cv2.resize 224 -> 112, flip, transpose, cast (cv2 is not timed)"} \
        if a.input_size else {}
    print(json.dumps({
        "tool": "ingest_bench", "clips": N, "frames": T, "source": src, "crop_mirror_cutout": bool(a.crop or a.input_size), **half,
        "host_bytes_f32": px * 12, "host_bytes_u8": int(frames.numel()),
        "input_stage_f32": summary(stage[0]), "input_stage_u8": summary(stage[1]),
        "copy_only_f32": summary(stage[2]), "copy_only_u8": summary(stage[3]),
        "c5_step_f32": summary(steps[0]), "c5_step_u8": summary(steps[1]),
        "note": "pinned host batch -> device; input stage = copy + normalise + m3t_planes_to_cl4 (float32 route) against copy + %s "
                "(uint8 route); c5_step = the same stage inside the AffWild2VA training step (training_step + backward + clip); routes run "
                "alternately in one process, %d samples x %d calls (steps: %d x 3)" % ("m3t_video_ingest_half" if a.input_size else "m3t_video_ingest", a.samples, a.inner, a.step_samples)}),
        flush=True)


if __name__ == "__main__":
    main()
