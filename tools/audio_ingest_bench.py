#!/usr/bin/env python3
"""Time the audio input stage at the AudioSet pre-training shape (128 clips x 32 frames, 10 s of 16 kHz int16 PCM per clip, training draws)
on one MI355X, from a pinned host batch, both ways:

  per-clip route  the whole batch copied to the device, then per clip: crop, m3t.audio.melspec_db, m3t.audio.load_audio; torch.stack
                  (five launches, two GEMMs and five allocations per clip)
  batched route   m3t.audio.ingest on the same batch and draws (four launches and one GEMM for the batch)

and the AudioSet training step (training_step + backward, num_hidden 256) fed with ready [N, T, 200] features on the device against the
same step fed with the PCM batch.  The routes are run alternately in one process; each sample is a host clock around `--inner` repetitions
that end in a device synchronise; medians and the spread (min .. max) are printed as one JSON line.

    python tools/audio_ingest_bench.py [--clips 128] [--frames 32] [--seconds 10] [--samples 9] [--inner 3] [--step-samples 9]
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
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--step-samples", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audio_ingest_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import audio
    from models.audioset_model import AudioSet
    dev = torch.device("cuda", 0)
    N, T, S = a.clips, a.frames, int(a.seconds * 16000)
    rs = np.random.RandomState(0)
    t = np.arange(S) / 16000.0
    y = 0.4 * np.sin(2 * np.pi * 440 * t)[None] + 0.05 * rs.standard_normal((N, S))
    pcm = torch.from_numpy(np.round(y * 32767.0).clip(-32768, 32767).astype(np.int16)).pin_memory()
    random.seed(0)
    draws = [audio.draw_audioset(S, T, True) for _ in range(N)]
    if any(d["start"] + d["nsamples"] > S for d in draws):
        raise SystemExit("the per-clip route of this tool crops by slicing: clips must be at least as long as the longest crop")

    def per_clip():
        w = pcm.to(dev, non_blocking=True)
        rows = []
        for n, d in enumerate(draws):
            crop = w[n, d["start"]:d["start"] + d["nsamples"]].to(torch.float32) / 32768.0
            rows.append(audio.load_audio(audio.melspec_db(crop, d["fps"]), 0, T))
        return torch.stack(rows)

    def batched():
        return audio.ingest(pcm, draws, T)

    err = float((per_clip() - batched()).abs().max())
    stage = alternate([per_clip, batched], a.samples, a.inner)

    hp = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    hp.window = T
    torch.manual_seed(0)
    m = AudioSet(hp).to(dev).train()
    label = (torch.rand(N, 527, device=dev) < 0.01).float()
    feats = batched()

    def step(batch):
        for p in m.parameters():
            p.grad = None
        m.training_step(batch, 0)["loss"].backward()

    steps = alternate([lambda: step({"audio": feats, "label": label}),
                       lambda: step({"audio": pcm, "audio_aug": draws, "label": label})], a.step_samples, a.inner)
    per, bat = summary(stage[0]), summary(stage[1])
    print(json.dumps({
        "tool": "audio_ingest_bench", "clips": N, "frames": T, "samples_per_clip": S, "spectrogram_rows": int(sum(1 + d["nsamples"] // d["hop"] for d in draws)),
        "host_bytes_pcm": int(pcm.numel()) * 2,
        "per_clip_route": per, "batched_route": bat, "speedup": round(per["median_ms"] / bat["median_ms"], 2),
        "max_abs_diff_db": round(err, 6),
        "audioset_step_features": summary(steps[0]), "audioset_step_pcm": summary(steps[1]),
        "note": "pinned host int16 batch -> device; per-clip route = copy + per clip crop, melspec_db, load_audio + stack; batched route = "
                "m3t.audio.ingest (copy + 3 kernels + 1 GEMM); audioset_step = training_step + backward of AudioSet (num_hidden %d) fed with device "
                "features / with the PCM batch; routes run alternately in one process, %d samples x %d calls (steps: %d x %d)"
                % (hp.num_hidden, a.samples, a.inner, a.step_samples, a.inner)}), flush=True)


if __name__ == "__main__":
    main()
