#!/usr/bin/env python3
"""Time the per-batch input stage of the AffWild2 feature graph on one MI355X -- SENet features (512 wide), stacked log-Mel rows (40 bands)
and the labels of a batch of training windows -- at 32 clips x 300 frames and 96 clips x 32 frames, both ways:

  host route    the numpy restatement of the reference's __getitem__ per item (tests/collate_ref.py), np.stack per key (the DataLoader's
                default collate), one pinned buffer and one non-blocking copy per tensor
  device route  m3t.dataset.TrackStore.collate on the same items: one int table up, one launch

and the audio-only training step (AffWild2VA --modality audio, training_step + backward) with its batch built each way.  The routes are
run alternately in one process; each sample is a host clock around `--inner` repetitions that end in a device synchronise; medians and the
spread (min .. max) are printed as one JSON line, with the bytes of the store that was timed and of a 500-video set of 5 000 frames each
(computed from the row counts, by the formula the timed store's own `nbytes` is checked against).

    python tools/collate_bench.py [--videos 48] [--frames 1500] [--samples 9] [--inner 3] [--step-samples 7]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SE, MELS = 512, 40


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


def store_bytes(n_videos, frames, labelled=True):
    """se + mel (3 rows a frame + 2) + va + expr (int64) + the per-video table, as TrackStore.nbytes counts them"""
    per_video = frames * SE * 4 + (3 * frames + 2) * MELS * 4 + (frames * 2 * 4 + frames * 8 if labelled else 0) + 12 * 8
    return n_videos * per_video


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=48)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--step-samples", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collate_bench needs the GPU: a timing taken anywhere else says nothing")
    import collate_ref as R
    from m3t.dataset import TrackStore
    from models.model import AffWild2VA
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    videos = {}
    for v in range(a.videos):
        n = a.frames
        videos["v%03d" % v] = {"nb_frames": n, "fps": 30.0, "se": rs.standard_normal((n, SE)).astype(np.float32),
                               "mel": rs.standard_normal((3 * n + 2, MELS)).astype(np.float32),
                               "va": rs.uniform(-1, 1, (n, 2)).astype(np.float32), "expr": rs.randint(-1, 7, n).astype(np.int64)}
    names = list(videos)
    result = {"tool": "collate_bench", "videos": a.videos, "frames_per_video": a.frames, "se_width": SE, "n_mels": MELS, "shapes": {}}
    for N, W in ((32, 300), (96, 32)):
        store = TrackStore(videos, W, "train", se_dim=SE)
        assert store.nbytes == store_bytes(a.videos, a.frames), (store.nbytes, store_bytes(a.videos, a.frames))
        rnd = random.Random(N)
        items = [(rnd.randrange(a.videos), rnd.randrange(a.frames - W + 1)) for _ in range(N)]
        named = [(names[v], s, W) for v, s in items]

        def host():
            b = R.batch(videos, named, W, "train", se_dim=SE)
            return {k: (torch.from_numpy(np.ascontiguousarray(x)).pin_memory().to(dev, non_blocking=True) if k in R.DTYPES else x)
                    for k, x in b.items()}

        def device():
            return store.collate(items)

        h, d = host(), device()
        same = all(torch.equal(h[k], d[k]) for k in R.DTYPES if k in h)
        batch_bytes = sum(h[k].numel() * h[k].element_size() for k in R.DTYPES if k in h)
        stage = alternate([host, device], a.samples, a.inner)

        hp = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
        hp.modality, hp.window = "audio", W
        torch.manual_seed(0)
        m = AffWild2VA(hp).to(dev).train()

        def step(make):
            for p in m.parameters():
                p.grad = None
            m.training_step(make(), 0)["loss"].backward()

        steps = alternate([lambda: step(host), lambda: step(device), lambda: step(lambda: d)], a.step_samples, a.inner)
        hs, ds = summary(stage[0]), summary(stage[1])
        result["shapes"]["%dx%d" % (N, W)] = {
            "batch_bytes": batch_bytes, "bit_equal": bool(same), "host_route": hs, "device_route": ds,
            "speedup": round(hs["median_ms"] / ds["median_ms"], 2),
            "audio_step_host_fed": summary(steps[0]), "audio_step_device_fed": summary(steps[1]), "audio_step_ready_batch": summary(steps[2])}
        del store
    result["store_bytes_timed"] = store_bytes(a.videos, a.frames)
    result["store_bytes_500_videos_x_5000_frames"] = store_bytes(500, 5000)
    result["note"] = ("input stage = se_features [N, 512, W] + audio [N, W, 200] + valence, arousal, class_expr, expr_valid [N, W] of N training windows; "
                      "host route = numpy __getitem__ per item + np.stack + pin + copy per tensor; device route = TrackStore.collate (one table up, one "
                      "launch); audio_step = AffWild2VA --modality audio (loss %s) training_step + backward with the batch built by the host route / by "
                      "the store / ready on the device; routes run alternately in one process, %d samples x %d calls (steps: %d x %d)"
                      % (hp.loss, a.samples, a.inner, a.step_samples, a.inner))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
