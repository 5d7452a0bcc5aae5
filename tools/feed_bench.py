#!/usr/bin/env python3
"""Time the AffWild2 epoch feed (m3t.feed.AffWild2Feed) on one MI355X against the same stores driven by hand.  A synthetic Aff-Wild2 folder
is written to a temporary directory: `--videos` videos of `--video-frames` frames, every frame the 256 x 256 quality-95 4:2:0 fixture of
tests/golden/jpeg_cases.npz (45.6 KB), with SENet / AU / log-Mel tracks, labels and split files; scan_affwild reads it back.

  (a) c5      the C5 training step (AffWild2VA audiovisual / attention, training_step + backward + clip) at `--clips` x `--frames`, fed
              four ways: "store" -- the store leg of tools/frame_store_bench.py (FrameStore.decode of the next batch issued on a side
              stream before the step, the side tensors ready on the device); "feed_ahead" -- the same schedule with the whole next batch
              taken from the feed under the side stream (the feed launches on whatever stream is current); "hand" -- TrackStore.collate +
              FrameStore.decode + the draws of a ready plan, on the step's own stream; "feed" -- next(iter(feed)) on the step's own stream
  (b) audio   the audio-only step (training_step + backward) at `--audio-clips` x `--audio-frames`, fed by TrackStore.collate of ready items
              and by the feed
  (c) host    the host time of one batch of each feed by stage, with an idle queue and no synchronise inside: the plan (the sampler
              and the draws), the validation ahead of the launches, collate, decode

Legs alternate in one process, `--rounds` rounds after warm-up; each sample is a host clock around `--inner` steps that end in a device
synchronise.  One JSON line.

    python tools/feed_bench.py [--rounds 3] [--step-samples 5] [--inner 3] [--no-c5]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from frame_store_bench import rounds_of  # noqa: E402
from ingest_bench import summary  # noqa: E402


def write_corpus(root, videos, frames, data):
    """the folder scan_affwild reads: data/face_256/<name>/%05d.jpg, tracks, annotations; splits/ beside it"""
    rs = np.random.RandomState(0)
    d = os.path.join(root, "data")
    for sub in ("se101_feats", "AU_feats", "mel_spec", "annotations/VA_Set/Training_Set", "annotations/EXPR_Set/Training_Set", "splits"):
        os.makedirs(os.path.join(d if sub != "splits" else root, sub))
    names = ["v%02d" % v for v in range(videos)]
    for name in names:
        os.makedirs(os.path.join(d, "face_256", name))
        for i in range(frames):
            with open(os.path.join(d, "face_256", name, "%05d.jpg" % (i + 1)), "wb") as f:
                f.write(data)
        np.save(os.path.join(d, "se101_feats", name + ".npy"), rs.standard_normal((frames, 512)).astype(np.float32))
        np.save(os.path.join(d, "AU_feats", name + ".npy"), rs.standard_normal((frames, 268)).astype(np.float32))
        np.save(os.path.join(d, "mel_spec", name + ".npy"), rs.standard_normal((3 * frames + 2, 40)).astype(np.float32))
        with open(os.path.join(d, "annotations", "VA_Set", "Training_Set", name + ".txt"), "w") as f:
            f.write("valence,arousal\n" + "".join("%.4f,%.4f\n" % tuple(r) for r in rs.uniform(-1, 1, (frames, 2))))
        with open(os.path.join(d, "annotations", "EXPR_Set", "Training_Set", name + ".txt"), "w") as f:
            f.write("Neutral,Anger,Disgust,Fear,Happiness,Sadness,Surprise\n" + "".join("%d\n" % e for e in rs.randint(-1, 7, frames)))
    for fn, text in (("frames_fps.csv", "".join("%s,%d,30.0\n" % (n, frames) for n in names)), ("train.csv", "".join(n + "\n" for n in names)),
                     ("expr.csv", "".join("%s,Training_Set\n" % n for n in names))):
        with open(os.path.join(root, "splits", fn), "w") as f:
            f.write(text)
    return d, os.path.join(root, "splits")


def host_stages(feed, samples):
    """ms of one batch by stage, idle queue, the clock stopped before any synchronise"""
    from m3t import dataset, video
    feed.build_stores()
    plans = feed.plans()
    out = {"plan": [], "validate": [], "collate": [], "decode": []}
    for _ in range(samples + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = next(plans)
        t1 = time.perf_counter()
        if feed.visual:
            dataset.plan(feed.tracks.meta, p.items, feed.window, feed.split)
            video.plan((len(p.items), feed.window, feed.frames.height, feed.frames.width, 3), torch.uint8, p.aug)
        t2 = time.perf_counter()
        feed.tracks.collate(p.items)
        t3 = time.perf_counter()
        if feed.visual:
            feed.frames.decode(p.items)
        t4 = time.perf_counter()
        for k, dt in zip(("plan", "validate", "collate", "decode"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            out[k].append(dt * 1e3)
    torch.cuda.synchronize()
    return {k: summary(v[2:]) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--video-frames", type=int, default=64)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--audio-clips", type=int, default=96)
    ap.add_argument("--audio-frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-samples", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=9)
    ap.add_argument("--no-c5", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feed_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import feed as F
    from m3t.ddp import FlatGradDDP
    from models.model import AffWild2VA
    dev = torch.device("cuda", 0)
    data = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["full_256_q95.jpg"].tobytes()
    out = {"tool": "feed_bench", "fixture_bytes": len(data), "corpus": [a.videos, a.video_frames]}
    with tempfile.TemporaryDirectory() as root:
        path, splits = write_corpus(root, a.videos, a.video_frames, data)
        many = 1 << 20                                          # windows_per_epoch: an epoch that outlasts the run (the plan is drawn batch by batch)

        def hparams(**kw):
            hp = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
            hp.dataset_path, hp.splits_dir, hp.input_size, hp.release = path, splits, 256, "vipl"
            for k, v in kw.items():
                setattr(hp, k, v)
            return hp

        def seeds():
            random.seed(0)
            np.random.seed(0)
            torch.manual_seed(0)

        if not a.no_c5:
            N, T = a.clips, a.frames
            hp = hparams(modality="audiovisual", fusion_type="attention", loss="ccc_mtl", window=T, batch_size=N, cutout=True,
                         windows_per_epoch=many // a.videos)
            t0 = time.perf_counter()
            corpus = F.scan_affwild(path, "train", hp.modality, "vipl", 256, splits, False, T)
            scan_ms = (time.perf_counter() - t0) * 1e3
            torch.manual_seed(12345)
            m = AffWild2VA(hp).to(dev).train()
            ddp = FlatGradDDP(m, max_norm=1.0)
            seeds()
            t0 = time.perf_counter()
            fd = F.AffWild2Feed(corpus, T, N, "train", hp.modality, True, 256, "vipl", hp.windows_per_epoch, visual=m.visual).build_stores()
            torch.cuda.synchronize()
            out["c5_build"] = {"scan_ms": round(scan_ms, 2), "feed_and_stores_ms": round((time.perf_counter() - t0) * 1e3, 2),
                               "frame_store_bytes": fd.frames.nbytes, "track_store_bytes": fd.tracks.nbytes, "epoch_items": len(fd.sample_src)}
            ready = [p for _, p in zip(range(16), fd.plans())]  # plans for the two hand-driven legs
            turn = [0]

            def plan():
                turn[0] += 1
                return ready[turn[0] % len(ready)]

            def step(batch):
                ddp.zero_grad()
                m.training_step(batch, 0)["loss"].backward()
                ddp.finish()

            rest = {k: v for k, v in fd.tracks.collate(ready[0].items).items() if isinstance(v, torch.Tensor) and v.is_cuda}
            side = torch.cuda.Stream(dev)

            def issue():
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    p = plan()
                    fr, fi, _ = fd.frames.decode(p.items)
                    ev = torch.cuda.Event()
                    ev.record(side)
                return fr, fi, p.aug, ev
            state = [issue()]

            def store_leg():
                fr, fi, aug, ev = state[0]
                torch.cuda.current_stream().wait_event(ev)
                fr.record_stream(torch.cuda.current_stream())
                state[0] = issue()
                step(dict(rest, video=fr, video_aug=aug, video_frame_idx=fi))

            def hand_leg():
                p = plan()
                batch = fd.tracks.collate(p.items)
                batch["video"], batch["video_frame_idx"], _ = fd.frames.decode(p.items)
                batch["video_aug"] = p.aug
                step(batch)

            it = [iter(fd)]

            def feed_leg():
                step(next(it[0]))

            fd2 = F.AffWild2Feed(corpus, T, N, "train", hp.modality, True, 256, "vipl", hp.windows_per_epoch, visual=m.visual)
            fd2.tracks, fd2.frames = fd.tracks, fd.frames          # (the same stores: one copy of the corpus on the device)
            ahead_it = iter(fd2)

            def issue_feed():
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    batch = next(ahead_it)
                    ev = torch.cuda.Event()
                    ev.record(side)
                return batch, ev
            ahead = [None]

            def feed_ahead_leg():
                if ahead[0] is None:
                    ahead[0] = issue_feed()
                batch, ev = ahead[0]
                torch.cuda.current_stream().wait_event(ev)
                for v in batch.values():
                    if isinstance(v, torch.Tensor) and v.is_cuda:
                        v.record_stream(torch.cuda.current_stream())
                ahead[0] = issue_feed()
                step(batch)

            legs = rounds_of([store_leg, feed_ahead_leg, hand_leg, feed_leg], a.rounds, a.step_samples, a.inner)
            out["c5_step"] = {"store": legs[0], "feed_ahead": legs[1], "hand": legs[2], "feed": legs[3]}
            it[0].close()
            ahead_it.close()
            out["c5_host_per_batch"] = host_stages(fd, a.host_samples)
            del fd, m, ddp, rest, state

        N, T = a.audio_clips, a.audio_frames
        hp = hparams(modality="audio", window=T, batch_size=N, windows_per_epoch=many // a.videos)
        corpus = F.scan_affwild(path, "train", "audio", "vipl", 256, splits, False, T)
        torch.manual_seed(0)
        m = AffWild2VA(hp).to(dev).train()
        seeds()
        fd = F.AffWild2Feed(corpus, T, N, "train", "audio", windows_per_epoch=hp.windows_per_epoch).build_stores()
        ready = [p.items for _, p in zip(range(16), fd.plans())]
        turn = [0]

        def items():
            turn[0] += 1
            return ready[turn[0] % len(ready)]

        def astep(batch):
            for p in m.parameters():
                p.grad = None
            m.training_step(batch, 0)["loss"].backward()

        it = [iter(fd)]
        legs = rounds_of([lambda: astep(fd.tracks.collate(items())), lambda: astep(next(it[0]))], a.rounds, a.step_samples, a.inner)
        out["audio_step"] = {"batch": [N, T], "store_batches": legs[0], "feed": legs[1]}
        it[0].close()
        out["audio_host_per_batch"] = host_stages(fd, a.host_samples)
    out["note"] = ("c5_step: AffWild2VA audiovisual / attention training step (training_step + backward + clip) at %d x %d of 256-pixel frames; "
                   "audio_step: the audio-only step (training_step + backward); legs alternately in one process, %d rounds x %d samples x %d steps, "
                   "spread_ms = max - min of the rounds' medians; *_host_per_batch: host clock per stage with an idle queue, no synchronise inside"
                   % (a.clips, a.frames, a.rounds, a.step_samples, a.inner))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
