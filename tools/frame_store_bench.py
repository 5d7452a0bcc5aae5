#!/usr/bin/env python3
"""Time the resident JPEG frame store (m3t.jpeg.FrameStore, csrc/frame_store.hip) on one MI355X against what it replaces: jpeg.pack of
every batch on the host.  The set is the 256 x 256 quality-95 4:2:0 fixture of tests/golden/jpeg_cases.npz, `--videos` videos of
`--video-frames` frames; a batch is `--clips` windows of `--frames` frames (8 x 64 = 512, one C5 step) at random starts.

  (a) host     the host time of one FrameStore.decode call with an idle queue (plan_frames, the small upload, issuing the launches; the
               clock stops before any synchronise), beside jpeg.pack of the same 512 frames in the same process
  (b) device   m3t_jpeg_gather alone, FrameStore.decode as a caller sees it, jpeg.decode of a pre-packed batch (copies included)
  (c) step     the C5 training step of tools/jpeg_bench.py fed four ways, the next batch issued on a side stream before the step:
               a ready pinned uint8 batch; pre-packed JpegBatches (pack left out); the store, everything per step included;
               and pack inside the loop on one core -- the parent's whole per-step cost; and the pre-packed feed given the identity
               frame index the store's feed carries, to tell the ingest's index table from the store's own cost
  (d) build    the store's nbytes and the one-time build time per frame

Routes alternate in one process, `--rounds` rounds; each sample is a host clock around `--inner` calls that end in a device
synchronise.  One JSON line.

    python tools/frame_store_bench.py [--rounds 3] [--samples 7] [--inner 3] [--step-samples 5] [--no-step]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_bench import alternate, summary  # noqa: E402


def rounds_of(fns, rounds, samples, inner):
    """alternate(), `rounds` times -> per function (summary over all samples, [median of each round])"""
    per = [[] for _ in fns]
    for _ in range(rounds):
        for i, ts in enumerate(alternate(fns, samples, inner)):
            per[i].append(ts)
    out = []
    for rs in per:
        meds = [sorted(r)[len(r) // 2] for r in rs]
        out.append(dict(summary([t for r in rs for t in r]), round_medians_ms=[round(m, 4) for m in meds], spread_ms=round(max(meds) - min(meds), 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--video-frames", type=int, default=256)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--step-samples", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_store_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import _lib, jpeg
    dev = torch.device("cuda", 0)
    data = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["full_256_q95.jpg"].tobytes()
    N, T = a.clips, a.frames
    videos = {"v%02d" % v: [data] * a.video_frames for v in range(a.videos)}
    t0 = time.perf_counter()
    store = jpeg.FrameStore(videos, T)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    n_frames = a.videos * a.video_frames
    out = {"tool": "frame_store_bench", "fixture_bytes": len(data), "batch": [N, T],
           "store": {"frames": n_frames, "nbytes": store.nbytes, "chunks": len(store.chunks), "build_ms": round(build_ms, 2),
                     "build_us_per_frame": round(1e3 * build_ms / n_frames, 2)}}
    rs = random.Random(0)
    batches = [[(rs.randrange(a.videos), rs.randrange(a.video_frames - T + 1)) for _ in range(N)] for _ in range(16)]
    turn = [0]

    def items():
        turn[0] += 1
        return batches[turn[0] % len(batches)]

    flat = [data] * (N * T)
    packed = jpeg.pack(flat, pin=True)
    frames, _, status = store.decode(batches[0])
    want, _ = jpeg.decode(packed)
    assert torch.equal(frames.view(N * T, 256, 256, 3), want) and not status.any().item()

    # (a) host time with an idle queue: the clock stops when the call returns, the synchronise comes after it
    host = {"store_decode": [], "plan_frames": [], "pack": []}
    for r in range(a.rounds):
        for name in ("store_decode", "plan_frames", "pack"):
            ts = []
            for _ in range(a.samples):
                torch.cuda.synchronize()
                it = items()
                t0 = time.perf_counter()
                if name == "store_decode":
                    store.decode(it)
                elif name == "plan_frames":
                    jpeg.plan_frames(store.records, it, T)
                else:
                    jpeg.pack(flat, pin=True)
                ts.append((time.perf_counter() - t0) * 1e3)
            host[name].append(ts)
    out["host_per_step"] = {k: dict(summary([t for r in v for t in r]), round_medians_ms=[round(sorted(r)[len(r) // 2], 4) for r in v])
                            for k, v in host.items()}

    # (b) device time
    p = jpeg.plan_frames(store.records, batches[0], T)
    s_d = torch.empty(p.stream_bytes, dtype=torch.uint8, device=dev)
    rows_h = np.ascontiguousarray(p.rows, np.int32)
    rows_d = torch.from_numpy(rows_h.reshape(-1)).to(dev)
    lib = _lib.load()

    def gather_resident():                                    # the launch alone: its table is on the device already
        _lib.check(lib.m3t_jpeg_gather(store._addr.ctypes.data, store._size.ctypes.data, len(store.chunks), store._addr_d.data_ptr(),
                                       rows_h.ctypes.data, rows_d.data_ptr(), rows_h.shape[0], s_d.data_ptr(), p.stream_bytes,
                                       torch.cuda.current_stream().cuda_stream), "m3t_jpeg_gather")

    dev_rows = rounds_of([gather_resident, lambda: store.decode(items()), lambda: jpeg.decode(packed)], a.rounds, a.samples, a.inner)
    out["device"] = {"gather": dev_rows[0], "store_decode": dev_rows[1], "decode_prepacked": dev_rows[2], "stream_bytes": p.stream_bytes}

    if not a.no_step:
        from m3t import video
        from m3t.ddp import FlatGradDDP
        from models.model import AffWild2VA
        np_rs = np.random.RandomState(0)
        random.seed(0)
        np.random.seed(0)
        aug = [video.draw_affwild(256, True, True, True, random.random() > 0.5, resize=True) for _ in range(N)]
        ready = torch.from_numpy(np_rs.randint(0, 256, (N, T, 256, 256, 3)).astype(np.uint8)).pin_memory()
        hp = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
        hp.modality, hp.fusion_type, hp.loss, hp.window = "audiovisual", "attention", "ccc_mtl", T
        torch.manual_seed(12345)
        m = AffWild2VA(hp).to(dev).train()
        f = lambda arr: torch.from_numpy(arr).to(dev)
        rest = {"se_features": f(np_rs.standard_normal((N, 512, T)).astype(np.float32)), "audio": f(np_rs.standard_normal((N, T, 200)).astype(np.float32)),
                "label_valence": f(np_rs.uniform(-1, 1, (N, T)).astype(np.float32)), "label_arousal": f(np_rs.uniform(-1, 1, (N, T)).astype(np.float32)),
                "class_expr": f(np_rs.randint(0, 7, (N, T)).astype(np.int64)), "expr_valid": f(np_rs.uniform(size=(N, T)) < 0.7)}
        ddp = FlatGradDDP(m, max_norm=1.0)
        side = torch.cuda.Stream(dev)

        def step(batch):
            ddp.zero_grad()
            m.training_step(batch, 0)["loss"].backward()
            ddp.finish()

        def fed(make):
            """a step whose frames were issued on the side stream before the previous step; make() -> (frames [N, T, ...], frame_idx)"""
            def issue():
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    fr, fi = make()
                    ev = torch.cuda.Event()
                    ev.record(side)
                return fr, fi, ev
            state = [issue()]

            def run():
                fr, fi, ev = state[0]
                torch.cuda.current_stream().wait_event(ev)
                fr.record_stream(torch.cuda.current_stream())
                state[0] = issue()
                batch = dict(rest, video=fr, video_aug=aug)
                if fi is not None:
                    batch["video_frame_idx"] = fi
                step(batch)
            return run

        # the store hands the step a frame index (here the identity: every frame is present); the pre-packed feed has none, so the ingest
        # skips that table -- the fifth route gives the pre-packed feed the same table, to tell that cost from the store's own
        identity = torch.arange(T, dtype=torch.int32).repeat(N, 1)

        def from_store():
            fr, fi, _ = store.decode(items())
            return fr, fi

        steps = rounds_of([lambda: step(dict(rest, video=ready, video_aug=aug)),
                           fed(lambda: (jpeg.decode(packed)[0].view(N, T, 256, 256, 3), None)),
                           fed(from_store),
                           fed(lambda: (jpeg.decode(jpeg.pack(flat, pin=True))[0].view(N, T, 256, 256, 3), None)),
                           fed(lambda: (jpeg.decode(packed)[0].view(N, T, 256, 256, 3), identity))],
                          a.rounds, a.step_samples, 3)
        out["c5_step"] = {"u8_ready": steps[0], "prepacked": steps[1], "store": steps[2], "pack_in_loop": steps[3],
                          "prepacked_with_frame_idx": steps[4]}
    out["note"] = ("host_per_step: host clock around one call with an idle queue, no synchronise inside; device: host clock around %d calls "
                   "ending in a synchronise; c5_step: AffWild2VA training step (training_step + backward + clip), the next batch issued on a "
                   "side stream before the step; routes alternately in one process, %d rounds x %d samples (steps: %d x 3); spread_ms = max - min "
                   "of the rounds' medians" % (a.inner, a.rounds, a.samples, a.step_samples))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
