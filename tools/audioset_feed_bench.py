#!/usr/bin/env python3
"""Time the AudioSet pre-training step (training_step + backward, num_hidden 256) at the reference's shape -- 128 clips x 32 frames, 10 s
of 16 kHz int16 PCM per clip, the training draws of tools/audio_ingest_bench.py -- on one MI355X, fed three ways:

  (a) features   ready [128, 32, 200] features on the device (no input stage at all)
  (b) host PCM   a pinned host int16 batch [128, 160000] through m3t.audio.ingest: the whole clips cross the bus every step
  (c) store      the epoch feed of m3t/audioset.py: the clips resident on the device, a batch = one table upload, the label launch and the
                 ingest's launches reading the crops in place (the BatchPlans are made ahead, as the draws of (b) are; their host cost is
                 reported beside it, and a fourth leg iterates the feed itself, the epoch's draws made inside the loop)

The legs alternate in one process; each sample is a host clock around `--inner` steps that end in a device synchronise; `--rounds` rounds of
`--samples` samples; per leg the median of the rounds' medians and their spread (min .. max) are printed as one JSON line, with the host
milliseconds a batch costs (plan: the loader's draws; table: validation + the per-clip table), the label launch alone, the store's bytes
and its build time per 1 000 files.  The tool writes its own corpus (`--files` synthetic clips, 320 KB each) into a temporary folder.

    python tools/audioset_feed_bench.py [--files 512] [--clips 128] [--frames 32] [--seconds 10] [--rounds 3] [--samples 9] [--inner 20]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
import wave

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


def median(xs):
    return sorted(xs)[len(xs) // 2]


def summary(rounds):
    """rounds: [[samples] per round] -> the median of the rounds' medians, their spread, and the extreme samples"""
    meds = [median(r) for r in rounds]
    flat = [x for r in rounds for x in r]
    return {"median_ms": round(median(meds), 4), "round_medians_ms": [round(m, 4) for m in meds], "spread_ms": [round(min(meds), 4), round(max(meds), 4)],
            "min_ms": round(min(flat), 4), "max_ms": round(max(flat), 4)}


def write_corpus(root, files, S):
    """`files` clips of S samples (a 440 Hz tone + noise) with the three csv files of an AudioSet folder; class 0 .. 526, one or two labels"""
    rs = np.random.RandomState(0)
    t = np.arange(S) / 16000.0
    tone = 0.4 * np.sin(2 * np.pi * 440 * t)
    os.makedirs(os.path.join(root, "balanced_train_segments"))
    with open(os.path.join(root, "class_labels_indices.csv"), "w") as f:
        f.write("index,mid,display_name\n" + "".join('%d,/m/%05d,"Sound %d"\n' % (i, i, i) for i in range(527)))
    rows = ["# synthetic", "# num_ytids=%d" % files, "# YTID, start_seconds, end_seconds, positive_labels"]
    for k in range(files):
        y = np.round((tone + 0.05 * rs.standard_normal(S)) * 32767.0).clip(-32768, 32767).astype("<i2")
        with wave.open(os.path.join(root, "balanced_train_segments", "clip%05d.wav" % k), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(y.tobytes())
        labels = sorted({int(rs.randint(527)), int(rs.randint(527))})
        rows.append('clip%05d, 0.000, 10.000, "%s"' % (k, ",".join("/m/%05d" % i for i in labels)))
    with open(os.path.join(root, "balanced_train_segments.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audioset_feed_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import audio, audioset, wav
    from models.audioset_model import AudioSet
    dev = torch.device("cuda", 0)
    N, T, S = a.clips, a.frames, int(a.seconds * 16000)
    if a.files < N:
        raise SystemExit("--files must be at least --clips")
    with tempfile.TemporaryDirectory() as root:
        write_corpus(root, a.files, S)
        scan = audioset.scan_audioset(root, "train")
        random.seed(0)
        torch.manual_seed(0)
        feed = audioset.AudioSetFeed(scan, T, N, "train")
        t0 = time.perf_counter()
        feed.build_store()
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        plans = [p for p in feed.plan_epoch(0) if len(p.items) == N]
        plan_ms = (time.perf_counter() - t0) * 1e3 / len(feed)
        # (b)'s batch: the clips of the first plan, decoded again into one pinned host array
        pcm = torch.from_numpy(np.stack([wav.read_pcm16(scan.files[i])[0] for i in plans[0].items])).pin_memory()
    store = feed.store
    t0 = time.perf_counter()
    for p in plans * 8:
        store.plan(p.items, p.aug, T)
    table_ms = (time.perf_counter() - t0) * 1e3 / (8 * len(plans))

    hp = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    hp.window = T
    torch.manual_seed(0)
    m = AudioSet(hp).to(dev).train()
    first = feed.batch(plans[0])
    feats, label = first["audio"], first["label"]
    err = float((audio.ingest(pcm, plans[0].aug, T) - feats).abs().max())          # the two routes of the same clips and draws: the same bits

    def step(batch):
        for p in m.parameters():
            p.grad = None
        m.training_step(batch, 0)["loss"].backward()

    turn = [0]

    def from_store():
        turn[0] += 1
        step(feed.batch(plans[turn[0] % len(plans)]))

    def epochs():
        epoch = 0
        while True:
            epoch += 1
            feed.set_epoch(epoch)
            for batch in feed:
                if batch["audio"].shape[0] == N:
                    yield batch

    drawn = epochs()
    legs = [lambda: step({"audio": feats, "label": label}),
            lambda: step({"audio": pcm, "audio_aug": plans[0].aug, "label": label}),
            from_store,
            lambda: step(next(drawn))]                                         # (c) with the epoch's draws made in the loop
    rounds = [alternate(legs, a.samples, a.inner) for _ in range(a.rounds)]
    res = [summary([r[i] for r in rounds]) for i in range(4)]
    items = torch.tensor(plans[0].items, dtype=torch.int64, device=dev)
    label_ms = median(alternate([lambda: store.label_rows(items, N)], 9, 50)[0])
    input_ms = median(alternate([lambda: feed.batch(plans[1 % len(plans)])], 9, 10)[0])
    print(json.dumps({
        "tool": "audioset_feed_bench", "clips": N, "frames": T, "samples_per_clip": S, "files": a.files,
        "step_features": res[0], "step_host_pcm": res[1], "step_store": res[2], "step_store_drawing_in_the_loop": res[3],
        "store_below_host_pcm_by_more_than_the_spreads": res[2]["spread_ms"][1] < res[1]["spread_ms"][0],
        "host_pcm_minus_store_ms": round(res[1]["median_ms"] - res[2]["median_ms"], 4),
        "store_minus_features_ms": round(res[2]["median_ms"] - res[0]["median_ms"], 4),
        "feed_batch_alone_ms": round(input_ms, 4), "label_launch_ms": round(label_ms, 4),
        "host_plan_ms_per_batch": round(plan_ms, 4), "host_table_ms_per_batch": round(table_ms, 4),
        "host_bytes_pcm_per_batch": int(pcm.numel()) * 2, "store_bytes": store.nbytes,
        "store_build_s_per_1000_files": round(build_s * 1000.0 / a.files, 3), "max_abs_diff_db_store_vs_host_pcm": round(err, 6),
        "note": "training_step + backward of AudioSet (num_hidden %d); legs alternate in one process, %d rounds x %d samples x %d steps; "
                "median_ms = median of the rounds' medians, spread_ms = their min and max; plans and draws made ahead for (b) and (c)"
                % (hp.num_hidden, a.rounds, a.samples, a.inner)}), flush=True)


if __name__ == "__main__":
    main()
