#!/usr/bin/env python3
"""Time what the AudioSet feed's training-time augmentation costs on one MI355X: the pre-training step (training_step + backward,
num_hidden 256) at the reference's shape -- 128 clips x 32 frames out of the resident store, the corpus and the method of
tools/audioset_feed_bench.py -- fed three ways:

  (a) off          AudioSetFeed as it was: m3t_audio_db_stack, m3t_label_rows
  (b) masks        spec_augment (the reference's defaults: F = T = 20, one mask each): m3t_audio_db_stack_aug without a partner
  (c) masks+mixup  (b) and mixup_alpha: m3t_audio_db_stack_aug reading a second spectrogram per clip, m3t_label_rows_mix

The legs alternate in one process; each sample is a host clock around `--inner` steps that end in a device synchronise; `--rounds` rounds of
`--samples` samples; per leg the median of the rounds' medians and their spread.  (a) is the `step_store` leg of audioset_feed_bench: the
same kernels, so the two figures should sit inside each other's spreads.  The ingest's last kernel is also timed alone for the three legs,
on the spectrogram of one batch, with the bytes it has to move: per clip its nf x 40 spectrogram once (the maximum; the second pass over
the 3T + 2 rows it shows is served by the cache) and the [T, 200] rows it writes, plus the partner's spectrogram when mixing.

    python tools/audioset_aug_bench.py [--files 512] [--clips 128] [--frames 32] [--seconds 10] [--rounds 3] [--samples 9] [--inner 20] [--mixup_alpha 0.5]
"""
import argparse
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "m3f.pytorch_amd"), os.path.join(ROOT, "tools")]

from audioset_feed_bench import alternate, median, summary, write_corpus  # noqa: E402


def spectrogram(store, table, tab, N, R):
    """the ingest's launches up to the mel spectrogram [R, 40] (m3t.audio.ingest_planned without its last kernel)"""
    from m3t import _lib, audio
    from m3t.ops import lib, _stream, _p, sgemm
    dev, bins = store.wave.device, 1 + audio.N_FFT // 2
    win, dft, _ = audio._constants(dev)
    weights, bands, nnz = audio._mel_sparse(dev)
    frames = torch.empty(R, audio.N_FFT, dtype=torch.float32, device=dev)
    _lib.check(lib().m3t_audio_frame_batch(store.wave.data_ptr(), 1 if store.wave.dtype == torch.int16 else 0, store.wave.numel(), tab.data_ptr(), N, R,
                                           audio.N_FFT, 0, _p(win), _p(frames), _stream()), "m3t_audio_frame_batch")
    spec = torch.empty(R, 2 * bins, dtype=torch.float32, device=dev)
    sgemm(0, 0, R, 2 * bins, audio.N_FFT, frames, 0, audio.N_FFT, dft, 0, 2 * bins, spec, 0, 2 * bins, prec=0, exclusive=True)
    mel = torch.empty(R, audio.N_MELS, dtype=torch.float32, device=dev)
    _lib.check(lib().m3t_audio_power_mel(_p(spec), R, bins, audio.N_MELS, _p(weights), bands.data_ptr(), nnz, _p(mel), _stream()), "m3t_audio_power_mel")
    return mel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--mixup_alpha", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audioset_aug_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import _lib, audio, audioset
    from m3t.ops import lib, _stream, _p
    from models.audioset_model import AudioSet
    dev = torch.device("cuda", 0)
    N, T, S = a.clips, a.frames, int(a.seconds * 16000)
    if a.files < N:
        raise SystemExit("--files must be at least --clips")
    options = [("off", {}), ("masks", {"spec_augment": True}), ("masks_mixup", {"spec_augment": True, "mixup_alpha": a.mixup_alpha})]
    with tempfile.TemporaryDirectory() as root:
        write_corpus(root, a.files, S)
        scan = audioset.scan_audioset(root, "train")
        feeds, plans = [], []
        for _, kw in options:
            random.seed(0)
            np.random.seed(0)
            torch.manual_seed(0)
            feed = audioset.AudioSetFeed(scan, T, N, "train", **kw)
            if feeds:
                feed.store = feeds[0].store                                    # one resident store behind the three feeds
            feed.build_store()
            feeds.append(feed)
            plans.append([p for p in feed.plan_epoch(0) if len(p.items) == N])
    store = feeds[0].store

    hp = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    hp.window = T
    torch.manual_seed(0)
    m = AudioSet(hp).to(dev).train()

    def step(batch):
        for p in m.parameters():
            p.grad = None
        m.training_step(batch, 0)["loss"].backward()

    turn = [0]

    def leg(i):
        def run():
            turn[0] += 1
            step(feeds[i].batch(plans[i][turn[0] % len(plans[i])]))
        return run

    rounds = [alternate([leg(i) for i in range(3)], a.samples, a.inner) for _ in range(a.rounds)]
    res = [summary([r[i] for r in rounds]) for i in range(3)]
    feed_ms = [median(alternate([lambda i=i: feeds[i].batch(plans[i][0])], 9, 10)[0]) for i in range(3)]

    # the last kernel alone, on one batch's spectrogram: the three forms of its launch
    plan = plans[2][0]
    items, table, R = store.plan(plan.items, plan.aug, T)
    plain = [{k: d[k] for k in ("fps", "hop", "start", "nsamples")} for d in plan.aug]
    out = torch.empty(N, T, 5 * audio.N_MELS, dtype=torch.float32, device=dev)
    kernels, tables = [], []
    for draws, mix in ((plain, None), (plan.aug, None), (plan.aug, plan.mix)):
        t = audio.plan_aug(draws, table, mix)
        flat, split = audio.pack_tables(table, t)
        tab, aug_tab, _ = split(torch.from_numpy(flat).to(dev))
        tables.append((tab, aug_tab))
    mel = spectrogram(store, table, tables[0][0], N, R)
    for tab, aug_tab in tables:
        if aug_tab is None:
            kernels.append(lambda tab=tab: _lib.check(lib().m3t_audio_db_stack(_p(mel), R, tab.data_ptr(), N, T, audio.N_MELS, 3, 5, 1e-10, 80.0,
                                                                                _p(out), _stream()), "m3t_audio_db_stack"))
        else:
            kernels.append(lambda tab=tab, g=aug_tab: _lib.check(lib().m3t_audio_db_stack_aug(_p(mel), R, tab.data_ptr(), N, g[0].data_ptr(), g[1].data_ptr(),
                                                                                             T, audio.N_MELS, 3, 5, 1e-10, 80.0, _p(out), _stream()),
                                                                 "m3t_audio_db_stack_aug"))
    k_rounds = [alternate(kernels, 9, 200) for _ in range(a.rounds)]
    k_res = [summary([r[i] for r in k_rounds]) for i in range(3)]
    own = int(table[:, 5].sum()) * audio.N_MELS * 4 + out.numel() * 4
    k_bytes = [own, own, own + int(table[np.asarray(plan.mix[0]), 5].sum()) * audio.N_MELS * 4]
    for r, b in zip(k_res, k_bytes):
        r["bytes"] = b
        r["gb_per_s"] = round(b / (r["median_ms"] * 1e-3) / 1e9, 1)

    spread = lambda r: r["spread_ms"][1] - r["spread_ms"][0]
    print(json.dumps({
        "tool": "audioset_aug_bench", "clips": N, "frames": T, "samples_per_clip": S, "files": a.files, "mixup_alpha": a.mixup_alpha,
        "step_off": res[0], "step_masks": res[1], "step_masks_mixup": res[2],
        "masks_minus_off_ms": round(res[1]["median_ms"] - res[0]["median_ms"], 4),
        "masks_mixup_minus_off_ms": round(res[2]["median_ms"] - res[0]["median_ms"], 4),
        "widest_round_spread_ms": round(max(spread(r) for r in res), 4),
        "feed_batch_alone_ms": {name: round(v, 4) for (name, _), v in zip(options, feed_ms)},
        "last_kernel_off": k_res[0], "last_kernel_masks": k_res[1], "last_kernel_masks_mixup": k_res[2],
        "spectrogram_rows": R,
        "note": "training_step + backward of AudioSet (num_hidden %d); legs alternate in one process, %d rounds x %d samples x %d steps; "
                "median_ms = median of the rounds' medians, spread_ms = their min and max; plans made ahead; the last kernel alone: %d rounds x 9 "
                "samples x 200 back-to-back launches (launch overhead included), bytes = the spectrograms it must read once + the rows it writes"
                % (hp.num_hidden, a.rounds, a.samples, a.inner, a.rounds)}), flush=True)


if __name__ == "__main__":
    main()
