#!/usr/bin/env python3
"""Time the wave conversion (csrc/resample.hip, m3t.audio.decode_waves) on one MI355X, on a synthetic AudioSet folder of `--files` clips of
`--seconds` s at 44.1 kHz stereo 16-bit, beside the same clips written as 16 kHz mono 16-bit (the device's own conversion, rounded):

  store build     WaveStore(convert=True) over the 44.1 kHz folder against WaveStore() over the 16 kHz one, seconds per 1 000 files
                  (file reads included: the page cache is warm after the first round)
  convert launch  m3t_wave_convert over one chunk of raw bytes resident on the device, against the pinned host-to-device copy of those bytes
  AudioSet step   training_step + backward (num_hidden 256, `--clips` x `--frames`) fed by either store
  mel track       one `--track_seconds` s 44.1 kHz stereo wav through m3t.melspec.extract_melspec (load_wave + melspec_db + one read-back)

The legs of a pair alternate in one process; per leg the median of the rounds' medians and their spread (min .. max), as
tools/audioset_feed_bench.py reports them; one JSON line.

    python tools/resample_bench.py [--files 128] [--clips 64] [--frames 32] [--seconds 10] [--track_seconds 300] [--rounds 3] [--samples 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audioset_feed_bench import alternate, median, summary  # noqa: E402


def write_wav(path, pcm, rate):
    """int16 [frames, channels] -> a canonical 44-byte-header file"""
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, "<i2").tobytes())


def write_folders(root, files, frames):
    """two AudioSet folders with the same csv files: <root>/src (44.1 kHz stereo noise + a tone) and <root>/k16 (filled by the caller)"""
    rs = np.random.RandomState(0)
    tone = 0.3 * np.sin(2 * np.pi * 440 * np.arange(frames) / 44100.0)
    rows = ["# synthetic", "# num_ytids=%d" % files, "# YTID, start_seconds, end_seconds, positive_labels"]
    for sub in ("src", "k16"):
        os.makedirs(os.path.join(root, sub, "balanced_train_segments"))
        with open(os.path.join(root, sub, "class_labels_indices.csv"), "w") as f:
            f.write("index,mid,display_name\n" + "".join('%d,/m/%05d,"Sound %d"\n' % (i, i, i) for i in range(527)))
    for k in range(files):
        y = tone[:, None] + 0.1 * rs.standard_normal((frames, 2))
        write_wav(os.path.join(root, "src", "balanced_train_segments", "clip%05d.wav" % k), np.round(y * 32767).clip(-32768, 32767), 44100)
        rows.append('clip%05d, 0.000, 10.000, "/m/%05d"' % (k, k % 527))
    for sub in ("src", "k16"):
        with open(os.path.join(root, sub, "balanced_train_segments.csv"), "w") as f:
            f.write("\n".join(rows) + "\n")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--track_seconds", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import audio, audioset, melspec, wav
    from models.audioset_model import AudioSet
    dev = torch.device("cuda", 0)
    N, T = a.clips, a.frames
    if a.files < N:
        raise SystemExit("--files must be at least --clips")
    with tempfile.TemporaryDirectory() as root:
        write_folders(root, a.files, int(a.seconds * 44100))
        src = audioset.scan_audioset(os.path.join(root, "src"), "train", convert=True)
        flat, offs, lens = audio.decode_waves(src.files)
        for f, o, n in zip(src.files, offs, lens):                               # the same clips as a converted folder would hold them
            pcm = torch.round(flat[o:o + n] * 32767).clamp(-32768, 32767).to(torch.int16).cpu().numpy()
            write_wav(f.replace(os.sep + "src" + os.sep, os.sep + "k16" + os.sep), pcm[:, None], 16000)
        k16 = audioset.scan_audioset(os.path.join(root, "k16"), "train")
        assert k16.lengths().tolist() == src.lengths().tolist()

        # ---- store build, the two folders in turn
        build = [[], []]
        stores = [None, None]
        for _ in range(a.rounds + 1):                                            # (the first round warms the page cache and the allocator)
            for i, scan in enumerate((src, k16)):
                stores[i] = None
                s, stores[i] = timed(lambda: audioset.WaveStore(scan.files, scan.labels, scan.lengths(), convert=scan.convert))
                build[i].append(s * 1000.0 / a.files)
        build = [b[1:] for b in build]

        # ---- the convert launch against the copy of the same bytes
        bodies = [wav.read_wave(f) for f in src.files]
        infos = [b[1] for b in bodies]
        sizes = [int(b[0].shape[0]) for b in bodies]
        byte_offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        host = torch.from_numpy(np.concatenate([b[0] for b in bodies])).pin_memory()
        raw = torch.empty_like(host, device=dev)
        _, _, total, groups = audio.plan_convert(infos, byte_offs, host.numel())
        out = torch.empty(total, dtype=torch.float32, device=dev)
        legs = [lambda: raw.copy_(host, non_blocking=True), lambda: audio.convert_planned(raw, groups, out)]
        rounds = [alternate(legs, a.samples, a.inner) for _ in range(a.rounds)]
        copy_ms, conv_ms = (summary([r[i] for r in rounds]) for i in range(2))
        same_bits = bool(torch.equal(out, flat))

        # ---- the AudioSet step fed by either store
        hp = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
        hp.window = T
        torch.manual_seed(0)
        m = AudioSet(hp).to(dev).train()
        random.seed(0)
        draws = [audio.draw_audioset(int(src.lengths()[i]), T, True) for i in range(N)]
        items = list(range(N))

        def step(store):
            for p in m.parameters():
                p.grad = None
            m.training_step(store.batch(items, draws, T), 0)["loss"].backward()

        rounds = [alternate([lambda: step(stores[0]), lambda: step(stores[1])], a.samples, a.inner) for _ in range(a.rounds)]
        step_conv, step_16k = (summary([r[i] for r in rounds]) for i in range(2))

        # ---- one long track through m3t.melspec
        frames = int(a.track_seconds * 44100)
        rs = np.random.RandomState(1)
        track = os.path.join(root, "track.wav")
        write_wav(track, np.round(0.2 * rs.standard_normal((frames, 2)) * 32767).clip(-32768, 32767), 44100)
        mel = []
        for r in range(a.rounds + 1):
            dst = os.path.join(root, "track%d.npy" % r)
            s, rc = timed(lambda: melspec.extract_melspec((30.0, track, dst)))
            assert rc == 0
            mel.append(s * 1e3)
        rows = int(np.load(dst).shape[0])

    sm = lambda xs: {"median": round(median(xs), 3), "spread": [round(min(xs), 3), round(max(xs), 3)]}
    print(json.dumps({
        "tool": "resample_bench", "files": a.files, "seconds": a.seconds, "source": "44.1 kHz stereo int16",
        "store_build_s_per_1000_files_convert": sm(build[0]), "store_build_s_per_1000_files_16k": sm(build[1]),
        "store_bytes_convert": stores[0].nbytes, "store_bytes_16k": stores[1].nbytes,
        "raw_bytes": int(host.numel()), "h2d_copy_ms": copy_ms, "convert_launch_ms": conv_ms,
        "convert_gsamples_out_per_s": round(total / conv_ms["median_ms"] / 1e6, 3), "convert_equals_decode_waves_bits": same_bits,
        "step_ms_store_convert": step_conv, "step_ms_store_16k": step_16k, "clips": N, "frames": T,
        "mel_track_seconds": a.track_seconds, "mel_track_rows": rows, "mel_track_ms_first": round(mel[0], 2), "mel_track_ms": sm(mel[1:]),
        "note": "legs of a pair alternate in one process; %d rounds (after one warm-up round for the builds and the track); "
                "median = median of the rounds' medians, spread = their min and max" % a.rounds}), flush=True)


if __name__ == "__main__":
    main()
