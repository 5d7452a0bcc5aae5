"""The AffWild2 mel tracks from the wavs, on the device: the reference's process/extract_melspec.py, rule for rule.

    python -m m3t.melspec SRC_WAV_DIR DST_DIR [--splits_dir splits]

  * `<splits_dir>/frames_fps.csv` lists `video,frames,fps`; only videos of fps >= 15 get a track (extract_melspec.py:32-39);
  * the wav of video `v` is SRC_WAV_DIR/v.wav with `_left` / `_right` taken out of the name: the two halves of a split-screen video share
    one sound track (:10);
  * a `.npy` that exists is left alone (:11);
  * `np.save(DST_DIR/v.npy, melspec_db(load_wave(wav), fps))`: float32 [rows, 40], rows = 1 + samples // hop (:13-20).  load_wave is
    `librosa.load(wav, sr=16000)` on the device (m3t/wav.py's wider reader, csrc/resample.hip), melspec_db the log-Mel of m3t/audio.py;
  * a file that fails is reported by name and the run goes on (:23-25); progress lines as the reference prints them (:45-46).

The reference spreads the files over 16 host processes; here the videos go one after the other through the device, shortest first, so
that the caching allocator grows its blocks step by step instead of splitting large ones, with ONE read-back per video (the track).
`pad_mode` is m3t.audio.melspec_db's ('constant' is librosa >= 0.10's STFT padding, 'reflect' the older one)."""
import argparse
import os
import sys

import numpy as np

from . import audio, wav


def tasks_from_csv(src_dir, dst_dir, splits_dir="splits"):
    """[(fps, wav path, npy path)] in the csv's order: extract_melspec.py:32-39 and the renaming of :10"""
    with open(os.path.join(splits_dir, "frames_fps.csv"), "r") as f:
        rows = [l.split(",") for l in f.read().splitlines()]
    tasks = []
    for vid_name, _, fps in rows:
        fps = float(fps)
        if fps >= 15:
            src = os.path.join(src_dir, vid_name.replace("_left", "").replace("_right", "") + ".wav")
            tasks.append((fps, src, os.path.join(dst_dir, vid_name + ".npy")))
    return tasks


def extract_melspec(task, pad_mode="constant"):
    """one video: 1 = the track was there already, 0 = written, -1 = failed (reported by name)"""
    fps, src_wav, dst_npy = task
    if os.path.exists(dst_npy):
        return 1
    try:
        spec = audio.melspec_db(audio.load_wave(src_wav), fps, pad_mode=pad_mode)
        np.save(dst_npy, spec.cpu().numpy())                         # (time, channels); the one read-back
        return 0
    except Exception as e:
        print("Exception on {}: {}".format(src_wav, e))
        return -1


def _frames(task):
    try:
        info = wav.probe_wave(task[1])
        return audio.converted_length(info.frames, info.rate)
    except (OSError, ValueError):
        return 0                                                     # (it fails again, by name, when its turn comes)


def run(src_dir, dst_dir, splits_dir="splits", pad_mode="constant"):
    """every task of the csv, shortest wav first -> {npy path: result}"""
    tasks = tasks_from_csv(src_dir, dst_dir, splits_dir)
    order = sorted(range(len(tasks)), key=lambda i: (_frames(tasks[i]), i))
    results, ncomplete = {}, 0
    for i in order:
        result = extract_melspec(tasks[i], pad_mode)
        results[tasks[i][2]] = result
        ncomplete += 1
        if result <= 0:
            print("Finished {}, result: {}, progress: {}/{}".format(tasks[i][1], result, ncomplete, len(tasks)), flush=True)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m m3t.melspec", description=__doc__.splitlines()[0])
    ap.add_argument("src_dir")
    ap.add_argument("dst_dir")
    ap.add_argument("--splits_dir", default="splits")
    ap.add_argument("--pad_mode", default="constant", choices=("constant", "reflect"))
    a = ap.parse_args(argv)
    run(a.src_dir, a.dst_dir, a.splits_dir, a.pad_mode)
    return 0


if __name__ == "__main__":
    sys.exit(main())
