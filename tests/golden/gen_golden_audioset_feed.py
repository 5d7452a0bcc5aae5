#!/usr/bin/env python3
"""Generate tests/golden/audioset_feed_cases.npz: a tiny synthetic AudioSet tree and what the REFERENCE's loader makes of it -- its
`AudioSetDataset` (models/audioset_dataset.py), loaded read-only by path and iterated through a `DataLoader(num_workers=0)` with the
arguments of the reference's `train_dataloader` / `val_dataloader` (models/audioset_model.py:129-145), for four configurations.  Only
recorded data is written: the tree's files, the items in order (got by wrapping `__getitem__` in a subclass), a transcript of every
`random.choice` / `random.randint` call (got by wrapping those functions, not by editing the reference), the `random` and torch generator
states after each epoch (as CRC32), and every batch's `audio` and `label`.

The reference imports librosa, which is absent where this project is developed.  A stub module of our own stands in:
  load                        a 16-bit mono read with Python's `wave` module, / 32768 to float32, the rate asserted to be 16 000;
  feature.melspectrogram      oracle.stft_power(y, n_fft, hop, win_length, "constant") @ oracle.mel_filterbank(sr, n_fft, n_mels).T, transposed;
  core.power_to_db            oracle.power_to_db.
That is this project's RESTATEMENT of librosa's published algorithm (m3t/audio.py gives its terms), NOT a run of librosa: the log-Mel
stays unpinned end to end, as DESIGN.md says.  What this file pins is everything around it: the scan, the order, the draws, the crop with
np.pad 'wrap', the stacking, the labels.

The tree (window 4, batch 2; tone + 0.05 noise, the signal of tests/audio_ingest_ref.py, as int16):
  train   a 16000 samples; b 3000, two labels, wraps at 15 / 17 / 19 fps; c 2133, exactly nsamples at 30 fps, wraps at every other rate;
          gone, listed without a file; d 9000, two labels, one of them class 526; e 4267, never wraps (nsamples is 4266 at 15 fps)
  val     v1 1000, wraps more than once; v2 2134; v3 8000
The class file's display names hold commas and quotes; the segment files have their three header lines and quoted label lists.

    M3T_REFERENCE=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_audioset_feed.py
"""
import importlib.util
import io
import os
import random
import sys
import tempfile
import types
import wave
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from oracle import m3t_oracle as O  # noqa: E402
import audio_ingest_ref as A  # noqa: E402

WINDOW, BATCH = 4, 2
#          name          split   epochs world rank seed
CONFIGS = [("train", "train", 2, 1, 0, 158),            # (a seed whose two epochs meet every branch named above: main() asserts it)
           ("val", "val", 1, 1, 0, 22),
           ("train_w2r0", "train", 1, 2, 0, 23),
           ("train_w2r1", "train", 1, 2, 1, 23)]
TRAIN = [("a", 16000, [0]), ("b", 3000, [3, 137]), ("c", 2133, [72]), ("gone", 0, [5]), ("d", 9000, [526, 1]), ("e", 4267, [300])]
VAL = [("v1", 1000, [4]), ("v2", 2134, [526, 0, 9]), ("v3", 8000, [137])]


# ---- the stub -------------------------------------------------------------------------------------------------------------------------
def _load(path, sr=None):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2 and w.getframerate() == 16000 == sr
        y = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    return y.astype(np.float32) / np.float32(32768.0), 16000


def _melspectrogram(y=None, sr=None, n_fft=None, hop_length=None, win_length=None, n_mels=None):
    return (O.stft_power(y, n_fft, hop_length, win_length, "constant") @ O.mel_filterbank(sr, n_fft, n_mels).T).T


def load_reference():
    ref = os.environ.get("M3T_REFERENCE")
    if not ref:
        raise SystemExit("set M3T_REFERENCE to the reference's checkout")
    librosa = types.ModuleType("librosa")
    librosa.load = _load
    librosa.feature = types.ModuleType("librosa.feature")
    librosa.feature.melspectrogram = _melspectrogram
    librosa.core = types.ModuleType("librosa.core")
    librosa.core.power_to_db = O.power_to_db
    sys.modules["librosa"], sys.modules["librosa.feature"], sys.modules["librosa.core"] = librosa, librosa.feature, librosa.core
    spec = importlib.util.spec_from_file_location("reference_audioset_dataset", os.path.join(ref, "models", "audioset_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the tree -------------------------------------------------------------------------------------------------------------------------
def mid(i):
    return "/m/%05x" % (7919 * i + 11) if i % 3 else "/t/dd%05d" % i


def _wav(n, seed):
    y = np.clip(np.round(A.signal(n, seed).astype(np.float64) * 32767.0), -32768, 32767).astype("<i2")
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(y.tobytes())
    return buf.getvalue()


def build_tree():
    """-> {relative path: bytes}"""
    files = {}
    lines = ["index,mid,display_name"]
    for i in range(527):
        name = "Sound %d" % i
        if i % 5 == 0:
            name = 'Sound %d, the "loud" kind, and others' % i
        lines.append('%d,%s,"%s"' % (i, mid(i), name.replace('"', '""')))
    files["class_labels_indices.csv"] = ("\n".join(lines) + "\n").encode()
    for fold, clips, seed0 in (("balanced_train_segments", TRAIN, 100), ("eval_segments", VAL, 200)):
        rows = ["# Segments csv created Sun Mar  5 10:54:31 2017",
                "# num_ytids=%d, num_segs=%d, num_unique_labels=527, num_positive_labels=%d" % (len(clips), len(clips), sum(len(c[2]) for c in clips)),
                "# YTID, start_seconds, end_seconds, positive_labels"]
        for k, (name, n, labels) in enumerate(clips):
            rows.append('%s, %d.000, %d.000, "%s"' % (name, 10 * k, 10 * k + 10, ",".join(mid(i) for i in labels)))
            if n:
                files["%s/%s.wav" % (fold, name)] = _wav(n, seed0 + k)
        files["%s.csv" % fold] = ("\n".join(rows) + "\n").encode()
    return files


def write_tree(files, root):
    for rel, data in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(data)


# ---- the transcript -------------------------------------------------------------------------------------------------------------------
class Transcript:
    """wraps random.choice and random.randint; every call is recorded as (kind, argument, result): choice (length, the value), randint (b of
    randint(0, b), the value)"""

    def __init__(self):
        self.kind, self.arg, self.val = [], [], []
        self.orig = (random.choice, random.randint)

    def __enter__(self):
        choice0, randint0 = self.orig

        def choice(seq):
            v = choice0(seq)
            self.kind.append("choice"), self.arg.append(len(seq)), self.val.append(float(v))
            return v

        def randint(a, b):
            assert a == 0
            v = randint0(a, b)
            self.kind.append("randint"), self.arg.append(int(b)), self.val.append(float(v))
            return v

        random.choice, random.randint = choice, randint
        return self

    def __exit__(self, *exc):
        random.choice, random.randint = self.orig


def crc(data):
    return np.array([zlib.crc32(data)], np.uint32)


# ---- the run --------------------------------------------------------------------------------------------------------------------------
def record(ref, root, cfg, out):
    name, split, epochs, world, rank, seed = cfg
    order = []

    class Recording(ref.AudioSetDataset):
        def __getitem__(self, i):
            order.append(int(i))
            return super().__getitem__(i)

    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    pre = "%s." % name
    ds = Recording(split, root, WINDOW)
    if world > 1:             # audioset_model.py:132-134, with the rank and world a process group would give
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rank)
        loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, num_workers=0, sampler=sampler)
    else:
        loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=split == "train", num_workers=0)
    sizes = []
    for e in range(epochs):
        del order[:]
        if world > 1:
            sampler.set_epoch(e)
        with Transcript() as tr:
            n_batches = 0
            for b, batch in enumerate(loader):
                n_batches += 1
                assert sorted(batch) == ["audio", "label"]
                audio, label = batch["audio"].numpy(), batch["label"].numpy()
                assert audio.shape[1:] == (WINDOW, 200) and np.isfinite(audio).all() and label.dtype == np.float32
                out["%se%d.b%d.audio" % (pre, e, b)] = audio
                out["%se%d.b%d.label" % (pre, e, b)] = label
                sizes.append(audio.shape[0])
        ep = "%se%d." % (pre, e)
        out[ep + "items"] = np.array(order, np.int64)
        out[ep + "tr_kind"], out[ep + "tr_arg"], out[ep + "tr_val"] = np.array(tr.kind), np.array(tr.arg, np.int64), np.array(tr.val, np.float64)
        out[ep + "random_crc"] = crc(repr(random.getstate()).encode())
        out[ep + "torch_crc"] = crc(torch.get_rng_state().numpy().tobytes())
        out[ep + "n_batches"] = np.array([n_batches], np.int64)
    out[pre + "args"] = np.array([WINDOW, BATCH, seed, epochs, world, rank], np.int64)
    out[pre + "split"] = np.array([split])
    out[pre + "files"] = np.array([os.path.relpath(f, root) for f, _ in ds.files])
    out[pre + "labels"] = np.stack([l for _, l in ds.files]).astype(np.uint8)
    assert all(set(np.unique(l)) <= {0.0, 1.0} for _, l in ds.files)
    print("%-12s %d clips, batches of %s, %d draws in the last epoch" % (name, len(ds), sizes, len(tr.kind)))
    return sizes


def main():
    ref = load_reference()
    files = build_tree()
    out = {"tree/" + rel: np.frombuffer(data, np.uint8) for rel, data in files.items()}
    out["configs"] = np.array([c[0] for c in CONFIGS])
    with tempfile.TemporaryDirectory() as root:
        write_tree(files, root)
        sizes = {cfg[0]: record(ref, root, cfg, out) for cfg in CONFIGS}
    # what the set is there to cover
    assert sizes["train"] == [2, 2, 1, 2, 2, 1] and sizes["val"] == [2, 1] and sizes["train_w2r0"] == sizes["train_w2r1"] == [2, 1]
    assert [os.path.basename(f) for f in out["train.files"]] == ["a.wav", "b.wav", "c.wav", "d.wav", "e.wav"]
    assert out["train.labels"].sum(1).tolist() == [1, 2, 1, 2, 1] and out["train.labels"][3, 526] == 1
    assert out["val.labels"].sum(1).tolist() == [1, 3, 1]
    assert out["train.e0.items"].tolist() != out["train.e1.items"].tolist() or out["train.e0.tr_val"].tolist() != out["train.e1.tr_val"].tolist()
    met = set()
    for e in (0, 1):                # (item, fps) pairs of the training epochs: b = 1, c = 2, e = 4
        fps = out["train.e%d.tr_val" % e][0::2].tolist()
        met |= set(zip(out["train.e%d.items" % e].tolist(), fps))
    assert (2, 30.0) in met and (4, 15.0) in met and any(i == 2 and f < 30 for i, f in met)
    assert any(i == 1 and f <= 19 for i, f in met) and any(i == 1 and f >= 22 for i, f in met)
    assert len(out["val.e0.tr_kind"]) == 0 and out["val.e0.items"].tolist() == [0, 1, 2]
    assert sorted(set(out["train_w2r0.e0.items"].tolist()) | set(out["train_w2r1.e0.items"].tolist())) == [0, 1, 2, 3, 4]
    path = os.path.join(HERE, "audioset_feed_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote audioset_feed_cases.npz %7.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
