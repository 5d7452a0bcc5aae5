#!/usr/bin/env python3
"""Generate tests/golden/feed_cases.npz: a tiny synthetic Aff-Wild2 tree and what the REFERENCE's loader makes of it -- its
`AffWild2SequenceDataset` (models/dataset.py), loaded read-only by path and iterated through a `DataLoader(num_workers=0)`, for six
configurations.  Only recorded data is written: the tree's files, the items in order, a transcript of every `random.*` and
`np.random.randint` call (got by wrapping those functions, not by editing the reference), every non-video array of every batch, and for
`video` a CRC32 per frame plus the first batch in full.

The reference imports tqdm and cv2, both absent where this project is developed.  Two stub modules of our own stand in:
  tqdm   the identity.
  cv2    imread: a Pillow decode turned to BGR, None for a missing file (the device decode is pinned to Pillow's bits, m3t/jpeg.py);
         flip(img, 1): a reversal;
         resize: ONLY 224 x 224 -> 112 x 112, as `(a + b + c + d + 2) >> 2` over every 2 x 2 block.  That is this project's stated
         assumption about OpenCV's resize for an exact halving of an 8-bit image (m3t/video.py gives its source), NOT a run of OpenCV.

The tree (frames of 128 x 128, smooth content; window 4 or 5, batch 2 throughout):
  A   11 frames, expression labels holding -1 and 7, files 00001.jpg and 00006.jpg missing
  B    7 frames, no expression labels, an SE track two rows short
  C    5 frames at 12 fps, no mel file
  D    9 frames, frames 5..7 unannotated (-5, -5): the two window plans differ
  E    3 frames (val and test only): shorter than the window
  P, Q 5 frames of 256 x 256 each, a split of their own: the halving branch
With four training videos (two at 256) a training epoch of the visual modalities has an even number of items, so its last batch is full;
the short last batch is met by train/audio (C dropped: 9 items), val (9) and test (11).

    M3T_REFERENCE=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_feed.py
"""
import importlib.util
import io
import os
import random
import sys
import tempfile
import types
import zlib

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

BATCH = 2
#         name                 split    modality       window cutout resample input stride seed  run
CONFIGS = [("train_av_cutout", "train", "audiovisual", 4, True, False, 128, 1, 11, "run128"),
           ("train_v_resample", "train", "visual", 5, False, True, 128, 1, 12, "run128"),
           ("train_audio", "train", "audio", 4, False, False, 128, 1, 13, "run128"),
           ("val_av", "val", "audiovisual", 4, False, False, 128, 1, 14, "run128"),
           ("test_av", "test", "audiovisual", 4, False, False, 128, 2, 15, "run128"),
           ("train_v_256", "train", "visual", 4, True, False, 256, 1, 16, "run256")]
WINDOWS_PER_EPOCH = 3


# ---- the stubs ------------------------------------------------------------------------------------------------------------------------
def _imread(path):
    if not os.path.exists(path):
        return None
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def _flip(img, code):
    assert code == 1
    return img[:, ::-1]


def _resize(img, size):
    assert img.shape == (224, 224, 3) and tuple(size) == (112, 112) and img.dtype == np.uint8, "the stub halves 224 -> 112 and nothing else"
    s = img.astype(np.uint16)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def load_reference():
    ref = os.environ.get("M3T_REFERENCE")
    if not ref:
        raise SystemExit("set M3T_REFERENCE to the reference's checkout")
    cv2 = types.ModuleType("cv2")
    cv2.imread, cv2.flip, cv2.resize = _imread, _flip, _resize
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, **kw: it
    sys.modules["cv2"], sys.modules["tqdm"] = cv2, tqdm
    spec = importlib.util.spec_from_file_location("reference_dataset", os.path.join(ref, "models", "dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the tree -------------------------------------------------------------------------------------------------------------------------
def _frame(size, v, k):
    """a smooth colour picture that differs per video and frame, and is not mirror symmetric"""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64) / size
    r = 128 + 100 * np.sin(2.0 * x + 0.7 * v + 0.3 * k) * np.cos(1.3 * y)
    g = 40 + 170 * x * (1 - 0.5 * y) + 5 * k
    b = 128 + 90 * np.cos(3.0 * y + 0.5 * v) + 30 * x - 4 * k
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def _jpeg(img):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=85)
    return buf.getvalue()


def _npy(a):
    buf = io.BytesIO()
    np.save(buf, a)
    return buf.getvalue()


def build_tree():
    """-> {relative path: bytes}"""
    rs = np.random.RandomState(2026)
    q = lambda *shape: (rs.randint(-48, 49, shape) / 16.0).astype(np.float32)     # few distinct values: the file compresses
    files = {}
    #        name frames fps  size missing   se rows expr  mel
    videos = [("A", 11, 30.0, 128, (0, 5), None, True, True),
              ("B", 7, 25.0, 128, (), 5, False, True),
              ("C", 5, 12.0, 128, (), None, True, False),
              ("D", 9, 30.0, 128, (), None, True, True),
              ("E", 3, 30.0, 128, (), None, True, True),
              ("P", 5, 30.0, 256, (), None, True, True),
              ("Q", 5, 25.0, 256, (), None, False, True)]
    fps_lines = []
    for vi, (name, n, fps, size, missing, se_rows, has_expr, has_mel) in enumerate(videos):
        fps_lines.append("%s,%d,%s" % (name, n, fps))
        for k in range(n):
            if k not in missing:
                files["data/face_%d/%s/%05d.jpg" % (size, name, k + 1)] = _jpeg(_frame(size, vi, k))
        va = rs.randint(-64, 65, (n, 2)) / 64.0
        if name == "D":
            va[5:8] = -5.0
        expr = rs.randint(0, 7, n)
        if name == "A":
            expr[[2, 9]] = -1
            expr[[4, 7]] = 7
        va_txt = "valence,arousal\n" + "".join("%.6f,%.6f\n" % (a, b) for a, b in va)
        ex_txt = "Neutral,Anger,Disgust,Fear,Happiness,Sadness,Surprise\n" + "".join("%d\n" % e for e in expr)
        for fold in ("Training_Set", "Validation_Set"):
            if fold == "Training_Set" and name == "E":
                continue
            if fold == "Validation_Set" and name not in "ACDE":
                continue
            files["data/annotations/VA_Set/%s/%s.txt" % (fold, name)] = va_txt.encode()
        if has_expr:
            files["data/annotations/EXPR_Set/%s/%s.txt" % ("Validation_Set" if name == "E" else "Training_Set", name)] = ex_txt.encode()
        files["data/se101_feats/%s.npy" % name] = _npy(q(se_rows or n, 512))
        files["data/AU_feats/%s.npy" % name] = _npy(q(n, 268))
        if has_mel:
            files["data/mel_spec/%s.npy" % name] = _npy(q(3 * n + 1, 40))
    expr_csv = "".join("%s,%s\n" % (nm, "Validation_Set" if nm == "E" else "Training_Set") for nm, *_, he, _ in videos if he)
    for run, splits in (("run128", {"train": "ABCD", "val": "AECD", "test": "ACE"}), ("run256", {"train": "PQ"})):
        files["%s/splits/frames_fps.csv" % run] = ("\n".join(fps_lines) + "\n").encode()
        files["%s/splits/expr.csv" % run] = expr_csv.encode()
        for split, names in splits.items():
            files["%s/splits/%s.csv" % (run, split)] = "".join("%s\n" % c for c in names).encode()
    return files


def write_tree(files, root):
    for rel, data in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(data)


# ---- the transcript -------------------------------------------------------------------------------------------------------------------
class Transcript:
    """wraps random.shuffle / choice / random / randint and np.random.randint; every call is recorded as (kind, argument, result):
    shuffle (length, 0 -- the shuffled list is kept beside it), choice (length, the value), random (0, the value), randint (b of
    randint(0, b), the value), np_randint (high, the value)"""

    def __init__(self):
        self.kind, self.arg, self.val, self.shuffled = [], [], [], []
        self.orig = {"shuffle": random.shuffle, "choice": random.choice, "random": random.random, "randint": random.randint,
                     "np_randint": np.random.randint}

    def rec(self, kind, arg, val):
        self.kind.append(kind)
        self.arg.append(int(arg))
        self.val.append(float(val))

    def __enter__(self):
        o = self.orig

        def shuffle(x):
            o["shuffle"](x)
            self.shuffled.append(list(x))
            self.rec("shuffle", len(x), 0)

        def choice(seq):
            v = o["choice"](seq)
            self.rec("choice", len(seq), v)
            return v

        def rnd():
            v = o["random"]()
            self.rec("random", 0, v)
            return v

        def randint(a, b):
            assert a == 0
            v = o["randint"](a, b)
            self.rec("randint", b, v)
            return v

        def np_randint(high):
            v = o["np_randint"](high)
            self.rec("np_randint", high, v)
            return v

        random.shuffle, random.choice, random.random, random.randint, np.random.randint = shuffle, choice, rnd, randint, np_randint
        return self

    def __exit__(self, *exc):
        o = self.orig
        random.shuffle, random.choice, random.random, random.randint, np.random.randint = (
            o["shuffle"], o["choice"], o["random"], o["randint"], o["np_randint"])


# ---- the run --------------------------------------------------------------------------------------------------------------------------
def record(ref, root, cfg, out):
    name, split, modality, window, cutout, resample, input_size, stride, seed, run = cfg
    os.chdir(os.path.join(root, run))                        # the reference opens splits/... and its cache files relative to the directory it runs in
    for f in os.listdir("."):
        if f.endswith(".pkl"):
            os.remove(f)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    pre = "%s." % name
    with Transcript() as tr:
        ds = ref.AffWild2SequenceDataset(split, os.path.join(root, "data"), window, WINDOWS_PER_EPOCH, cutout, "vipl", input_size, modality,
                                         resample, stride)
        loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=split == "train", num_workers=0)
        names, starts, lengths, crcs = [], [], [], []
        n_batches = 0
        for b, batch in enumerate(loader):
            n_batches += 1
            names.extend(batch["vid_name"])
            starts.extend(batch["start"].tolist())
            lengths.extend(batch["length"].tolist())
            for k, v in batch.items():
                if k in ("vid_name", "start", "length"):
                    continue
                v = v.numpy()
                if k != "video":
                    out["%sb%d.%s" % (pre, b, k)] = v
                    continue
                assert v.dtype == np.float32 and v.shape[1:] == (3, window, 112, 112)
                for n in range(v.shape[0]):
                    crcs.append([zlib.crc32(np.ascontiguousarray(v[n, :, t]).tobytes()) for t in range(window)])
                if b == 0:
                    # uint8, the cutout's fill 127.5 (the only value that is no integer) recorded as 0: what the normalisation
                    # maps it to, and what the ingest writes there under the identity table
                    whole = np.where(v == 127.5, 0, v)
                    assert np.array_equal(whole, np.floor(whole)) and whole.min() >= 0 and whole.max() <= 255
                    out[pre + "video0"] = whole.astype(np.uint8)
    out[pre + "args"] = np.array([window, int(cutout), int(resample), input_size, stride, seed, WINDOWS_PER_EPOCH, BATCH, n_batches], np.int64)
    out[pre + "strs"] = np.array([split, modality, run])
    out[pre + "vid_name"], out[pre + "start"], out[pre + "length"] = np.array(names), np.array(starts, np.int64), np.array(lengths, np.int64)
    out[pre + "tr_kind"], out[pre + "tr_arg"], out[pre + "tr_val"] = np.array(tr.kind), np.array(tr.arg, np.int64), np.array(tr.val, np.float64)
    if tr.shuffled:
        out[pre + "shuffled"] = np.array(tr.shuffled[0], np.int64)
    if crcs:
        out[pre + "crc"] = np.array(crcs, np.uint32)
    out[pre + "torch_state_crc"] = np.array([zlib.crc32(torch.get_rng_state().numpy().tobytes())], np.uint32)
    out[pre + "files"] = np.array(ds.files)
    out[pre + "nb_frames"] = np.array([ds.nb_frames[f] for f in ds.files], np.int64)
    if split != "test":
        for f in ds.files:
            out["%sva.%s" % (pre, f)] = ds.labels_va[f]
            if f in ds.labels_expr:
                out["%sexpr.%s" % (pre, f)] = ds.labels_expr[f]
    if split == "train":
        for f in ds.files:
            out["%savail.%s" % (pre, f)] = np.array(ds.avail_windows[f], np.int64)
        caches = [f for f in os.listdir(".") if f.endswith(".pkl")]
        assert len(caches) == 1
        out[pre + "cache_name"] = np.array(caches)
    kinds = set(tr.kind)
    print("%-18s %2d items in %d batches, %3d draws (%s)" % (name, len(names), n_batches, len(tr.kind), ", ".join(sorted(kinds))))
    return tr


def main():
    ref = load_reference()
    files = build_tree()
    out = {"tree/" + rel: np.frombuffer(data, np.uint8) for rel, data in files.items()}
    out["configs"] = np.array([c[0] for c in CONFIGS])
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as root:
        write_tree(files, root)
        try:
            trs = {cfg[0]: record(ref, root, cfg, out) for cfg in CONFIGS}
        finally:
            os.chdir(cwd)
    # what the set is there to cover
    mirrors = [v > 0.5 for k, v in zip(trs["train_av_cutout"].kind, trs["train_av_cutout"].val) if k == "random"]
    assert any(mirrors) and not all(mirrors)
    assert "np_randint" in trs["train_av_cutout"].kind and "np_randint" in trs["train_v_256"].kind
    assert set(trs["train_audio"].kind) == {"shuffle", "choice"} and set(trs["val_av"].kind) == {"random"}
    assert not np.array_equal(out["train_av_cutout.va.D"], out["train_v_resample.va.D"])
    assert out["train_v_resample.avail.D"].tolist() != out["train_av_cutout.avail.D"].tolist()
    assert list(out["train_audio.files"]) == ["A", "B", "D"]
    for name in ("train_audio", "val_av", "test_av"):
        assert len(out[name + ".start"]) % BATCH == 1, name
    assert out["val_av.length"].min() < 4 and out["test_av.length"].min() == 1
    path = os.path.join(HERE, "feed_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote feed_cases.npz %7.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
