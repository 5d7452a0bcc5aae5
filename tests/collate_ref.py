"""numpy restatement of the reference loader's `AffWild2SequenceDataset.__getitem__` minus `load_video` (models/dataset.py:241-343), written
from its rules with numpy's own slicing and np.pad, plus the default collate (np.stack per key), the fixture videos of the collate tests and
direct `random` transcripts of the window plans.  It does not import the reference (whose loader needs cv2) and shares no code with
m3t/dataset.py or csrc/collate.hip."""
import random
from collections import OrderedDict

import numpy as np


def load_audio(mel, start, w_len, step=3, width=5):
    rows = []
    for i in range(w_len):
        ctx = mel[(start + i) * step:(start + i) * step + width]
        if len(ctx) < width:
            ctx = np.pad(ctx, ((0, width - len(ctx)), (0, 0)), "constant")
        rows.append(ctx.reshape(-1))
    return np.stack(rows)


def getitem(vid, name, start, track_len, window, split, se_dim=512, au_dim=256, step=3, width=5, n_mels=40):
    """one window of one video (a dict as m3t.dataset.layout takes it) -> the reference's item, numpy arrays"""
    item = {"vid_name": name, "start": start, "length": track_len}
    pad = window - track_len
    for key, kind, dim in (("se_features", "se", se_dim), ("au_features", "au", au_dim)):
        if vid.get(kind) is None:
            continue
        f = vid[kind][start:start + track_len, :dim].transpose()
        if f.shape[-1] < track_len:
            f = np.pad(f, ((0, 0), (0, track_len - f.shape[-1])), "edge")
        if pad:
            f = np.pad(f, ((0, 0), (0, pad)), "edge")
        item[key] = np.ascontiguousarray(f)
    if "mel" in vid or vid["fps"] < 15:
        if vid["fps"] < 15:
            audio = np.zeros((window, width * n_mels), np.float32)
        else:
            audio = load_audio(vid["mel"], start, track_len, step, width)
        if len(audio) < window:
            audio = np.pad(audio, ((0, window - len(audio)), (0, 0)), "edge")
        item["audio"] = audio[:window]
    if split != "test":
        va = vid["va"][start:start + track_len]
        has_expr = vid.get("expr") is not None
        expr = vid["expr"][start:start + track_len].astype(np.int64) if has_expr else np.zeros(track_len, np.int64)
        valid = np.array([has_expr] * track_len) & (expr >= 0)
        expr = np.clip(expr, 0, 6)
        if pad:
            va = np.pad(va, ((0, pad), (0, 0)), "edge")
            expr = np.pad(expr, (0, pad), "edge")
            valid = np.pad(valid, (0, pad), "edge")
        item["label_valence"], item["label_arousal"] = va[..., 0], va[..., 1]
        item["class_expr"], item["expr_valid"] = expr, valid
    return item


def batch(videos, items, window, split, audio=True, **kw):
    """the DataLoader's default collate of getitem over `items` = [(name, start, track_len)]: np.stack per key, names as a list"""
    rows = [getitem(videos[name], name, start, tl, window, split, **kw) for name, start, tl in items]
    out = {"vid_name": [r["vid_name"] for r in rows], "start": np.array([r["start"] for r in rows], np.int64),
           "length": np.array([r["length"] for r in rows], np.int64)}
    for k in rows[0]:
        if k not in out and (audio or k != "audio"):
            out[k] = np.stack([r[k] for r in rows])
    return out


DTYPES = {"se_features": np.float32, "au_features": np.float32, "audio": np.float32, "label_valence": np.float32,
          "label_arousal": np.float32, "class_expr": np.int64, "expr_valid": np.bool_}


def fixture(se_width=512, au_width=268, n_mels=40, seed=0, au=True, se=True):
    """the four videos of the collate tests: A 23 frames with expr labels holding -1 and 7 and 71 mel rows; B 17 frames whose se track has
    only 15 rows, no expr labels, 40 mel rows (the contexts run out mid-window); C 9 frames at 12 fps (zero audio); D 16 plain frames"""
    rs = np.random.RandomState(seed)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)

    def vid(n, fps, se_rows=None, mel_rows=None, expr=True):
        d = {"nb_frames": n, "fps": fps, "mel": f32(mel_rows or 3 * n + 2, n_mels),
             "va": rs.uniform(-1, 1, (n, 2)).astype(np.float32), "has_image": rs.uniform(size=n) < 0.8}
        if se:
            d["se"] = f32(se_rows or n, se_width)
        if au:
            d["au"] = f32(n, au_width)
        if expr:
            d["expr"] = rs.randint(0, 7, n).astype(np.int64)
        return d
    v = OrderedDict()
    v["A"] = vid(23, 30.0, mel_rows=71)
    v["A"]["expr"][[2, 9, 22]] = -1
    v["A"]["expr"][[5, 17]] = 7
    v["A"]["va"][4] = (-5.0, -5.0)                       # an unannotated frame: passes through as stored
    v["B"] = vid(17, 25.0, se_rows=15, mel_rows=40, expr=False)
    v["C"] = vid(9, 12.0, mel_rows=9)
    v["D"] = vid(16, 30.0)
    return v


def train_transcript(n_videos, windows_per_epoch, avail, seed):
    """what the reference draws from `random` for one epoch read in order: shuffle in __init__ (:137-138), choice per __getitem__ (:246)"""
    random.seed(seed)
    src = list(range(n_videos)) * windows_per_epoch
    random.shuffle(src)
    return [(v, random.choice(avail[v])) for v in src]
