"""numpy restatement of the video ingest (include/m3t_hip.h, m3t_video_ingest) and the golden cases' parameters, shared by
tests/test_ingest_host.py and tests/test_gpu_ingest.py.

    f = frame_idx[n][t];  v = 0 if f < 0 else frames[n][f][cy + y][cx + (W-1-x if mirror else x)][c]
    o = 0.0 inside the cutout else lut[n][v]

tests/golden/ingest.npz (tests/golden/gen_golden_ingest.py) holds what the reference's two `load_video` functions return for the same
frames, presence masks and seeds, normalised by torch's float32 `(x - 127.5) / 127.5` on the host.
"""
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def ingest_ref(frames, geom, frame_idx, lut, H, W, fill=0.0):
    """frames uint8 [N, Ts, Hs, Ws, 3], geom int [N, 8], frame_idx int [N, T] or None, lut float32 [256] or [N, 256] -> float32 [N, 3, T, H, W];
    fill: what the cutout writes (0.0 after normalisation; 127.5 before it, dataset.py:16)"""
    frames, geom, lut = np.asarray(frames), np.asarray(geom), np.asarray(lut, np.float32)
    N, Ts = frames.shape[:2]
    if frame_idx is None:
        frame_idx = np.tile(np.arange(Ts), (N, 1))
    frame_idx = np.asarray(frame_idx)
    T = frame_idx.shape[1]
    out = np.empty((N, 3, T, H, W), np.float32)
    for n in range(N):
        cy, cx, mirror, y1, y2, x1, x2 = (int(v) for v in geom[n, :7])
        tab = lut[n] if lut.ndim == 2 else lut
        for t in range(T):
            f = int(frame_idx[n, t])
            if f < 0:
                img = np.zeros((H, W, 3), np.uint8)
            else:
                img = frames[n, f, cy:cy + H, cx:cx + W]
                if mirror:
                    img = img[:, ::-1]
            o = tab[img]                                     # [H, W, 3]
            o[y1:y2, x1:x2] = fill
            out[n, :, t] = o.transpose(2, 0, 1)
    return out


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "ingest.npz"))
    cases = []
    for name in z["names"]:
        name = str(name)
        g = lambda k: z["%s.%s" % (name, k)]
        input_size, training, crop, cutout, start, length, window, seed = (int(v) for v in g("args"))
        cases.append({"name": name, "kind": name.split("_")[0], "frames": g("frames"), "present": g("present").astype(bool), "out": g("out"),
                      "input_size": input_size, "training": bool(training), "crop": bool(crop), "cutout": bool(cutout), "start": start,
                      "length": length, "window": window, "seed": seed})
    return cases


def case_params(video, c):
    """the draws and the frame indices of golden case `c` from m3t.video, under the case's seeds, as the reference's call sites consume them
    (dataset.py:256-261: the mirror draw, then load_video; vox2_dataset.py:89-92 likewise)"""
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    if c["kind"] == "aff":
        mirror = random.random() > 0.5
        aug = video.draw_affwild(c["input_size"], c["training"], c["crop"], c["cutout"], mirror)
    else:
        aug = video.draw_vox2(c["input_size"], c["training"], c["crop"])
    fidx = video.frame_index(c["present"], c["start"], c["length"], c["window"])
    return aug, fidx


def case_tables(video, aug, fidx, norm=None):
    """(geom [1, 8], frame_idx [1, T], lut [256]) of one clip for ingest_ref"""
    norm = video.norm_lut() if norm is None else norm
    geom = np.zeros((1, 8), np.int32)
    geom[0, :7] = (aug["cy"], aug["cx"], int(aug["mirror"])) + tuple(aug["cutout"] or (0, 0, 0, 0))
    lut = norm if aug["table"] is None else norm[aug["table"]]
    return geom, fidx[None], lut


def batch_ref(video, frames, aug=None, frame_idx=None, norm=None, raw=False):
    """ingest_ref for a batch described as m3t.video.ingest takes it (draws per clip, frame indices).  raw=True: what the reference's loader
    hands the model BEFORE normalisation -- float32 pixel values 0..255, the jitter tables applied, the cutout filled with 127.5."""
    import torch
    N = frames.shape[0]
    T, H, W, geom, fidx, tables = video.plan(frames.shape, torch.uint8, aug, frame_idx)
    norm = np.arange(256, dtype=np.float32) if raw else (video.norm_lut() if norm is None else norm)
    lut = np.stack([norm if t is None else norm[t] for t in tables]) if any(t is not None for t in tables) else norm
    return ingest_ref(frames, geom, fidx, lut, H, W, fill=127.5 if raw else 0.0)
