"""numpy restatement of the halving video ingest (include/m3t_hip.h, m3t_video_ingest_half) and the golden cases' parameters, shared by
tests/test_ingest_resize_host.py and tests/test_gpu_ingest_resize.py.

    f  = frame_idx[n][t];  xs = W-1-x if mirror else x
    s  = the sum of frames[n][f][cy+2y .. cy+2y+1][cx+2xs .. cx+2xs+1][c]
    v  = 0 if f < 0 else (s + 2) >> 2
    o  = 0.0 inside the cutout (output coordinates) else lut[n][v]

tests/golden/ingest_resize.npz (tests/golden/gen_golden_ingest_resize.py) holds what the reference's `load_video` returns at input_size 256
for the same frames, presence masks and seeds -- with `cv2.resize` stubbed by the 2 x 2 rule, which is OpenCV's documented behaviour for this
shape but was not produced by a run of OpenCV -- normalised by torch's float32 `(x - 127.5) / 127.5` on the host, and the state of both
random generators after the reference's call.
"""
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def halve(img):
    """uint8 [..., 2H, 2W, C] -> uint8 [..., H, W, C]: (a + b + c + d + 2) >> 2 over each 2 x 2 block, in integers"""
    a = np.asarray(img).astype(np.uint32)
    s = a[..., 0::2, 0::2, :] + a[..., 0::2, 1::2, :] + a[..., 1::2, 0::2, :] + a[..., 1::2, 1::2, :]
    return ((s + 2) >> 2).astype(np.uint8)


def rounding_image():
    """uint8 [8, 8, 3]: 2 x 2 blocks whose sums cover every residue mod 4 and the extremes -- four 255s (255), 0 0 0 1 (0), 0 0 1 1 (1: the
    half rounds up), 0 1 1 1 (1), 255 255 255 254 (255), 255 255 254 254 (255), 254 254 254 255 (254); the three channels are rotations"""
    blocks = [(255, 255, 255, 255), (0, 0, 0, 1), (0, 0, 1, 1), (0, 1, 1, 1), (255, 255, 255, 254), (255, 255, 254, 254), (254, 254, 254, 255),
              (0, 0, 0, 0), (1, 2, 3, 4), (0, 255, 0, 255), (0, 255, 0, 0), (255, 0, 255, 255), (7, 7, 7, 8), (100, 101, 102, 104),
              (128, 127, 127, 127), (2, 0, 0, 0)]
    img = np.zeros((8, 8, 3), np.uint8)
    for c in range(3):
        for i, b in enumerate(blocks):
            y, x = 2 * (i // 4), 2 * (i % 4)
            r = b[c:] + b[:c]
            img[y, x, c], img[y, x + 1, c], img[y + 1, x, c], img[y + 1, x + 1, c] = r
    want = np.array([(sum(b) + 2) >> 2 for b in blocks], np.uint8).reshape(4, 4)
    return img, np.repeat(want[:, :, None], 3, 2)


def ingest_half_ref(frames, geom, frame_idx, lut, H, W, fill=0.0):
    """frames uint8 [N, Ts, Hs, Ws, 3], geom int [N, 8], frame_idx int [N, T] or None, lut float32 [256] or [N, 256] -> float32 [N, 3, T, H, W]
    (H, W: the output size; the window in the source is 2H x 2W); fill: what the cutout writes (0.0 after normalisation; 127.5 before it)"""
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
                img = halve(frames[n, f, cy:cy + 2 * H, cx:cx + 2 * W])
                if mirror:
                    img = img[:, ::-1]
            o = tab[img]                                     # [H, W, 3]
            o[y1:y2, x1:x2] = fill
            out[n, :, t] = o.transpose(2, 0, 1)
    return out


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "ingest_resize.npz"))
    cases = []
    for name in z["names"]:
        name = str(name)
        g = lambda k: z["%s.%s" % (name, k)]
        input_size, training, crop, cutout, start, length, window, seed = (int(v) for v in g("args"))
        cases.append({"name": name, "frames": g("frames"), "present": g("present").astype(bool), "out": g("out"),
                      "rng_py": g("rng_py"), "rng_np": g("rng_np"),
                      "input_size": input_size, "training": bool(training), "crop": bool(crop), "cutout": bool(cutout), "start": start,
                      "length": length, "window": window, "seed": seed})
    return cases


def rng_state():
    """(python's `random` state, numpy's global state) as two integer arrays: the 624 words and the position of each generator"""
    py = random.getstate()
    nps = np.random.get_state()
    assert py[0] == 3 and py[2] is None and nps[0] == "MT19937" and nps[3] == 0
    return np.array(py[1], np.int64), np.concatenate([np.asarray(nps[1], np.int64), [int(nps[2])]])


def case_params(video, c):
    """the draws and the frame indices of golden case `c` from m3t.video, under the case's seeds, as the reference's call site consumes them
    (dataset.py:256-261: the mirror draw, then load_video)"""
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    mirror = random.random() > 0.5
    aug = video.draw_affwild(c["input_size"], c["training"], c["crop"], c["cutout"], mirror, resize=True)
    fidx = video.frame_index(c["present"], c["start"], c["length"], c["window"])
    return aug, fidx


def batch_ref(video, frames, aug, frame_idx=None, norm=None, raw=False):
    """ingest_half_ref for a batch described as m3t.video.ingest takes it (draws with "scale": 2 per clip, frame indices).  raw=True: what the
    reference's loader hands the model BEFORE normalisation -- float32 pixel values 0..255, the jitter tables applied, the cutout 127.5."""
    import torch
    T, H, W, geom, fidx, tables = video.plan(frames.shape, torch.uint8, aug, frame_idx)
    assert video.batch_scale(aug) == 2
    norm = np.arange(256, dtype=np.float32) if raw else (video.norm_lut() if norm is None else norm)
    lut = np.stack([norm if t is None else norm[t] for t in tables]) if any(t is not None for t in tables) else norm
    return ingest_half_ref(frames, geom, fidx, lut, H, W, fill=127.5 if raw else 0.0)
