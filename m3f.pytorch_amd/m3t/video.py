"""Video ingest on the GPU: the counterpart of m3t/audio.py for the video half of the reference's loaders.

The reference's `load_video` (`models/dataset.py:46-80`, `models/vox2_dataset.py:14-50`) crops, mirrors, colour-jitters
(`models/cv_augment.py:6-37`), cuts out (`dataset.py:16-31`), transposes THWC -> CTHW and casts to float32 on the host, and the
task modules normalise on the device (`models/model.py:106`: `(x - 127.5) / 127.5`).  Here the model takes the uint8 frames as decoded,
`[N, Ts, Hs, Ws, 3]`, and ONE kernel (csrc/ingest.hip, m3t_video_ingest) does all of it and hands the first convolution its operand:

  draw_affwild / draw_vox2   one clip's augmentation parameters, consuming `random` / `np.random` in the reference's order
  frame_index                which stored frame each output frame shows (missing frames, short windows)
  norm_lut / jitter_lut      the 256-entry float tables the kernel gathers from
  ingest                     frames + draws -> ops.VideoCL (layout "cl") or float32 planes [N, 3, T, H, W] (layout "planes")

Every value the kernel writes is an entry of a table built here, so the result has the bits of the reference's float32 arithmetic.
The `cv2.resize` branch of `dataset.py:73` (`input_size > 128`) is covered for the reference's default, the 256-pixel face tracks:
`draw_affwild(256, ..., resize=True)` crops 224 x 224 and m3t_video_ingest_half halves it to 112 x 112 (a draw with `"scale": 2`).  224 -> 112
is an exact factor of 2 on both axes, where OpenCV's `resize` replaces INTER_LINEAR for 8-bit images by its integer INTER_AREA path: every
output channel is `(a + b + c + d + 2) >> 2` over its 2 x 2 source block, a uint8 again, so the table gather follows unchanged.  That rule is
taken from OpenCV's published source (modules/imgproc/src/resize.cpp: `resize` switches INTER_LINEAR to INTER_AREA when both integer
factors are 2, noting that the two agree there, and the 2 x 2 case of its fast area kernel sums four values, adds 2 and shifts by 2); cv2 is
not installed where this project is developed, so it has NOT been checked against a run of the real `cv2.resize` -- tests/test_ingest_resize_host.py holds that check for whoever has OpenCV.
Out of scope: every other resize factor (an `input_size > 128` whose crop is not 224 would need cv2's general fixed-point bilinear, which
is not pinned) -- the draws raise ValueError for it, as does the default `resize=False` -- and decoding, which stays on the host.
"""
import random

import numpy as np
import torch

from . import ops
from .ops import M3THipError, video_ingest, video_ingest_half


def norm_lut(device=None):
    """float32 [256]: (v - 127.5) / 127.5 (models/model.py:106).  device=None: numpy's float32 arithmetic (= torch's on the host, the
    reference's bits).  With a device: the same expression evaluated BY torch ON that device and read back once -- what the task modules'
    float32 route computes there, so that a uint8 batch and the float32 batch of the same frames give the same bits (a device back-end is
    free to divide by a scalar as a multiplication by its reciprocal, which differs from the host's division in the last bit)."""
    if device is None:
        return ((np.arange(256, dtype=np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else None))
    t = _DEVICE_NORM.get(key)
    if t is None:
        x = torch.arange(256, dtype=torch.float32, device=device)
        t = _DEVICE_NORM[key] = ((x - 127.5) / 127.5).cpu().numpy()
    return t


_DEVICE_NORM = {}


def jitter_table(brightness, contrast):
    """uint8 [256]: adjust_contrast(adjust_brightness(v)) of models/cv_augment.py:16,33, the tables built exactly as there"""
    bt = np.array([i * brightness for i in range(0, 256)]).clip(0, 255).astype('uint8')
    ct = np.array([(i - 74) * contrast + 74 for i in range(0, 256)]).clip(0, 255).astype('uint8')
    return ct[bt]


def jitter_lut(brightness, contrast, norm=None):
    """float32 [256]: norm[contrast_table[brightness_table[v]]] (vox2_dataset.py:43-45 in front of the normalisation)"""
    norm = norm_lut() if norm is None else np.asarray(norm, np.float32)
    return norm[jitter_table(brightness, contrast)]


def _crop(input_size, training, crop, resize=False):
    """(crop_x, crop_y, size) of dataset.py:54-61 / vox2_dataset.py:21-27.  resize: the caller takes the 224 -> 112 halving of dataset.py:73"""
    if not crop:
        return 0, 0, int(input_size)
    if input_size > 128 and not resize:
        raise ValueError("input_size %d > 128: the reference resizes the crop with cv2.resize (dataset.py:73), which the ingest covers only "
                         "for a 224-pixel crop halved to 112 (input_size 256), on request: draw_affwild(..., resize=True)" % input_size)
    if input_size > 128 and input_size * 7 // 8 != 224:
        raise ValueError("input_size %d > 128: the reference resizes the %d-pixel crop to 112 with cv2.resize (dataset.py:73); only the exact "
                         "halving of a 224-pixel crop is covered" % (input_size, input_size * 7 // 8))
    if training:
        cx = random.randint(0, input_size // 8)
        cy = random.randint(0, input_size // 8)
    else:
        cx, cy = input_size // 16, input_size // 16
    return cx, cy, input_size * 7 // 8


def draw_affwild(input_size, training, crop, cutout, mirror=False, resize=False):
    """One clip's draws of models/dataset.py:46-80.  `mirror` is the caller's `random.random() > 0.5`, drawn BEFORE this call as at
    dataset.py:258; then crop_x, crop_y (random.randint), then the cutout's y, x (np.random.randint).  Frames are input_size squares.
    resize=True admits the reference's 256-pixel branch (dataset.py:61,73; input_size > 128 with a 224-pixel crop): the draw then carries
    `"scale": 2`, its `size` is the 224-pixel window in the source and its cutout is drawn on the 112 x 112 output, which is what
    sequence_cutout sees.  Any other input_size > 128 raises, with or without it."""
    cx, cy, size = _crop(input_size, training, crop, resize)
    scale = 2 if (crop and resize and input_size > 128) else 1
    cut = None
    if cutout and training:                                   # sequence_cutout, dataset.py:16-31 (one hole)
        h = w = size // scale
        length = h // 2
        y = np.random.randint(h)
        x = np.random.randint(w)
        cut = (int(np.clip(y - length, 0, h)), int(np.clip(y + length, 0, h)), int(np.clip(x - length, 0, w)), int(np.clip(x + length, 0, w)))
    d = {"cy": cy, "cx": cx, "size": size, "mirror": bool(mirror and training), "cutout": cut, "table": None}
    if scale != 1:
        d["scale"] = scale
    return d


def draw_vox2(input_size, training, crop):
    """One clip's draws of models/vox2_dataset.py: the mirror draw of its call site (:91, made in every mode), crop_x, crop_y, then
    brightness and contrast (random.uniform(0.9, 1.1), training only)."""
    mirror = random.random() > 0.5
    cx, cy, size = _crop(input_size, training, crop)
    table = None
    if training:
        brightness = random.uniform(0.9, 1.1)
        contrast = random.uniform(0.9, 1.1)
        table = jitter_table(brightness, contrast)
    return {"cy": cy, "cx": cx, "size": size, "mirror": bool(mirror and training), "cutout": None, "table": table}


def frame_index(present, start, length, window):
    """int32 [window]: the position in the stored clip (the array `present` describes) that output frame i shows, for a window that reads
    frames start .. start + length - 1: a missing frame shows the previous one this window read (dataset.py:67), -1 before the first
    present one (zeros, dataset.py:68), and frames past `length` repeat the last (np.pad 'edge', dataset.py:312)."""
    present = np.asarray(present).astype(bool)
    if not (0 <= start and 0 < length <= window and start + length <= present.shape[0]):
        raise ValueError("frame_index: window [%d, %d) does not fit %d stored frames / %d output frames" % (start, start + length, present.shape[0], window))
    out = np.empty(window, np.int32)
    last = -1
    for i in range(length):
        if present[start + i]:
            last = start + i
        out[i] = last
    out[length:] = last
    return out


def batch_scale(aug):
    """the one scale of a batch's draws (1: m3t_video_ingest; 2: m3t_video_ingest_half); ValueError for mixed or unknown scales"""
    if not aug:
        return 1
    scales = {a.get("scale", 1) for a in aug}
    if len(scales) != 1:
        raise ValueError("ingest: the clips of a batch must share one scale, got %s" % sorted(scales, key=str))
    scale = scales.pop()
    if scale not in (1, 2):
        raise ValueError("ingest: scale must be 1 or 2, got %r" % (scale,))
    return int(scale)


def plan(shape, dtype, aug=None, frame_idx=None):
    """Host validation of an ingest call, before anything touches a device: returns (T, H, W, geom int32 [N, 8], frame_idx int32 [N, T] or
    None, tables: list of per-clip uint8 [256] or None).  ValueError for a wrong shape or dtype, a crop window outside the frame, clips of
    different output sizes, a cutout outside the output, a frame index outside [-1, Ts).  A draw may carry "scale" (absent: 1; 2: the
    window `size` in the source is halved, m3t_video_ingest_half): one scale per batch, an even size, H = W = size // scale; the window is
    checked with `size`, the cutout with the output size."""
    if dtype != torch.uint8 or len(shape) != 5 or shape[4] != 3:
        raise ValueError("ingest: frames must be uint8 [N, Ts, Hs, Ws, 3], got %s %s" % (dtype, list(shape)))
    N, Ts, Hs, Ws = (int(v) for v in shape[:4])
    if min(N, Ts, Hs, Ws) <= 0:
        raise ValueError("ingest: empty frames %s" % (list(shape),))
    geom = np.zeros((N, 8), np.int32)
    tables = [None] * N
    H, W = Hs, Ws
    if aug is not None:
        if len(aug) != N:
            raise ValueError("ingest: %d draws for %d clips" % (len(aug), N))
        sizes = {int(a["size"]) for a in aug}
        if len(sizes) != 1:
            raise ValueError("ingest: the clips of a batch must share one output size, got %s" % sorted(sizes))
        size = sizes.pop()
        scale = batch_scale(aug)
        if size % scale:
            raise ValueError("ingest: scale %d needs an even crop window, got %d" % (scale, size))
        H = W = size // scale
        for n, a in enumerate(aug):
            cy, cx = int(a["cy"]), int(a["cx"])
            if H <= 0 or cy < 0 or cx < 0 or cy + size > Hs or cx + size > Ws:
                raise ValueError("ingest: clip %d: crop window (%d, %d) + %d outside the %d x %d frame" % (n, cy, cx, size, Hs, Ws))
            cut = a.get("cutout") or (0, 0, 0, 0)
            if not (0 <= cut[0] <= cut[1] <= H and 0 <= cut[2] <= cut[3] <= W):
                raise ValueError("ingest: clip %d: cutout %s outside the %d x %d output" % (n, tuple(cut), H, W))
            geom[n, :7] = (cy, cx, 1 if a.get("mirror") else 0) + tuple(int(v) for v in cut)
            tb = a.get("table")
            if tb is not None:
                tb = np.asarray(tb)
                if tb.dtype != np.uint8 or tb.shape != (256,):
                    raise ValueError("ingest: clip %d: the jitter table must be uint8 [256]" % n)
                tables[n] = tb
    T = Ts
    if frame_idx is not None:
        fi = np.asarray(frame_idx.cpu() if isinstance(frame_idx, torch.Tensor) else frame_idx)
        if fi.ndim != 2 or fi.shape[0] != N or fi.shape[1] <= 0 or not np.issubdtype(fi.dtype, np.integer):
            raise ValueError("ingest: frame_idx must be integers [N, T], got %s %s" % (fi.dtype, list(fi.shape)))
        if fi.min() < -1 or fi.max() >= Ts:
            raise ValueError("ingest: frame_idx outside [-1, %d)" % Ts)
        frame_idx = np.ascontiguousarray(fi, np.int32)
        T = int(fi.shape[1])
    return T, H, W, geom, frame_idx, tables


def ingest(frames_u8, aug=None, frame_idx=None, layout="cl", norm=None):
    """frames_u8: uint8 [N, Ts, Hs, Ws, 3] as decoded (tensor or array; a host tensor is copied to the device with non_blocking=True -- pin
    it to overlap the copy; a non-contiguous or misaligned one is made contiguous).  aug: one draw per clip (draw_affwild / draw_vox2) or
    None = no crop, mirror, cutout, plain normalisation; draws with "scale": 2 (draw_affwild(..., resize=True)) halve the window.  frame_idx: integers [N, T] (frame_index) or None = the stored frames in order.
    norm: the 256-entry normalisation table the jitter tables are composed in front of (default norm_lut(); "device": norm_lut(device)).
    -> ops.VideoCL (layout "cl": a channels-last stem's first convolution takes it as it is) or float32 [N, 3, T, H, W] ("planes").
    Everything is validated on the host first (ValueError); the small tables reach the device in one copy."""
    if layout not in ("cl", "planes"):
        raise ValueError("ingest: layout must be 'cl' or 'planes'")
    if isinstance(frames_u8, np.ndarray):
        frames_u8 = torch.from_numpy(frames_u8)
    if not isinstance(frames_u8, torch.Tensor):
        raise ValueError("ingest: frames must be a tensor or an array")
    T, H, W, geom, fidx, tables = plan(tuple(frames_u8.shape), frames_u8.dtype, aug, frame_idx)
    on_device = isinstance(norm, str) and norm == "device"
    if not on_device:
        norm = norm_lut() if norm is None else np.ascontiguousarray(norm, np.float32)
        if norm.shape != (256,):
            raise ValueError("ingest: norm must be float32 [256]")
    if not torch.cuda.is_available():
        raise M3THipError("m3t.video needs the GPU: the M3T path has no CPU fallback")
    dev = frames_u8.device if frames_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if on_device:
        norm = norm_lut(dev)
    N = geom.shape[0]
    if any(t is not None for t in tables):
        lut = np.stack([norm if t is None else norm[t] for t in tables])
    else:
        lut = norm
    parts = [geom.reshape(-1)] + ([fidx.reshape(-1)] if fidx is not None else []) + [lut.reshape(-1).view(np.int32)]
    small = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=True)       # geom | frame_idx | tables: one copy
    o = 8 * N
    g_d = small[:o].view(N, 8)
    f_d = None
    if fidx is not None:
        f_d = small[o:o + N * T].view(N, T)
        o += N * T
    l_d = small[o:].view(torch.float32).view(lut.shape)
    fr = frames_u8.to(dev, non_blocking=True) if not frames_u8.is_cuda else frames_u8
    if not fr.is_contiguous():
        fr = fr.contiguous()
    if fr.data_ptr() % 16 != 0:
        fr = fr.clone()
    entry = video_ingest_half if batch_scale(aug) == 2 else video_ingest
    return entry(fr, f_d, T, g_d, l_d, H, W, layout)


def ingest_for(visual, frames_u8, aug=None, frame_idx=None):
    """the task modules' uint8 route: ingest for the front-end `visual` -- layout "cl" where its first Conv3d runs on the channels-last chain
    (models.backbone.Conv3d.cl_chain; a models.backbone.VA_VGGFace on the chain), planes otherwise -- with the normalisation table of the
    device, so that the result has the bits of the modules' float32 route, `(x - 127.5) / 127.5` evaluated by torch on that device."""
    on_chain = getattr(visual, "on_chain", None)             # (models.backbone.VA_VGGFace: Conv2d layers, the whole front-end is the chain)
    if on_chain is not None:
        cl = bool(on_chain())
    else:
        first = next((m for m in visual.modules() if isinstance(m, torch.nn.Conv3d)), None)
        cl = first is not None and getattr(first, "cl_chain", False) and ops.STEM_CL[0]
    return ingest(frames_u8, aug, frame_idx, "cl" if cl else "planes", norm="device")
