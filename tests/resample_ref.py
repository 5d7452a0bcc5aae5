"""The conversion rule of DESIGN.md 4c in numpy, for tests/test_wave_host.py, tests/test_resample_host.py and tests/test_gpu_resample.py:
what `librosa.load(path, sr=16000)` of the reference's era (librosa 0.7, res_type='kaiser_best', resampy 0.2.2, fix=True, scale=False) does
to a wav file, restated from the libraries' published sources.  Neither library (nor libsndfile) is a dependency: this is the project's
own text, shares no code with m3t/, and tests/test_resample_host.py holds a check against the real libraries for where they exist.

  wav_bytes / write_wav   a RIFF/WAVE file written with `struct`, every kind and channel count, plain or EXTENSIBLE
  samples / noise         integer (or float32) samples of a kind from 0.25-sigma Gaussian noise
  decode, to_mono         the sample-to-float rule and librosa.to_mono
  registers               the time register of every output: 'accumulated' (np.add.accumulate, resampy's), 'loop' (the plain Python loop),
                          'exact' (the rational t * rate / 16000 rounded once)
  resample(x, rate, acc)  resampy's resample_f + librosa's fix_length; acc=float64 is the oracle, acc=float32 the yardstick: resampy's own
                          arithmetic, every partial sum stored to a float32 output
  load(raw, rate, channels, kind, acc)   decode -> to_mono -> resample
"""
import struct
from fractions import Fraction

import numpy as np

SR = 16000
KINDS = ("u8", "i16", "i24", "i32", "f32")
KIND_BYTES = {"u8": 1, "i16": 2, "i24": 3, "i32": 4, "f32": 4}
NUM_ZEROS, NUM_TABLE, ROLLOFF, BETA = 64, 512, 0.9475937167399596, 14.769656459379492
PCM_GUID = struct.pack("<IHH", 1, 0, 0x10) + bytes.fromhex("800000aa00389b71")
FLOAT_GUID = struct.pack("<IHH", 3, 0, 0x10) + bytes.fromhex("800000aa00389b71")


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def noise(n, channels, seed, sigma=0.25):
    """float64 [n, channels] in (-1, 1): Gaussian noise of `sigma`"""
    return np.clip(np.random.RandomState(seed).normal(0.0, sigma, (n, channels)), -0.999, 0.999)


def samples(y, kind):
    """float64 [n, channels] in (-1, 1) -> the samples as stored: uint8 / int16 / int32 (24-bit values for i24) / float32"""
    if kind == "u8":
        return np.round(y * 127 + 128).astype(np.uint8)
    if kind == "i16":
        return np.round(y * 32767).astype(np.int16)
    if kind == "i24":
        return np.round(y * 8388607).astype(np.int32)
    if kind == "i32":
        return np.round(y * 2147483647).astype(np.int64).astype(np.int32)
    return y.astype(np.float32)


def body(s, kind):
    """the interleaved little-endian bytes of samples [n, channels]"""
    if kind == "i24":
        b = s.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    return np.ascontiguousarray(s, {"u8": "u1", "i16": "<i2", "i32": "<i4", "f32": "<f4"}[kind]).tobytes()


def wav_bytes(data, rate, channels, kind, extensible=False, extra=b"", tag=None, bits=None, valid_bits=None, data_size=None):
    """a RIFF/WAVE file around the body `data`; `extra`: chunks put between 'fmt ' and 'data'; tag / bits / valid_bits / data_size
    override what the kind gives (to write files the reader must refuse)"""
    bits = 8 * KIND_BYTES[kind] if bits is None else bits
    base = 3 if kind == "f32" else 1
    tag = base if tag is None else tag
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        guid = struct.pack("<IHH", tag, 0, 0x10) + bytes.fromhex("800000aa00389b71")
        fmt += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 0) + guid
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra
    chunks += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def write_wav(path, y, rate, kind, **kw):
    """float64 [n, channels] -> the file at `path`; returns the samples as stored"""
    s = samples(y, kind)
    with open(str(path), "wb") as f:
        f.write(wav_bytes(body(s, kind), rate, y.shape[1], kind, **kw))
    return s


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def decode(raw, channels, kind):
    """the 'data' body (bytes or uint8 array) -> float32 [frames, channels], libsndfile's normalised read as documented"""
    raw = np.frombuffer(bytes(raw), np.uint8)
    fb = channels * KIND_BYTES[kind]
    raw = raw[:len(raw) // fb * fb]
    if kind == "u8":
        y = ((raw.astype(np.float64) - 128.0) / 128.0).astype(np.float32)
    elif kind == "i16":
        y = (raw.view("<i2").astype(np.float64) / 32768.0).astype(np.float32)
    elif kind == "i24":
        t = raw.reshape(-1, 3).astype(np.int64)
        v = t[:, 0] + (t[:, 1] << 8) + (t[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        y = (v.astype(np.float64) / 8388608.0).astype(np.float32)
    elif kind == "i32":
        y = (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        y = raw.view("<f4").copy()
    return y.reshape(-1, channels)


def to_mono(y):
    """librosa.to_mono = np.mean over the channel axis of a float32 array: the channels added in order in float32, divided by the count"""
    acc = y[:, 0].copy()
    for c in range(1, y.shape[1]):
        acc = (acc + y[:, c]).astype(np.float32)
    return (acc / np.float32(y.shape[1])).astype(np.float32)


def filter_table(rate):
    """(win, delta) float64 [32769] for a source of `rate` Hz"""
    n = NUM_ZEROS * NUM_TABLE
    j = np.arange(n + 1)
    sinc_win = ROLLOFF * np.sinc(ROLLOFF * (j / NUM_TABLE))                   # resampy's sinc_window: the taper multiplies this product
    win = np.kaiser(2 * n + 1, BETA)[n + j] * sinc_win
    ratio = float(SR) / rate
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return win, delta


def lengths(n_in, rate):
    """(n_res, n_out): resampy's int(n * ratio) and librosa's int(ceil(n * ratio)), in float64 as written"""
    ratio = float(SR) / rate
    return int(n_in * ratio), int(np.ceil(n_in * ratio))


def registers(count, rate, register="accumulated"):
    inc = rate / float(SR)
    if register == "accumulated":
        steps = np.full(max(count, 1), inc)
        steps[0] = 0.0
        return np.add.accumulate(steps)[:count]
    if register == "loop":
        r, out = 0.0, np.zeros(count)
        for t in range(count):
            out[t] = r
            r += inc
        return out
    if register == "exact":
        return np.array([float(Fraction(t * rate, SR)) for t in range(count)], np.float64).reshape(count)
    raise ValueError(register)


def resample(x, rate, acc=np.float64, register="accumulated"):
    """x: mono float32 [n_in] at `rate` Hz -> `acc` [n_out] at 16 kHz.  Every partial sum is float64(y) + w * x in float64, stored to `acc`
    (resampy's output array is float32: acc=np.float32 is resampy's own arithmetic)."""
    x = np.asarray(x, np.float32)
    n_in = x.shape[0]
    n_res, n_out = lengths(n_in, rate)
    out = np.zeros(n_out, acc)
    if rate == SR:
        out[:] = x
        return out
    if n_res == 0:
        return out
    xd = x.astype(np.float64)
    win, delta = filter_table(rate)
    nwin = win.shape[0]
    ratio = float(SR) / rate
    scale = min(1.0, ratio)
    step = int(scale * NUM_TABLE)
    r = registers(n_res, rate, register)
    n = r.astype(np.int64)
    y = np.zeros(n_res, acc)

    def wing(frac, count_cap, sign):
        idx = frac * NUM_TABLE
        off = idx.astype(np.int64)
        eta = idx - off
        cnt = np.minimum(count_cap, (nwin - off) // step)
        for i in range(int(cnt.max(initial=0))):
            m = np.flatnonzero(i < cnt)
            w = win[off[m] + i * step] + eta[m] * delta[off[m] + i * step]
            src = n[m] - i if sign < 0 else n[m] + i + 1
            y[m] = (y[m].astype(np.float64) + w * xd[src]).astype(acc)

    frac = scale * (r - n)
    wing(frac, n + 1, -1)
    wing(scale - frac, n_in - n - 1, +1)
    out[:n_res] = y
    return out


def load(raw, rate, channels, kind, acc=np.float64, register="accumulated"):
    """librosa.load(sr=16000) of a file whose 'data' body is `raw`"""
    return resample(to_mono(decode(raw, channels, kind)), rate, acc, register)


# ---- a synthetic AudioSet folder of mixed files --------------------------------------------------------------------------------------
MIXED = [  # name, rate, channels, kind, frames, classes
    ("a44", 44100, 2, "i16", 2947, (3, 300)),
    ("b48", 48000, 1, "f32", 3001, (526,)),
    ("c16", 16000, 1, "i16", 2133, (0,)),
    ("d22", 22050, 3, "i24", 1500, (7, 8)),
    ("e16", 16000, 1, "i16", 9000, (41,)),
]
ALL16 = [("p", 16000, 1, "i16", 3000, (1,)), ("q", 16000, 1, "i16", 2133, (2, 5)), ("r", 16000, 1, "i16", 9000, (526,))]


def write_audioset_tree(root, clips=MIXED, fold="balanced_train_segments"):
    """an AudioSet folder as scan_audioset reads it, its clips written by write_wav from noise seeded by their position
    -> (str(root), {name: (body bytes, rate, channels, kind)})"""
    import os
    root = str(root)
    os.makedirs(os.path.join(root, fold), exist_ok=True)
    with open(os.path.join(root, "class_labels_indices.csv"), "w") as f:
        f.write("index,mid,display_name\n" + "".join('%d,/m/%03d,"class %d"\n' % (i, i, i) for i in range(527)))
    bodies, lines = {}, ["# header 1", "# header 2", "# YTID, start_seconds, end_seconds, positive_labels"]
    for k, (name, rate, channels, kind, frames, classes) in enumerate(clips):
        s = write_wav(os.path.join(root, fold, name + ".wav"), noise(frames, channels, 100 + k), rate, kind)
        bodies[name] = (body(s, kind), rate, channels, kind)
        lines.append('%s, 0.000, 10.000, "%s"' % (name, ",".join("/m/%03d" % c for c in classes)))
    with open(os.path.join(root, fold + ".csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return root, bodies
