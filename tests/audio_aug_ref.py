"""The numpy oracle of the augmented AudioSet ingest (tests/test_audio_aug_host.py, tests/test_gpu_audio_aug.py) and the reference's record
of its own spec_augment (tests/golden/spec_augment_cases.npz, written by tests/golden/gen_golden_spec_augment.py).  Shares no code with
m3t/audio.py or the kernels.

  mask_rows    the reference's spec_augment (models/audioset_dataset.py:17-55) seen from the stacked rows: cell (i, k*40 + b) of [T, 200] shows
               band b of frame 3i + k, and is 0.0 iff a frequency mask holds b or a time mask holds 3i + k
  mix_rows     out[n] = lam32[n] * x[n] + om32[n] * x[partner[n]] in float32: two rounded products, one rounded sum
  mix_labels   the same formula on the clips' 0/1 rows"""
import functools
import random
import zlib

import numpy as np

from conftest import load_golden

N_MELS, STEP, WIDTH = 40, 3, 5


@functools.lru_cache(None)
def golden():
    return load_golden("spec_augment_cases")


def cases():
    g = golden()
    return [(c, int(tau), float(F), float(T), int(nf), int(nt)) for c, (tau, F, T, nf, nt) in enumerate(g["cases"])]


def seeds():
    return [int(s) for s in golden()["seeds"]]


def random_crc():
    return zlib.crc32(repr(random.getstate()).encode())


def numpy_crc():
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    return zlib.crc32(keys.tobytes() + repr((kind, int(pos), int(has_gauss), float(gauss))).encode())


def zero_pattern(draw, tau):
    """bool [40, tau]: the cells a draw {"fmask": [(f0, f)..], "tmask": [(t0, t)..]} sets to zero, as slices"""
    z = np.zeros((N_MELS, tau), bool)
    for f0, f in draw.get("fmask", ()):
        z[f0:f0 + f, :] = True
    for t0, t in draw.get("tmask", ()):
        z[:, t0:t0 + t] = True
    return z


def mask_rows(x, draw):
    """x: one clip's stacked rows [T, 200] float32 -> a masked copy; the zero is an assignment"""
    out = np.array(x, np.float32, copy=True)
    T = out.shape[0]
    cells = out.reshape(T, WIDTH, N_MELS)
    for i in range(T):
        for k in range(WIDTH):
            frame = STEP * i + k
            for b in range(N_MELS):
                if any(f0 <= b < f0 + f for f0, f in draw.get("fmask", ())) or any(t0 <= frame < t0 + t for t0, t in draw.get("tmask", ())):
                    cells[i, k, b] = 0.0
    return out


def weights(lam):
    lam32 = np.asarray(lam, np.float64).astype(np.float32)
    return lam32, np.float32(1) - lam32


def mix_rows(x, partner, lam):
    """x: [N, ...] float32 -> float32, bit for bit what two rounded float32 products and one rounded float32 sum give"""
    x = np.asarray(x, np.float32)
    lam32, om32 = weights(lam)
    shape = (-1,) + (1,) * (x.ndim - 1)
    a = (lam32.reshape(shape) * x).astype(np.float32)
    b = (om32.reshape(shape) * x[np.asarray(partner)]).astype(np.float32)
    return (a + b).astype(np.float32)


def mix_labels(rows, partner, lam):
    """rows: uint8 [N, C] (0 / 1) -> float32 [N, C]"""
    return mix_rows(np.asarray(rows).astype(np.float32), partner, lam)


def augment(x, draws, mix=None):
    """the whole rule on the un-augmented rows x [N, T, 200] of a batch: masks per clip, then the mix"""
    out = np.stack([mask_rows(x[n], d) for n, d in enumerate(draws)])
    return out if mix is None else mix_rows(out, mix[0], mix[1])
