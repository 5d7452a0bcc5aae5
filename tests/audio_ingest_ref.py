"""Shared helpers of the batched audio ingest tests (tests/test_audio_ingest_host.py, tests/test_gpu_audio_ingest.py): the signal family of
tests/test_gpu_audio.py::test_logmel_vs_oracle, the reference's temporal crop restated in numpy (models/audioset_dataset.py:63-70, np.pad
'wrap' included) and the float64 reference of one clip, O.load_audio(O.melspec_db(crop, fps, pad_mode, top_db), 0, T)."""
import numpy as np

from oracle import m3t_oracle as O

TOL_DB = 2e-3          # tests/test_gpu_audio.py's tolerance: fp32 DFT by GEMM against the fp64 FFT


def signal(n, seed, second_tone=True, noise=0.05):
    """440 Hz (+ 3100 Hz after 0.3 s) + noise * randn, float32 at 16 kHz"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    y = 0.4 * np.sin(2 * np.pi * 440 * t)
    if second_tone:
        y = y + 0.2 * np.sin(2 * np.pi * 3100 * t + 1.0) * (t > 0.3)
    return (y + noise * rs.standard_normal(n)).astype(np.float32)


def draw(fps, start, length=4, nsamples=None):
    """a hand-made draw in the format of m3t.audio.draw_audioset"""
    hop = int(1 / 3 * 1 / fps * 16000)
    return {"fps": fps, "hop": hop, "start": start, "nsamples": int(length / fps * 16000) if nsamples is None else nsamples}


def crop(y, start, nsamples):
    """audioset_dataset.py:63-70"""
    tot = len(y)
    if nsamples > tot:
        y = np.pad(y, (0, nsamples - tot + 5), 'wrap')
    assert 0 <= start and start + nsamples <= len(y)
    return y[start:start + nsamples]


def mel_db(y, d, pad_mode="constant", top_db=80.0):
    """[nf, 40] float64: the oracle's log-Mel spectrogram of the clip's crop"""
    assert d["hop"] == int(1 / 3 * 1 / d["fps"] * 16000)
    return O.melspec_db(crop(np.asarray(y), d["start"], d["nsamples"]).astype(np.float64), d["fps"], pad_mode, top_db)


def reference(clips, draws, T, pad_mode="constant", top_db=80.0):
    """[N, T, 200] float64"""
    return np.stack([O.load_audio(mel_db(y, d, pad_mode, top_db), 0, T) for y, d in zip(clips, draws)])


def max_err(got, ref, what):
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, "detach") else got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    print("%s: max |ingest - oracle| = %.3e dB (bound %.0e)" % (what, err, TOL_DB))
    return err
