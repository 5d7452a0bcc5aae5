"""CPU-side checks of the batched audio ingest (m3t/audio.py): draw_audioset consumes `random` as the reference's load_audio does
(models/audioset_dataset.py:60-69), plan_waves builds the per-clip table and validates on the host before anything touches a device, and a
valid call without a GPU fails loudly.  No GPU here."""
import random

import numpy as np
import pytest
import torch

import audio_ingest_ref as A
from m3t import audio


def _reference_draws(tot_samples, length, is_training):
    """audioset_dataset.py:60-69, the lines that draw, restated inline"""
    fps = random.choice([15.0, 17.0, 19.0, 22.0, 23.976, 24.0, 25.0, 29.97, 30.0]) if is_training else 30.0
    nsamples = int(length / fps * 16000)
    if nsamples > tot_samples:
        tot_samples = tot_samples + (nsamples - tot_samples + 5)         # len(np.pad(y, (0, nsamples - tot_samples + 5), 'wrap'))
    start = random.randint(0, tot_samples - nsamples) if is_training else (tot_samples - nsamples) // 2
    return fps, nsamples, start, int(1 / 3 * 1 / fps * 16000)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("tot,length", [(160000, 32), (20000, 32), (1500, 4), (2133, 4)])      # long; wraps below 25.6 fps; wraps always; tot == nsamples at 30 fps
def test_draws_consume_random_in_the_references_order(tot, length, training):
    assert audio.FPS_VALUES == [15.0, 17.0, 19.0, 22.0, 23.976, 24.0, 25.0, 29.97, 30.0]
    for seed in range(6):
        random.seed(seed)
        fps, ns, start, hop = _reference_draws(tot, length, training)
        want = random.getstate()
        random.seed(seed)
        d = audio.draw_audioset(tot, length, training)
        assert random.getstate() == want
        assert d == {"fps": fps, "hop": hop, "start": start, "nsamples": ns}
        assert hop == audio.hop_length(fps)
        A.crop(np.zeros(tot, np.float32), d["start"], d["nsamples"])       # the draw fits the (padded) clip
    if not training:
        random.seed(3)
        s0 = random.getstate()
        audio.draw_audioset(tot, length, False)
        assert random.getstate() == s0


def test_the_modulo_is_the_references_wrap_padding():
    """c[j] = y[(start + j) mod len] against np.pad(y, (0, nsamples - len + 5), 'wrap')[start : start + nsamples], more than one period included"""
    for tot, ns in [(1500, 2133), (700, 2133), (5, 40), (1, 7)]:
        y = np.arange(tot, dtype=np.float32)
        for start in range(0, 6):
            assert np.array_equal(A.crop(y, start, ns), y[(start + np.arange(ns)) % tot])


def test_plan_builds_the_table():
    clips = [np.zeros(6000, np.int16), np.zeros(1500, np.int16), np.zeros(9000, np.int16)]
    draws = [A.draw(15.0, 0), A.draw(30.0, 3), A.draw(30.0, 3111)]
    wave, table, R = audio.plan_waves(clips, draws, 4)
    assert wave.dtype == torch.int16 and wave.shape == (16500,) and table.dtype == np.int64 and R == 39
    assert table.tolist() == [[0, 6000, 0, 4266, 355, 13, 0, 0], [6000, 1500, 3, 2133, 177, 13, 13, 0], [7500, 9000, 3111, 2133, 177, 13, 26, 0]]
    # [N, S] with lengths: the rows are the clips, nothing is repacked
    batch = torch.zeros(3, 9000, dtype=torch.float32)
    wave, table, R = audio.plan_waves(batch, draws, 4, lengths=[6000, 1500, 9000])
    assert wave.dtype == torch.float32 and wave.data_ptr() == batch.data_ptr() and table[:, 0].tolist() == [0, 9000, 18000]
    assert table[:, 1].tolist() == [6000, 1500, 9000] and R == 39
    # no draws: the evaluation draws
    _, table, _ = audio.plan_waves(batch, None, 4)
    assert table[:, 2:6].tolist() == [[(9000 - 2133) // 2, 2133, 177, 13]] * 3


def _d(**kw):
    return dict({"fps": 30.0, "hop": 177, "start": 0, "nsamples": 2133}, **kw)


@pytest.mark.parametrize("waves,aug,length,lengths", [
    (torch.zeros(2, 3000, dtype=torch.float64), None, 4, None),                      # wrong dtype
    (torch.zeros(2, 3000, dtype=torch.int32), None, 4, None),
    (np.zeros((2, 3000), np.uint8), None, 4, None),
    (torch.zeros(3000, dtype=torch.int16), None, 4, None),                           # wrong rank
    (torch.zeros(2, 4, 200), None, 4, None),
    ([np.zeros((2, 3000), np.float32)], None, 4, None),
    ([np.zeros(3000, np.float32), np.zeros(3000, np.int16)], None, 4, None),         # two dtypes in one batch
    ("clip.wav", None, 4, None),
    (torch.zeros(2, 3000, dtype=torch.int16), [_d()], 4, None),                      # one draw for two clips
    (torch.zeros(1, 3000, dtype=torch.int16), [_d(hop=0)], 4, None),
    (torch.zeros(1, 3000, dtype=torch.int16), [_d(hop=-177)], 4, None),
    (torch.zeros(1, 3000, dtype=torch.int16), [_d(nsamples=0)], 4, None),
    (torch.zeros(1, 3000, dtype=torch.int16), None, 0, None),                        # length
    (torch.zeros(1, 3000, dtype=torch.int16), None, -4, None),
    (torch.zeros(1, 3000, dtype=torch.int16), [_d(start=-1)], 4, None),
    (torch.zeros(1, 3000, dtype=torch.int16), [_d(start=3000)], 4, None),            # start outside [0, max(len, nsamples + 5))
    (torch.zeros(1, 1500, dtype=torch.int16), [_d(start=2138)], 4, None),
    (torch.zeros(2, 0, dtype=torch.int16), None, 4, None),                           # empty clips
    ([np.zeros(3000, np.float32), np.zeros(0, np.float32)], None, 4, None),
    (torch.zeros(2, 3000, dtype=torch.int16), None, 4, [3000, 0]),
    (torch.zeros(2, 3000, dtype=torch.int16), None, 4, [3000, 3001]),                # a length beyond the row
    (torch.zeros(2, 3000, dtype=torch.int16), None, 4, [3000]),
    (torch.zeros(2, 3000, dtype=torch.int16), None, 4, [3000.0, 2000.0]),
    ([], None, 4, None),
])
def test_ingest_validates_on_the_host(waves, aug, length, lengths, monkeypatch):
    """ValueError before any device is touched: neither the availability query nor the library is reached"""
    def touched(*a, **k):
        raise AssertionError("the wrapper reached the device before validating")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(audio, "lib", touched)
    with pytest.raises(ValueError):
        audio.plan_waves(waves, aug, length, lengths)
    with pytest.raises(ValueError):
        audio.ingest(waves, aug, length, lengths)


def test_start_in_the_wrap_padding_is_valid():
    audio.plan_waves(torch.zeros(1, 1500, dtype=torch.int16), [_d(start=2137)], 4)     # the last start of randint(0, 5) + ... within nsamples + 5
    audio.plan_waves(torch.zeros(1, 3000, dtype=torch.int16), [_d(start=2999)], 4)


def test_bad_pad_mode_and_tracks_raise(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the wrapper reached the device before validating")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    with pytest.raises(ValueError):
        audio.ingest(torch.zeros(1, 3000, dtype=torch.int16), pad_mode="edge")
    mel = np.zeros((47, 40), np.float32)
    for starts, lens, window in [([0], [9], 8), ([0], [0], 8), ([-1], [4], 8), ([0, 1], [4], 8), ([0], [4], 0)]:
        with pytest.raises(ValueError):
            audio.load_audio_batch([mel], starts, lens, window)
    with pytest.raises(ValueError):
        audio.load_audio_batch([mel, np.zeros((47, 41), np.float32)], [0, 0], [4, 4], 8)
    with pytest.raises(ValueError):
        audio.load_audio_batch(mel, [0], [4], 8)


def test_valid_call_without_a_gpu_fails_loudly(monkeypatch):
    from m3t.ops import M3THipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(M3THipError):
        audio.ingest(torch.zeros(2, 3000, dtype=torch.int16))
    with pytest.raises(M3THipError):
        audio.ingest([np.zeros(3000, np.float32)], [_d()], 4)
    with pytest.raises(M3THipError):
        audio.load_audio_batch([np.zeros((47, 40), np.float32)], [0], [4], 8)
