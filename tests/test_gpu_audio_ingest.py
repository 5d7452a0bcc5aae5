"""The batched audio ingest on the MI355X (m3t.audio.ingest / load_audio_batch over csrc/audio_ingest.hip + m3t_sgemm): decoded PCM of a
ragged batch -> [N, T, 200] against the numpy oracle, clip by clip, O.load_audio(O.melspec_db(crop, fps, pad_mode, top_db), 0, T) with the crop
built in numpy (np.pad 'wrap' included).  Tolerance: the 2e-3 dB of tests/test_gpu_audio.py::test_logmel_vs_oracle (fp32 DFT by GEMM
against the fp64 FFT); parity with librosa itself stays unpinned as for the per-clip path.  Every case prints its measured maximum error.
length = 4 gives 13 mel frames per clip at every FPS_VALUES entry, so each case is a few thousand spectrogram cells."""
import argparse

import numpy as np
import pytest
import torch

import audio_ingest_ref as A
from conftest import load_golden
from golden.recipe import fill_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 4


def _ragged():
    """the issue's table: (fps, stored samples, start)"""
    rows = [(15.0, 6000, 0), (23.976, 2669, 0), (30.0, 1500, 3), (30.0, 9000, 3111)]
    clips = [A.signal(n, 10 + i) for i, (_, n, _) in enumerate(rows)]
    draws = [A.draw(fps, start, T) for fps, _, start in rows]
    assert draws[1]["nsamples"] == 2669 and draws[2]["nsamples"] == 2133 > 1500            # tot == nsamples; a clip that wraps
    return clips, draws


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_ragged_batch_vs_oracle(pad_mode):
    from m3t import audio
    clips, draws = _ragged()
    ref = A.reference(clips, draws, T, pad_mode)
    got = audio.ingest(clips, draws, T, pad_mode=pad_mode)
    assert got.shape == (4, T, 200) and got.dtype == torch.float32 and got.is_cuda
    assert A.max_err(got, ref, "ragged/" + pad_mode) < A.TOL_DB
    # the same clips stored in the rows of one [N, S] array with their lengths: the same table but for the offsets
    S = max(len(c) for c in clips)
    packed = np.full((4, S), 7.0, np.float32)
    for n, c in enumerate(clips):
        packed[n, :len(c)] = c
    got2 = audio.ingest(torch.from_numpy(packed), draws, T, lengths=[len(c) for c in clips], pad_mode=pad_mode)
    assert torch.equal(got2, got)


def test_int16_and_float32_give_the_same_bits():
    from m3t import audio
    clips, draws = _ragged()
    pcm = [np.clip(np.round(c * 32767.0), -32768, 32767).astype(np.int16) for c in clips]
    as_float = [(p.astype(np.float32) / np.float32(32768.0)) for p in pcm]
    a = audio.ingest(pcm, draws, T)
    b = audio.ingest(as_float, draws, T)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert A.max_err(a, A.reference(as_float, draws, T), "int16") < A.TOL_DB


def test_a_clips_floor_never_sees_its_neighbours():
    from m3t import audio
    loud = [A.signal(3000, 21), A.signal(3000, 22)]
    batch = np.stack([loud[0], np.zeros(3000, np.float32), loud[1]])
    got = audio.ingest(batch, None, T)                                   # the evaluation draws: 30 fps, centred crop
    d = audio.draw_audioset(3000, T, False)
    assert (d["fps"], d["nsamples"], d["start"]) == (30.0, 2133, (3000 - 2133) // 2)
    ref = A.reference(loud, [d, d], T)
    assert A.max_err(got[[0, 2]], ref, "isolation") < A.TOL_DB
    silent = got[1].reshape(T, 5, 40)
    rows = (3 * torch.arange(T)[:, None] + torch.arange(5)[None, :]).to(silent.device)      # mel row of each stacked slot; nf = 13
    assert int((rows >= 13).sum()) == 1
    assert torch.allclose(silent[rows < 13], torch.full_like(silent[rows < 13], -100.0))
    assert torch.equal(silent[rows >= 13], torch.zeros_like(silent[rows >= 13]))            # the reference's zero padding, not the floor


def test_the_floor_follows_rows_no_output_frame_shows():
    from m3t import audio
    d = A.draw(30.0, 0, T, nsamples=5000)                                # hand-made: hop 177 -> 29 rows, of which 14 are stacked
    assert d["hop"] == 177 and 1 + d["nsamples"] // d["hop"] == 29
    y = A.signal(5000, 4)
    y[3200:] *= 10.0 ** (30.0 / 20.0)                                    # 30 dB louder, from row 17 on only (row 16 ends at sample 3087)
    assert 16 * 177 + 255 < 3200
    mel = A.mel_db(y, d, top_db=35.0)
    quiet = A.mel_db(A.signal(5000, 4), d, top_db=35.0)
    assert (mel[:14] == mel.min()).mean() > 0.9 > 0.6 > (quiet[:14] == quiet.min()).mean()  # the unseen tail sets the floor of the shown rows
    got = audio.ingest([y], [d], T, top_db=35.0)
    assert A.max_err(got, A.reference([y], [d], T, top_db=35.0), "unseen tail") < A.TOL_DB


def test_active_floor():
    from m3t import audio
    y = A.signal(2669, 0, second_tone=False)
    d = A.draw(23.976, 0, T)
    mel = A.mel_db(y, d, top_db=35.0)
    share = float((mel == mel.max() - 35.0).mean())
    assert mel.shape == (13, 40) and 0.25 <= share <= 0.75, share          # a condition of the case, not a measurement (0.47)
    got = audio.ingest([y], [d], T, top_db=35.0)
    assert A.max_err(got, A.reference([y], [d], T, top_db=35.0), "active floor") < A.TOL_DB


def test_stacking_past_the_end_is_zero():
    from m3t import audio
    clips, draws = _ragged()                                             # 4-frame draws: nf = 13
    got = audio.ingest(clips, draws, 6)
    assert got.shape == (4, 6, 200)
    assert A.max_err(got, A.reference(clips, draws, 6), "past the end") < A.TOL_DB
    cells = got.reshape(4, 6, 5, 40)
    rows = 3 * torch.arange(6)[:, None] + torch.arange(5)[None, :]
    past = (rows >= 13).to(got.device)
    assert int(past.sum()) == 10                                        # slots 13 | 13 .. 16 | 15 .. 19 of output frames 3, 4, 5
    assert torch.equal(cells[:, past], torch.zeros_like(cells[:, past]))
    assert bool((cells[:, ~past] != 0).all())


def test_load_audio_batch_matches_the_references_stacking():
    from m3t import audio
    g = load_golden("audio_stack")
    tags = ("head", "mid", "tail", "past")
    args = [[int(v) for v in g["args." + t]] for t in tags]
    window = max(w for _, w in args) + 2
    starts, lens = [s for s, _ in args] + [0], [w for _, w in args] + [window]
    got = audio.load_audio_batch([g["mel"]] * 5, starts, lens, window, valid=[1, 1, 1, 1, 0])
    assert got.shape == (5, window, 200) and got.dtype == torch.float32
    out = got.cpu().numpy()
    for n, (tag, (_, w_len)) in enumerate(zip(tags, args)):
        assert np.array_equal(out[n, :w_len], g["out." + tag]), tag
        assert np.array_equal(out[n, w_len:], np.repeat(g["out." + tag][-1:], window - w_len, 0)), tag       # np.pad 'edge'
    assert not out[4].any()                                              # fps < 15: a zero clip
    assert np.array_equal(audio.load_audio_batch([g["mel"]] * 5, starts, lens, window).cpu().numpy()[4, :window],
                          audio.load_audio(g["mel"], 0, window).cpu().numpy())


def _audioset(seed, training=False):
    from models.audioset_model import AudioSet
    ns = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.num_hidden, ns.window = 16, T
    m = fill_module(AudioSet(ns), seed).to(DEV)
    return m.train() if training else m.eval()


def test_audioset_module_takes_pcm(monkeypatch):
    from m3t import audio
    rs = np.random.RandomState(5)
    pcm = torch.from_numpy(np.stack([np.round(A.signal(3000, 30 + i) * 32767.0).astype(np.int16) for i in range(3)]))
    label = torch.from_numpy((rs.uniform(size=(3, 527)) < 0.02).astype(np.float32)).to(DEV)
    feats = audio.ingest(pcm, None, T)
    m = _audioset(3)
    with torch.no_grad():
        assert torch.equal(m(pcm), m(feats))
    a, b = m.validation_step({"audio": pcm, "label": label}, 0), m.validation_step({"audio": feats, "label": label}, 0)
    assert torch.equal(a["val_loss"], b["val_loss"]) and torch.equal(a["correct"], b["correct"])
    # ragged clips with draws: the batch keys reach the ingest
    draws = [A.draw(30.0, 5, T), A.draw(15.0, 0, T), A.draw(25.0, 100, T)]
    lens = torch.tensor([2500, 3000, 2800])
    v = m.validation_step({"audio": pcm, "audio_aug": draws, "audio_len": lens, "label": label}, 0)
    w = m.validation_step({"audio": audio.ingest(pcm, draws, T, lengths=lens), "label": label}, 0)
    assert torch.equal(v["val_loss"], w["val_loss"]) and not torch.equal(v["val_loss"], a["val_loss"])
    # one training step on PCM
    mt = _audioset(3, training=True)
    loss = mt.training_step({"audio": pcm, "label": label}, 0)["loss"]
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    grads = [p.grad for p in mt.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and all(float(g.abs().max()) > 0 for g in grads)
    # a [N, T, 200] float batch still takes the old path
    calls = []
    real = audio.ingest
    monkeypatch.setattr(audio, "ingest", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        m(feats)
        m.validation_step({"audio": feats, "label": label}, 0)
    mt.training_step({"audio": feats, "label": label}, 0)
    assert calls == []
    with torch.no_grad():
        m(pcm)
    assert calls == [1]
