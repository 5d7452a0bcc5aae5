"""Audio front-end on the GPU: the log-Mel features the reference extracts offline
(`process/extract_melspec.py:8-20`) and the context stacking of `models/dataset.py:83-95` that turns them into the
`[T, 200]` rows `AffWild2VA.forward` consumes as `batch['audio']`.

  melspec_db(y, fps)               = librosa.power_to_db(librosa.feature.melspectrogram(y=y, sr=16000, n_fft=512,
                                       hop_length=int(1/3 * 1/fps * 16000), win_length=400, n_mels=40)).T   -> [frames, 40]
  load_audio(mel, start_idx, w_len) = models/dataset.py:83-95 (rows (start+i)*3 .. +5, zero padded, flattened) -> [w_len, 200]

librosa is a third-party dependency the reference does not pin (requirements.txt has no version) and it is absent from
this image, so the spectrogram half is restated from librosa's published algorithm -- periodic Hann window of
`win_length` centred in `n_fft`, `center=True` framing, power spectrum, Slaney mel filterbank (`htk=False`,
`norm='slaney'`, 0..sr/2), `power_to_db(ref=1, amin=1e-10, top_db=80)` -- and its parity is UNPINNED: it is checked
against the numpy oracle only.  `pad_mode` defaults to librosa >= 0.10's zero padding ('constant'); older librosa
reflected ('reflect').  The stacking half is pinned on the reference's own function.

Constants (window, DFT matrix, filterbank) are built once on the host in float64; the data path is HIP:
m3t_frame_window -> m3t_sgemm (DFT, fp32-accurate) -> m3t_power_spectrum -> m3t_sgemm (mel) -> m3t_power_to_db.

The batched ingest (csrc/audio_ingest.hip) is the input stage of the audio tasks: audio AS DECODED (16 kHz PCM, int16 or float32), a whole
batch of ragged clips at once, to the `[N, T, 200]` rows of the reference's AudioSet loader (`models/audioset_dataset.py:58-87`: random fps,
temporal crop with np.pad 'wrap', the spectrogram above, the context stack) in three kernels and one GEMM however many clips there are:

  draw_audioset(tot, length, training)   one clip's draws, consuming `random` in the reference's order
  plan_waves(...)                        host validation + the per-clip table, before anything touches a device
  ingest(waves, aug, length)             m3t_audio_frame_batch -> m3t_sgemm (ONE DFT product) -> m3t_audio_power_mel -> m3t_audio_db_stack
  draw_spec_augment(tau, F, T, ..)       the mask draws of the reference's spec_augment (`audioset_dataset.py:17-55`), in its order
  plan_aug(aug, table, mix)              host validation + the two tables of the augmented last kernel (m3t_audio_db_stack_aug): masks from
                                         the draws, mix = (partner, lam); None when neither is present, and the call is what it was
  load_audio_batch(mels, starts, ...)    the AffWild2 loader's collate step (`models/dataset.py:83-95, :276-306`): N pre-extracted tracks
                                         -> [N, window, 200] in one launch, edge padding and the "fps < 15 -> zeros" rule included

The wave conversion (csrc/resample.hip) is what `librosa.load(path, sr=16000)` does in front of both: any WAV rate, 1..8 channels,
PCM 8/16/24/32 or float32 -> 16 kHz mono float32, from the raw bytes, one launch per source rate for a ragged batch:

  decode_waves(files or (bytes, WaveInfo) pairs)   -> (flat float32 device buffer, offsets, lengths)
  load_wave(path)                                  = librosa.load(path, sr=16000)[0] (process/extract_melspec.py:13)
  converted_length(frames, rate)                   a clip's length after conversion, from its header alone (what an epoch plan needs)
  plan_convert(...)                                host validation + the per-clip table, before anything touches a device

Wav reading is m3t/wav.py (on the host: headers and raw bytes), the resident store of a split's clips m3t/audioset.py, the AffWild2 mel
tracks m3t/melspec.py.
"""
import ctypes as C
import math
import os
import random

import numpy as np
import torch

from . import _lib
from . import wav as _wav
from .ops import lib, _stream, _p, sgemm, workspace, M3THipError

SR, N_FFT, WIN, N_MELS = 16000, 512, 400, 40
_CONST = {}


def hop_length(fps):
    """process/extract_melspec.py:15"""
    return int(1 / 3 * 1 / fps * 16000)


def mel_filterbank(sr=SR, n_fft=N_FFT, n_mels=N_MELS):
    """librosa.filters.mel(htk=False, norm='slaney', fmin=0, fmax=sr/2) -> [n_mels, 1 + n_fft/2] float64"""
    def hz_to_mel(f):
        f = np.asarray(f, np.float64)
        mel = f / (200.0 / 3)
        logstep = math.log(6.4) / 27.0
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / logstep, mel)

    def mel_to_hz(m):
        m = np.asarray(m, np.float64)
        logstep = math.log(6.4) / 27.0
        return np.where(m >= 15.0, 1000.0 * np.exp(logstep * (m - 15.0)), m * (200.0 / 3))

    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w


def _constants(device):
    key = (device.type, device.index)
    c = _CONST.get(key)
    if c is None:
        win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(WIN) / WIN)           # periodic Hann (scipy get_window fftbins=True)
        pad = (N_FFT - WIN) // 2
        win = np.concatenate([np.zeros(pad), win, np.zeros(N_FFT - WIN - pad)])
        bins = 1 + N_FFT // 2
        k, n = np.arange(bins)[None, :], np.arange(N_FFT)[:, None]
        ang = 2 * np.pi * k * n / N_FFT
        dft = np.concatenate([np.cos(ang), -np.sin(ang)], 1)                # [n_fft, 2*bins]: re | im
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
        c = (dev(win), dev(dft), dev(mel_filterbank().T))                   # mel as [bins, n_mels]
        _CONST[key] = c
    return c


def melspec_db(y, fps=30.0, pad_mode="constant", top_db=80.0):
    """y: 1-D float waveform at 16 kHz (array or tensor) -> [frames, 40] float32 CUDA tensor of log-Mel energies (dB),
    frames = 1 + len(y) // hop."""
    if not torch.cuda.is_available():
        raise M3THipError("m3t.audio needs the GPU: the M3T path has no CPU fallback")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError("pad_mode must be 'constant' or 'reflect'")
    dev = torch.device("cuda", torch.cuda.current_device())
    y = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).detach().to(dev, torch.float32).reshape(-1).contiguous()
    n, hop = int(y.numel()), hop_length(fps)
    if n == 0 or hop <= 0:
        raise M3THipError("melspec_db: empty waveform or non-positive hop")
    win, dft, melT = _constants(dev)
    bins = 1 + N_FFT // 2
    nf = 1 + n // hop
    frames = torch.empty(nf, N_FFT, dtype=torch.float32, device=dev)
    _lib.check(lib().m3t_frame_window(_p(y), n, N_FFT, hop, 1 if pad_mode == "reflect" else 0, _p(win), _p(frames), nf,
                                      _stream()), "m3t_frame_window")
    spec = torch.empty(nf, 2 * bins, dtype=torch.float32, device=dev)
    sgemm(0, 0, nf, 2 * bins, N_FFT, frames, 0, N_FFT, dft, 0, 2 * bins, spec, 0, 2 * bins, prec=0, exclusive=True)
    power = torch.empty(nf, bins, dtype=torch.float32, device=dev)
    _lib.check(lib().m3t_power_spectrum(_p(spec), nf, bins, _p(power), _stream()), "m3t_power_spectrum")
    mel = torch.empty(nf, N_MELS, dtype=torch.float32, device=dev)
    sgemm(0, 0, nf, N_MELS, bins, power, 0, bins, melT, 0, N_MELS, mel, 0, N_MELS, prec=0, exclusive=True)
    out = torch.empty_like(mel)
    ws = workspace(dev)
    _lib.check(lib().m3t_power_to_db(_p(mel), mel.numel(), 1e-10, float(top_db), _p(out), _p(ws), ws.numel() * 4, _stream()),
               "m3t_power_to_db")
    return out


def load_audio(mel_spec, start_idx, w_len):
    """models/dataset.py:83-95 with the .npy already in memory: mel_spec [frames, 40] (array, tensor or path) ->
    [w_len, 200] float32 CUDA tensor: row i = mel rows (start_idx + i)*3 .. +5, zero padded past the end."""
    if isinstance(mel_spec, str):
        mel_spec = np.load(mel_spec)
    dev = torch.device("cuda", torch.cuda.current_device())
    mel = torch.as_tensor(np.asarray(mel_spec) if not isinstance(mel_spec, torch.Tensor) else mel_spec).detach().to(dev, torch.float32).contiguous()
    out = torch.empty(int(w_len), 5 * mel.shape[1], dtype=torch.float32, device=dev)
    _lib.check(lib().m3t_stack_context(_p(mel), mel.shape[0], mel.shape[1], int(start_idx), int(w_len), 3, 5, _p(out), _stream()),
               "m3t_stack_context")
    return out


# ---- batched ingest: decoded PCM -> [N, T, 200] (csrc/audio_ingest.hip) ---------------------------------------------------------------
FPS_VALUES = [15.0, 17.0, 19.0, 22.0, 23.976, 24.0, 25.0, 29.97, 30.0]      # audioset_dataset.py:13
_MEL_SPARSE = {}


MAX_MASKS = 4                           # masks of each kind a clip may carry (csrc/audio_aug_core.h)
_AUG_INTS = 20                          # n_freq, n_time, partner, 0, (f0, f) x 4, (t0, t) x 4


def draw_spec_augment(tau, F=20, T=20, n_freq=1, n_time=1, name="clip"):
    """The draws of the reference's spec_augment (models/audioset_dataset.py:17-55) for a spectrogram [1, 40, tau], consuming np.random and
    `random` in its order: per frequency mask f = int(np.random.uniform(0.0, F)) then f0 = random.randint(0, 40 - f); then per time mask
    t = int(np.random.uniform(0.0, T)) then t0 = random.randint(0, tau - t).  -> {"fmask": [(f0, f), ..], "tmask": [(t0, t), ..]}: bands
    f0 .. f0 + f - 1 and frames t0 .. t0 + t - 1 become 0.0.  A draw the reference's randint would refuse (f > 40, t > tau) is a
    ValueError that names the clip; so are more than MAX_MASKS masks of a kind.  Host only."""
    tau, n_freq, n_time = int(tau), int(n_freq), int(n_time)
    if not (0 <= n_freq <= MAX_MASKS and 0 <= n_time <= MAX_MASKS):
        raise ValueError("spec_augment: %s: %d frequency and %d time masks asked for; 0 .. %d of each are taken" % (name, n_freq, n_time, MAX_MASKS))
    fmask, tmask = [], []
    for _ in range(n_freq):
        f = int(np.random.uniform(low=0.0, high=F))
        if f > N_MELS:
            raise ValueError("spec_augment: %s: a frequency mask of %d bands does not fit the %d there are" % (name, f, N_MELS))
        fmask.append((random.randint(0, N_MELS - f), f))
    for _ in range(n_time):
        t = int(np.random.uniform(low=0.0, high=T))
        if t > tau:
            raise ValueError("spec_augment: %s: a time mask of %d frames does not fit the %d there are" % (name, t, tau))
        tmask.append((random.randint(0, tau - t), t))
    return {"fmask": fmask, "tmask": tmask}


def draw_audioset(tot_samples, length, training, spec_aug=None, name="clip"):
    """One clip's draws of models/audioset_dataset.py:60-69 for a decoded clip of `tot_samples` samples: random.choice(FPS_VALUES) (training
    only; 30.0 otherwise), nsamples = int(length / fps * 16000), then random.randint(0, tot' - nsamples) (training) or the centre, where
    tot' = nsamples + 5 when the clip is shorter than nsamples (the np.pad(..., 'wrap') of :65-68) and tot_samples otherwise.
    spec_aug: None, or draw_spec_augment's keyword arguments (F, T, n_freq, n_time): a TRAINING draw then goes on with that function's
    draws for tau = 1 + nsamples // hop, after the ones above, and carries its two keys; an evaluation draw never does."""
    fps = random.choice(FPS_VALUES) if training else 30.0
    nsamples = int(length / fps * 16000)
    tot = int(tot_samples)
    if nsamples > tot:
        tot = nsamples + 5
    start = random.randint(0, tot - nsamples) if training else (tot - nsamples) // 2
    d = {"fps": fps, "hop": hop_length(fps), "start": start, "nsamples": nsamples}
    if training and spec_aug is not None:
        d.update(draw_spec_augment(1 + nsamples // d["hop"], name=name, **spec_aug))
    return d


def plan_aug(aug, table, mix=None):
    """Host validation of the augmentation of an ingest call, before anything touches a device.  aug: the clips' draws (those that carry
    draw_spec_augment's "fmask" / "tmask" are masked); table: plan_waves' for the same clips; mix: None or (partner int [N], lam float [N]).
    -> None when no draw carries a mask and mix is None: the call takes the un-augmented route.  Otherwise (ints int32 [N, 20], weights
    float32 [N, 2]) of include/m3t_hip.h (m3t_audio_db_stack_aug): counts, partner (-1 without mix), the mask pairs; lam32 =
    np.float32(lam) and om32 = np.float32(1) - lam32.  ValueError, with the clip named, for more than MAX_MASKS masks of a kind, a mask
    outside [0, 40] / [0, nf], a partner outside the batch, a lam outside [0, 1]."""
    N = int(table.shape[0])
    masked = aug is not None and any(("fmask" in a or "tmask" in a) for a in aug)
    if not masked and mix is None:
        return None
    if aug is None:
        raise ValueError("ingest: mix goes with training draws; aug=None (the evaluation draws) is never augmented")
    ints = np.zeros((N, _AUG_INTS), np.int32)
    ints[:, 2] = -1
    weights = np.zeros((N, 2), np.float32)
    weights[:, 0] = 1.0
    for n, a in enumerate(aug):
        for kind, (key, col, limit, what) in enumerate((("fmask", 4, N_MELS, "bands"), ("tmask", 12, int(table[n, 5]), "frames"))):
            pairs = list(a.get(key, ()))
            if len(pairs) > MAX_MASKS:
                raise ValueError("ingest: clip %d: %d masks under %r; at most %d are taken" % (n, len(pairs), key, MAX_MASKS))
            ints[n, kind] = len(pairs)
            for q, (lo, width) in enumerate(pairs):
                lo, width = int(lo), int(width)
                if lo < 0 or width < 0 or lo + width > limit:
                    raise ValueError("ingest: clip %d: mask %s %d .. %d lies outside the clip's %d" % (n, what, lo, lo + width, limit))
                ints[n, col + 2 * q], ints[n, col + 2 * q + 1] = lo, width
    if mix is not None:
        partner, lam = np.asarray(mix[0]), np.asarray(mix[1], np.float64)
        if partner.shape != (N,) or lam.shape != (N,) or not np.issubdtype(partner.dtype, np.integer):
            raise ValueError("ingest: mix needs (partner int [%d], lam float [%d])" % (N, N))
        for n in np.flatnonzero((partner < 0) | (partner >= N)):
            raise ValueError("ingest: clip %d: its partner %d is outside the batch of %d" % (n, partner[n], N))
        for n in np.flatnonzero(~((lam >= 0.0) & (lam <= 1.0))):
            raise ValueError("ingest: clip %d: lam %r is outside [0, 1]" % (n, float(lam[n])))
        ints[:, 2] = partner
        weights[:, 0] = lam.astype(np.float32)
        weights[:, 1] = np.float32(1) - weights[:, 0]
    return ints, weights


def pack_tables(table, tables, extra=None):
    """plan_waves' table, plan_aug's two (or None) and an optional int64 tail as ONE int64 array, so that they reach the device in one copy,
    and the function that cuts the device copy up again: -> (flat int64 array, split(device tensor) -> (tab, (ints, weights) | None, tail))"""
    N = int(table.shape[0])
    parts = [table.reshape(-1)]
    if tables is not None:
        parts += [np.ascontiguousarray(tables[0]).reshape(-1).view(np.int64), np.ascontiguousarray(tables[1]).reshape(-1).view(np.int64)]
    if extra is not None:
        parts.append(np.asarray(extra, np.int64).reshape(-1))
    a = 8 * N                                    # in int64 words: the clip table, then 20 int32 and 2 float32 per clip, then the tail
    m = a + (_AUG_INTS // 2) * N
    b = m + N if tables is not None else a

    def split(dev):
        aug_tab = None if tables is None else (dev[a:m].view(torch.int32), dev[m:b].view(torch.float32))
        return dev[:a], aug_tab, dev[b:]

    return np.concatenate(parts), split


def plan_waves(waves, aug=None, length=32, lengths=None, offsets=None):
    """Host validation of an ingest call, before anything touches a device: returns (wave, table, R) -- the flat sample buffer (a 1-D int16 or
    float32 tensor on the device `waves` lives on), the per-clip table int64 [N, 8] = off, len, start, nsamples, hop, nf, row_off, 0
    (include/m3t_hip.h) and the number of spectrogram rows of the batch.  ValueError for a wrong dtype or rank, a draw count different from
    N, hop <= 0, nsamples <= 0, length <= 0, a start outside [0, max(len, nsamples + 5)), an empty clip.
    The store form, `offsets` given: `waves` is a flat 1-D tensor that is read in place (a resident store, m3t.audioset.WaveStore) and clip n
    is waves[offsets[n] : offsets[n] + lengths[n]]; clips may repeat or overlap.  No sample is copied or looked at; ValueError for an
    offset or a length that leaves the buffer.  The table is the list form's but for the offsets."""
    if int(length) <= 0:
        raise ValueError("ingest: length must be positive, got %r" % (length,))
    if offsets is not None:
        if not isinstance(waves, torch.Tensor) or waves.dim() != 1 or not waves.is_contiguous():
            raise ValueError("ingest: with offsets, waves must be one flat contiguous 1-D tensor")
        if lengths is None:
            raise ValueError("ingest: offsets go with the clips' lengths")
        offs = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets)
        lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)
        if offs.ndim != 1 or lens.shape != offs.shape or not (np.issubdtype(offs.dtype, np.integer) and np.issubdtype(lens.dtype, np.integer)):
            raise ValueError("ingest: offsets and lengths must be integers [N]")
        offs, lens = offs.astype(np.int64), lens.astype(np.int64)
        total = int(waves.numel())
        for n in np.flatnonzero((offs < 0) | (lens <= 0) | (offs > total - lens)):
            raise ValueError("ingest: clip %d: samples %d .. %d lie outside the buffer's %d (or the clip is empty)"
                             % (n, offs[n], int(offs[n]) + int(lens[n]), total))
        wave = waves.detach()
    elif isinstance(waves, (list, tuple)):
        clips = [np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w) for w in waves]
        if not clips:
            raise ValueError("ingest: no clips")
        if lengths is not None:
            raise ValueError("ingest: `lengths` goes with a [N, S] batch, a list carries its own")
        if any(c.ndim != 1 for c in clips) or len({c.dtype for c in clips}) != 1:
            raise ValueError("ingest: a list must hold 1-D arrays of one dtype")
        lens = np.array([c.shape[0] for c in clips], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        wave = torch.from_numpy(np.ascontiguousarray(np.concatenate(clips)))
    else:
        if isinstance(waves, np.ndarray):
            waves = torch.from_numpy(np.ascontiguousarray(waves))
        if not isinstance(waves, torch.Tensor):
            raise ValueError("ingest: waves must be a tensor, an array or a list of 1-D arrays")
        if waves.dim() != 2:
            raise ValueError("ingest: waves must be [N, S], got %s" % (list(waves.shape),))
        N, S = int(waves.shape[0]), int(waves.shape[1])
        if lengths is None:
            lens = np.full(N, S, np.int64)
        else:
            lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)
            if lens.shape != (N,) or not np.issubdtype(lens.dtype, np.integer):
                raise ValueError("ingest: lengths must be integers [N]")
            lens = lens.astype(np.int64)
            if N and lens.max() > S:
                raise ValueError("ingest: a length beyond the %d stored samples" % S)
        offs = np.arange(N, dtype=np.int64) * S
        wave = waves.detach().contiguous().reshape(-1)
    if wave.dtype not in (torch.int16, torch.float32):
        raise ValueError("ingest: waves must be int16 or float32, got %s" % wave.dtype)
    N = int(lens.shape[0])
    if N == 0 or lens.min() <= 0:
        raise ValueError("ingest: an empty clip")
    if aug is None:
        aug = [draw_audioset(int(n), int(length), False) for n in lens]
    if len(aug) != N:
        raise ValueError("ingest: %d draws for %d clips" % (len(aug), N))
    table = np.zeros((N, 8), np.int64)
    table[:, 0], table[:, 1] = offs, lens
    for n, a in enumerate(aug):
        start, ns, hop = int(a["start"]), int(a["nsamples"]), int(a["hop"])
        if hop <= 0 or ns <= 0:
            raise ValueError("ingest: clip %d: hop %d and nsamples %d must be positive" % (n, hop, ns))
        if not 0 <= start < max(int(lens[n]), ns + 5):
            raise ValueError("ingest: clip %d: start %d outside [0, %d)" % (n, start, max(int(lens[n]), ns + 5)))
        table[n, 2:6] = (start, ns, hop, 1 + ns // hop)
    table[1:, 6] = np.cumsum(table[:-1, 5])
    return wave, table, int(table[:, 5].sum())


def _mel_sparse(device):
    """the filterbank's non-zero runs: (weights float32 [nnz], bands int32 [2 n_mels + 1] = offsets | first bins, nnz) on `device`"""
    key = (device.type, device.index)
    c = _MEL_SPARSE.get(key)
    if c is None:
        fb = mel_filterbank()
        w, offs, first = [], [0], []
        for b in range(N_MELS):
            nz = np.nonzero(fb[b])[0]
            lo, hi = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
            w.append(fb[b, lo:hi])
            offs.append(offs[-1] + hi - lo)
            first.append(lo)
        w = np.concatenate(w).astype(np.float32)
        bands = np.array(offs + first, np.int32)
        c = _MEL_SPARSE[key] = (torch.from_numpy(w).to(device), torch.from_numpy(bands).to(device), int(w.shape[0]))
    return c


def ingest(waves, aug=None, length=32, lengths=None, pad_mode="constant", top_db=80.0, offsets=None, mix=None):
    """waves: decoded 16 kHz PCM, int16 or float32: [N, S] (tensor or array; `lengths` int [N] for ragged clips stored in rows of S), a
    list of 1-D arrays, or -- with `offsets` and `lengths`, int [N] -- one flat buffer read in place (plan_waves' store form: nothing is
    copied when it lives on the device).  A host tensor is copied to the device with non_blocking=True -- pin it to overlap the copy.
    aug: one draw per clip (draw_audioset) or None = the evaluation draws (30 fps, centred crop).  -> float32 device tensor
    [N, length, 200]: per clip what load_audio(melspec_db(crop, fps), 0, length) gives (audioset_dataset.py:58-87), the dB floor taken from the clip's own maximum.
    Everything is validated on the host first (ValueError); the per-clip table reaches the device in one copy; three kernels and one GEMM.
    Training-time augmentation, opt-in (plan_aug): draws that carry draw_spec_augment's "fmask" / "tmask" have those bands and frames of
    their dB spectrogram set to 0.0 before the stack (the reference's spec_augment, audioset_dataset.py:17-55); mix = (partner, lam) then
    gives out[n] = lam32[n] x[n] + om32[n] x[partner[n]] over the masked rows x.  Both happen inside the last kernel
    (m3t_audio_db_stack_aug in place of m3t_audio_db_stack): still three kernels, one GEMM and one table copy.  With neither present
    the call is what it was."""
    if pad_mode not in ("constant", "reflect"):
        raise ValueError("pad_mode must be 'constant' or 'reflect'")
    wave, table, R = plan_waves(waves, aug, length, lengths, offsets)
    tables = plan_aug(aug, table, mix)
    if not torch.cuda.is_available():
        raise M3THipError("m3t.audio needs the GPU: the M3T path has no CPU fallback")
    dev = wave.device if wave.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if tables is None:
        tab = torch.from_numpy(table.reshape(-1)).to(dev, non_blocking=True)
        return ingest_planned(wave.to(dev, non_blocking=True), tab, table.shape[0], R, length, pad_mode, top_db)
    flat, split = pack_tables(table, tables)
    tab, aug_tab, _ = split(torch.from_numpy(flat).to(dev, non_blocking=True))
    return ingest_planned(wave.to(dev, non_blocking=True), tab, table.shape[0], R, length, pad_mode, top_db, aug_tab)


def ingest_planned(wave, tab, N, R, length=32, pad_mode="constant", top_db=80.0, aug_tab=None):
    """ingest's launches for a batch that is planned and on the device: wave, the flat sample buffer; tab, plan_waves' table as a device
    int64 tensor (N * 8 values, 8-byte aligned -- it may be a slice of a larger upload); R, the table's row count; aug_tab, None or
    plan_aug's two tables on the device (int32, N * 20 values; float32, N * 2 values; slices of the same upload, pack_tables)."""
    if pad_mode not in ("constant", "reflect"):
        raise ValueError("pad_mode must be 'constant' or 'reflect'")
    if not (wave.is_cuda and tab.is_cuda and tab.dtype == torch.int64 and tab.is_contiguous() and tab.numel() == 8 * N and wave.dim() == 1):
        raise ValueError("ingest_planned: a flat device buffer and a device int64 table of %d x 8 values are needed" % N)
    if aug_tab is not None:
        ai, af = aug_tab
        if not (ai.is_cuda and af.is_cuda and ai.dtype == torch.int32 and af.dtype == torch.float32 and ai.is_contiguous() and af.is_contiguous()
                and ai.numel() == _AUG_INTS * N and af.numel() == 2 * N):
            raise ValueError("ingest_planned: the augmentation needs device tables of %d x %d int32 and %d x 2 float32 values" % (N, _AUG_INTS, N))
    dev = wave.device
    N, T, R, bins = int(N), int(length), int(R), 1 + N_FFT // 2
    win, dft, _ = _constants(dev)
    weights, bands, nnz = _mel_sparse(dev)
    L, st = lib(), _stream()
    frames = torch.empty(R, N_FFT, dtype=torch.float32, device=dev)
    _lib.check(L.m3t_audio_frame_batch(wave.data_ptr(), 1 if wave.dtype == torch.int16 else 0, wave.numel(), tab.data_ptr(), N, R, N_FFT,
                                       1 if pad_mode == "reflect" else 0, _p(win), _p(frames), st), "m3t_audio_frame_batch")
    spec = torch.empty(R, 2 * bins, dtype=torch.float32, device=dev)
    sgemm(0, 0, R, 2 * bins, N_FFT, frames, 0, N_FFT, dft, 0, 2 * bins, spec, 0, 2 * bins, prec=0, exclusive=True)
    mel = torch.empty(R, N_MELS, dtype=torch.float32, device=dev)
    _lib.check(L.m3t_audio_power_mel(_p(spec), R, bins, N_MELS, _p(weights), bands.data_ptr(), nnz, _p(mel), st), "m3t_audio_power_mel")
    out = torch.empty(N, T, 5 * N_MELS, dtype=torch.float32, device=dev)
    if aug_tab is None:
        _lib.check(L.m3t_audio_db_stack(_p(mel), R, tab.data_ptr(), N, T, N_MELS, 3, 5, 1e-10, float(top_db), _p(out), st), "m3t_audio_db_stack")
    else:
        _lib.check(L.m3t_audio_db_stack_aug(_p(mel), R, tab.data_ptr(), N, aug_tab[0].data_ptr(), aug_tab[1].data_ptr(), T, N_MELS, 3, 5, 1e-10,
                                            float(top_db), _p(out), st), "m3t_audio_db_stack_aug")
    return out


def load_audio_batch(mels, starts, track_lens, window, valid=None):
    """The AffWild2 loader's audio half as a collate step (models/dataset.py:83-95, :276-306).  mels: N pre-extracted tracks, a list of
    [rows_n, 40] arrays or tensors (or one [N, rows, 40]); starts, track_lens: int [N], 0 < track_len <= window; valid: bool [N] or None
    (the loader's `fps >= 15`).  -> float32 device tensor [N, window, 200]: row i < track_len is load_audio(mel_n, start_n, track_len_n)'s,
    rows track_len .. window-1 repeat row track_len-1 (np.pad 'edge'), an invalid clip is zeros.  One launch."""
    window = int(window)
    if isinstance(mels, (np.ndarray, torch.Tensor)):
        if mels.ndim != 3:
            raise ValueError("load_audio_batch: mels must be a list of [rows, n_mels] tracks or one [N, rows, n_mels] batch")
        mels = list(mels)
    N = len(mels)
    starts, track_lens = np.asarray(starts, np.int64).reshape(-1), np.asarray(track_lens, np.int64).reshape(-1)
    valid = np.ones(N, bool) if valid is None else np.asarray(valid).astype(bool).reshape(-1)
    if N == 0 or window <= 0 or starts.shape != (N,) or track_lens.shape != (N,) or valid.shape != (N,):
        raise ValueError("load_audio_batch: %d tracks need %d starts, track lengths and valid flags, and a positive window" % (N, N))
    if starts.min() < 0 or track_lens.min() <= 0 or track_lens.max() > window:
        raise ValueError("load_audio_batch: starts must be >= 0 and 0 < track_len <= window")
    if any(m.ndim != 2 or m.shape[1] != mels[0].shape[1] or m.shape[0] <= 0 for m in mels):
        raise ValueError("load_audio_batch: every track must be [rows > 0, n_mels]")
    if not torch.cuda.is_available():
        raise M3THipError("m3t.audio needs the GPU: the M3T path has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    n_mels = int(mels[0].shape[1])
    rows = np.array([m.shape[0] for m in mels], np.int64)
    table = np.zeros((N, 4), np.int64)
    table[1:, 0] = np.cumsum(rows[:-1])
    table[:, 1], table[:, 2], table[:, 3] = rows, starts, np.where(valid, track_lens, 0)
    tab = torch.from_numpy(table.reshape(-1)).to(dev, non_blocking=True)
    if all(isinstance(m, torch.Tensor) for m in mels):
        flat = torch.cat([m.detach().to(dev, torch.float32) for m in mels]).contiguous()
    else:
        flat = torch.from_numpy(np.concatenate([np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m, np.float32) for m in mels])).to(dev, non_blocking=True)
    out = torch.empty(N, window, 5 * n_mels, dtype=torch.float32, device=dev)
    _lib.check(lib().m3t_stack_context_batch(_p(flat), int(rows.sum()), n_mels, tab.data_ptr(), N, window, 3, 5, _p(out), _stream()),
               "m3t_stack_context_batch")
    return out


# ---- wave conversion: a WAV of any rate, channel count and depth -> 16 kHz mono float32 (csrc/resample.hip) --------------
NUM_ZEROS, PRECISION, ROLLOFF, KAISER_BETA = 64, 9, 0.9475937167399596, 14.769656459379492       # resampy's 'kaiser_best'
TILE, SEG = 256, 64                     # outputs of a workgroup; outputs per host-accumulated register start (csrc/resample.hip)
MAX_RATE = 384000                       # the tile's span of source frames must fit 64 KB of LDS
STAGE_BYTES = 64 << 20
_ALIGN = 16
_RES_TABLE, _RES_STARTS = {}, {}


def converted_length(frames, rate):
    """len(librosa.load(path, sr=16000)[0]) for a file of `frames` frames at `rate` Hz: int(ceil(frames * (16000.0 / rate))) in float64 AS
    WRITTEN (librosa.resample's n_samples: the rule is the float64 expression, not integer arithmetic).  Host only."""
    return int(np.ceil(int(frames) * (float(SR) / int(rate))))


def resampled_length(frames, rate):
    """the outputs the filter computes, resampy's int(frames * ratio); the rest up to converted_length is fix_length's 0.0"""
    return int(int(frames) * (float(SR) / int(rate)))


def resample_filter(rate):
    """-> float64 [32769, 2] = (win, delta) of DESIGN.md 4c for a source of `rate` Hz: the right half of
    kaiser(2n + 1, beta) * rolloff * sinc(rolloff * j / 512), n = 64 * 512, times ratio when ratio < 1; delta = diff(win) and a last 0."""
    n = NUM_ZEROS << PRECISION
    win = np.kaiser(2 * n + 1, KAISER_BETA)[n:] * (ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, num=n + 1, endpoint=True)))
    ratio = float(SR) / int(rate)
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return np.ascontiguousarray(np.stack([win, delta], 1), np.float64)


def register_starts(rate, n_out):
    """float64 [4 ceil(n_out / 256)]: the time register r_t at t = 0, 64, 128, ..., where r_0 = 0.0 and r_{t+1} = r_t + rate / 16000.0 by
    sequential float64 additions (np.add.accumulate; resampy's `time_register += time_increment`).  Depends on the rate only."""
    count = (TILE // SEG) * -(-int(n_out) // TILE)
    steps = np.full(count * SEG, int(rate) / float(SR))
    steps[0] = 0.0
    return np.ascontiguousarray(np.add.accumulate(steps)[::SEG])


def plan_convert(infos, byte_offsets, n_bytes, out_offsets=None, names=None):
    """Host validation of a convert call, before anything touches a device.  infos: one m3t.wav.WaveInfo per clip; byte_offsets: where each
    clip's 'data' body starts in the byte buffer of `n_bytes`; out_offsets: where its outputs start (default: packed in order).
    -> (out_offsets int64 [F], lengths int64 [F], total outputs, {rate: (clip indices, table int64 [N, 8], tiles)}), the table of
    include/m3t_hip.h (m3t_wave_convert).  ValueError, with the clip named, for an empty clip, a kind / channel count / rate outside
    what the kernel takes, a body that leaves the buffer or starts off its sample's alignment."""
    F = len(infos)
    if F == 0:
        raise ValueError("decode_waves: no clips")
    names = ["clip %d" % i for i in range(F)] if names is None else names
    offs = np.asarray(byte_offsets, np.int64).reshape(-1)
    if offs.shape != (F,):
        raise ValueError("decode_waves: %d byte offsets for %d clips" % (offs.shape[0], F))
    lengths = np.zeros(F, np.int64)
    for i, w in enumerate(infos):
        if not (0 <= int(w.kind) < len(_wav.KIND_BYTES) and 1 <= int(w.channels) <= _wav.MAX_CHANNELS):
            raise ValueError("%s: kind %r with %r channels is not a sample format the convert kernel takes" % (names[i], w.kind, w.channels))
        if not 1 <= int(w.rate) <= MAX_RATE:
            raise ValueError("%s: sampled at %d Hz; 1 .. %d Hz is taken" % (names[i], w.rate, MAX_RATE))
        if int(w.frames) <= 0:
            raise ValueError("%s: an empty clip (no whole frame in its 'data' chunk)" % (names[i],))
        sample = _wav.KIND_BYTES[w.kind]
        if offs[i] < 0 or offs[i] % (1 if w.kind == _wav.KIND_I24 else sample) or int(w.frames) * sample * int(w.channels) > n_bytes - offs[i]:
            raise ValueError("%s: bytes %d .. %d lie outside the buffer's %d (or off the sample's alignment)"
                             % (names[i], offs[i], offs[i] + int(w.frames) * sample * int(w.channels), n_bytes))
        lengths[i] = converted_length(w.frames, w.rate)
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    out_offsets = np.asarray(out_offsets, np.int64)
    groups = {}
    for rate in sorted({int(w.rate) for w in infos}):
        idx = np.array([i for i, w in enumerate(infos) if int(w.rate) == rate], np.int64)
        table = np.zeros((idx.shape[0], 8), np.int64)
        for r, i in enumerate(idx):
            w = infos[i]
            table[r, :7] = (offs[i], w.frames, w.channels, w.kind, out_offsets[i], resampled_length(w.frames, rate), lengths[i])
        tiles = -(-table[:, 6] // TILE)
        table[1:, 7] = np.cumsum(tiles[:-1])
        groups[rate] = (idx, table, int(tiles.sum()))
    return out_offsets, lengths, int(lengths.sum()), groups


def _filter_on(dev, rate):
    key = (dev.type, dev.index, rate if rate > SR else 0)            # (upsampling does not scale the table: one for every such rate)
    t = _RES_TABLE.get(key)
    if t is None:
        t = _RES_TABLE[key] = torch.from_numpy(resample_filter(rate)).to(dev)
    return t


def _starts_on(dev, rate, n_out):
    key = (dev.type, dev.index, rate)
    need = (TILE // SEG) * -(-int(n_out) // TILE)
    t = _RES_STARTS.get(key)
    if t is None or t.numel() < need:
        t = _RES_STARTS[key] = torch.from_numpy(register_starts(rate, n_out)).to(dev)
    return t


def convert_planned(raw, groups, out):
    """the launches of a planned convert: raw, the uint8 device buffer of the clips' bodies; groups, plan_convert's; out, the flat float32
    device buffer the tables' output offsets point into.  One table upload, one launch per distinct rate; nothing is read back."""
    dev = raw.device
    tab = torch.from_numpy(np.concatenate([t.reshape(-1) for _, t, _ in groups.values()])).to(dev, non_blocking=True)
    row = 0
    for rate, (idx, table, tiles) in groups.items():
        N = int(table.shape[0])
        filt = starts = None
        if rate != SR:
            filt, starts = _filter_on(dev, rate), _starts_on(dev, rate, int(table[:, 6].max()))
        _lib.check(lib().m3t_wave_convert(raw.data_ptr(), raw.numel(), tab.data_ptr() + 64 * row, N, tiles, rate,
                                          None if filt is None else filt.data_ptr(),
                                          None if starts is None else starts.data_ptr(), 0 if starts is None else starts.numel(),
                                          _p(out), out.numel(), _stream()), "m3t_wave_convert")
        row += N


def decode_waves(items, device=None, chunk_bytes=STAGE_BYTES):
    """items: .wav paths, or (bytes, WaveInfo) pairs as m3t.wav.read_wave gives them (a uint8 array or a bytes object: the 'data' body).
    -> (flat float32 device buffer, offsets int64 [F], lengths int64 [F] on the host): clip i, as `librosa.load(path, sr=16000)[0]` of the
    reference's era gives it, is buffer[offsets[i] : offsets[i] + lengths[i]].
    The headers are read first (the buffer's size is known before a sample is); then the bodies go up in chunks of at most `chunk_bytes`
    through ONE pinned stage (a longer clip goes on its own), each chunk converted with one launch per distinct rate in it -- a call whose
    bodies fit one chunk is one upload and one launch per rate.  The host never holds more than a chunk; nothing is read back."""
    if not torch.cuda.is_available():
        raise M3THipError("m3t.audio needs the GPU: the M3T path has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    items = list(items)
    names = [str(it) if isinstance(it, (str, bytes, os.PathLike)) else "clip %d" % i for i, it in enumerate(items)]
    infos = [_wav.probe_wave(it) if isinstance(it, (str, bytes, os.PathLike)) else it[1] for it in items]
    sizes = np.array([int(w.frames) * w.frame_bytes for w in infos], np.int64)
    padded = (sizes + _ALIGN - 1) // _ALIGN * _ALIGN
    out_offsets, lengths, total, _ = plan_convert(infos, np.zeros(len(items), np.int64), int(sizes.max(initial=0)), names=names)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    cap = max(int(chunk_bytes), _ALIGN)
    stage, copied = None, None
    lo = 0
    with torch.cuda.device(dev):
        while lo < len(items):
            hi, fill = lo + 1, int(padded[lo])
            while hi < len(items) and fill + padded[hi] <= cap:
                fill += int(padded[hi])
                hi += 1
            if stage is None or stage.numel() < fill:
                stage = torch.empty(max(fill, min(cap, int(padded.sum()))), dtype=torch.uint8, pin_memory=True)
            elif copied is not None:
                copied.synchronize()                                  # the stage is free again once the previous chunk's copy has ended
            host, offs, pos = stage.numpy(), [], 0
            for i in range(lo, hi):
                it = items[i]
                if isinstance(it, (str, bytes, os.PathLike)):
                    body, info = _wav.read_wave(it)
                    if info != infos[i]:
                        raise ValueError("%s: its header read %r when the call was planned and reads %r now" % (names[i], tuple(infos[i]), tuple(info)))
                else:
                    body = np.frombuffer(it[0], np.uint8) if isinstance(it[0], (bytes, bytearray, memoryview)) else np.asarray(it[0], np.uint8).reshape(-1)
                    if body.shape[0] < sizes[i]:
                        raise ValueError("%s: %d bytes given, its WaveInfo asks for %d" % (names[i], body.shape[0], sizes[i]))
                host[pos:pos + sizes[i]] = body[:sizes[i]]
                offs.append(pos)
                pos += int(padded[i])
            raw = torch.empty(fill, dtype=torch.uint8, device=dev)
            raw.copy_(stage[:fill], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
            _, _, _, groups = plan_convert(infos[lo:hi], offs, fill, out_offsets[lo:hi], names[lo:hi])
            convert_planned(raw, groups, out)
            lo = hi
    return out, out_offsets, lengths


def load_wave(path):
    """`librosa.load(path, sr=16000)[0]` (process/extract_melspec.py:13) -> float32 device tensor [converted_length]"""
    return decode_waves([path])[0]
