"""The wave conversion on the GPU (csrc/resample.hip through m3t.audio.decode_waves / load_wave, the `convert` option of m3t.audioset, and
m3t.melspec) against the float64 oracle of tests/resample_ref.py.

The bar (the project's standing bound for fp32 operators): max |device - oracle| <= 4 x the max abs error of the float32-accumulate
restatement (resampy's own arithmetic: float64 weights, every partial sum stored to float32) on the same clip.  Where that yardstick is 0
-- a clip too short to reach the filter, a 16 kHz clip -- the device output is compared for equality.  Inputs are 0.25-sigma noise: the
rule's DC gain is not 1 (the truncated index step), so no ideal sine is used.  Same kernels on the same bytes are compared bit for bit.

Beyond the bar: the kernel is written in resampy's own arithmetic (float64 weights and products, every partial sum rounded to float32, left
wing then right wing in tap order, every operation rounded on its own), which is IEEE arithmetic on both sides -- so the device output must
BE the float32-accumulate restatement, bit for bit, and `held` asserts that too."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_ingest_ref as A
import resample_ref as R

pytestmark = pytest.mark.gpu
BAR = 4.0
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m3f.pytorch_amd")
KIND_ID = {k: i for i, k in enumerate(R.KINDS)}


@functools.lru_cache(None)
def clip(frames, rate, channels=1, kind="f32", seed=0):
    """-> (body bytes, WaveInfo, oracle float64 [n_out], the float32-accumulate restatement [n_out]) of a noise clip; computed once per shape"""
    from m3t import wav
    data = R.body(R.samples(R.noise(frames, channels, seed + frames), kind), kind)
    return data, wav.WaveInfo(rate, channels, KIND_ID[kind], frames, 0), R.load(data, rate, channels, kind), R.load(data, rate, channels, kind, np.float32)


def held(got, want, yard32, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    yard = float(np.abs(yard32.astype(np.float64) - want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: |device - oracle| = %.3e, yardstick %.3e, ratio %s, peak %.2f"
          % (what, err, yard, "%.2f" % (err / yard) if yard else "-", np.abs(want).max()))
    if yard == 0.0:
        assert got.tobytes() == want.astype(np.float32).tobytes(), what
    else:
        assert err <= BAR * yard, (what, err, yard)
    assert got.tobytes() == yard32.tobytes(), what + ": not resampy's arithmetic bit for bit"
    return got


def convert_one(frames, rate, channels=1, kind="f32", seed=0):
    from m3t import audio
    data, info, want, yard = clip(frames, rate, channels, kind, seed)
    out, offs, lens = audio.decode_waves([(data, info)])
    assert offs.tolist() == [0] and lens.tolist() == [want.shape[0]] and out.dtype == torch.float32 and out.is_cuda
    return held(out, want, yard, "%d Hz x %d %s ch%d" % (rate, frames, kind, channels))


def frames_for(n_out, rate):
    """the smallest frame count that converts to n_out outputs"""
    return next(n for n in range(1, 10 * n_out * max(1, rate // 16000 + 1)) if R.lengths(n, rate)[1] == n_out)


# ---------------------------------------------------------------------------------------------- one clip against the oracle
@pytest.mark.parametrize("rate,frames", [(44100, 2947), (48000, 3000), (48000, 3001), (22050, 1500), (8000, 700), (11025, 900)])
def test_a_clip_of_every_rate_meets_the_bar(rate, frames):
    got = convert_one(frames, rate)
    n_res, n_out = R.lengths(frames, rate)
    assert got.shape == (n_out,) and (n_res == n_out or got[-1] == 0.0)
    if (rate, frames) == (44100, 2947):
        # the side rule: with an exact register the oracle itself moves by 3e-4 at every 160th output -- far outside the bar
        data, _, want, yard = clip(frames, rate)
        other = R.load(data, rate, 1, "f32", register="exact")
        assert got.shape == (1070,) and np.abs(other - want).max() > 100 * BAR * np.abs(yard - want).max()


@pytest.mark.parametrize("rate", [44100, 8000])
@pytest.mark.parametrize("frames", [1, 2, 5, 193])
def test_clips_shorter_than_a_filter_wing(rate, frames):
    got = convert_one(frames, rate)
    if rate == 44100 and frames <= 2:
        assert got.tolist() == [0.0]                                             # n_res == 0: only the padded sample


@pytest.mark.parametrize("rate", [44100, 48000, 32000])
def test_output_counts_around_one_tile(rate):
    from m3t import audio
    for n_out in (audio.TILE - 1, audio.TILE, audio.TILE + 1):
        assert convert_one(frames_for(n_out, rate), rate).shape == (n_out,)


def test_output_counts_around_one_tile_when_upsampling():
    """8 kHz doubles the count: 254, 256 and 258 outputs (one tile less two, one tile, one tile and two)"""
    for frames in (127, 128, 129):
        assert convert_one(frames, 8000).shape == (2 * frames,)


def test_every_kind_and_channel_count_in_one_ragged_batch():
    """u8, i16, i24, i32, f32 x 1, 2, 3 channels at 44.1 kHz in ONE call; 24-bit x 3 channels puts frames at odd addresses"""
    from m3t import audio
    shapes = [(600 + 7 * c + k, 44100, c, kind, 3) for k, kind in enumerate(R.KINDS) for c in (1, 2, 3)]
    clips = [clip(*s) for s in shapes]
    out, offs, lens = audio.decode_waves([(c[0], c[1]) for c in clips])
    assert lens.tolist() == [c[2].shape[0] for c in clips] and offs.tolist() == np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    assert out.numel() == int(lens.sum())
    for s, c, o, n in zip(shapes, clips, offs, lens):
        held(out[o:o + n], c[2], c[3], "batch %s ch%d" % (s[3], s[2]))


def test_a_16_khz_clip_is_decoded_and_down_mixed_only():
    for kind, channels in (("i16", 1), ("i24", 3), ("u8", 2), ("i32", 1), ("f32", 2)):
        data, info, want, yard = clip(777, 16000, channels, kind)
        assert yard.tobytes() == want.astype(np.float32).tobytes()
        got = convert_one(777, 16000, channels, kind)
        assert got.tobytes() == R.to_mono(R.decode(data, channels, kind)).tobytes()


# ---------------------------------------------------------------------------------------------- batch forms
def test_a_mixed_batch_equals_each_clip_alone_and_a_rerun_bit_for_bit(tmp_path):
    from m3t import audio, wav
    shapes = [(2947, 44100, 2, "i16"), (3001, 48000, 1, "f32"), (700, 8000, 1, "u8"), (5, 44100, 3, "i24"), (2133, 16000, 1, "i16"),
              (1500, 22050, 2, "i32"), (193, 44100, 1, "f32"), (900, 11025, 2, "i16"), (1, 48000, 1, "i16")]
    clips = [clip(*s) for s in shapes]
    items = [(c[0], c[1]) for c in clips]
    out, offs, lens = audio.decode_waves(items)
    again, offs2, lens2 = audio.decode_waves(items)
    assert torch.equal(out, again) and offs.tolist() == offs2.tolist() and lens.tolist() == lens2.tolist()
    for it, c, o, n in zip(items, clips, offs, lens):
        alone = audio.decode_waves([it])[0]
        assert torch.equal(out[o:o + n], alone), c[1]
        held(alone, c[2], c[3], "alone %r" % (tuple(c[1]),))
    # a stage of 4 KB: several chunks, a clip longer than the stage on its own -- the same bits
    small, offs3, lens3 = audio.decode_waves(items, chunk_bytes=4096)
    assert torch.equal(out, small) and offs3.tolist() == offs.tolist()
    # files on disk (header and body read by m3t.wav) against the bytes handed over
    paths = []
    for k, (frames, rate, channels, kind) in enumerate(shapes):
        p = str(tmp_path / ("c%d.wav" % k))
        with open(p, "wb") as f:
            f.write(R.wav_bytes(clips[k][0], rate, channels, kind, extensible=bool(k & 1)))
        paths.append(p)
    from_files, _, lens4 = audio.decode_waves(paths)
    assert torch.equal(out, from_files) and lens4.tolist() == lens.tolist()
    assert torch.equal(audio.load_wave(paths[0]), out[:lens[0]])
    assert [audio.converted_length(wav.probe_wave(p).frames, wav.probe_wave(p).rate) for p in paths] == lens.tolist()


def test_the_entry_point_refuses_bad_arguments_and_skips_a_row_that_leaves_the_buffers():
    from m3t import _lib, audio
    lib = _lib.load()
    data, info, want, yard = clip(900, 44100)
    raw = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    filt, starts = audio._filter_on(raw.device, 44100), audio._starts_on(raw.device, 44100, want.shape[0])
    st = torch.cuda.current_stream().cuda_stream
    n_out = want.shape[0]
    n_res = R.lengths(900, 44100)[0]

    def call(rows, out, n_bytes=raw.numel(), rate=44100, tiles=None, table=filt.data_ptr(), n_starts=None):
        tab = torch.tensor(rows, dtype=torch.int64).reshape(-1).cuda()
        tiles = sum(-(-r[6] // audio.TILE) for r in rows) if tiles is None else tiles
        rc = lib.m3t_wave_convert(raw.data_ptr(), n_bytes, tab.data_ptr(), len(rows), tiles, rate, table, starts.data_ptr(),
                                  starts.numel() if n_starts is None else n_starts, out.data_ptr(), out.numel(), st)
        torch.cuda.synchronize()
        return rc

    good = [0, 900, 1, 4, 0, n_res, n_out, 0]
    out = torch.full((n_out + 8,), 7.0, device="cuda")
    assert call([good], out) == 0
    held(out[:n_out], want, yard, "raw entry point")
    assert bool((out[n_out:] == 7.0).all())
    for bad in ([0, 901, 1, 4, 0, n_res, n_out, 0],          # a frame past the bytes
                [2, 899, 1, 4, 0, n_res, n_out, 0],          # float32 off its alignment
                [0, 900, 9, 4, 0, n_res, n_out, 0],          # channels
                [0, 900, 1, 5, 0, n_res, n_out, 0],          # kind
                [0, 900, 1, 4, 16, n_res, n_out, 0],         # outputs past the buffer
                [0, 900, 1, 4, 0, n_out + 1, n_out, 0],      # n_res > n_out
                [-4, 900, 1, 4, 0, n_res, n_out, 0]):
        out = torch.full((n_out + 8,), 7.0, device="cuda")
        assert call([bad], out) == 0 and bool((out == 7.0).all()), bad
    out = torch.full((n_out + 8,), 7.0, device="cuda")
    assert call([good], out, n_starts=1) == 0 and bool((out == 7.0).all())      # too few register starts: nothing is written
    assert call([good], out, tiles=0) == 0 and bool((out == 7.0).all())
    assert call([good], out, rate=0) == _lib.M3T_EINVAL
    assert call([good], out, rate=1000000) == _lib.M3T_EINVAL                    # the tile's span would not fit the LDS
    assert call([good], out, table=None) == _lib.M3T_EINVAL
    assert call([good], out, n_bytes=0) == _lib.M3T_EINVAL


# ---------------------------------------------------------------------------------------------- the AudioSet store and feed
def test_a_16k_16_bit_mono_clip_in_a_converting_store_is_int16_over_32768(tmp_path):
    from m3t import audioset
    root, bodies = R.write_audioset_tree(tmp_path / "t", R.ALL16)
    scan = audioset.scan_audioset(root, "train", convert=True)
    store = audioset.WaveStore(scan.files, scan.labels, scan.lengths(), convert=True)
    assert store.wave.dtype == torch.float32 and store.wave.dim() == 1 and store.lengths.tolist() == [3000, 2133, 9000]
    assert store.nbytes == 4 * 14133 + 3 * 527
    got = store.wave.cpu().numpy()
    for (name, *_), o, n in zip(R.ALL16, store.offsets, store.lengths):
        pcm = np.frombuffer(bodies[name][0], "<i2")
        assert got[o:o + n].tobytes() == (pcm.astype(np.float32) / np.float32(32768)).tobytes()


def test_an_all_16k_folder_feeds_the_same_bits_with_and_without_convert(tmp_path):
    from m3t import audioset
    root, _ = R.write_audioset_tree(tmp_path / "t", R.ALL16)
    batches = []
    for convert in (False, True):
        feed = audioset.AudioSetFeed(audioset.scan_audioset(root, "train", convert=convert), 4, 2, "train", sampler=[2, 0, 1])
        random.seed(21)
        batches.append(list(feed))
        assert feed.store.wave.dtype == (torch.float32 if convert else torch.int16)
    assert len(batches[0]) == len(batches[1]) == 2
    for a, b in zip(*batches):
        assert torch.equal(a["audio"], b["audio"]) and torch.equal(a["label"], b["label"])
        assert tuple(a["audio"].shape)[1:] == (4, 200)


def test_a_mixed_folder_feeds_what_ingest_makes_of_the_converted_clips(tmp_path):
    from m3t import audio, audioset
    root, bodies = R.write_audioset_tree(tmp_path / "t")
    with pytest.raises(ValueError):                                              # without the option: refused, as before
        audioset.AudioSetFeed(audioset.scan_audioset(root, "train"), 4, 2, "train")
    scan = audioset.scan_audioset(root, "train", convert=True)
    flat, offs, lens = audio.decode_waves(scan.files)
    assert lens.tolist() == scan.lengths().tolist()
    clips = [flat[o:o + n].cpu().numpy() for o, n in zip(offs, lens)]
    for (name, rate, channels, kind, frames, _), c in zip(R.MIXED, clips):      # and the clips are the oracle's
        held(torch.from_numpy(c), R.load(bodies[name][0], rate, channels, kind), R.load(bodies[name][0], rate, channels, kind, np.float32),
             "mixed/" + name)
    feed = audioset.AudioSetFeed(scan, 4, 2, "train", sampler=[4, 0, 3, 1, 2])
    random.seed(31)
    plans = feed.plan_epoch(0)
    random.seed(31)
    got = list(feed)
    assert len(got) == len(plans) == 3
    for plan, batch in zip(plans, got):
        want = audio.ingest([clips[i] for i in plan.items], plan.aug, 4)
        assert torch.equal(batch["audio"], want), plan
        assert batch["label"].cpu().numpy().tobytes() == scan.labels[plan.items].astype(np.float32).tobytes()
    assert torch.equal(feed.store.wave, flat) and feed.store.offsets.tolist() == offs.tolist()


# ---------------------------------------------------------------------------------------------- the mel tracks
def test_melspec_on_a_three_video_tree(tmp_path):
    """v1_left / v1_right share v1.wav (44.1 kHz stereo), `slow` is under 15 fps, v2's track exists already, `gone` has no wav: the files
    the reference's script would leave, the rows of melspec_db(load_wave(.), fps) bit for bit, and within 2e-3 dB of the float64 resample
    followed by the float64 log-Mel (white noise: every band far above the dB floor)."""
    from m3t import audio
    src, dst, splits = tmp_path / "wav", tmp_path / "mel", tmp_path / "splits"
    for d in (src, dst, splits):
        d.mkdir()
    (splits / "frames_fps.csv").write_text("v1_left,90,30.0\nv1_right,90,30.0\nslow,40,12.5\nv2,70,25.0\ngone,10,30.0\n")
    y1 = R.noise(44100 * 3 // 2, 2, 77)
    s1 = R.write_wav(src / "v1.wav", y1, 44100, "i16")
    R.write_wav(src / "slow.wav", R.noise(4000, 1, 78), 16000, "i16")
    R.write_wav(src / "v2.wav", R.noise(4000, 1, 79), 48000, "f32")
    kept = np.arange(80, dtype=np.float32).reshape(2, 40)
    np.save(str(dst / "v2.npy"), kept)
    res = subprocess.run([sys.executable, "-m", "m3t.melspec", str(src), str(dst), "--splits_dir", str(splits)], cwd=PKG,
                         env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(str(dst))) == ["v1_left.npy", "v1_right.npy", "v2.npy"]
    assert "Exception on %s" % (src / "gone.wav") in res.stdout and "result: -1" in res.stdout and res.stdout.count("result: 0") == 2
    assert np.load(str(dst / "v2.npy")).tobytes() == kept.tobytes()
    left, right = np.load(str(dst / "v1_left.npy")), np.load(str(dst / "v1_right.npy"))
    wave = audio.load_wave(str(src / "v1.wav"))
    want = audio.melspec_db(wave, 30.0).cpu().numpy()
    assert left.dtype == np.float32 and left.shape == (1 + wave.numel() // audio.hop_length(30.0), 40)
    assert left.tobytes() == right.tobytes() == want.tobytes()
    y64 = R.load(R.body(s1, "i16"), 44100, 2, "i16")
    assert y64.shape == (wave.numel(),) == (24000,)
    ref = A.mel_db(y64, A.draw(30.0, 0, nsamples=y64.shape[0]))
    assert ref.min() > ref.max() - 60.0                                          # far from the floor at max - 80
    assert A.max_err(left, ref, "mel track") < A.TOL_DB
