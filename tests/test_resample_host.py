"""The host half of the wave conversion (m3t.audio.converted_length / resample_filter / register_starts / plan_convert, the `convert` option of
m3t.audioset) against tests/resample_ref.py, and the held check of that oracle against the real resampy / librosa where they exist.
No GPU: nothing here initialises a device."""
import math
import random

import numpy as np
import pytest

import resample_ref as R
from m3t import audio, audioset, wav

RATES = [8000, 11025, 22050, 32000, 44100, 48000, 96000]


# ---------------------------------------------------------------------------------------------- lengths
@pytest.mark.parametrize("rate", RATES + [16000])
def test_converted_length_is_the_oracle_s_for_1_to_2000_frames(rate):
    got = [audio.converted_length(n, rate) for n in range(1, 2001)]
    assert got == [R.lengths(n, rate)[1] for n in range(1, 2001)]
    assert [audio.resampled_length(n, rate) for n in range(1, 2001)] == [R.lengths(n, rate)[0] for n in range(1, 2001)]
    for n in (1, 3, 441, 882, 1323, 1999, 2000):                                 # the output the oracle really returns
        assert R.resample(np.zeros(n, np.float32), rate).shape == (audio.converted_length(n, rate),)
    if rate == 16000:
        assert got == list(range(1, 2001))


def test_the_float64_rule_at_the_exact_multiples():
    """The lengths are the float64 expressions as written, not integer arithmetic.  Where n * 16000 is a multiple of the rate (the multiples
    of 441 at 44.1 / 22.05 / 11.025 kHz, of 3 at 48 kHz) a rounding of the product would show as n_res one short or n_out one long.  What
    this finds: for the seven rates and 1 .. 2000 frames the product lands on the integer every time, so both rules give the same lengths
    there and n_res == n_out exactly at the multiples; at a rate whose ratio is not so kind (16000 / 12345) the float64 rule is the one
    that is followed, whatever integer arithmetic says."""
    for rate in RATES:
        for n in range(1, 2001):
            n_res, n_out = audio.resampled_length(n, rate), audio.converted_length(n, rate)
            assert (n_res, n_out) == (n * 16000 // rate, -(-n * 16000 // rate)), (rate, n)
            assert (n_res == n_out) == ((n * 16000) % rate == 0)
    for n in range(1, 20001):
        p = n * (16000.0 / 12345)
        assert (audio.resampled_length(n, 12345), audio.converted_length(n, 12345)) == (int(p), int(math.ceil(p)))


# ---------------------------------------------------------------------------------------------- the table and the registers
@pytest.mark.parametrize("rate", RATES)
def test_the_filter_table_is_the_oracle_s(rate):
    got = audio.resample_filter(rate)
    win, delta = R.filter_table(rate)
    assert got.dtype == np.float64 and got.shape == (32769, 2) and got.flags.c_contiguous
    assert got[:, 0].tobytes() == win.tobytes() and got[:, 1].tobytes() == delta.tobytes()
    assert got[-1, 1] == 0.0 and got[0, 0] == R.ROLLOFF * min(1.0, 16000.0 / rate)


@pytest.mark.parametrize("rate", RATES + [12345])
def test_the_per_tile_register_starts_equal_the_plain_loop_s_bit_for_bit(rate):
    n_out = 5 * audio.TILE + 7
    starts = audio.register_starts(rate, n_out)
    loop = R.registers(6 * audio.TILE, rate, "loop")
    assert starts.dtype == np.float64 and starts.shape == (6 * audio.TILE // audio.SEG,)
    assert starts.tobytes() == loop[::audio.SEG].tobytes()
    assert R.registers(6 * audio.TILE, rate, "accumulated").tobytes() == loop.tobytes()
    # what a lane does: carry on from its wave's start with the same additions
    inc = rate / 16000.0
    for s in (0, 1, len(starts) - 1):
        r = starts[s]
        for l in range(audio.SEG):
            assert r == loop[s * audio.SEG + l]
            r = r + inc


def test_the_accumulated_register_is_not_the_exact_one_at_44100():
    """2 947 frames at 44.1 kHz: the register crosses an integer every 160 outputs, and which side an output lands on is decided by the
    accumulated rounding -- an exact-rational register gives other samples there.  At 48 kHz (increment 3.0) the two are the same."""
    x = R.to_mono(R.decode(R.body(R.samples(R.noise(2947, 1, 0), "f32"), "f32"), 1, "f32"))
    acc, exact = R.resample(x, 44100), R.resample(x, 44100, register="exact")
    d = np.abs(acc - exact)
    print("44.1 kHz: accumulated vs exact register, max |diff| = %.3e at outputs %s" % (d.max(), np.flatnonzero(d > 1e-6)[:8].tolist()))
    assert acc.shape == (1070,) and 1e-4 < d.max() < 1e-3
    assert all(t % 160 == 0 for t in np.flatnonzero(d > 1e-6))
    x48 = x[:1200]
    assert R.resample(x48, 48000).tobytes() == R.resample(x48, 48000, register="exact").tobytes()


# ---------------------------------------------------------------------------------------------- the launch plan
def test_plan_convert_builds_the_table_of_the_header():
    infos = [wav.WaveInfo(44100, 2, wav.KIND_I16, 2947, 44), wav.WaveInfo(16000, 1, wav.KIND_I16, 600, 44),
             wav.WaveInfo(44100, 3, wav.KIND_I24, 193, 44), wav.WaveInfo(48000, 1, wav.KIND_F32, 3001, 44)]
    offs = [0, 11792, 12992, 14736]
    out_offsets, lengths, total, groups = audio.plan_convert(infos, offs, 14736 + 12004)
    assert lengths.tolist() == [1070, 600, 71, 1001] and out_offsets.tolist() == [0, 1070, 1670, 1741] and total == 2742
    assert list(groups) == [16000, 44100, 48000]
    idx, table, tiles = groups[44100]
    assert idx.tolist() == [0, 2] and tiles == 5 + 1
    assert table.tolist() == [[0, 2947, 2, wav.KIND_I16, 0, 1069, 1070, 0], [12992, 193, 3, wav.KIND_I24, 1670, 70, 71, 5]]
    assert groups[16000][1].tolist() == [[11792, 600, 1, wav.KIND_I16, 1070, 600, 600, 0]] and groups[16000][2] == 3
    assert groups[48000][1].tolist() == [[14736, 3001, 1, wav.KIND_F32, 1741, 1000, 1001, 0]] and groups[48000][2] == 4
    ok = wav.WaveInfo(44100, 2, wav.KIND_I16, 10, 44)
    for bad, why in [((ok._replace(frames=0), 0, 100), "an empty clip"), ((ok._replace(channels=9), 0, 1000), "9 channels"),
                     ((ok._replace(kind=5), 0, 1000), "kind 5"), ((ok._replace(rate=0), 0, 1000), "sampled at 0 Hz"),
                     ((ok._replace(rate=768000), 0, 1000), "sampled at 768000 Hz"), ((ok, 1, 1000), "alignment"),
                     ((ok, 0, 39), r"bytes 0 \.\. 40 lie outside the buffer's 39"), ((ok, -2, 1000), "outside the buffer"),
                     ((ok._replace(kind=wav.KIND_F32, channels=1), 6, 1000), "alignment")]:
        with pytest.raises(ValueError, match=why):
            audio.plan_convert([bad[0]], [bad[1]], bad[2])
    audio.plan_convert([ok._replace(kind=wav.KIND_I24)], [7], 1000)              # 24-bit bodies need no alignment
    with pytest.raises(ValueError, match="no clips"):
        audio.plan_convert([], [], 0)


# ---------------------------------------------------------------------------------------------- the AudioSet plan
def test_plan_epoch_with_convert_draws_from_the_converted_lengths(tmp_path):
    root, _ = R.write_audioset_tree(tmp_path / "mixed")
    with pytest.raises(wav.Unsupported, match=r"a44\.wav: 2 channels: only mono is taken"):
        audioset.scan_audioset(root, "train").lengths()                          # without the option: refused as before
    scan = audioset.scan_audioset(root, "train", convert=True)
    want = [R.lengths(frames, rate)[1] for _, rate, _, _, frames, _ in R.MIXED]
    assert scan.convert and scan.lengths().tolist() == want == [1070, 1001, 2133, 1089, 9000]
    assert [int(np.flatnonzero(row)[0]) for row in scan.labels] == [3, 526, 0, 7, 41]
    order = [4, 0, 3, 1, 2]
    feed = audioset.AudioSetFeed(scan, 4, 2, "train", sampler=order)
    random.seed(11)
    plans = feed.plan_epoch(0)
    random.seed(11)
    draws = [audio.draw_audioset(want[i], 4, True) for i in order]
    assert [p.items for p in plans] == [[4, 0], [3, 1], [2]] and [d for p in plans for d in p.aug] == draws
    assert any(d["nsamples"] > want[i] for d, i in zip(draws, order))            # a converted clip shorter than its crop: the wrap rule's tot
    assert feed.store is None                                                    # nothing touched a device
    with pytest.raises(ValueError, match="scanned with convert=True"):
        audioset.AudioSetFeed(scan, 4, 2, "train", convert=False)
    # an all-16 kHz folder plans the same epoch with and without the option
    root16, _ = R.write_audioset_tree(tmp_path / "all16", R.ALL16)
    a, b = audioset.scan_audioset(root16, "train"), audioset.scan_audioset(root16, "train", convert=True)
    assert a.lengths().tolist() == b.lengths().tolist() == [3000, 2133, 9000] and not a.convert
    random.seed(5)
    pa = audioset.AudioSetFeed(a, 4, 2, "train", sampler=[2, 0, 1]).plan_epoch(0)
    random.seed(5)
    assert pa == audioset.AudioSetFeed(b, 4, 2, "train", sampler=[2, 0, 1]).plan_epoch(0)


def test_the_driver_s_convert_audio_flag_reaches_the_scan(tmp_path):
    import importlib.util
    import os
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m3f.pytorch_amd")
    spec = importlib.util.spec_from_file_location("pretrain_audioset", os.path.join(pkg, "pretrain_audioset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    root, _ = R.write_audioset_tree(tmp_path / "mixed")
    plain = mod.make_parser().parse_args(["--dataset_path", root, "--window", "4", "--batch_size", "2"])
    assert not hasattr(plain, "convert_audio")                                   # the reference's namespace, unless the flag is given
    with pytest.raises(wav.Unsupported, match=r"a44\.wav"):
        audioset.feed_from_hparams(plain, "train")
    given = mod.make_parser().parse_args(["--dataset_path", root, "--window", "4", "--batch_size", "2", "--convert_audio"])
    feed = audioset.feed_from_hparams(given, "train")
    assert given.convert_audio is True and feed.convert and feed.scan.convert and feed.lengths.tolist() == [1070, 1001, 2133, 1089, 9000]


def test_an_empty_clip_is_refused_by_name_with_convert(tmp_path):
    root, _ = R.write_audioset_tree(tmp_path / "t", R.ALL16)
    p = tmp_path / "t" / "balanced_train_segments" / "q.wav"
    p.write_bytes(R.wav_bytes(b"\1", 44100, 2, "i16"))
    with pytest.raises(ValueError, match=r"q\.wav: an empty clip"):
        audioset.scan_audioset(root, "train", convert=True).lengths()


def test_the_mel_track_tasks_follow_the_reference_s_script(tmp_path):
    from m3t import melspec
    (tmp_path / "splits").mkdir()
    (tmp_path / "splits" / "frames_fps.csv").write_text("v1_left,100,30.0\nv1_right,100,30.0\nslow,50,12.5\nv2,80,25\nedge,10,15\n")
    tasks = melspec.tasks_from_csv("SRC", "DST", str(tmp_path / "splits"))
    j = lambda *a: "/".join(a)
    assert [(f, s.replace("\\", "/"), d.replace("\\", "/")) for f, s, d in tasks] == [
        (30.0, j("SRC", "v1.wav"), j("DST", "v1_left.npy")), (30.0, j("SRC", "v1.wav"), j("DST", "v1_right.npy")),
        (25.0, j("SRC", "v2.wav"), j("DST", "v2.npy")), (15.0, j("SRC", "edge.wav"), j("DST", "edge.npy"))]


# ---------------------------------------------------------------------------------------------- held: the real libraries
def test_the_oracle_against_the_real_resampy_and_librosa(tmp_path):
    """The check nobody on this project could run.  resampy's 'kaiser_best' table must be the oracle's; resampy 0.2.x's output must be the
    float32-accumulate restatement's bit for bit (later resampy changed the register rule: there only the table is compared); a librosa
    before 0.10 (kaiser_best by default) must load a 44.1 kHz stereo 16-bit file to the same samples.  Skipped where they are absent."""
    resampy = pytest.importorskip("resampy")
    half, precision, rolloff = resampy.filters.get_filter("kaiser_best")
    win, _ = R.filter_table(8000)
    assert precision == 512 and abs(rolloff - R.ROLLOFF) < 1e-15 and np.abs(np.asarray(half) - win).max() < 1e-12
    x = R.to_mono(R.decode(R.body(R.samples(R.noise(2947, 2, 0), "i16"), "i16"), 2, "i16"))
    if tuple(int(v) for v in resampy.__version__.split(".")[:2]) <= (0, 2):
        got = resampy.resample(x, 44100, 16000, filter="kaiser_best")
        want = R.resample(x, 44100, np.float32)
        assert got.dtype == np.float32 and got.tobytes() == want[:got.shape[0]].tobytes()
        librosa = pytest.importorskip("librosa")
        if tuple(int(v) for v in librosa.__version__.split(".")[:2]) < (0, 10):
            path = str(tmp_path / "s.wav")
            R.write_wav(path, R.noise(2947, 2, 0), 44100, "i16")
            y, sr = librosa.load(path, sr=16000)
            assert sr == 16000 and y.tobytes() == R.resample(x, 44100, np.float32).tobytes()
