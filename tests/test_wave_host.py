"""The wider host reader (m3t/wav.py: probe_wave, read_wave, parse_wave, to_float, to_mono): every accepted kind and channel count written by
hand with `struct` (and by Python's `wave` module where it can write the kind), the chunk rules of the 16-bit reader on the new path,
and every refusal by name.  The decode rule is checked against tests/resample_ref.py.  No GPU."""
import struct
import wave

import numpy as np
import pytest

import resample_ref as R
from m3t import wav

KIND_ID = {"u8": wav.KIND_U8, "i16": wav.KIND_I16, "i24": wav.KIND_I24, "i32": wav.KIND_I32, "f32": wav.KIND_F32}


def put(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_kind_and_channel_count_reads_back_its_bytes(tmp_path, kind, channels, extensible):
    frames, rate = 37, 44100
    s = R.samples(R.noise(frames, channels, 5 + channels), kind)
    data = R.body(s, kind)
    path = put(tmp_path, "c.wav", R.wav_bytes(data, rate, channels, kind, extensible=extensible))
    raw, info = wav.read_wave(path)
    assert info == wav.probe_wave(path) == wav.WaveInfo(rate, channels, KIND_ID[kind], frames, 68 if extensible else 44)
    assert raw.dtype == np.uint8 and raw.tobytes() == data and info.frame_bytes == channels * R.KIND_BYTES[kind]
    raw2, info2 = wav.parse_wave(open(path, "rb").read(), "mem")
    assert info2 == info and raw2.tobytes() == data
    y = wav.to_float(raw, info)
    want = R.decode(data, channels, kind)
    assert y.dtype == np.float32 and y.shape == (frames, channels) and y.tobytes() == want.tobytes()
    assert wav.to_mono(y).tobytes() == R.to_mono(want).tobytes()


def test_the_decode_rule_at_the_ends_of_every_range():
    cases = [("u8", np.array([[0], [128], [255]], np.uint8), [-1.0, 0.0, 127 / 128]),
             ("i16", np.array([[-32768], [0], [32767]], np.int16), [-1.0, 0.0, 32767 / 32768]),
             ("i24", np.array([[-8388608], [-1], [8388607]], np.int32), [-1.0, -1 / 8388608, 8388607 / 8388608]),
             ("i32", np.array([[-2147483648], [2147483647], [16777217]], np.int32), [-1.0, 1.0, float(np.float32(16777217 / 2147483648))])]
    for kind, s, want in cases:
        data = R.body(s, kind)
        raw, info = wav.parse_wave(R.wav_bytes(data, 8000, 1, kind))
        got = wav.to_float(raw, info)[:, 0]
        assert got.tolist() == [float(np.float32(v)) for v in want], kind
        assert got.tobytes() == R.decode(data, 1, kind)[:, 0].tobytes()
    # three channels: summed in channel order in float32, then divided (not pairwise, not float64)
    y = np.array([[1e8, 1.0, -1e8], [0.1, 0.2, 0.3]], np.float32)
    want = [(np.float32(np.float32(y[r, 0] + y[r, 1]) + y[r, 2]) / np.float32(3)) for r in range(2)]
    assert wav.to_mono(y).tolist() == [float(v) for v in want] and wav.to_mono(y)[0] == 0.0


@pytest.mark.parametrize("width,kind", [(1, "u8"), (2, "i16"), (3, "i24"), (4, "i32")])
@pytest.mark.parametrize("channels", [1, 2])
def test_files_of_the_wave_module(tmp_path, width, kind, channels):
    s = R.samples(R.noise(50, channels, width), kind)
    path = str(tmp_path / "w.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(22050)
        w.writeframes(R.body(s, kind))
    raw, info = wav.read_wave(path)
    assert info == wav.WaveInfo(22050, channels, KIND_ID[kind], 50, 44) and raw.tobytes() == R.body(s, kind)


def test_the_chunk_rules_hold_on_the_wider_path(tmp_path):
    s = R.samples(R.noise(10, 2, 1), "i24")
    data = R.body(s, "i24")                                                      # 60 bytes
    extra = b"LIST" + struct.pack("<I", 5) + b"INFOx\0" + b"fact" + struct.pack("<I", 4) + struct.pack("<I", 10)
    whole = R.wav_bytes(data, 48000, 2, "i24", extra=extra)
    raw, info = wav.parse_wave(whole)
    assert info == wav.WaveInfo(48000, 2, wav.KIND_I24, 10, 44 + len(extra)) and raw.tobytes() == data
    for size in (0, 0xFFFFFFFF):                                                 # a pipe writer's open sizes: to the end of the file
        raw, info = wav.parse_wave(R.wav_bytes(data, 48000, 2, "i24", data_size=size))
        assert info.frames == 10 and raw.tobytes() == data
    # truncated: cut at the last whole frame (6 bytes a frame); the RIFF size field is not trusted
    cut = whole[:len(whole) - 8]
    raw, info = wav.parse_wave(cut)
    assert info.frames == 8 and raw.tobytes() == data[:48]
    path = put(tmp_path, "cut.wav", cut)
    assert wav.probe_wave(path) == wav.read_wave(path)[1] == info
    # an odd body takes its pad byte: a chunk after 'data' is not mistaken for samples
    odd = R.wav_bytes(R.body(R.samples(R.noise(3, 1, 2), "u8"), "u8"), 8000, 1, "u8") + b"LIST" + struct.pack("<I", 0)
    raw, info = wav.parse_wave(odd)
    assert info.frames == 3 and raw.shape == (3,)
    # no whole frame: the reader gives an empty body, the caller refuses the clip
    raw, info = wav.parse_wave(R.wav_bytes(b"\1\2", 8000, 1, "i32"))
    assert info.frames == 0 and raw.shape == (0,)


def test_refusals_by_name(tmp_path):
    data = bytes(64)

    def refused(blob, why, name="bad.wav"):
        with pytest.raises(wav.Unsupported, match=why) as e:
            wav.read_wave(put(tmp_path, name, blob))
        assert name in str(e.value)
        with pytest.raises(wav.Unsupported, match=why):
            wav.probe_wave(str(tmp_path / name))

    refused(R.wav_bytes(data, 16000, 1, "f32", bits=64), "64-bit IEEE float")
    refused(R.wav_bytes(data, 16000, 1, "f32", bits=64, extensible=True), "64-bit IEEE float")
    refused(R.wav_bytes(data, 8000, 1, "u8", tag=6), "format tag 0x0006")              # A-law
    refused(R.wav_bytes(data, 8000, 1, "u8", tag=7), "format tag 0x0007")              # mu-law
    refused(R.wav_bytes(data, 8000, 1, "u8", tag=2, bits=4), "format tag 0x0002")      # MS ADPCM
    refused(R.wav_bytes(data, 8000, 1, "u8", tag=0x11, bits=4), "format tag 0x0011")   # IMA ADPCM
    refused(R.wav_bytes(data, 8000, 1, "i16", bits=12), "12-bit PCM")
    refused(R.wav_bytes(data, 8000, 1, "i16", bits=64), "64-bit PCM")
    refused(R.wav_bytes(data, 8000, 0, "i16"), "0 channels")
    refused(R.wav_bytes(data, 8000, 9, "i16"), "9 channels")
    refused(R.wav_bytes(data, 0, 1, "i16"), "sample rate of 0")
    refused(R.wav_bytes(data, 8000, 1, "i24", extensible=True, valid_bits=20), "20 valid bits in a 24-bit container")
    ext = R.wav_bytes(data, 8000, 1, "i16", extensible=True)
    refused(ext[:44] + b"\xff" * 16 + ext[60:], "neither PCM nor IEEE float")
    refused(b"RF64" + R.wav_bytes(data, 8000, 1, "i16")[4:], "not a RIFF/WAVE file")
    refused(b"RIFX" + R.wav_bytes(data, 8000, 1, "i16")[4:], "not a RIFF/WAVE file")
    refused(b"RIFF" + struct.pack("<I", 4) + b"WAVE", "no 'fmt ' and no 'data' chunk")
    refused(b"RIFF" + struct.pack("<I", 76) + b"WAVE" + b"data" + struct.pack("<I", 64) + data, "no 'fmt ' chunk before 'data'")
    refused(R.wav_bytes(data, 8000, 1, "i16")[:36], "no 'data' chunk")
    with pytest.raises(OSError):
        wav.read_wave(str(tmp_path / "absent.wav"))


def test_the_sixteen_bit_reader_is_as_it_was(tmp_path):
    """what read_wave now takes, read_pcm16 still refuses, in its own words"""
    stereo = put(tmp_path, "s.wav", R.wav_bytes(bytes(8), 16000, 2, "i16"))
    with pytest.raises(wav.Unsupported, match=r"2 channels: only mono is taken \(no down-mix here\)"):
        wav.read_pcm16(stereo)
    f32 = put(tmp_path, "f.wav", R.wav_bytes(bytes(8), 16000, 1, "f32"))
    with pytest.raises(wav.Unsupported, match=r"IEEE float samples \(format tag 3\): only 16-bit PCM is taken"):
        wav.probe_pcm16(f32)
    mono = R.samples(R.noise(9, 1, 3), "i16")
    y, rate = wav.read_pcm16(put(tmp_path, "m.wav", R.wav_bytes(R.body(mono, "i16"), 44100, 1, "i16")))
    assert rate == 44100 and y.tobytes() == mono.tobytes()
