"""The host WAV reader (m3t/wav.py): files written by Python's `wave` module round-trip, hand-built byte strings cover the chunk rules
(a 'LIST' before 'data', an odd chunk with its pad byte, WAVE_FORMAT_EXTENSIBLE, the open 'data' sizes of a pipe writer, a truncated file),
and everything that is not 16-bit mono PCM is refused with the file named.  No GPU."""
import struct
import wave

import numpy as np
import pytest

from m3t import wav

PCM_GUID = bytes.fromhex("0100000000001000800000aa00389b71")
FLOAT_GUID = bytes.fromhex("0300000000001000800000aa00389b71")


def chunk(cid, body, size=None):
    """a chunk with its pad byte; `size` overrides the size field"""
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def fmt(tag=1, channels=1, rate=16000, bits=16, ext=None):
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if ext is not None:
        body += struct.pack("<HHI", 22, bits, 4) + ext
    return chunk(b"fmt ", body)


def riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def samples(n, seed=0):
    return np.random.RandomState(seed).randint(-32768, 32768, n).astype(np.int16)


def put(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("n,rate", [(1, 16000), (2133, 16000), (16001, 44100)])
def test_files_of_the_wave_module_round_trip(tmp_path, n, rate):
    y = samples(n, n)
    y[0] = -32768
    path = str(tmp_path / "clip.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(y.astype("<i2").tobytes())
    got, sr = wav.read_pcm16(path)
    assert sr == rate and got.dtype == np.int16 and got.flags.writeable and np.array_equal(got, y)
    assert wav.probe_pcm16(path) == (n, rate)


def test_other_chunks_are_skipped_and_odd_ones_carry_their_pad_byte(tmp_path):
    y = samples(101)
    data = chunk(b"data", y.tobytes())
    listed = chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 14) + b"Lavf58.29.100\0")
    odd = chunk(b"junk", b"abc")                                        # 3 bytes + the pad byte: without it 'data' is not found
    assert len(odd) == 12
    for name, blob in (("list", riff(fmt(), listed, data)), ("odd", riff(fmt(), odd, data)), ("both", riff(odd, fmt(), listed, odd, data)),
                       ("after", riff(fmt(), data, listed))):
        got, sr = wav.read_pcm16(put(tmp_path, name + ".wav", blob))
        assert sr == 16000 and np.array_equal(got, y), name
    # a 'data' chunk of an odd number of bytes: the last whole sample ends the clip
    got, _ = wav.read_pcm16(put(tmp_path, "oddData.wav", riff(fmt(), chunk(b"data", y.tobytes() + b"\x7f"), listed)))
    assert np.array_equal(got, y)


def test_extensible_with_the_pcm_sub_format(tmp_path):
    y = samples(64, 3)
    got, sr = wav.read_pcm16(put(tmp_path, "ext.wav", riff(fmt(tag=0xFFFE, ext=PCM_GUID), chunk(b"data", y.tobytes()))))
    assert sr == 16000 and np.array_equal(got, y)
    with pytest.raises(wav.Unsupported, match=r"extf\.wav.*sub-format"):
        wav.read_pcm16(put(tmp_path, "extf.wav", riff(fmt(tag=0xFFFE, ext=FLOAT_GUID[:2] + b"\1" + FLOAT_GUID[3:]), chunk(b"data", y.tobytes()))))
    with pytest.raises(wav.Unsupported, match=r"extfloat\.wav.*float"):
        wav.read_pcm16(put(tmp_path, "extfloat.wav", riff(fmt(tag=0xFFFE, ext=FLOAT_GUID), chunk(b"data", y.tobytes()))))


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF])
def test_an_open_data_size_means_to_the_end_of_the_file(tmp_path, size):
    y = samples(333, 5)
    blob = riff(fmt(), chunk(b"LIST", b"INFO"), chunk(b"data", y.tobytes(), size=size))
    blob = blob[:4] + struct.pack("<I", 0xFFFFFFFF) + blob[8:]             # (the pipe writer leaves the RIFF size open too)
    got, _ = wav.read_pcm16(put(tmp_path, "pipe.wav", blob))
    assert np.array_equal(got, y)
    assert wav.probe_pcm16(str(tmp_path / "pipe.wav")) == (333, 16000)


def test_truncated_data_is_cut_at_the_last_whole_sample(tmp_path):
    y = samples(500, 6)
    whole = riff(fmt(), chunk(b"data", y.tobytes()))
    got, _ = wav.read_pcm16(put(tmp_path, "cut.wav", whole[:-301]))       # 150 samples and one byte are missing
    assert np.array_equal(got, y[:349])
    assert wav.probe_pcm16(str(tmp_path / "cut.wav"))[0] == 349


def test_bytes_in_memory_parse_the_same(tmp_path):
    y = samples(77, 8)
    got, sr = wav.parse_pcm16(riff(fmt(rate=8000), chunk(b"data", y.tobytes())), "mem")
    assert sr == 8000 and np.array_equal(got, y)


@pytest.mark.parametrize("name,blob,why", [
    ("eight.wav", riff(fmt(bits=8), chunk(b"data", b"\x80" * 64)), "8-bit"),
    ("twentyfour.wav", riff(fmt(bits=24), chunk(b"data", b"\0" * 66)), "24-bit"),
    ("float.wav", riff(fmt(tag=3, bits=32), chunk(b"data", b"\0" * 64)), "float"),
    ("stereo.wav", riff(fmt(channels=2), chunk(b"data", b"\0" * 64)), "2 channels"),
    ("adpcm.wav", riff(fmt(tag=2, bits=4), chunk(b"data", b"\0" * 64)), "format tag 0x0002"),
    ("nofmt.wav", riff(chunk(b"data", b"\0" * 64), fmt()), "no 'fmt ' chunk before 'data'"),
    ("nodata.wav", riff(fmt(), chunk(b"LIST", b"INFO")), "no 'data' chunk"),
    ("ogg.wav", b"OggS" + b"\0" * 60, "not a RIFF/WAVE"),
    ("avi.wav", b"RIFF" + struct.pack("<I", 56) + b"AVI " + b"\0" * 52, "not a RIFF/WAVE"),
    ("short.wav", b"RIFF", "not a RIFF/WAVE"),
])
def test_everything_else_is_refused_with_the_file_named(tmp_path, name, blob, why):
    path = put(tmp_path, name, blob)
    with pytest.raises(wav.Unsupported) as e:
        wav.read_pcm16(path)
    assert path in str(e.value) and why in str(e.value), str(e.value)
    assert isinstance(e.value, ValueError)
    with pytest.raises(wav.Unsupported):
        wav.probe_pcm16(path)


def test_the_int16_sample_over_32768_is_what_the_device_applies():
    """librosa's float32 sample of a 16-bit file is int16 / 32768 (m3t/wav.py's text); every such quotient is exact in float32, so the
    int16 samples are all a clip has to bring"""
    every = np.arange(-32768, 32768, dtype=np.int32)
    as_float = every.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(as_float.astype(np.float64) * 32768.0, every.astype(np.float64))
