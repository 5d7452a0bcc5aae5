"""A host reader for the one kind of audio file the AudioSet stage needs: RIFF/WAVE, 16-bit PCM, mono (numpy only).

    read_pcm16(path) -> (int16 ndarray [S], sample_rate)
    probe_pcm16(path) -> (S, sample_rate)      from the chunk headers alone: what an epoch plan needs of a clip
    parse_pcm16(bytes, name)                   read_pcm16 on a file already in memory
    Unsupported(ValueError)                    every refusal: it names the file and the reason

The reference loads its clips with `librosa.load(path, sr=16000)` (models/audioset_dataset.py:61), that is libsndfile behind soundfile.  This
module is NOT a run of libsndfile: the rule below is this project's own, written from the RIFF/WAVE layout (Microsoft / IBM "Multimedia
Programming Interface and Data Specifications 1.0"; WAVE_FORMAT_EXTENSIBLE as in Microsoft's "Multiple channel audio data and WAVE files").
What makes it enough: for a 16-bit file librosa's float32 sample is the int16 sample / 32768, and that division is what `pcm()` in
csrc/audio_ingest.hip applies on the device, exactly -- so the int16 samples as stored are all a clip has to bring.

Accepted:
  * 'RIFF' <size> 'WAVE', then chunks: 4-byte id, 4-byte little-endian size, the body, one pad byte after an odd-sized body;
  * a 'fmt ' chunk before 'data' with format tag 1 (WAVE_FORMAT_PCM), or 0xFFFE (WAVE_FORMAT_EXTENSIBLE) whose sub-format GUID is the PCM one;
    16 bits a sample (for EXTENSIBLE also 16 valid bits), one channel;
  * any other chunk (ffmpeg's 'LIST', 'fact', ...) is skipped; the RIFF size field is not trusted (a pipe writer leaves it wrong);
  * a 'data' size of 0 or 0xFFFFFFFF (ffmpeg writing to a pipe) means "to the end of the file";
  * a 'data' chunk longer than the file is cut at the last whole sample.
Everything else raises Unsupported: other bit depths, float, more than one channel, compressed formats, no 'fmt ' before 'data', no 'data',
not RIFF/WAVE (RF64 and big-endian RIFX included).  The rate is returned, the caller decides.

The wider reader, for what `librosa.load(path, sr=16000)` takes of the wavs ffmpeg cuts out of a video (process/extract_melspec.py:13) or
of an AudioSet folder that was not converted (models/audioset_dataset.py:61): the same chunk walk, other 'fmt ' rule.

    probe_wave(path) -> WaveInfo(rate, channels, kind, frames, data_offset)    from the chunk headers alone
    read_wave(path)  -> (uint8 ndarray: the 'data' body as stored, cut at the last whole frame; WaveInfo)
    parse_wave(bytes, name)                                                    read_wave on a file already in memory
    to_float(raw, info), to_mono(y)                                            the decode and down-mix rule, on the host

Accepted there: tag 1 (PCM) of 8 (unsigned), 16, 24 or 32 bits, tag 3 (IEEE float) of 32 bits, or EXTENSIBLE with either sub-format GUID and
as many valid bits as container bits; 1 to 8 channels; any positive rate.  Refused by name: 64-bit float, A-law / mu-law, ADPCM and every other
tag, 0 or more than 8 channels, RF64 / RIFX.  The bytes are not decoded on the host: csrc/resample.hip turns them into 16 kHz mono float32
(m3t.audio.decode_waves) by libsndfile's normalised-read rule as its documentation states it -- (u8 - 128) / 128, i16 / 32768,
i24 / 8388608, i32 / 2147483648 rounded once to float32, float32 as stored -- and librosa.to_mono (the channels summed in order in float32,
divided by their count).  Again our text, not a run of libsndfile.
"""
import collections
import io
import os
import struct

import numpy as np

WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
_PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")      # KSDATAFORMAT_SUBTYPE_PCM after its two-byte format tag
_OPEN_SIZES = (0, 0xFFFFFFFF)


class Unsupported(ValueError):
    """a file read_pcm16 does not take; the message names the file and the reason"""


def _walk(f, total, name, fmt_rule):
    """the chunk walk both readers share: -> (what `fmt_rule(data, size, refuse)` made of the 'fmt ' body, byte offset of the 'data' body,
    its bytes inside the file); reads the chunk headers and the first 40 bytes of 'fmt ' only.  `name` is what a refusal calls the file."""
    def refuse(why):
        raise Unsupported("%s: %s" % (name, why))

    f.seek(0)
    head = f.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        refuse("not a RIFF/WAVE file (it starts with %r)" % (head,))
    pos, fmt = 12, None
    while pos + 8 <= total:
        f.seek(pos)
        hdr = f.read(8)
        if len(hdr) < 8:
            break
        cid, size = hdr[:4], struct.unpack("<I", hdr[4:])[0]
        body = pos + 8
        if cid == b"fmt ":
            data = f.read(min(size, 40))
            if size < 16 or body + size > total or len(data) < min(size, 40):
                refuse("a 'fmt ' chunk of %d bytes (16 at least, inside the file)" % size)
            fmt = fmt_rule(data, size, refuse)
        elif cid == b"data":
            if fmt is None:
                refuse("no 'fmt ' chunk before 'data'")
            avail = total - body
            return fmt, body, avail if size in _OPEN_SIZES else min(size, avail)
        pos = body + size + (size & 1)
    refuse("no 'data' chunk" if fmt is not None else "no 'fmt ' and no 'data' chunk")


def _pcm16_rule(data, size, refuse):
    tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", data, 0)
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if size < 40:
            refuse("WAVE_FORMAT_EXTENSIBLE with a 'fmt ' chunk of %d bytes (40 at least)" % size)
        valid_bits, sub = struct.unpack_from("<H", data, 18)[0], data[24:40]
        if sub[2:] != _PCM_GUID_TAIL:
            refuse("WAVE_FORMAT_EXTENSIBLE with a sub-format that is not PCM (%s)" % sub.hex())
        tag = struct.unpack_from("<H", sub, 0)[0]
        if tag == WAVE_FORMAT_PCM and valid_bits not in (0, bits):
            refuse("%d valid bits in a %d-bit container: only 16 in 16 is taken" % (valid_bits, bits))
    if tag == WAVE_FORMAT_IEEE_FLOAT:
        refuse("IEEE float samples (format tag 3): only 16-bit PCM is taken")
    if tag != WAVE_FORMAT_PCM:
        refuse("format tag 0x%04x, a compressed or unknown format: only PCM (1) is taken" % tag)
    if bits != 16:
        refuse("%d-bit samples: only 16-bit PCM is taken" % bits)
    if channels != 1:
        refuse("%d channels: only mono is taken (no down-mix here)" % channels)
    if rate <= 0:
        refuse("a sample rate of %d" % rate)
    return rate


def locate(f, total, name):
    """walk the chunks of the open binary file `f` of `total` bytes -> (sample_rate, byte offset of the first sample, samples); reads the
    chunk headers and the 'fmt ' body only.  `name` is what a refusal calls the file."""
    rate, body, nbytes = _walk(f, total, name, _pcm16_rule)
    return rate, body, nbytes // 2


def _read(f, total, name):
    rate, body, n = locate(f, total, name)
    f.seek(body)
    raw = f.read(2 * n)
    return np.frombuffer(raw, dtype="<i2", count=len(raw) // 2).astype(np.int16), rate


def parse_pcm16(data, name="<bytes>"):
    """read_pcm16 on the bytes of a file already in memory; `name` is what a refusal calls it"""
    return _read(io.BytesIO(data), len(data), name)


def read_pcm16(path):
    """-> (int16 ndarray [S] (a copy, writable), sample_rate).  Unsupported for anything but 16-bit mono PCM in RIFF/WAVE (see the module's
    text); OSError for a file that cannot be read.  Our rule, not libsndfile's."""
    with open(path, "rb") as f:
        return _read(f, os.fstat(f.fileno()).st_size, str(path))


def probe_pcm16(path):
    """-> (samples, sample_rate) of a file read_pcm16 takes, from its chunk headers alone (the samples are not read)"""
    with open(path, "rb") as f:
        rate, _, n = locate(f, os.fstat(f.fileno()).st_size, str(path))
    return n, rate


# ---- the wider reader: every rate, 1..8 channels, PCM 8/16/24/32 and float32 -----------------------------------------------------------
KIND_U8, KIND_I16, KIND_I24, KIND_I32, KIND_F32 = 0, 1, 2, 3, 4
KIND_NAMES = ("u8", "i16", "i24", "i32", "f32")
KIND_BYTES = (1, 2, 3, 4, 4)
MAX_CHANNELS = 8
_PCM_KINDS = {8: KIND_U8, 16: KIND_I16, 24: KIND_I24, 32: KIND_I32}


class WaveInfo(collections.namedtuple("WaveInfo", "rate channels kind frames data_offset")):
    """what probe_wave reads off a file's headers: the sample rate, the channel count, the sample kind (KIND_*), the whole frames of the
    'data' body and the body's byte offset in the file"""
    __slots__ = ()

    @property
    def frame_bytes(self):
        return self.channels * KIND_BYTES[self.kind]


def _wave_rule(data, size, refuse):
    tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", data, 0)
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if size < 40:
            refuse("WAVE_FORMAT_EXTENSIBLE with a 'fmt ' chunk of %d bytes (40 at least)" % size)
        valid_bits, sub = struct.unpack_from("<H", data, 18)[0], data[24:40]
        if sub[2:] != _PCM_GUID_TAIL:
            refuse("WAVE_FORMAT_EXTENSIBLE with a sub-format that is neither PCM nor IEEE float (%s)" % sub.hex())
        tag = struct.unpack_from("<H", sub, 0)[0]
        if valid_bits not in (0, bits):
            refuse("%d valid bits in a %d-bit container: only full containers are taken" % (valid_bits, bits))
    if tag == WAVE_FORMAT_PCM:
        if bits not in _PCM_KINDS:
            refuse("%d-bit PCM samples: 8, 16, 24 and 32 bits are taken" % bits)
        kind = _PCM_KINDS[bits]
    elif tag == WAVE_FORMAT_IEEE_FLOAT:
        if bits != 32:
            refuse("%d-bit IEEE float samples: only 32-bit float is taken" % bits)
        kind = KIND_F32
    else:
        refuse("format tag 0x%04x, a compressed or unknown format (A-law, mu-law, ADPCM, ...): only PCM (1) and IEEE float (3) are taken" % tag)
    if not 1 <= channels <= MAX_CHANNELS:
        refuse("%d channels: 1 to %d are taken" % (channels, MAX_CHANNELS))
    if rate <= 0:
        refuse("a sample rate of %d" % rate)
    return rate, channels, kind


def _locate_wave(f, total, name):
    (rate, channels, kind), body, nbytes = _walk(f, total, name, _wave_rule)
    return WaveInfo(rate, channels, kind, nbytes // (channels * KIND_BYTES[kind]), body)


def _read_wave(f, total, name):
    info = _locate_wave(f, total, name)
    f.seek(info.data_offset)
    raw = np.frombuffer(f.read(info.frames * info.frame_bytes), np.uint8)
    if raw.shape[0] % info.frame_bytes:                              # (a file that shrank under us: still whole frames only)
        raw = raw[:raw.shape[0] - raw.shape[0] % info.frame_bytes]
        info = info._replace(frames=raw.shape[0] // info.frame_bytes)
    return raw, info


def probe_wave(path):
    """-> WaveInfo(rate, channels, kind, frames, data_offset) of a file read_wave takes, from its chunk headers alone"""
    with open(path, "rb") as f:
        return _locate_wave(f, os.fstat(f.fileno()).st_size, str(path))


def read_wave(path):
    """-> (uint8 ndarray: the 'data' body as stored, interleaved, cut at the last whole frame; WaveInfo).  Unsupported for what the module's
    text does not list; OSError for a file that cannot be read.  The samples are NOT decoded here: m3t.audio.decode_waves does that on the
    device, and `to_float` / `to_mono` below state the rule."""
    with open(path, "rb") as f:
        return _read_wave(f, os.fstat(f.fileno()).st_size, str(path))


def parse_wave(data, name="<bytes>"):
    """read_wave on the bytes of a file already in memory"""
    return _read_wave(io.BytesIO(data), len(data), name)


def to_float(raw, info):
    """the sample-to-float rule on the host -> float32 [frames, channels]: (u8 - 128) / 128, i16 / 32768, i24 / 8388608, i32 / 2147483648
    rounded once to float32, float32 as stored.  What csrc/resample.hip applies on the device; written from libsndfile's documentation of
    its normalised float read, not a run of it."""
    raw = np.ascontiguousarray(raw, np.uint8)[:info.frames * info.frame_bytes]
    if info.kind == KIND_U8:
        y = (raw.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif info.kind == KIND_I16:
        y = raw.view("<i2").astype(np.float32) / np.float32(32768)
    elif info.kind == KIND_I24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        y = (v - ((v & 0x800000) << 1)).astype(np.float32) / np.float32(8388608)
    elif info.kind == KIND_I32:
        y = (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        y = raw.view("<f4").astype(np.float32)
    return y.reshape(info.frames, info.channels)


def to_mono(y):
    """librosa.to_mono on [frames, channels] float32: the channels summed in channel order in float32, then divided by their count"""
    acc = y[:, 0].astype(np.float32)
    for c in range(1, y.shape[1]):
        acc = acc + y[:, c]
    return acc / np.float32(y.shape[1])
