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
not RIFF/WAVE (RF64 and big-endian RIFX included).  Resampling is out of scope: the rate is returned, the caller decides.
"""
import io
import os
import struct

import numpy as np

WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
_PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")      # KSDATAFORMAT_SUBTYPE_PCM after its two-byte format tag
_OPEN_SIZES = (0, 0xFFFFFFFF)


class Unsupported(ValueError):
    """a file read_pcm16 does not take; the message names the file and the reason"""


def locate(f, total, name):
    """walk the chunks of the open binary file `f` of `total` bytes -> (sample_rate, byte offset of the first sample, samples); reads the
    chunk headers and the 'fmt ' body only.  `name` is what a refusal calls the file."""
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
            fmt = rate
        elif cid == b"data":
            if fmt is None:
                refuse("no 'fmt ' chunk before 'data'")
            avail = total - body
            n = avail if size in _OPEN_SIZES else min(size, avail)
            return fmt, body, n // 2
        pos = body + size + (size & 1)
    refuse("no 'data' chunk" if fmt is not None else "no 'fmt ' and no 'data' chunk")


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
