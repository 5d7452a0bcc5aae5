"""Batched baseline-JPEG decode on the GPU: the step in front of m3t/video.py.

The first line of the reference's `load_video` (`models/dataset.py:64`) is `cv2.imread` of one JPEG per frame -- on the host, at about
0.7 ms a 256 x 256 frame and core, which a training step of 512 frames cannot be fed from.  Here the files' bytes go to the device as
they are and two launches (csrc/jpeg.hip, m3t_jpeg_decode; the rules in csrc/jpeg_core.h) write the uint8 `[N, Ts, H, W, 3]` buffer every
later stage takes:

  parse        one file's header, on the host: size, mode, tables, restart interval, where the scan lies; Unsupported for the rest
  pack         a flat list of files (bytes or None) -> JpegBatch: ONE byte buffer of scan data, the segment and image tables, the
               quantisation and Huffman tables deduplicated by content (a dataset batch carries two and four), the lookup form built here
  decode       JpegBatch -> (frames uint8 [n, H, W, 3] on the device, or into a caller's `out` at `slots`; status int32 [n] on the device)
               walk="sequential": one lane walks a segment's symbols; walk="parallel": a workgroup walks it, every lane a sub-sequence
               of `sub_bytes` (self-synchronising Huffman decoding, csrc/jpeg_par.h); walk="auto": by segment size, the thresholds
               AUTO_MIN_BYTES / AUTO_SUB_BYTES below.  Both walks give the same frames and the same status for every input.
  load_clips   clips[n][t] of bytes / paths / None -> (frames [N, Ts, H, W, 3], present [N, Ts], status); `present` is what
               video.frame_index takes, an absent frame is zeros (the reference's `img is None`)

In scope: baseline sequential DCT (SOF0), 8 bits, Huffman, one interleaved scan, 1 component (gray) or 3 (YCbCr, luma 1x1 / 2x1 / 2x2,
chroma 1x1), up to four tables of each kind, restart intervals; APPn / COM are skipped and EXIF orientation is ignored.  Everything else
-- progressive, extended, lossless, arithmetic, 12 bits, 16-bit quantisation tables, four components, other sampling factors, several
scans, missing tables, a missing EOI -- raises Unsupported (a ValueError that names the reason) before anything touches a device.  All
images of a batch share one size.

What is pinned: the bits are those of libjpeg-turbo with its default settings -- the ISLOW integer IDCT, "fancy" chroma upsampling over
the component's real size, the 16-bit fixed-point colour conversion -- as Pillow decodes (tests/golden/jpeg_cases.npz holds Pillow's
pixels and every comparison is exact).  What is NOT pinned by a run: OpenCV.  `cv2.imread` is the reference's decoder; it bundles
libjpeg-turbo and by its published source sets neither the DCT method nor the upsampling option, so it should give the same bits, but cv2
is not installed where this project is developed -- tests/test_jpeg_cv2_host.py holds that comparison for whoever has it.  IJG libjpeg 7
and later upsample differently and are not the target.  The default channel order is "bgr", what `cv2.imread` returns and the ingest's
goldens assume.

`status` stays on the device: 0 = decoded; otherwise bit flags (TRUNC, CODE, RST, EXTRA below).  A damaged stream still fills its frame
(zero bits past a truncation, flat blocks after a bad code) and never touches another frame.  A stream whose damage leaves it a valid
JPEG -- a flipped bit inside a coefficient's value -- decodes to the pixels it now describes with status 0; no decoder can tell.
There is no host fallback: without a GPU decode raises, and the host route is the caller's own decoder.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import M3THipError

TRUNC, CODE, RST, EXTRA = _lib.M3T_JPEG_TRUNC, _lib.M3T_JPEG_CODE, _lib.M3T_JPEG_RST, _lib.M3T_JPEG_EXTRA
IMG_COLS, SEG_COLS, QUANT_INTS, HUFF_INTS, LUT_BITS = 16, 4, 32, 384, 9       # csrc/jpeg_core.h
MODES = {(1, 1, 1): "gray", (3, 1, 1): "444", (3, 2, 1): "422", (3, 2, 2): "420"}
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


WALKS = ("sequential", "parallel", "auto")
# what walk="auto" does, chosen by measurement on the MI355X (NOTEBOOK section 16; tools/jpeg_bench.py --sweep --crossover prints the
# tables): segments of at least AUTO_MIN_BYTES take the parallel walk with sub-sequences of AUTO_SUB_BYTES.  512 dataset frames (45 KB a
# segment) decode in 2.8 ms instead of 24.1 and from 4 KB up the parallel walk won at every size measured; under 2 KB a segment the two
# walks are within a third of each other with either sign.  (AUTO_MIN_BYTES = None would make "auto" sequential.)
AUTO_MIN_BYTES = 4096
AUTO_SUB_BYTES = 256


class Unsupported(ValueError):
    """a stream outside the decoder's scope; the message names the reason"""


class Header:
    """One file's header.  height, width; components (1 or 3); hs, vs (luma sampling); mode ("gray", "444", "422", "420");
    quant: per component, uint8 [64] in zig-zag order as stored; dc, ac: per component, (counts uint8 [16], symbols uint8 [k]);
    restart_interval (MCUs, 0 = none); scan_offset, scan_end: the entropy-coded bytes data[scan_offset:scan_end]."""
    __slots__ = ("height", "width", "components", "hs", "vs", "mode", "quant", "dc", "ac", "restart_interval", "scan_offset", "scan_end")

    @property
    def mcus(self):
        return (-(-self.width // (8 * self.hs))) * (-(-self.height // (8 * self.vs)))


_SOF_REASON = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive DCT (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
               0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
               0xCA: "arithmetic coding, progressive (SOF10)", 0xCB: "arithmetic coding, lossless (SOF11)", 0xCD: "arithmetic coding (SOF13)",
               0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def parse(data):
    """bytes of one JPEG file -> Header.  Host only.  Unsupported for everything outside the scope named in the module docstring."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported("not a JPEG stream: no SOI marker")
    quant, dcs, acs = {}, {}, {}
    frame = None
    ri = 0
    p = 2
    while True:
        if p + 4 > n:
            raise Unsupported("truncated header: no SOS marker")
        if data[p] != 0xFF:
            raise Unsupported("garbage between segments at byte %d" % p)
        m = data[p + 1]
        if m == 0xFF:                                   # fill byte
            p += 1
            continue
        if m == 0xD9:
            raise Unsupported("EOI before any scan")
        seg_len = (data[p + 2] << 8) | data[p + 3]
        body = data[p + 4:p + 2 + seg_len]
        if seg_len < 2 or p + 2 + seg_len > n:
            raise Unsupported("truncated header segment 0x%02X" % m)
        if m == 0xDB:                                   # DQT
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq != 0:
                    raise Unsupported("16-bit quantisation tables")
                if tq > 3 or q + 65 > len(body):
                    raise Unsupported("malformed DQT segment")
                quant[tq] = np.frombuffer(body[q + 1:q + 65], np.uint8).copy()
                q += 65
        elif m == 0xC4:                                 # DHT
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                if tc > 1 or th > 3 or q + 17 > len(body):
                    raise Unsupported("malformed DHT segment")
                counts = np.frombuffer(body[q + 1:q + 17], np.uint8).copy()
                k = int(counts.sum())
                if k > 256 or q + 17 + k > len(body):
                    raise Unsupported("malformed DHT segment")
                code = 0
                for length in range(1, 17):             # the code space must hold the counts
                    code += int(counts[length - 1])
                    if code > (1 << length):
                        raise Unsupported("malformed DHT segment: more codes than the lengths allow")
                    code <<= 1
                (acs if tc else dcs)[th] = (counts, np.frombuffer(body[q + 17:q + 17 + k], np.uint8).copy())
                q += 17 + k
        elif m == 0xC0:
            if frame is not None:
                raise Unsupported("two frame headers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise Unsupported("malformed SOF0 segment")
            frame = body
        elif m in _SOF_REASON:
            if m == 0xC1 and len(body) >= 1 and body[0] == 12:
                raise Unsupported("12-bit samples (extended sequential DCT, SOF1)")
            raise Unsupported(_SOF_REASON[m])
        elif m == 0xCC:
            raise Unsupported("arithmetic coding (DAC)")
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported("malformed DRI segment")
            ri = (body[0] << 8) | body[1]
        elif m == 0xDA:
            break
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass                                        # APPn, COM
        else:
            raise Unsupported("unexpected marker 0x%02X in the header" % m)
        p += 2 + seg_len
    if frame is None:
        raise Unsupported("a scan without a frame header")
    if frame[0] != 8:
        raise Unsupported("%d-bit samples" % frame[0])
    h = Header()
    h.height, h.width, nc = (frame[1] << 8) | frame[2], (frame[3] << 8) | frame[4], frame[5]
    if h.height <= 0 or h.width <= 0:
        raise Unsupported("an empty image (%d x %d)" % (h.height, h.width))
    if nc not in (1, 3):
        raise Unsupported("%d components (only gray and YCbCr)" % nc)
    comps = [(frame[6 + 3 * c], frame[7 + 3 * c] >> 4, frame[7 + 3 * c] & 15, frame[8 + 3 * c]) for c in range(nc)]
    if nc == 1:
        h.hs = h.vs = 1                                 # a single component's scan is not interleaved: its factors do not matter
    else:
        h.hs, h.vs = comps[0][1], comps[0][2]
        if (nc, h.hs, h.vs) not in MODES or any(c[1] != 1 or c[2] != 1 for c in comps[1:]):
            raise Unsupported("sampling factors %s (luma 1x1, 2x1 or 2x2 with chroma 1x1 only)" % "/".join("%dx%d" % (c[1], c[2]) for c in comps))
    h.components, h.mode = nc, MODES[(nc, h.hs, h.vs)]
    if len(body) < 4 or len(body) != 4 + 2 * body[0]:
        raise Unsupported("malformed SOS segment")
    if body[0] != nc:
        raise Unsupported("multiple scans: the first scan holds %d of %d components" % (body[0], nc))
    if tuple(body[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
        raise Unsupported("a spectral selection or successive approximation in a sequential scan")
    h.quant, h.dc, h.ac = [], [], []
    for c in range(nc):
        cid, tabs = body[1 + 2 * c], body[2 + 2 * c]
        if cid != comps[c][0]:
            raise Unsupported("the scan's components are not in the frame's order")
        if comps[c][3] not in quant:
            raise Unsupported("missing quantisation table %d" % comps[c][3])
        if (tabs >> 4) not in dcs:
            raise Unsupported("missing DC Huffman table %d" % (tabs >> 4))
        if (tabs & 15) not in acs:
            raise Unsupported("missing AC Huffman table %d" % (tabs & 15))
        h.quant.append(quant[comps[c][3]])
        h.dc.append(dcs[tabs >> 4])
        h.ac.append(acs[tabs & 15])
    h.restart_interval = ri
    h.scan_offset = p + 2 + seg_len
    # the scan ends at the first marker that is neither a stuffed FF 00 nor RSTn
    a = np.frombuffer(data, np.uint8, offset=h.scan_offset)
    nxt = a[1:]
    hit = np.flatnonzero((a[:-1] == 0xFF) & (nxt != 0) & ((nxt & 0xF8) != 0xD0) & (nxt != 0xFF))
    if hit.size == 0:
        raise Unsupported("missing EOI marker")
    h.scan_end = h.scan_offset + int(hit[0])
    after = data[h.scan_end + 1]
    if after != 0xD9:
        raise Unsupported("multiple scans (marker 0x%02X after the first scan)" % after)
    return h


def huff_lookup(counts, symbols):
    """int32 [HUFF_INTS]: the table's lookup form (include/m3t_hip.h): uint16 lut[512] | maxcode[18] | valoff[18] | symbols[256]"""
    out = np.zeros(HUFF_INTS, np.int32)
    lut = out[:256].view(np.uint16)
    maxcode, valoff = out[256:274], out[274:292]
    out[292:356].view(np.uint8)[:len(symbols)] = symbols
    maxcode[:] = -1
    code, k = 0, 0
    for length in range(1, 17):
        cnt = int(counts[length - 1])
        if cnt:
            valoff[length] = k - code
            if length <= LUT_BITS:
                for j in range(cnt):
                    lo = (code + j) << (LUT_BITS - length)
                    lut[lo:lo + (1 << (LUT_BITS - length))] = (length << 8) | int(symbols[k + j])
            code += cnt
            k += cnt
            maxcode[length] = code - 1
        code <<= 1
    return out


class JpegBatch:
    """What m3t_jpeg_decode takes (include/m3t_hip.h).  stream: uint8 host tensor, the scan data of every image, zero padded to 16 bytes
    (pin it to overlap its copy: pack(..., pin=True)); tables: int32 array images | segments | slots placeholder | quant | huff;
    n, n_segs, n_quant, n_huff, height, width; present: bool [n]; headers: the parsed Header of each item (None where absent)."""
    __slots__ = ("stream", "tables", "n", "n_segs", "n_quant", "n_huff", "height", "width", "present", "headers")

    @property
    def images(self):
        return self.tables[:self.n * IMG_COLS].reshape(self.n, IMG_COLS)

    @property
    def segments(self):
        o = self.n * IMG_COLS
        return self.tables[o:o + self.n_segs * SEG_COLS].reshape(self.n_segs, SEG_COLS)

    @property
    def slots(self):
        o = self.n * IMG_COLS + self.n_segs * SEG_COLS
        return self.tables[o:o + self.n]

    @property
    def quant(self):
        o = self.n * IMG_COLS + self.n_segs * SEG_COLS + self.n
        return self.tables[o:o + self.n_quant * QUANT_INTS].view(np.uint16).reshape(self.n_quant, 64)

    @property
    def huff(self):
        o = self.n * IMG_COLS + self.n_segs * SEG_COLS + self.n + self.n_quant * QUANT_INTS
        return self.tables[o:o + self.n_huff * HUFF_INTS].reshape(self.n_huff, HUFF_INTS)


def pack(items, pin=False):
    """items: a flat list of `bytes` (one JPEG file each) or None (an absent frame) -> JpegBatch.  Host only.  ValueError for an empty list,
    a list of None only, or images of different sizes; Unsupported from parse."""
    items = list(items)
    if not items:
        raise ValueError("jpeg.pack: no items")
    headers = [None if it is None else parse(it) for it in items]
    sizes = sorted({(h.height, h.width) for h in headers if h is not None})
    if not sizes:
        raise ValueError("jpeg.pack: every item is absent, the batch has no size")
    if len(sizes) != 1:
        raise ValueError("jpeg.pack: the images of a batch must share one size, got %s" % ", ".join("%d x %d" % s for s in sizes))
    n = len(items)
    quants, huffs = {}, {}
    qrows, hrows = [], []

    def q_index(q):
        key = q.tobytes()
        if key not in quants:
            quants[key] = len(qrows)
            nat = np.zeros(64, np.uint16)
            nat[ZIGZAG] = q
            qrows.append(nat.view(np.int32))
        return quants[key]

    def h_index(t):
        key = t[0].tobytes() + t[1].tobytes()
        if key not in huffs:
            huffs[key] = len(hrows)
            hrows.append(huff_lookup(t[0], t[1]))
        return huffs[key]

    images = np.zeros((n, IMG_COLS), np.int32)
    segs, chunks = [], []
    pos = 0
    for i, (it, h) in enumerate(zip(items, headers)):
        if h is None:
            continue
        scan = np.frombuffer(it, np.uint8, count=h.scan_end - h.scan_offset, offset=h.scan_offset)
        mcus = h.mcus
        ri = h.restart_interval if 0 < h.restart_interval < mcus else mcus
        want = -(-mcus // ri)
        at = np.flatnonzero((scan[:-1] == 0xFF) & ((scan[1:] & 0xF8) == 0xD0)) if scan.size > 1 else np.zeros(0, np.int64)
        starts = np.concatenate([[0], at + 2])
        ends = np.concatenate([at, [scan.size]])
        marks = np.concatenate([[-1], scan[at + 1] & 7]) if at.size else np.array([-1])
        found = starts.size
        flags = 1 | (2 if found != want else 0)          # bit 1: the markers found are not the markers the MCU count asks for
        row0 = len(segs)
        for k in range(want):
            if k < found:
                segs.append((i, pos + int(starts[k]), int(ends[k] - starts[k]), int(marks[k])))
            else:
                segs.append((i, pos + scan.size, 0, -2))
        images[i, :7] = (flags, h.components, h.hs, h.vs, ri, row0, want)
        for c in range(h.components):
            images[i, 7 + c] = q_index(h.quant[c])
            images[i, 10 + c] = h_index(h.dc[c])
            images[i, 13 + c] = h_index(h.ac[c])
        chunks.append(scan)
        pos += scan.size
    b = JpegBatch()
    padded = (pos + 15) // 16 * 16 + 16
    b.stream = torch.zeros(padded, dtype=torch.uint8)
    if pin and torch.cuda.is_available():
        b.stream = b.stream.pin_memory()
    if chunks:
        np.concatenate(chunks, out=b.stream.numpy()[:pos])
    seg_arr = np.asarray(segs, np.int32).reshape(-1, SEG_COLS)
    b.n, b.n_segs, b.n_quant, b.n_huff = n, len(segs), len(qrows), len(hrows)
    b.tables = np.concatenate([images.reshape(-1), seg_arr.reshape(-1), np.arange(n, dtype=np.int32)] +
                              [np.asarray(r, np.int32) for r in qrows] + hrows).astype(np.int32, copy=False)
    b.height, b.width = sizes[0]
    b.present = np.array([h is not None for h in headers])
    b.headers = headers
    return b


def _stream():
    return torch.cuda.current_stream().cuda_stream


def par_max_bytes():
    """the largest segment (bytes) the parallel walk takes in this build; larger ones go to the sequential walk"""
    return int(_lib.load().m3t_jpeg_par_max_bytes())


def par_lanes(lanes=None):
    """the workgroup size of the parallel walk (64, 128 or 256 lanes; results do not depend on it): set it, or read it with None"""
    rc = int(_lib.load().m3t_jpeg_par_lanes(0 if lanes is None else int(lanes)))
    if lanes is not None and (int(lanes) == 0 or rc < 0):
        raise ValueError("jpeg.par_lanes: 64, 128 or 256")
    return rc


def _walk_args(walk, sub_bytes, par_min_bytes, par_max_bytes):
    """-> the (walk, sub_bytes, par_min_bytes, par_max_bytes) ints of m3t_jpeg_decode_walk; ValueError for what it would refuse"""
    if walk not in WALKS:
        raise ValueError("jpeg.decode: walk must be one of %s" % ", ".join(repr(w) for w in WALKS))
    if sub_bytes is None:
        sub_bytes = AUTO_SUB_BYTES
    if not (isinstance(sub_bytes, (int, np.integer)) and 16 <= sub_bytes <= 4096 and sub_bytes % 16 == 0):
        raise ValueError("jpeg.decode: sub_bytes must be a multiple of 16 in [16, 4096]")
    for name, v in (("par_min_bytes", par_min_bytes), ("par_max_bytes", par_max_bytes)):
        if v is not None and not (isinstance(v, (int, np.integer)) and 0 <= v < 2 ** 31):
            raise ValueError("jpeg.decode: %s must be a non-negative int" % name)
    if walk == "sequential" or (walk == "auto" and AUTO_MIN_BYTES is None and par_min_bytes is None):
        return 0, int(sub_bytes), 0, 0
    if par_min_bytes is None:
        par_min_bytes = 0 if walk == "parallel" else AUTO_MIN_BYTES
    if par_max_bytes is None:
        par_max_bytes = 2 ** 31 - 1
    return 1, int(sub_bytes), int(par_min_bytes), int(par_max_bytes)


def decode(batch, out=None, slots=None, order="bgr", walk="auto", sub_bytes=None, par_min_bytes=None, par_max_bytes=None, stats=False):
    """JpegBatch -> (frames, status).  out=None: frames is a new uint8 [n, H, W, 3] on the current device.  With `out`, a contiguous uint8
    device tensor [N, Ts, H, W, 3], and slots (n pairs (clip, frame), all different): image i goes to out[slots[i]], every other frame of
    `out` is left as it is, and frames is `out`.  An absent item writes zeros.  order: "bgr" (cv2.imread's) or "rgb".  status: int32 [n]
    on the device (0, or TRUNC | CODE | RST | EXTRA).  Everything runs on the current stream without a host synchronisation; the stream
    bytes and the tables travel in one copy each.
    walk: "sequential" (every segment on one lane), "parallel" (every segment of par_min_bytes <= bytes <= min(par_max_bytes,
    par_max_bytes()) by a workgroup in sub-sequences of sub_bytes, the rest sequentially; par_min_bytes defaults to 0) or "auto" (the
    same routing with the measured defaults: par_min_bytes = AUTO_MIN_BYTES, sub_bytes = AUTO_SUB_BYTES).  Frames and status do not depend on any of it.  stats=True: -> (frames, status, walk_stats), the last an int32
    [n_segs, 2] device tensor: (sub-sequences, exchange passes) of a segment the parallel walk took, (0, 0) of any other."""
    if order not in ("bgr", "rgb"):
        raise ValueError("jpeg.decode: order must be 'bgr' or 'rgb'")
    walk_i, sub_i, min_i, max_i = _walk_args(walk, sub_bytes, par_min_bytes, par_max_bytes)
    if not isinstance(batch, JpegBatch):
        raise ValueError("jpeg.decode: batch must be a JpegBatch (jpeg.pack)")
    n, H, W = batch.n, batch.height, batch.width
    if (out is None) != (slots is None):
        raise ValueError("jpeg.decode: out and slots go together")
    tables = batch.tables
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.dim() == 5 and tuple(out.shape[2:]) == (H, W, 3)):
            raise ValueError("jpeg.decode: out must be uint8 [N, Ts, %d, %d, 3]" % (H, W))
        if not (out.is_cuda and out.is_contiguous()):
            raise M3THipError("jpeg.decode: out must be a contiguous device tensor")
        sl = np.asarray(slots, np.int64).reshape(-1, 2) if len(slots) else np.zeros((0, 2), np.int64)
        N, Ts = int(out.shape[0]), int(out.shape[1])
        if sl.shape[0] != n or (sl < 0).any() or (sl[:, 0] >= N).any() or (sl[:, 1] >= Ts).any():
            raise ValueError("jpeg.decode: slots must be %d (clip, frame) pairs inside [%d, %d)" % (n, N, Ts))
        flat = sl[:, 0] * Ts + sl[:, 1]
        if np.unique(flat).size != n:
            raise ValueError("jpeg.decode: two images share a slot")
        tables = tables.copy()
        o = n * IMG_COLS + batch.n_segs * SEG_COLS
        tables[o:o + n] = flat
        dst_slots = N * Ts
    else:
        dst_slots = n
    if not torch.cuda.is_available():
        raise M3THipError("m3t.jpeg needs the GPU: the M3T path has no CPU fallback")
    lib = _lib.load()
    dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        tables = np.ascontiguousarray(tables, np.int32)
        t_d = torch.from_numpy(tables).to(dev, non_blocking=True)
        s_d = batch.stream.to(dev, non_blocking=True)
        ws_bytes = int(lib.m3t_jpeg_workspace_bytes(n, H, W))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        walk_stats = torch.empty(batch.n_segs, 2, dtype=torch.int32, device=dev) if stats else None
        _lib.check(lib.m3t_jpeg_decode_walk(s_d.data_ptr(), s_d.numel(), tables.ctypes.data, t_d.data_ptr(), n, batch.n_segs, batch.n_quant,
                                            batch.n_huff, H, W, out.data_ptr(), dst_slots, 0 if order == "bgr" else 1, ws.data_ptr(), ws_bytes,
                                            status.data_ptr(), walk_i, sub_i, min_i, max_i,
                                            walk_stats.data_ptr() if stats and batch.n_segs else None, _stream()), "m3t_jpeg_decode_walk")
    return (out, status, walk_stats) if stats else (out, status)


def _read(item):
    if item is None or isinstance(item, (bytes, bytearray, memoryview)):
        return None if item is None else bytes(item)
    try:
        with open(os.fspath(item), "rb") as f:
            return f.read()
    except (FileNotFoundError, IsADirectoryError, NotADirectoryError):
        return None                                     # the reference's `img is None`


def load_clips(clips, order="bgr", threads=8, pin=False, walk="auto", sub_bytes=None):
    """clips[n][t]: bytes, a path, or None, every clip of one length Ts -> (frames uint8 [N, Ts, H, W, 3] on the device, present bool
    [N, Ts] (numpy), status int32 [N Ts] on the device, clip-major).  A None entry or a file that does not exist is absent: present is
    False and its frame zero -- what video.frame_index(present[n], ...) then routes around (dataset.py:64-68).  Files are read by a
    small thread pool (at most 16 threads).  walk, sub_bytes: decode's."""
    clips = [list(c) for c in clips]
    if not clips or not clips[0] or any(len(c) != len(clips[0]) for c in clips):
        raise ValueError("jpeg.load_clips: clips must be a non-empty list of equally long lists")
    N, Ts = len(clips), len(clips[0])
    flat = [it for c in clips for it in c]
    if any(it is not None and not isinstance(it, (bytes, bytearray, memoryview)) for it in flat):
        with ThreadPoolExecutor(max(1, min(int(threads), 16))) as pool:
            flat = list(pool.map(_read, flat))
    else:
        flat = [_read(it) for it in flat]
    batch = pack(flat, pin=pin)
    frames, status = decode(batch, order=order, walk=walk, sub_bytes=sub_bytes)
    return frames.view(N, Ts, batch.height, batch.width, 3), batch.present.reshape(N, Ts), status
