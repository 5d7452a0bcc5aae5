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

pack is per-batch host work (header walks, marker scans, table builds, one concatenation) and nothing it computes depends on the batch.
The resident store does it once for a whole set of videos and cuts a batch from the device:

  frame_records   every file of a set read and parsed ONCE -> FrameRecords: per-frame rows, the set's tables, the scan bytes in chunks
  plan_frames     a batch of windows (video, start[, track_len]) -> FramePlan: the decode's int table, the gather table, frame_idx;
                  host validation and vectorised indexing only
  gather_host     the gather in numpy (the kernel's oracle); gather: m3t_jpeg_gather (csrc/frame_store.hip) as it is
  FrameStore      the chunks on the device; decode(items) -> (frames [N, window, H, W, 3], frame_idx, status): plan_frames, one small
                  upload, one device-to-device gather, the decode above; batches(items, batch_size)

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
    dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        tables = np.ascontiguousarray(tables, np.int32)
        t_d = torch.from_numpy(tables).to(dev, non_blocking=True)
        s_d = batch.stream.to(dev, non_blocking=True)
        status, walk_stats = _decode_on_device(s_d, tables, t_d, (n, batch.n_segs, batch.n_quant, batch.n_huff, H, W), out, dst_slots, order,
                                               (walk_i, sub_i, min_i, max_i), stats, dev)
    return (out, status, walk_stats) if stats else (out, status)


def _decode_on_device(s_d, tables_h, tables_d, counts, out, dst_slots, order, walk_ints, stats, dev):
    """The one call of m3t_jpeg_decode_walk (decode and FrameStore.decode share it): the stream s_d and the int table (host array and device
    tensor, the same ints) are on `dev`, the current device; -> (status int32 [n], walk_stats int32 [n_segs, 2] or None), on the current stream."""
    n, n_segs, n_quant, n_huff, H, W = counts
    lib = _lib.load()
    ws_bytes = int(lib.m3t_jpeg_workspace_bytes(n, H, W))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    walk_stats = torch.empty(n_segs, 2, dtype=torch.int32, device=dev) if stats else None
    _lib.check(lib.m3t_jpeg_decode_walk(s_d.data_ptr(), s_d.numel(), tables_h.ctypes.data, tables_d.data_ptr(), n, n_segs, n_quant, n_huff, H, W,
                                        out.data_ptr(), dst_slots, 0 if order == "bgr" else 1, ws.data_ptr(), ws_bytes, status.data_ptr(),
                                        *walk_ints, walk_stats.data_ptr() if stats and n_segs else None, _stream()), "m3t_jpeg_decode_walk")
    return status, walk_stats


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


# ---- the resident frame store -----------------------------------------------------------------------------------------------------------
# Nothing pack computes depends on the batch: a file's header, tables, segment list and scan bytes are the same in every epoch.  So they are
# found ONCE (frame_records), the scan bytes stay on the device (FrameStore), and a batch of windows is a few vectorised index operations
# on the host (plan_frames), one device-to-device gather (m3t_jpeg_gather, csrc/frame_store.hip) and the decode as it is.
GATHER_COLS = 4                     # chunk, source offset, destination offset, bytes (include/m3t_hip.h)
STREAM_MAX = 2 ** 31 - 1 - 2048     # the largest stream m3t_jpeg_decode_walk takes: its segment offsets are `int` (csrc/jpeg_core.h)
_READ_AHEAD = 256                   # files in flight between the reader threads and the parser


def _excl_cumsum(a):
    out = np.zeros(a.shape[0], np.int64)
    np.cumsum(a[:-1], out=out[1:])
    return out


class FrameRecords:
    """What frame_records found, per frame f of the whole set (the videos' frames one after the other, video v at video_off[v] ..
    video_off[v + 1]):
      present bool [F]; chunk int32 [F], offset int64 [F] (a multiple of 16), nbytes int32 [F]: where the frame's scan lies;
      images  int32 [F, 16]: pack's row -- flags, components, luma h, luma v, MCUs per segment, 0, segments, then the quantisation, DC and
              AC table of each component as indices into `quant` / `huff` (the set's tables, deduplicated by content);
      seg_row int64 [F]: the frame's first row of segs int32 [S, 3] = offset relative to the frame's scan, length, restart marker;
      quant   int32 [Q, 32], huff int32 [Hf, 384]: pack's lookup forms;
      chunk_sizes int64 [C]; chunks: the host chunks (uint8 arrays), or None where every chunk was handed on as it filled;
      names, height, width, chunk_bytes."""
    __slots__ = ("names", "index", "video_off", "present", "chunk", "offset", "nbytes", "images", "seg_row", "segs", "quant", "huff",
                 "chunk_sizes", "chunks", "height", "width", "chunk_bytes")

    def _video(self, video):
        if isinstance(video, str):
            if video not in self.index:
                raise ValueError("frame store: unknown video %r" % (video,))
            return self.index[video]
        v = int(video)
        if not 0 <= v < len(self.names):
            raise ValueError("frame store: unknown video %d (the store holds %d)" % (v, len(self.names)))
        return v

    def has_image(self, video):
        """bool [frames of the video]: what TrackStore's videos[name]['has_image'] takes"""
        v = self._video(video)
        return self.present[self.video_off[v]:self.video_off[v + 1]].copy()

    @property
    def n_frames(self):
        return int(self.video_off[-1])


def frame_records(videos, chunk_bytes=1 << 30, on_unsupported="raise", threads=8, _sink=None):
    """videos: an ordered mapping name -> a sequence of `bytes`, a path or None, one entry per frame (frame i is the reference's
    '{:05d}.jpg'.format(i + 1)) -> FrameRecords.  Host only.  Every file is read (by a pool of `threads` threads, at most 16) and parsed
    exactly once.  The scan bytes go into chunks: a frame's scan starts on a 16-byte boundary and is zero padded to one, never straddles a
    chunk, a chunk holds at most chunk_bytes (a multiple of 16 below 2^31), a single frame larger than that gets a chunk of its own.  A
    missing file or None is an absent frame; a file parse refuses raises Unsupported with the video and the frame in front of the reason
    (on_unsupported="raise") or is an absent frame ("absent").  ValueError (naming the video and frame) where two frames differ in size,
    and for a set without a single frame to decode.
    _sink(index, chunk): called with every chunk as it fills (a view of the staging buffer, valid during the call); the records then keep
    no chunk, and the host memory held at any time is one chunk and the tables (FrameStore uploads through it)."""
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes <= 0 or chunk_bytes % 16 or chunk_bytes >= 2 ** 31:
        raise ValueError("frame_records: chunk_bytes must be a positive multiple of 16 below 2^31")
    if on_unsupported not in ("raise", "absent"):
        raise ValueError("frame_records: on_unsupported must be 'raise' or 'absent'")
    names = list(videos)
    if not names:
        raise ValueError("frame_records: no videos")
    counts = [len(videos[nm]) for nm in names]
    F = int(sum(counts))
    r = FrameRecords()
    r.names, r.index, r.chunk_bytes = names, {nm: i for i, nm in enumerate(names)}, chunk_bytes
    r.video_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    r.present = np.zeros(F, bool)
    r.chunk, r.offset, r.nbytes = np.zeros(F, np.int32), np.zeros(F, np.int64), np.zeros(F, np.int32)
    r.images, r.seg_row = np.zeros((F, IMG_COLS), np.int32), np.zeros(F, np.int64)
    quants, huffs, qrows, hrows = {}, {}, [], []

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

    stage = np.zeros(min(chunk_bytes, 1 << 20), np.uint8)      # grows to one chunk; zero wherever no scan byte has been written
    pos, sizes, kept, segs, n_segs, size, first = 0, [], None if _sink else [], [], 0, None, None

    def flush():
        nonlocal pos
        if pos == 0:
            return
        if _sink:
            _sink(len(sizes), stage[:pos])
        else:
            kept.append(stage[:pos].copy())
        sizes.append(pos)
        stage[:pos] = 0
        pos = 0

    def entries():
        for v, nm in enumerate(names):
            for i, it in enumerate(videos[nm]):
                yield v, i, it

    with ThreadPoolExecutor(max(1, min(int(threads), 16))) as pool:
        todo, f = entries(), 0
        while True:
            group = [e for _, e in zip(range(_READ_AHEAD), todo)]
            if not group:
                break
            for (v, i, _), data in zip(group, pool.map(_read, [e[2] for e in group])):
                f += 1
                if data is None:
                    continue
                try:
                    h = parse(data)
                except Unsupported as e:
                    if on_unsupported == "absent":
                        continue
                    raise Unsupported("video %r, frame %d: %s" % (names[v], i, e)) from None
                if size is None:
                    size, first = (h.height, h.width), (names[v], i)
                if (h.height, h.width) != size:
                    raise ValueError("frame_records: video %r, frame %d is %d x %d; the frames of a store share one size, and video %r, "
                                     "frame %d is %d x %d" % ((names[v], i, h.height, h.width) + first + size))
                scan = np.frombuffer(data, np.uint8, count=h.scan_end - h.scan_offset, offset=h.scan_offset)
                padded = (scan.size + 15) // 16 * 16
                if pos and pos + padded > chunk_bytes:
                    flush()
                if pos + padded > stage.size:                   # grow towards one chunk; past it only for a single oversize frame
                    if padded >= 2 ** 31:
                        raise ValueError("frame_records: video %r, frame %d: a scan of %d bytes" % (names[v], i, scan.size))
                    grown = np.zeros(max(pos + padded, min(2 * stage.size, chunk_bytes)), np.uint8)
                    grown[:pos] = stage[:pos]
                    stage = grown
                stage[pos:pos + scan.size] = scan
                # the segments, exactly as pack finds them
                mcus = h.mcus
                ri = h.restart_interval if 0 < h.restart_interval < mcus else mcus
                want = -(-mcus // ri)
                at = np.flatnonzero((scan[:-1] == 0xFF) & ((scan[1:] & 0xF8) == 0xD0)) if scan.size > 1 else np.zeros(0, np.int64)
                rows = np.empty((want, 3), np.int32)
                rows[:] = (scan.size, 0, -2)
                found = at.size + 1
                k = min(found, want)
                rows[:k, 0] = np.concatenate([[0], at + 2])[:k]
                rows[:k, 1] = (np.concatenate([at, [scan.size]]) - np.concatenate([[0], at + 2]))[:k]
                rows[:k, 2] = np.concatenate([[-1], scan[at + 1] & 7])[:k]
                g = f - 1
                r.present[g], r.chunk[g], r.offset[g], r.nbytes[g], r.seg_row[g] = True, len(sizes), pos, scan.size, n_segs
                r.images[g, :7] = (1 | (2 if found != want else 0), h.components, h.hs, h.vs, ri, 0, want)
                for c in range(h.components):
                    r.images[g, 7 + c], r.images[g, 10 + c], r.images[g, 13 + c] = q_index(h.quant[c]), h_index(h.dc[c]), h_index(h.ac[c])
                segs.append(rows)
                n_segs += want
                pos += padded
                if padded > chunk_bytes:
                    flush()
    flush()
    if size is None:
        raise ValueError("frame_records: no frame of the set can be decoded, the store has no size")
    r.segs = np.concatenate(segs).astype(np.int32, copy=False) if segs else np.zeros((0, 3), np.int32)
    r.quant = np.stack(qrows).astype(np.int32, copy=False)
    r.huff = np.stack(hrows).astype(np.int32, copy=False)
    r.chunk_sizes, r.chunks = np.asarray(sizes, np.int64), kept
    r.height, r.width = size
    return r


class FramePlan:
    """What plan_frames made of a batch.  N, window, n = N window; tables: the ONE int table of m3t_jpeg_decode_walk (JpegBatch's layout,
    slots the identity) with n_segs, n_quant, n_huff; rows: the gather table int32 [m, 4]; stream_bytes; frame_idx int32 [N, window];
    present bool [n]; height, width."""
    __slots__ = ("N", "window", "n", "tables", "n_segs", "n_quant", "n_huff", "rows", "stream_bytes", "frame_idx", "present", "height", "width")

    def batch(self, stream):
        """-> the JpegBatch this plan describes over `stream`, the gathered bytes (a uint8 host tensor or array of stream_bytes)"""
        stream = stream if isinstance(stream, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(stream, np.uint8))
        if stream.dtype != torch.uint8 or stream.numel() != self.stream_bytes:
            raise ValueError("FramePlan.batch: the stream must be %d uint8" % self.stream_bytes)
        b = JpegBatch()
        b.stream, b.tables = stream, self.tables
        b.n, b.n_segs, b.n_quant, b.n_huff, b.height, b.width = self.n, self.n_segs, self.n_quant, self.n_huff, self.height, self.width
        b.present, b.headers = self.present, [None] * self.n
        return b


def plan_frames(records, items, window):
    """Host validation of a batch of windows over a FrameRecords, before anything touches a device -> FramePlan.  items: [(video, start[,
    track_len])], video an index or a name, track_len = window when left out (dataset.plan's items).  Image n window + t is frame start + t
    of item n; a slot past track_len or an absent frame is an absent image (the decode zero-fills it).  ValueError: an unknown video, a
    negative start, track_len outside [1, window], start + track_len past the video's frames, a batch whose gathered bytes would not fit
    the decode's `int` offsets.  Everything per frame and per segment is vectorised indexing; only the items are walked."""
    window = int(window)
    if window <= 0:
        raise ValueError("plan_frames: window must be positive, got %r" % (window,))
    N = len(items)
    tab = np.zeros((N, 3), np.int64)
    for n, it in enumerate(items):
        if len(it) not in (2, 3):
            raise ValueError("plan_frames: item %d: expected (video, start[, track_len]), got %r" % (n, it))
        try:
            v = records._video(it[0])
        except ValueError as e:
            raise ValueError("plan_frames: item %d: %s" % (n, e)) from None
        start, tl = int(it[1]), window if len(it) == 2 else int(it[2])
        frames = int(records.video_off[v + 1] - records.video_off[v])
        if start < 0:
            raise ValueError("plan_frames: item %d: start %d is negative" % (n, start))
        if not 1 <= tl <= window:
            raise ValueError("plan_frames: item %d: track_len %d outside [1, %d]" % (n, tl, window))
        if start + tl > frames:
            raise ValueError("plan_frames: item %d: frames %d .. %d run past the %d frames of %s"
                             % (n, start, start + tl - 1, frames, records.names[v]))
        tab[n] = (v, start, tl)
    p = FramePlan()
    p.N, p.window, p.n, p.height, p.width = N, window, N * window, records.height, records.width
    t = np.arange(window, dtype=np.int64)
    inside = t[None, :] < tab[:, 2:3]
    frame = np.where(inside, records.video_off[tab[:, 0]][:, None] + tab[:, 1:2] + t[None, :], 0)
    p.present = (inside & records.present[frame]).reshape(-1)
    idx = np.flatnonzero(p.present)                              # the images to decode, and the frames behind them
    fr = frame.reshape(-1)[idx]
    nbytes = (records.nbytes[fr].astype(np.int64) + 15) // 16 * 16
    to = _excl_cumsum(nbytes)
    p.stream_bytes = int(nbytes.sum()) + 16
    if p.stream_bytes > STREAM_MAX:
        raise ValueError("plan_frames: the batch gathers %d bytes; the decode's segment offsets are int, at most %d" % (p.stream_bytes, STREAM_MAX))
    p.rows = np.stack([records.chunk[fr].astype(np.int64), records.offset[fr], to, nbytes], axis=1).astype(np.int32).reshape(-1, GATHER_COLS)
    images = np.zeros((p.n, IMG_COLS), np.int32)
    img = records.images[fr]                                     # (a copy: fancy indexing)
    n_seg = img[:, 6].astype(np.int64)
    seg0 = _excl_cumsum(n_seg)
    p.n_segs = int(n_seg.sum())
    img[:, 5] = seg0
    src = np.repeat(records.seg_row[fr] - seg0, n_seg) + np.arange(p.n_segs, dtype=np.int64)
    segs = np.empty((p.n_segs, SEG_COLS), np.int32)
    segs[:, 0] = np.repeat(idx, n_seg)
    segs[:, 1] = records.segs[src, 0] + np.repeat(to, n_seg)      # rebased to the batch stream
    segs[:, 2:] = records.segs[src, 1:]
    comp = np.arange(3)[None, :] < img[:, 1:2]                   # the table columns an image names: one per component
    for cols, name, store in ((slice(7, 10), "n_quant", records.quant), (slice(10, 16), "n_huff", records.huff)):
        named = comp if name == "n_quant" else np.concatenate([comp, comp], axis=1)
        used = np.unique(img[:, cols][named])
        img[:, cols] = np.where(named, np.searchsorted(used, img[:, cols]), 0)
        setattr(p, name, int(used.size))
        if name == "n_quant":
            quant = store[used]
        else:
            huff = store[used]
    images[idx] = img
    p.tables = np.concatenate([images.reshape(-1), segs.reshape(-1), np.arange(p.n, dtype=np.int32), quant.reshape(-1),
                               huff.reshape(-1)]).astype(np.int32, copy=False)
    from . import video                                          # (here: m3t.video loads the operator layer, which parse and pack do without)
    rows = []
    for v, start, tl in tab:
        present = records.present[records.video_off[v]:records.video_off[v + 1]]
        rows.append(video.frame_index(present[start:start + tl], 0, int(tl), window))
    p.frame_idx = np.stack(rows).astype(np.int32) if rows else np.zeros((0, window), np.int32)
    return p


def gather_host(chunks, rows, stream_bytes):
    """m3t_jpeg_gather in numpy: the host chunks (FrameRecords.chunks) and a gather table -> the batch stream, uint8 [stream_bytes].
    The kernel's oracle, and what hands a store-built batch to csrc/jpeg_host_check.cpp."""
    out = np.zeros(int(stream_bytes), np.uint8)
    for chunk, src, to, nbytes in np.asarray(rows, np.int64).reshape(-1, GATHER_COLS):
        part = np.asarray(chunks[chunk][src:src + nbytes])
        if part.size != nbytes or to < 0 or to + nbytes > out.size - 16:
            raise ValueError("gather_host: row (%d, %d, %d, %d) does not fit" % (chunk, src, to, nbytes))
        out[to:to + nbytes] = part
    return out


def gather(chunks, rows, dst, dst_bytes=None):
    """m3t_jpeg_gather as it is: chunks, a list of uint8 device tensors; rows, int32 [m, 4]; dst, a uint8 device tensor of which the first
    dst_bytes (default: all) are written, on the current stream.  M3THipError for whatever the entry point refuses."""
    if not torch.cuda.is_available():
        raise M3THipError("m3t.jpeg needs the GPU: the M3T path has no CPU fallback")
    rows = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, GATHER_COLS))
    addr = np.array([c.data_ptr() for c in chunks], np.int64)
    size = np.array([c.numel() for c in chunks], np.int64)
    addr_d = torch.from_numpy(addr).to(dst.device) if len(chunks) else None
    rows_d = torch.from_numpy(rows.reshape(-1)).to(dst.device) if rows.size else None
    _lib.check(_lib.load().m3t_jpeg_gather(addr.ctypes.data, size.ctypes.data, len(chunks), addr_d.data_ptr() if len(chunks) else None,
                                           rows.ctypes.data, rows_d.data_ptr() if rows.size else None, rows.shape[0], dst.data_ptr(),
                                           dst.numel() if dst_bytes is None else int(dst_bytes), _stream()), "m3t_jpeg_gather")
    return dst


class FrameStore:
    """The scan bytes of a set of videos' JPEG frames on the current device, and the decode of a batch of windows from them.

    videos: frame_records' mapping; window: frames per item.  The files are read and parsed once, here; each chunk is uploaded as it fills
    through one pinned staging buffer and stays on the device.  decode(items) costs the host plan_frames and two small copies.
    There is no CPU path.  Out of scope: a disk cache of the parsed store, a host-resident arena for a corpus that does not fit the device,
    prefetch threads and DDP sharding, the file-system scan that produces `videos`, frames of different sizes in one store."""

    def __init__(self, videos, window, chunk_bytes=1 << 30, on_unsupported="raise", threads=8):
        self.window = int(window)
        if self.window <= 0:
            raise ValueError("FrameStore: window must be positive")
        if not torch.cuda.is_available():
            raise M3THipError("m3t.jpeg.FrameStore needs the GPU: the M3T path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.chunks, staging = [], [None]

        def upload(index, chunk):
            if staging[0] is None or staging[0].numel() < chunk.size:
                staging[0] = torch.empty(chunk.size, dtype=torch.uint8).pin_memory()
            staging[0].numpy()[:chunk.size] = chunk
            self.chunks.append(staging[0][:chunk.size].to(self.device, non_blocking=True))
            torch.cuda.current_stream().synchronize()           # the staging buffer is written again for the next chunk

        self.records = frame_records(videos, chunk_bytes, on_unsupported, threads, _sink=upload)
        self.names, self.height, self.width = self.records.names, self.records.height, self.records.width
        self._addr = np.array([c.data_ptr() for c in self.chunks], np.int64)
        self._size = np.array([c.numel() for c in self.chunks], np.int64)
        self._addr_d = torch.from_numpy(self._addr).to(self.device)

    @property
    def nbytes(self):
        """bytes of device memory the store holds"""
        return int(self._size.sum()) + 8 * len(self.chunks)

    def has_image(self, video):
        """bool [frames of the video]: what TrackStore's videos[name]['has_image'] takes"""
        return self.records.has_image(video)

    def decode(self, items, out=None, order="bgr", walk="auto", sub_bytes=None, par_min_bytes=None, par_max_bytes=None, stats=False):
        """items: [(video, start[, track_len])] -> (frames, frame_idx, status[, walk_stats]).  frames: uint8 [N, window, H, W, 3] on the
        store's device (`out`, filled, where one of that shape is given): frame start + t of item n at [n, t], zeros where that frame is
        absent or t >= track_len.  frame_idx: int32 [N, window] host tensor, video.frame_index per item: batch['video_frame_idx'] and what
        video.ingest takes.  status: int32 [N window] on the device, jpeg.decode's.  order, walk, sub_bytes, par_min_bytes, par_max_bytes,
        stats: jpeg.decode's.  plan_frames first (ValueError), then on the current stream and without a host synchronisation: one upload
        of the two small tables, m3t_jpeg_gather into a fresh stream buffer, m3t_jpeg_decode_walk."""
        if order not in ("bgr", "rgb"):
            raise ValueError("FrameStore.decode: order must be 'bgr' or 'rgb'")
        walk_ints = _walk_args(walk, sub_bytes, par_min_bytes, par_max_bytes)
        p = plan_frames(self.records, items, self.window)
        H, W, dev = self.height, self.width, self.device
        if torch.cuda.current_device() != dev.index:
            raise M3THipError("FrameStore.decode: the store lives on %s, the current device is cuda:%d" % (dev, torch.cuda.current_device()))
        shape = (p.N, p.window, H, W, 3)
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == shape):
                raise ValueError("FrameStore.decode: out must be uint8 %s" % (list(shape),))
            if not (out.is_cuda and out.device == dev and out.is_contiguous()):
                raise M3THipError("FrameStore.decode: out must be a contiguous tensor on %s" % (dev,))
        frame_idx = torch.from_numpy(p.frame_idx)
        m = int(p.rows.shape[0])
        if m == 0:                                              # nothing to decode: zeros, without a launch of the decode
            out = torch.zeros(shape, dtype=torch.uint8, device=dev) if out is None else out.zero_()
            status = torch.zeros(p.n, dtype=torch.int32, device=dev)
            return (out, frame_idx, status, torch.zeros(0, 2, dtype=torch.int32, device=dev)) if stats else (out, frame_idx, status)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        both = np.concatenate([p.rows.reshape(-1), p.tables])   # the gather's rows in front: 16 bytes each, the table behind them aligned
        both_d = torch.from_numpy(both).to(dev, non_blocking=True)
        rows_h, tables_h = both[:m * GATHER_COLS], both[m * GATHER_COLS:]
        s_d = torch.empty(p.stream_bytes, dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().m3t_jpeg_gather(self._addr.ctypes.data, self._size.ctypes.data, len(self.chunks), self._addr_d.data_ptr(),
                                               rows_h.ctypes.data, both_d.data_ptr(), m, s_d.data_ptr(), p.stream_bytes, _stream()),
                   "m3t_jpeg_gather")
        status, walk_stats = _decode_on_device(s_d, tables_h, both_d[m * GATHER_COLS:], (p.n, p.n_segs, p.n_quant, p.n_huff, H, W), out, p.n,
                                               order, walk_ints, stats, dev)
        return (out, frame_idx, status, walk_stats) if stats else (out, frame_idx, status)

    def batches(self, items, batch_size):
        """decode() over consecutive slices of `items`; the last one may be short"""
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batches: batch_size must be positive")
        for i in range(0, len(items), batch_size):
            yield self.decode(items[i:i + batch_size])
