"""The JPEG fixtures and the damaged streams shared by tests/test_jpeg_host.py, tests/test_jpeg_par_host.py and tests/test_gpu_jpeg*.py
(tests/golden/jpeg_cases.npz, written by tests/golden/gen_golden_jpeg.py), the packed-batch file csrc/jpeg_host_check.cpp -- the one host
program, which runs the kernels' text for both walks, the workgroup's schedule included -- reads, and the rule the tests hold a damaged
stream's result to."""
import functools
import struct

import numpy as np

from conftest import load_golden
import jpeg_ref

FAMILY = ["f_420_q95", "f_444_q60", "f_422_q85", "f_gray_q80", "f_opt_q90", "f_rst_blocks2", "f_rst_rows1_q100", "f_sat_q50"]
MAGIC = 0x4A504731
CANARY = 0xA5


@functools.lru_cache(None)
def load():
    """-> (cases {name: (bytes, rgb uint8 [H, W, 3])}, refusals {name: bytes})"""
    d = load_golden("jpeg_cases")
    cases = {k[:-4]: (d[k].tobytes(), d[k[:-4] + ".rgb"]) for k in d if k.endswith(".jpg") and not k.startswith("refuse_")}
    refusals = {k[:-4]: d[k].tobytes() for k in d if k.startswith("refuse_")}
    return cases, refusals


def header_segments(data):
    """[(marker, start, end)] of the segments in front of the scan, SOS included (end: one past the segment)"""
    out, p = [], 2
    while True:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + n))
        if m == 0xDA:
            return out
        p += 2 + n


def split(data):
    """(head, scan, tail): everything through the SOS header, the entropy-coded bytes with their restart markers, the EOI"""
    start = header_segments(data)[-1][2]
    assert data[-2:] == b"\xff\xd9"
    return data[:start], data[start:-2], data[-2:]


@functools.lru_cache(None)
def damaged():
    """The fixed-seed set of damaged streams: [(name, kind, bytes, base case)], kind in trunc / flip / rst.  Built from the 40 x 56 4:2:0
    case and the restart case: truncations of the scan at 16 offsets (+ 4 of the restart case), 200 single-byte flips inside the scan,
    one removed and one swapped RSTn.  A flip that turns two bytes into a marker other than RSTn makes the FILE one the host refuses
    (jpeg.Unsupported: it reads as a second scan or a missing EOI); such a draw is counted and drawn again, so 200 reach the decoder."""
    from m3t import jpeg
    cases, _ = load()
    out = []
    for base, n_trunc in (("f_420_q95", 16), ("f_rst_blocks2", 4)):
        head, scan, tail = split(cases[base][0])
        for k in np.linspace(1, len(scan) - 2, n_trunc).astype(int):
            out.append(("%s_trunc%d" % (base, k), "trunc", head + scan[:k] + tail, base))
    rs = np.random.RandomState(20250)
    refused = 0
    for base in ("f_420_q95", "f_rst_blocks2"):
        head, scan, tail = split(cases[base][0])
        done = 0
        while done < 100:
            k, bit = int(rs.randint(len(scan))), int(rs.randint(8))
            b = bytearray(scan)
            b[k] ^= 1 << bit
            data = head + bytes(b) + tail
            try:
                jpeg.parse(data)
            except jpeg.Unsupported:
                refused += 1
                continue
            out.append(("%s_flip%d_%d" % (base, k, bit), "flip", data, base))
            done += 1
    assert refused < 20, refused
    head, scan, tail = split(cases["f_rst_blocks2"][0])
    at = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert len(at) >= 3
    out.append(("rst_removed", "rst", head + scan[:at[1]] + scan[at[1] + 2:] + tail, "f_rst_blocks2"))
    b = bytearray(scan)
    b[at[0] + 1], b[at[1] + 1] = b[at[1] + 1], b[at[0] + 1]
    out.append(("rst_swapped", "rst", head + bytes(b) + tail, "f_rst_blocks2"))
    return out


def damaged_batch():
    """-> (items, names): the damaged streams with an undamaged neighbour in front of, between every 8 of, and behind them"""
    cases, _ = load()
    items, names = [], []
    for j, (name, kind, data, base) in enumerate(damaged()):
        if j % 8 == 0:
            items.append(cases[FAMILY[(j // 8) % len(FAMILY)]][0])
            names.append(FAMILY[(j // 8) % len(FAMILY)])
        items.append(data)
        names.append(name)
    items.append(cases["f_420_q95"][0])
    names.append("f_420_q95")
    return items, names


@functools.lru_cache(None)
def _ref_of_damaged(name):
    data = {d[0]: d[2] for d in damaged()}[name]
    try:
        return jpeg_ref.decode(data)[0]
    except jpeg_ref.DecodeError:
        return None


def check_damaged_result(names, rgb, status):
    """rgb uint8 [n, H, W, 3], status int [n] of damaged_batch() as some decoder gave them.  The rule:
      * an undamaged neighbour is exact with status 0;
      * a truncated stream and a stream with a removed or swapped RSTn have a non-zero status;
      * wherever the pixels of a flipped stream differ from the golden, the status is non-zero -- except where the flip left a complete,
        valid stream (a bit of a coefficient's value, say), which no decoder can tell from an intact one: there the pixels must be exactly
        what the numpy restatement makes of the damaged file.
    Returns the number of streams in each class, for the callers' sanity checks."""
    cases, _ = load()
    kinds = {d[0]: (d[1], d[3]) for d in damaged()}
    count = {"neighbour": 0, "flagged": 0, "unchanged": 0, "valid": 0}
    for i, name in enumerate(names):
        if name not in kinds:
            assert status[i] == 0 and np.array_equal(rgb[i], cases[name][1]), "neighbour %d (%s)" % (i, name)
            count["neighbour"] += 1
            continue
        kind, base = kinds[name]
        if kind in ("trunc", "rst"):
            assert status[i] != 0, name
        if status[i] != 0:
            count["flagged"] += 1
        elif np.array_equal(rgb[i], cases[base][1]):
            count["unchanged"] += 1
        else:
            ref = _ref_of_damaged(name)
            assert ref is not None and np.array_equal(rgb[i], ref), "%s: pixels differ from the golden with status 0" % name
            count["valid"] += 1
    return count


def write_packed(path, batch, slots, dst_slots, order):
    """the input file of csrc/jpeg_host_check.cpp"""
    from m3t import jpeg
    tables = batch.tables.copy()
    o = batch.n * jpeg.IMG_COLS + batch.n_segs * jpeg.SEG_COLS
    tables[o:o + batch.n] = slots
    stream = batch.stream.numpy().tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<12i", MAGIC, batch.n, batch.n_segs, batch.n_quant, batch.n_huff, batch.height, batch.width,
                            {"bgr": 0, "rgb": 1}[order], dst_slots, len(stream), 0, 0))
        f.write(tables.astype("<i4").tobytes())
        f.write(stream)


def read_result(path, n, dst_slots, H, W):
    raw = np.fromfile(path, np.uint8)
    status = raw[:4 * n].view("<i4").astype(np.int64)
    return status, raw[4 * n:].reshape(dst_slots, H, W, 3)
