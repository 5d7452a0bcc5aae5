"""The JPEG decoder without a GPU (m3t/jpeg.py: parse, pack; csrc/jpeg_core.h compiled for the host by csrc/jpeg_host_check.cpp): the numpy
restatement of the rules (tests/jpeg_ref.py) against the goldens and a live Pillow, the header walk and the packed tables, every refusal,
and the device code's text run on the host -- every golden bit for bit, and the fixed-seed damaged streams with guard bytes around
everything it writes."""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref
from m3t import jpeg, _lib

CASES, REFUSALS = jpeg_cases.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_golden(name):
    data, rgb = CASES[name]
    assert np.array_equal(jpeg_ref.decode(data)[0], rgb)


def test_restatement_equals_a_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(77)
    for (h, w), kw in (((23, 37), dict(quality=75, subsampling=2)), ((24, 40), dict(quality=92, subsampling=1, optimize=True)),
                       ((9, 11), dict(quality=50, subsampling=0)), ((33, 18), dict(quality=88, subsampling=2, restart_marker_blocks=3))):
        arr = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        arr[h // 2:] = np.linspace(0, 255, w).astype(np.uint8)[None, :, None]
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "JPEG", **kw)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        assert np.array_equal(jpeg_ref.decode(buf.getvalue())[0], want), kw


@pytest.mark.parametrize("name", sorted(CASES))
def test_parse_fields(name):
    data, rgb = CASES[name]
    h = jpeg.parse(data)
    ref = jpeg_ref.read_header(data)
    assert (h.height, h.width) == rgb.shape[:2] == (ref["H"], ref["W"])
    assert h.components == len(ref["comps"])
    if "gray" in name:
        assert h.mode == "gray"
    elif "444" in name:
        assert h.mode == "444"
    elif "422" in name:
        assert h.mode == "422" and (h.hs, h.vs) == (2, 1)
    else:
        assert h.mode == "420" and (h.hs, h.vs) == (2, 2)
    assert h.restart_interval == ref["ri"] and (h.restart_interval > 0) == ("rst" in name)
    head, scan, tail = jpeg_cases.split(data)
    assert data[h.scan_offset:h.scan_end] == scan
    for c in range(h.components):
        assert list(h.quant[c]) == ref["quant"][ref["comps"][c][3]]
        for cls, tabs in ((0, h.dc), (1, h.ac)):
            table = ref["huff"][(cls, ref["tabs"][c][cls])]
            assert int(tabs[c][0].sum()) == len(table) == len(tabs[c][1])


def _walk_lookup(row, length, code):
    """the symbol the lookup form gives for one code, the way csrc/jpeg_core.h reads it"""
    lut = row[:256].view(np.uint16)
    v = code << (16 - length)
    e = int(lut[v >> 7])
    if e:
        return e >> 8, e & 255
    for ln in range(10, 17):
        c = v >> (16 - ln)
        if c <= row[256 + ln]:
            return ln, int(row[292:356].view(np.uint8)[(row[274 + ln] + c) & 255])
    return None


@pytest.mark.parametrize("name", ["f_420_q95", "f_opt_q90"])
def test_huffman_lookup_form(name):
    data = CASES[name][0]
    h = jpeg.parse(data)
    ref = jpeg_ref.read_header(data)
    for c in range(h.components):
        for cls, tabs in ((0, h.dc), (1, h.ac)):
            row = jpeg.huff_lookup(*tabs[c])
            for (length, code), sym in ref["huff"][(cls, ref["tabs"][c][cls])].items():
                assert _walk_lookup(row, length, code) == (length, sym)
    assert _walk_lookup(jpeg.huff_lookup(*h.ac[0]), 16, 0xFFFF) is None          # the all-ones pattern is no code


def test_pack_restart_segments():
    for name in ("f_rst_blocks2", "f_rst_rows1_q100", "f_420_q95"):
        data = CASES[name][0]
        b = jpeg.pack([data])
        h = jpeg.parse(data)
        ri = h.restart_interval or h.mcus
        assert b.n_segs == -(-h.mcus // ri) and tuple(b.images[0, :7]) == (1, h.components, h.hs, h.vs, ri, 0, b.n_segs)
        stream = b.stream.numpy().tobytes()
        assert len(stream) % 16 == 0
        rebuilt = b""
        for k, (img, off, ln, mark) in enumerate(b.segments):
            assert img == 0 and mark == (-1 if k == 0 else (k - 1) & 7)
            rebuilt += (b"" if k == 0 else bytes([0xFF, 0xD0 + mark])) + stream[off:off + ln]
            assert b"\xff\xd0" not in stream[off:off + ln]
        assert rebuilt == data[h.scan_offset:h.scan_end]


def test_pack_deduplicates_tables_over_a_mixed_batch():
    items = [CASES[n][0] for n in jpeg_cases.FAMILY] + [None, CASES["f_420_q95"][0]]
    b = jpeg.pack(items)
    assert (b.height, b.width, b.n) == (40, 56, 10) and list(b.present) == [True] * 8 + [False, True]
    quants, huffs = set(), set()
    for it in items:
        if it is None:
            continue
        ref = jpeg_ref.read_header(it)
        for c, comp in enumerate(ref["comps"]):
            quants.add(tuple(ref["quant"][comp[3]]))
            for cls in (0, 1):
                huffs.add((cls, tuple(sorted(ref["huff"][(cls, ref["tabs"][c][cls])].items()))))
    assert b.n_quant == len(quants) and b.n_huff == len(huffs)
    assert tuple(b.images[8]) == (0,) * 16 and np.array_equal(b.images[9, 7:], b.images[0, 7:])
    assert list(b.slots) == list(range(10))
    two = jpeg.pack([CASES["f_420_q95"][0]] * 5)                                 # a dataset batch: two quantisation, four Huffman tables
    assert (two.n_quant, two.n_huff) == (2, 4)
    nat = np.zeros(64, np.int64)
    nat[jpeg_ref.ZIGZAG] = jpeg_ref.read_header(items[0])["quant"][0]
    assert np.array_equal(two.quant[two.images[0, 7]], nat)
    with pytest.raises(ValueError, match="share one size"):
        jpeg.pack([CASES["f_420_q95"][0], CASES["e_16x16_420"][0]])
    with pytest.raises(ValueError):
        jpeg.pack([None, None])
    with pytest.raises(ValueError):
        jpeg.pack([])


def _patch(data, marker, offset, value, nth=0):
    """set body byte `offset` of the nth segment with this marker"""
    seg = [s for s in jpeg_cases.header_segments(data) if s[0] == marker][nth]
    b = bytearray(data)
    b[seg[1] + 4 + offset] = value
    return bytes(b)


def _without(data, marker, nth=0):
    seg = [s for s in jpeg_cases.header_segments(data) if s[0] == marker][nth]
    return data[:seg[1]] + data[seg[2]:]


def _as_marker(data, marker, new):
    seg = [s for s in jpeg_cases.header_segments(data) if s[0] == marker][0]
    b = bytearray(data)
    b[seg[1] + 1] = new
    return bytes(b)


def test_every_refusal_names_its_reason():
    base = CASES["f_420_q95"][0]
    sos = [s for s in jpeg_cases.header_segments(base) if s[0] == 0xDA][0]
    refusals = [
        (REFUSALS["refuse_progressive"], "progressive"),
        (REFUSALS["refuse_cmyk"], "4 components"),
        (_patch(_as_marker(base, 0xC0, 0xC1), 0xC1, 0, 12), "12-bit"),
        (_as_marker(base, 0xC0, 0xC1), "extended"),
        (_as_marker(base, 0xC0, 0xC3), "lossless"),
        (_as_marker(base, 0xC0, 0xC9), "arithmetic"),
        (_patch(base, 0xC0, 0, 12), "12-bit"),
        (_patch(base, 0xDB, 0, 0x10), "16-bit quantisation"),
        (_patch(base, 0xC0, 7, 0x41), "sampling factors"),
        (_patch(base, 0xC0, 10, 0x21), "sampling factors"),
        (base[:-2] + base[sos[1]:sos[2]] + b"\x00" + base[-2:], "multiple scans"),
        (_without(base, 0xDB, 0), "missing quantisation table"),
        (_without(base, 0xC4, 0), "missing DC Huffman table"),
        (_without(base, 0xC4, 1), "missing AC Huffman table"),
        (base[:-2], "missing EOI"),
        (base[:sos[2]], "missing EOI"),
        (b"\x00" + base, "no SOI"),
    ]
    for data, reason in refusals:
        with pytest.raises(jpeg.Unsupported, match=reason):
            jpeg.parse(data)
        with pytest.raises(ValueError, match=reason):
            jpeg.pack([base, data])
    assert issubclass(jpeg.Unsupported, ValueError)


# ---- the device code on the host ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg") / "jpeg_host_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", os.path.join(_lib.CSRC_DIR, "jpeg_host_check.cpp"), "-o", exe])
    return exe


def _run(exe, tmp_path, items, order="bgr"):
    """decode `items` into every second frame of a canary-filled destination -> (status [n], frames [n, H, W, 3] rgb)"""
    b = jpeg.pack(items)
    n = b.n
    slots = 2 * np.arange(n) + 1
    src, dst = str(tmp_path / "packed.bin"), str(tmp_path / "out.bin")
    jpeg_cases.write_packed(src, b, slots, 2 * n + 1, order)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    status, frames = jpeg_cases.read_result(dst, n, 2 * n + 1, b.height, b.width)
    assert (frames[0::2] == jpeg_cases.CANARY).all(), "a frame nobody named was written"
    out = frames[1::2]
    return status, (out[..., ::-1] if order == "bgr" else out)


def test_host_program_reproduces_every_golden(host_check, tmp_path):
    by_size = {}
    for name in sorted(CASES):
        by_size.setdefault(CASES[name][1].shape[:2], []).append(name)
    assert len(by_size[(40, 56)]) == 8
    for k, (size, names) in enumerate(sorted(by_size.items())):
        status, rgb = _run(host_check, tmp_path, [CASES[n][0] for n in names], order="rgb" if k % 2 else "bgr")
        assert not status.any(), (names, status)
        for i, n in enumerate(names):
            assert np.array_equal(rgb[i], CASES[n][1]), n


def test_host_program_absent_item_is_zeros(host_check, tmp_path):
    status, rgb = _run(host_check, tmp_path, [None, CASES["f_444_q60"][0], None])
    assert not status.any() and not rgb[0].any() and not rgb[2].any() and np.array_equal(rgb[1], CASES["f_444_q60"][1])


def test_host_program_on_damaged_streams(host_check, tmp_path):
    items, names = jpeg_cases.damaged_batch()
    assert sum(d[1] == "trunc" for d in jpeg_cases.damaged()) == 20 and sum(d[1] == "flip" for d in jpeg_cases.damaged()) == 200
    status, rgb = _run(host_check, tmp_path, items)
    count = jpeg_cases.check_damaged_result(names, rgb, status)
    print(count)
    assert count["flagged"] >= 22 and count["neighbour"] >= 28        # (20 truncations + 2 restart cases at the least)


def test_host_program_refuses_bad_tables(host_check, tmp_path):
    """the validation m3t_jpeg_decode applies before any launch (exit 2 = M3T_EINVAL's rule)"""
    b = jpeg.pack([CASES["f_rst_blocks2"][0], CASES["f_420_q95"][0]])

    def refused(mutate):
        c = jpeg.pack([CASES["f_rst_blocks2"][0], CASES["f_420_q95"][0]])
        mutate(c)
        src = str(tmp_path / "bad.bin")
        jpeg_cases.write_packed(src, c, np.arange(c.n), c.n, "bgr")
        return subprocess.run([host_check, src, str(tmp_path / "o.bin")], capture_output=True).returncode

    assert refused(lambda c: None) == 0
    def seg_outside(c): c.segments[b.n_segs - 1, 2] = c.stream.numel()
    def seg_negative(c): c.segments[0, 1] = -4
    def bad_sampling(c): c.images[1, 3] = 3
    def bad_count(c): c.images[0, 6] -= 1
    def bad_table(c): c.images[1, 13] = c.n_huff
    def bad_quant(c): c.images[1, 8] = -1
    def bad_lut(c): c.huff[0, 0] = 0x1F00
    for m in (seg_outside, seg_negative, bad_sampling, bad_count, bad_table, bad_quant, bad_lut):
        assert refused(m) == 2, m.__name__
