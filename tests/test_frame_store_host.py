"""The resident JPEG frame store without a GPU (m3t/jpeg.py: frame_records, plan_frames, gather_host): the records of a set of videos, a
planned batch against jpeg.pack of the same flat list, the device code's text (csrc/jpeg_host_check.cpp) decoding a store-built batch, and
every refusal -- all of it before anything touches a device."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch

import frame_store_cases as fsc
import jpeg_cases
from m3t import jpeg, video, _lib

CASES, REFUSALS = jpeg_cases.load()
W = fsc.WINDOW


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    videos, names = fsc.family_videos(tmp_path_factory.mktemp("frames"))
    return videos, names, jpeg.frame_records(videos, chunk_bytes=fsc.CHUNK_BYTES)


def test_records(family):
    videos, names, r = family
    assert r.names == ["a", "b", "c"] and (r.height, r.width) == (40, 56) and r.n_frames == 18
    assert r.video_off.tolist() == [0, 7, 15, 18]
    for v in names:
        want = [n is not None for n in names[v]]
        assert r.has_image(v).tolist() == want and r.has_image(r.names.index(v)).tolist() == want
    assert not r.has_image("a")[4] and r.has_image("b")[5]                      # the path that does not exist, the file on disk
    flat = [n for v in names for n in names[v]]
    assert len(r.chunks) == len(r.chunk_sizes) >= 4
    alone = 0
    for f, name in enumerate(flat):
        if name is None:
            assert not r.present[f] and not r.images[f].any()
            continue
        h = jpeg.parse(CASES[name][0])
        scan = CASES[name][0][h.scan_offset:h.scan_end]
        c, off, nb = int(r.chunk[f]), int(r.offset[f]), int(r.nbytes[f])
        padded = (nb + 15) // 16 * 16
        chunk = r.chunks[c]
        assert nb == len(scan) and off % 16 == 0 and off + padded <= chunk.size == r.chunk_sizes[c]        # no frame straddles a chunk
        assert chunk[off:off + nb].tobytes() == scan and not chunk[off + nb:off + padded].any()
        if padded > fsc.CHUNK_BYTES:                                             # larger than a chunk: a chunk of its own
            assert off == 0 and chunk.size == padded
            alone += 1
    assert alone == sum(n == "f_rst_rows1_q100" for n in flat) >= 1
    for c, chunk in enumerate(r.chunks):                                         # within the limit, and every byte is some frame's or zero
        assert chunk.size % 16 == 0 and (chunk.size <= fsc.CHUNK_BYTES or (r.chunk == c).sum() == 1)
        covered = np.zeros(chunk.size, bool)
        for f in np.flatnonzero(r.present & (r.chunk == c)):
            assert not covered[r.offset[f]:r.offset[f] + r.nbytes[f]].any()
            covered[r.offset[f]:r.offset[f] + r.nbytes[f]] = True
        assert not chunk[~covered].any()
    packed = jpeg.pack([None if n is None else CASES[n][0] for n in flat])
    assert (r.quant.shape[0], r.huff.shape[0]) == (packed.n_quant, packed.n_huff)            # deduplicated over the whole set
    assert r.segs.shape[0] == packed.n_segs
    one_chunk = jpeg.frame_records(videos)                                       # the default: everything fits one chunk
    assert len(one_chunk.chunks) == 1 and one_chunk.chunk_sizes[0] == sum(r.chunk_sizes)


def test_records_hand_every_chunk_on_once(family):
    videos, _, r = family
    seen = []
    s = jpeg.frame_records(videos, chunk_bytes=fsc.CHUNK_BYTES, _sink=lambda i, chunk: seen.append((i, chunk.copy())))
    assert s.chunks is None and [i for i, _ in seen] == list(range(len(r.chunks)))
    assert all(np.array_equal(c, k) for (_, c), k in zip(seen, r.chunks)) and np.array_equal(s.chunk_sizes, r.chunk_sizes)


def _planned_batch(r, items, window=W):
    p = jpeg.plan_frames(r, items, window)
    return p, p.batch(jpeg.gather_host(r.chunks, p.rows, p.stream_bytes))


def test_plan_equals_pack(family):
    videos, names, r = family
    p, b = _planned_batch(r, fsc.ITEMS)
    flat = fsc.flat_names(names, fsc.ITEMS, W)
    want = jpeg.pack(fsc.flat_files(flat))
    assert p.n == len(fsc.ITEMS) * W == want.n and p.present.tolist() == [n is not None for n in flat]
    fsc.assert_same_images(b, want)
    assert (b.n_quant, b.n_huff) == (want.n_quant, want.n_huff)                  # only the tables this batch names
    # the gather table: one row per present image, destinations ascending and back to back, 16-byte units
    assert p.rows.dtype == np.int32 and p.rows.shape == (int(p.present.sum()), 4) and not (p.rows[:, 1:] % 16).any()
    assert np.array_equal(p.rows[:, 2], np.concatenate([[0], np.cumsum(p.rows[:, 3])[:-1]]))
    assert p.stream_bytes == int(p.rows[:, 3].sum()) + 16 and not b.stream.numpy()[-16:].any()
    order = list(names)
    for n, it in enumerate(fsc.ITEMS):
        v = it[0] if isinstance(it[0], str) else order[it[0]]
        tl = W if len(it) == 2 else it[2]
        assert np.array_equal(p.frame_idx[n], video.frame_index(r.has_image(v)[it[1]:it[1] + tl], 0, tl, W)), it
    assert p.frame_idx.dtype == np.int32 and p.frame_idx[2].tolist() == [-1] * W and p.frame_idx[3, 0] == -1
    few = jpeg.plan_frames(r, [("c", 2, 1)], W)                                  # one 4:2:0 frame: two quantisation, four Huffman tables
    assert (few.n_quant, few.n_huff, few.rows.shape[0]) == (2, 4, 1)
    gray = jpeg.plan_frames(r, [("c", 1, 1)], W)                                 # one gray frame: one and two
    assert (gray.n_quant, gray.n_huff) == (1, 2) and not gray.tables[:jpeg.IMG_COLS][[8, 9, 11, 12, 14, 15]].any()
    none = jpeg.plan_frames(r, [("b", 0), ("b", 0, 2)], W)                       # nothing to decode
    assert none.rows.shape == (0, 4) and none.stream_bytes == 16 and (none.n_segs, none.n_quant, none.n_huff) == (0, 0, 0)
    assert not none.present.any() and (none.frame_idx == -1).all() and none.tables.size == none.n * (jpeg.IMG_COLS + 1)
    empty = jpeg.plan_frames(r, [], W)
    assert empty.n == 0 and empty.frame_idx.shape == (0, W)


# ---- the device code on the host ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg") / "jpeg_host_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", os.path.join(_lib.CSRC_DIR, "jpeg_host_check.cpp"), "-o", exe])
    return exe


def _run(exe, tmp_path, b):
    """decode the batch into every second frame of a canary-filled destination -> (status [n], frames [n, H, W, 3] rgb)"""
    n = b.n
    src, dst = str(tmp_path / "packed.bin"), str(tmp_path / "out.bin")
    jpeg_cases.write_packed(src, b, 2 * np.arange(n) + 1, 2 * n + 1, "rgb")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    status, frames = jpeg_cases.read_result(dst, n, 2 * n + 1, b.height, b.width)
    assert (frames[0::2] == jpeg_cases.CANARY).all(), "a frame nobody named was written"
    return status, frames[1::2]


def test_host_program_decodes_a_store_built_batch(family, host_check, tmp_path):
    _, names, r = family
    _, b = _planned_batch(r, fsc.ITEMS)
    status, rgb = _run(host_check, tmp_path, b)
    assert not status.any()
    for i, name in enumerate(fsc.flat_names(names, fsc.ITEMS, W)):
        assert np.array_equal(rgb[i], CASES[name][1]) if name is not None else not rgb[i].any(), (i, name)


def test_host_program_on_a_damaged_store(host_check, tmp_path):
    videos, names = fsc.damaged_video()
    r = jpeg.frame_records(videos, chunk_bytes=1 << 16)
    n = len(names)
    assert r.present.all() and len(r.chunks) > 1
    _, b = _planned_batch(r, [("damaged", 0, n)], n)
    fsc.assert_same_images(b, jpeg.pack(videos["damaged"]))
    status, rgb = _run(host_check, tmp_path, b)
    count = jpeg_cases.check_damaged_result(names, rgb, status)
    assert count["flagged"] >= 22 and count["neighbour"] >= 28                   # (20 truncations + 2 restart cases at the least)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(family, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a host-only call asked about the device")
    for name in ("is_available", "current_device", "device_count", "init"):
        monkeypatch.setattr(torch.cuda, name, no_device)
    good = CASES["f_420_q95"][0]
    assert len(REFUSALS) >= 2
    for name, data in sorted(REFUSALS.items()):
        videos = {"first": [good], "second": [good, None, data, good]}
        with pytest.raises(jpeg.Unsupported, match=r"video 'second', frame 2: "):
            jpeg.frame_records(videos)
        r = jpeg.frame_records(videos, on_unsupported="absent")
        assert r.has_image("second").tolist() == [True, False, False, True] and len(r.chunks) == 1
    with pytest.raises(jpeg.Unsupported, match="progressive"):
        jpeg.frame_records({"v": [REFUSALS["refuse_progressive"]]})
    with pytest.raises(ValueError, match=r"video 'v', frame 2 is 16 x 16.*share one size"):
        jpeg.frame_records({"u": [None, good], "v": [good, None, CASES["e_16x16_420"][0]]})
    with pytest.raises(ValueError, match="no frame"):
        jpeg.frame_records({"v": [None, REFUSALS["refuse_cmyk"]]}, on_unsupported="absent")
    for bad in (0, 24, 2 ** 31, -16):
        with pytest.raises(ValueError, match="chunk_bytes"):
            jpeg.frame_records({"v": [good]}, chunk_bytes=bad)
    with pytest.raises(ValueError, match="on_unsupported"):
        jpeg.frame_records({"v": [good]}, on_unsupported="skip")
    with pytest.raises(ValueError):
        jpeg.frame_records({})

    r = family[2]
    for items, reason in (([("d", 0)], "unknown video 'd'"), ([(3, 0)], "unknown video 3"), ([(-1, 0)], "unknown video -1"),
                          ([("a", -1)], "negative"), ([("a", 0, 0)], "track_len 0 outside"), ([("a", 0, W + 1)], "track_len %d outside" % (W + 1)),
                          ([("a", 4)], "run past the 7 frames of a"), ([("c", 0)], "run past the 3 frames of c"), ([("c", 3, 1)], "run past"),
                          ([("a", 0), ("a",)], "item 1: expected")):
        with pytest.raises(ValueError, match=reason):
            jpeg.plan_frames(r, items, W)
    with pytest.raises(ValueError, match="window"):
        jpeg.plan_frames(r, [("a", 0)], 0)
    huge = copy.copy(r)                                                          # a batch whose gathered bytes would reach 2^31
    huge.nbytes = np.full_like(r.nbytes, 2 ** 29)
    assert jpeg.plan_frames(huge, [("c", 0, 3)], W).stream_bytes == 3 * 2 ** 29 + 16
    with pytest.raises(ValueError, match="bytes"):
        jpeg.plan_frames(huge, [("c", 0, 3), ("c", 0, 1)], W)
    assert jpeg.plan_frames(r, fsc.ITEMS, W).n == len(fsc.ITEMS) * W            # (and the good batch still plans with the device out of reach)
    with pytest.raises(ValueError, match="does not fit"):
        jpeg.gather_host(r.chunks, [[0, 0, 0, 32]], 32)
