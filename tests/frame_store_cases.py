"""The videos, windows and comparisons shared by tests/test_frame_store_host.py and tests/test_gpu_frame_store.py: three "videos" made of
the eight 40 x 56 family streams with None entries, a file on disk and a path that does not exist; a batch of windows that covers the
corners of plan_frames; and the rule "a store-built batch describes the same images as jpeg.pack of the same flat list"."""
import numpy as np

import jpeg_cases

WINDOW = 4
CHUNK_BYTES = 2048          # several chunks for the family, and f_rst_rows1_q100 (a 3 234-byte scan) larger than one
# (video, start[, track_len]): two overlapping windows of "a"; a window of "b" that is entirely absent; one that starts on an absent frame;
# a short window; a video by index with a short window; a window that ends on the last frame of its video
ITEMS = [("a", 0), ("a", 2), ("b", 0), ("b", 3), ("c", 0, 3), (2, 1, 2), ("a", 3, 4)]


def family_videos(tmp_path):
    """-> (videos: name -> [bytes | path | None], names: name -> [fixture name | None])"""
    cases, _ = jpeg_cases.load()
    F = jpeg_cases.FAMILY
    on_disk = str(tmp_path / "00006.jpg")
    with open(on_disk, "wb") as f:
        f.write(cases[F[6]][0])
    missing = str(tmp_path / "no_such_dir" / "00005.jpg")
    names = {"a": [F[0], None, F[1], F[2], None, F[3], F[4]],
             "b": [None, None, None, None, F[5], F[6], F[7], F[0]],
             "c": [F[7], F[3], F[5]]}
    videos = {v: [None if n is None else cases[n][0] for n in row] for v, row in names.items()}
    videos["a"][4] = missing
    videos["b"][5] = on_disk
    return videos, names


def flat_names(names, items, window):
    """the fixture name (or None) behind every image n window + t of the batch, as plan_frames lays it out"""
    order = list(names)
    out = []
    for it in items:
        row = names[it[0] if isinstance(it[0], str) else order[it[0]]]
        tl = window if len(it) == 2 else it[2]
        out.extend(row[it[1] + t] if t < tl else None for t in range(window))
    return out


def flat_files(flat):
    cases, _ = jpeg_cases.load()
    return [None if n is None else cases[n][0] for n in flat]


def damaged_video():
    """-> (videos, names): one video made of jpeg_cases.damaged_batch()"""
    items, names = jpeg_cases.damaged_batch()
    return {"damaged": items}, names


def assert_same_images(got, want):
    """two JpegBatch describe the same images: per image the present flag and the geometry, the CONTENTS of the tables behind the indices,
    the same number of segments with equal lengths and markers, and equal bytes behind every segment"""
    from m3t import jpeg
    assert (got.n, got.height, got.width) == (want.n, want.height, want.width)
    assert np.array_equal(got.present, want.present)
    assert got.stream.numel() % 16 == 0 and list(got.slots) == list(range(got.n))
    gs, ws = got.stream.numpy(), want.stream.numpy()
    for i in range(got.n):
        g, w = got.images[i], want.images[i]
        assert np.array_equal(g[:5], w[:5]) and g[6] == w[6], i
        if not w[0] & 1:
            assert not g.any(), i
            continue
        for c in range(w[1]):
            assert np.array_equal(got.quant[g[7 + c]], want.quant[w[7 + c]]), (i, c)
            assert np.array_equal(got.huff[g[10 + c]], want.huff[w[10 + c]]), (i, c)
            assert np.array_equal(got.huff[g[13 + c]], want.huff[w[13 + c]]), (i, c)
        for k in range(w[6]):
            sg, sw = got.segments[g[5] + k], want.segments[w[5] + k]
            assert sg[0] == sw[0] == i and sg[2] == sw[2] and sg[3] == sw[3], (i, k)
            assert sg[1] >= 0 and sg[1] + sg[2] <= gs.size - 16, (i, k)
            assert np.array_equal(gs[sg[1]:sg[1] + sg[2]], ws[sw[1]:sw[1] + sw[2]]), (i, k)
    assert jpeg.IMG_COLS * got.n + jpeg.SEG_COLS * got.n_segs + got.n + jpeg.QUANT_INTS * got.n_quant + jpeg.HUFF_INTS * got.n_huff == got.tables.size
