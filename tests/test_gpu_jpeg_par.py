"""The parallel walk of the JPEG decode on the MI355X (csrc/jpeg.hip: jpeg_par_kernel, m3t_jpeg_decode_walk; rules in csrc/jpeg_par.h;
m3t/jpeg.py: decode(walk=...)).  Every comparison is exact: the frames are Pillow's bits from both fixture files at every sub-sequence
size, the sequential walk of the same call is the yardstick for damaged streams (frames and status words equal: the list of streams on
which the contract would let the RST bit differ is empty, because a segment with a marker inside takes its status from the sequential
reader), and routing, stats and the raw ABI behave as include/m3t_hip.h says."""
import functools
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
import jpeg_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES, _ = jpeg_cases.load()


@functools.lru_cache(None)
def all_cases():
    d = load_golden("jpeg_par_cases")
    out = dict(CASES)
    out.update({k[:-4]: (d[k].tobytes(), d[k[:-4] + ".rgb"]) for k in d if k.endswith(".jpg")})
    assert len(out) == len(CASES) + 6
    return out


def _jpeg():
    from m3t import jpeg
    return jpeg


def _check_stats(stats, taken):
    stats = stats.cpu().numpy()
    taken = np.asarray(taken, bool)
    assert stats.dtype == np.int32 and stats.shape == (len(taken), 2)
    assert (stats[~taken] == 0).all(), stats
    assert (stats[taken, 1] >= 1).all() and (stats[taken, 1] <= stats[taken, 0]).all(), stats
    return stats


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_every_golden_in_both_orders_at_three_sub_sequence_sizes(name):
    jpeg = _jpeg()
    data, rgb = all_cases()[name]
    b = jpeg.pack([data])
    for sub_bytes in (16, 32, 256):
        for order, want in (("bgr", rgb[..., ::-1]), ("rgb", rgb)):
            frames, status, stats = jpeg.decode(b, order=order, walk="parallel", sub_bytes=sub_bytes, stats=True)
            assert frames.dtype == torch.uint8 and frames.is_cuda and tuple(frames.shape) == (1,) + rgb.shape
            assert status.dtype == torch.int32 and status.tolist() == [0]
            assert np.array_equal(frames[0].cpu().numpy(), want), (sub_bytes, order)
            st = _check_stats(stats, np.ones(b.n_segs, bool))
            assert (st[:, 0] == -(-np.maximum(b.segments[:, 2] - _stuffed(b), 1) // sub_bytes)).all()


def _stuffed(b):
    """the FF 00 pairs of each segment: a sub-sequence is sub_bytes of the UNSTUFFED segment"""
    stream = b.stream.numpy().tobytes()
    return np.array([stream[o:o + n].count(b"\xff\x00") for _, o, n, _ in b.segments])


def test_family_batch_into_scattered_slots_with_mixed_routing():
    jpeg = _jpeg()
    names = jpeg_cases.FAMILY
    b = jpeg.pack([CASES[n][0] for n in names])
    slots = [(2, 3), (0, 0), (1, 2), (0, 3), (2, 0), (1, 1), (0, 1), (2, 2)]
    seg_bytes = b.segments[:, 2]
    seg_image = b.segments[:, 0]
    results = []
    for kw, taken in ((dict(walk="parallel"), np.ones(b.n_segs, bool)), (dict(walk="auto", par_min_bytes=1000), seg_bytes >= 1000)):
        out = torch.full((3, 4, 40, 56, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
        frames, status, stats = jpeg.decode(b, out=out, slots=slots, order="rgb", stats=True, **kw)
        assert frames is out and status.tolist() == [0] * 8
        got = out.cpu().numpy()
        for n, (c, t) in zip(names, slots):
            assert np.array_equal(got[c, t], CASES[n][1]), n
        for c in range(3):
            for t in range(4):
                if (c, t) not in slots:
                    assert (got[c, t] == jpeg_cases.CANARY).all(), (c, t)
        _check_stats(stats, taken)
        results.append((got, taken))
    taken = results[1][1]
    assert taken[seg_image == names.index("f_420_q95")].all() and not taken[seg_image == names.index("f_444_q60")].any()
    assert not taken[seg_image == names.index("f_rst_blocks2")].any()
    rows = taken[seg_image == names.index("f_rst_rows1_q100")]                # (quality 100: two of its three MCU rows pass 1000 bytes)
    assert rows.any() and not rows.all()                                      # one image, both walks
    assert np.array_equal(results[0][0], results[1][0])


def test_damaged_streams_equal_the_sequential_walk():
    jpeg = _jpeg()
    items, names = jpeg_cases.damaged_batch()
    b = jpeg.pack(items)
    n = b.n
    got = {}
    for walk in ("sequential", "parallel"):
        out = torch.full((n, 2, 40, 56, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
        frames, status, stats = jpeg.decode(b, out=out, slots=[(i, 1) for i in range(n)], order="rgb", walk=walk, sub_bytes=32, stats=True)
        got[walk] = (out.cpu().numpy(), status.cpu().numpy())
        assert (got[walk][0][:, 0] == jpeg_cases.CANARY).all()
        _check_stats(stats, np.full(b.n_segs, walk == "parallel"))
    assert np.array_equal(got["parallel"][0], got["sequential"][0])
    # the streams on which the RST bit may differ under the contract (a marker past the last consumed bit), one by one: none
    rst_may_differ = []
    differ = [names[i] for i in np.flatnonzero(got["parallel"][1] != got["sequential"][1])]
    assert differ == rst_may_differ
    count = jpeg_cases.check_damaged_result(names, got["parallel"][0][:, 1], got["parallel"][1])
    print(count)
    assert count["flagged"] >= 22 and count["neighbour"] >= 28


def test_markers_inside_a_segment_equal_the_sequential_walk():
    """FF FF 00 and a lone FF at the front, the middle and the end of a scan: staging sees every one of them, the sequential reader only
    those its look-ahead reaches; frames and every status bit must agree all the same"""
    jpeg = _jpeg()
    head, scan, tail = jpeg_cases.split(CASES["f_420_q95"][0])
    items = [CASES["f_420_q95"][0]]
    for at in (0, 1, 17, len(scan) // 2, len(scan) - 40, len(scan) - 6, len(scan) - 3, len(scan) - 2):
        s = bytearray(scan)
        s[at:at + 3] = b"\xff\xff\x00"
        items.append(head + bytes(s) + tail)
    for cut in (1, 300, len(scan) - 1):
        items.append(head + scan[:cut] + b"\xff" + tail)
    b = jpeg.pack(items)
    f0, s0 = jpeg.decode(b, walk="sequential")
    assert s0[0].item() == 0 and (s0[1:] != 0).all()
    for sub_bytes in (16, 64):
        f1, s1 = jpeg.decode(b, walk="parallel", sub_bytes=sub_bytes)
        assert torch.equal(f1, f0) and torch.equal(s1, s0)


def test_routing_of_the_dataset_frame():
    jpeg = _jpeg()
    data, rgb = CASES["full_256_q95"]
    b = jpeg.pack([data])
    assert 40000 < b.segments[0, 2] <= jpeg.par_max_bytes()
    frames, status, stats = jpeg.decode(b, walk="parallel", par_max_bytes=40000, stats=True)
    assert stats.tolist() == [[0, 0]] and status.tolist() == [0] and np.array_equal(frames[0].cpu().numpy(), rgb[..., ::-1])
    frames, status, stats = jpeg.decode(b, walk="parallel", stats=True)
    st = stats.tolist()
    assert st[0][0] == -(-(b.segments[0, 2] - _stuffed(b)[0]) // jpeg.AUTO_SUB_BYTES) and 1 <= st[0][1] <= st[0][0]
    assert status.tolist() == [0] and np.array_equal(frames[0].cpu().numpy(), rgb[..., ::-1])
    for bad in (dict(walk="fast"), dict(sub_bytes=24), dict(sub_bytes=0), dict(sub_bytes=8192), dict(par_min_bytes=-1), dict(par_max_bytes="x")):
        with pytest.raises(ValueError):
            jpeg.decode(b, **bad)


def test_results_do_not_depend_on_the_lane_count():
    jpeg = _jpeg()
    items = [all_cases()[n][0] for n in ("p_flat_420_q30", "full_256_q95")]
    b = jpeg.pack(items)
    before = jpeg.par_lanes()
    try:
        got = []
        for lanes in (64, 128, 256):
            assert jpeg.par_lanes(lanes) == lanes
            frames, status, stats = jpeg.decode(b, walk="parallel", sub_bytes=64, stats=True)
            got.append((frames.cpu(), status.cpu(), stats.cpu()))
        with pytest.raises(ValueError):
            jpeg.par_lanes(96)
    finally:
        jpeg.par_lanes(before)
    for i, n in enumerate(("p_flat_420_q30", "full_256_q95")):
        assert np.array_equal(got[0][0][i].numpy(), all_cases()[n][1][..., ::-1]), n
    for g in got[1:]:
        assert all(torch.equal(x, y) for x, y in zip(g, got[0]))


def test_raw_abi():
    jpeg = _jpeg()
    from m3t import _lib
    lib = _lib.load()
    b = jpeg.pack([CASES["f_420_q95"][0], CASES["f_rst_blocks2"][0]])
    n, H, W = b.n, b.height, b.width
    s_d = b.stream.to(DEV)
    t = np.ascontiguousarray(b.tables, np.int32)
    t_d = torch.from_numpy(t).to(DEV)
    ws = torch.empty(int(lib.m3t_jpeg_workspace_bytes(n, H, W)), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(out, status, stats, walk, sub_bytes, lo=0, hi=1 << 30):
        return lib.m3t_jpeg_decode_walk(s_d.data_ptr(), s_d.numel(), t.ctypes.data, t_d.data_ptr(), n, b.n_segs, b.n_quant, b.n_huff, H, W,
                                        out.data_ptr(), n, 0, ws.data_ptr(), ws.numel(), status.data_ptr(), walk, sub_bytes, lo, hi,
                                        None if stats is None else stats.data_ptr(), st)

    out = torch.full((n, H, W, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    stats = torch.full((b.n_segs, 2), -1, dtype=torch.int32, device=DEV)
    for walk, sub_bytes in ((1, 0), (1, 24), (1, 8192), (2, 32), (0, 24), (-1, 32)):
        assert call(out, status, stats, walk, sub_bytes) == _lib.M3T_EINVAL, (walk, sub_bytes)
    assert call(out, status, stats, 1, 32, lo=-1) == _lib.M3T_EINVAL
    torch.cuda.synchronize()
    assert (out == jpeg_cases.CANARY).all() and status.tolist() == [-1] * n and (stats == -1).all()      # refused before anything was launched
    assert lib.m3t_jpeg_par_max_bytes() >= 45 * 1024

    assert call(out, status, stats, 0, 32) == 0
    old = torch.full_like(out, jpeg_cases.CANARY)
    old_status = torch.full_like(status, -1)
    assert lib.m3t_jpeg_decode(s_d.data_ptr(), s_d.numel(), t.ctypes.data, t_d.data_ptr(), n, b.n_segs, b.n_quant, b.n_huff, H, W,
                               old.data_ptr(), n, 0, ws.data_ptr(), ws.numel(), old_status.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, old) and torch.equal(status, old_status) and status.tolist() == [0, 0] and not stats.any()
    assert np.array_equal(out[0].cpu().numpy(), CASES["f_420_q95"][1][..., ::-1])
    par = torch.full_like(out, jpeg_cases.CANARY)
    assert call(par, status, None, 1, 32) == 0                                                           # walk_stats may be NULL
    torch.cuda.synchronize()
    assert torch.equal(par, old) and status.tolist() == [0, 0]


def test_load_clips_feeds_the_ingest(tmp_path):
    jpeg = _jpeg()
    from m3t import video
    data, rgb = CASES["full_256_q95"]
    path = str(tmp_path / "00001.jpg")
    with open(path, "wb") as f:
        f.write(data)
    clips = [[None, data, path, str(tmp_path / "missing.jpg")], [path, None, None, data]]
    frames, present, status = jpeg.load_clips(clips, walk="parallel")
    assert tuple(frames.shape) == (2, 4, 256, 256, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    assert present.tolist() == [[False, True, True, False], [True, False, False, True]] and status.tolist() == [0] * 8
    host = np.zeros((2, 4, 256, 256, 3), np.uint8)
    host[present] = rgb[..., ::-1]
    assert np.array_equal(frames.cpu().numpy(), host)
    fidx = np.stack([video.frame_index(present[n], 0, 4, 6) for n in range(2)])
    random.seed(5)
    np.random.seed(5)
    aug = [video.draw_affwild(256, True, True, True, mirror=bool(n), resize=True) for n in range(2)]
    got = video.ingest(frames, aug, fidx, "planes")
    want = video.ingest(torch.from_numpy(host), aug, fidx, "planes")
    assert tuple(got.shape) == (2, 3, 6, 112, 112) and torch.equal(got, want)
    again = jpeg.load_clips(clips, walk="parallel", sub_bytes=64)
    assert torch.equal(again[0], frames)


def test_two_calls_in_a_row_are_identical():
    jpeg = _jpeg()
    items, _ = jpeg_cases.damaged_batch()
    for batch, sub_bytes in ((jpeg.pack(items), 32), (jpeg.pack([CASES["full_256_q95"][0]] * 3), 128)):
        a = jpeg.decode(batch, walk="parallel", sub_bytes=sub_bytes, stats=True)
        b = jpeg.decode(batch, walk="parallel", sub_bytes=sub_bytes, stats=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
