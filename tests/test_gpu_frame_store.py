"""The resident JPEG frame store on the MI355X (csrc/frame_store.hip: m3t_jpeg_gather; m3t/jpeg.py: FrameStore): every comparison here is
exact.  The gather against its numpy restatement with guard bytes behind the destination, the store's decode against jpeg.pack +
jpeg.decode of the same flat list (frames AND status words, all three walks, both orders, damaged streams included) and against Pillow's
goldens, the ingest of a store-built batch against the ingest of jpeg.load_clips, and the frame index against the track store's."""
import functools
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
import frame_store_cases as fsc
import jpeg_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES, _ = jpeg_cases.load()
W = fsc.WINDOW
STRIDE = 4096                     # bytes a workgroup of the gather moves in one step: 256 lanes, 16 bytes each


def _jpeg():
    from m3t import jpeg
    return jpeg


@functools.lru_cache(None)
def _par_cases():
    d = load_golden("jpeg_par_cases")
    return {k[:-4]: (d[k].tobytes(), d[k[:-4] + ".rgb"]) for k in d if k.endswith(".jpg")}


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    videos, names = fsc.family_videos(tmp_path_factory.mktemp("frames"))
    return videos, names, _jpeg().FrameStore(videos, W, chunk_bytes=fsc.CHUNK_BYTES)


# ---- the gather alone -----------------------------------------------------------------------------------------------------------------

def _chunks():
    rs = np.random.RandomState(11)
    host = [rs.randint(1, 256, size).astype(np.uint8) for size in (65536, 8192, 16384)]      # (no zero byte: a missed granule shows)
    return host, [torch.from_numpy(c).to(DEV) for c in host]


def _gathered(dev_chunks, rows, dst_bytes):
    dst = torch.full((dst_bytes + 64,), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    _jpeg().gather(dev_chunks, rows, dst, dst_bytes)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[dst_bytes:] == jpeg_cases.CANARY).all(), "bytes behind dst_bytes were written"
    return got[:dst_bytes]


def _rows(parts):
    """[(chunk, source offset, bytes, gap in front)] -> the gather table, destinations ascending"""
    rows, to = [], 0
    for chunk, src, nbytes, gap in parts:
        to += gap
        rows.append((chunk, src, to, nbytes))
        to += nbytes
    return np.asarray(rows, np.int32).reshape(-1, 4), to + 16


def test_gather_equals_its_restatement():
    jpeg = _jpeg()
    host, dev = _chunks()
    largest = (max(len(jpeg_cases.split(d)[1]) for d, _ in CASES.values()) + 15) // 16 * 16
    assert largest == 44992
    # 16 bytes; one granule short of and one over a workgroup's stride; the largest fixture; three chunks in no order; the same source
    # twice and overlapping sources; gaps between the rows, which the kernel zero-fills
    rows, dst_bytes = _rows([(2, 4096, 16, 0), (0, 1024, STRIDE - 16, 0), (1, 0, STRIDE + 16, 0), (0, 16, largest, 0), (2, 4096, 16, 0),
                             (0, 1024, STRIDE - 16, 48), (1, 16, STRIDE, 0), (0, 2048, 8192, 16), (2, 0, 16384, 0), (0, 65536 - 32, 32, 4096)])
    want = jpeg.gather_host(host, rows, dst_bytes)
    got = _gathered(dev, rows, dst_bytes)
    assert np.array_equal(got, want)
    assert (want[:-16] != 0).sum() == int(rows[:, 3].sum()) and not got[-16:].any()
    assert np.array_equal(_gathered(dev, rows, dst_bytes), got)                    # and again: the same bytes
    # dst larger than the rows need: zeros behind them
    assert np.array_equal(_gathered(dev, rows, dst_bytes + 3 * STRIDE), jpeg.gather_host(host, rows, dst_bytes + 3 * STRIDE))
    one, one_bytes = _rows([(1, 8192 - 48, 48, 0)])
    assert np.array_equal(_gathered(dev, one, one_bytes), jpeg.gather_host(host, one, one_bytes))
    assert not _gathered(dev, np.zeros((0, 4), np.int32), 16).any()                # m == 0 zero-fills
    assert not _gathered([], np.zeros((0, 4), np.int32), STRIDE + 16).any()


def test_gather_refuses_bad_tables():
    jpeg = _jpeg()
    from m3t import _lib
    lib = _lib.load()
    host, dev = _chunks()
    good, dst_bytes = _rows([(2, 4096, 16, 0), (0, 1024, 4080, 0), (1, 0, 4112, 0)])
    dst = torch.full((dst_bytes + 64,), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    addr = np.array([c.data_ptr() for c in dev], np.int64)
    size = np.array([c.numel() for c in dev], np.int64)
    addr_d = torch.from_numpy(addr).to(DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(rows=good, m=None, addr_h=addr, size_h=size, n_chunks=3, chunks_d=addr_d.data_ptr(), rows_d_off=0, rows_h_null=False,
             dst_ptr=dst.data_ptr(), nbytes=dst_bytes):
        rows = np.ascontiguousarray(rows, np.int32)
        rows_d = torch.from_numpy(np.concatenate([rows.reshape(-1), np.zeros(4, np.int32)])).to(DEV)
        return lib.m3t_jpeg_gather(addr_h.ctypes.data, size_h.ctypes.data, n_chunks, chunks_d, None if rows_h_null else rows.ctypes.data,
                                   None if rows_d_off is None else rows_d.data_ptr() + rows_d_off, rows.shape[0] if m is None else m,
                                   dst_ptr, nbytes, st)

    def changed(r, c, v):
        rows = good.copy()
        rows[r, c] = v
        return rows

    bad = {
        "m < 0": call(m=-1), "null dst": call(dst_ptr=None), "misaligned dst": call(dst_ptr=dst.data_ptr() + 8),
        "null host rows": call(rows_h_null=True), "null device rows": call(rows_d_off=None), "misaligned device rows": call(rows_d_off=4),
        "null device chunks": call(chunks_d=None), "misaligned chunk": call(addr_h=addr + np.array([0, 8, 0])),
        "null chunk": call(addr_h=addr * np.array([1, 1, 0])), "no chunks": call(n_chunks=0), "n_chunks < 0": call(n_chunks=-1),
        "chunk past the count": call(changed(0, 0, 3)), "chunk below 0": call(changed(0, 0, -1)), "chunk past a shorter count": call(n_chunks=2),
        "source past its chunk": call(changed(2, 1, 8192 - 4096)), "source past a shorter chunk": call(size_h=size - np.array([0, 4096, 0])),
        "negative source": call(changed(1, 1, -16)), "source not 16": call(changed(1, 1, 1032)), "length not 16": call(changed(0, 3, 8)),
        "negative length": call(changed(0, 3, -16)), "destination not 16": call(changed(2, 2, 4104)),
        "negative destination": call(changed(0, 2, -16)), "destinations descend": call(good[[1, 0, 2]]),
        "destinations overlap": call(changed(2, 2, 4080)), "past dst_bytes - 16": call(nbytes=dst_bytes - 16),
        "dst_bytes not 16": call(nbytes=dst_bytes + 8), "dst_bytes 0": call(nbytes=0), "dst_bytes < 0": call(nbytes=-16),
        "m == 0, null dst": call(np.zeros((0, 4), np.int32), dst_ptr=None),
    }
    torch.cuda.synchronize()
    assert {k: rc for k, rc in bad.items() if rc != _lib.M3T_EINVAL} == {}
    assert (dst == jpeg_cases.CANARY).all()                                       # refused before anything was launched
    with pytest.raises(_lib.M3THipError):
        jpeg.gather(dev, changed(0, 0, 3), dst, dst_bytes)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy()[:dst_bytes], jpeg.gather_host(host, good, dst_bytes))


# ---- the store's decode ---------------------------------------------------------------------------------------------------------------

def _golden_frames(flat, order, cases=None):
    cases = cases or CASES
    H, Wd = next(cases[n][1].shape[:2] for n in flat if n is not None)
    want = np.zeros((len(flat), H, Wd, 3), np.uint8)
    for i, n in enumerate(flat):
        if n is not None:
            want[i] = cases[n][1] if order == "rgb" else cases[n][1][..., ::-1]
    return want


def test_store_attributes(family):
    videos, names, store = family
    assert store.names == ["a", "b", "c"] and (store.height, store.width, store.window) == (40, 56, W)
    assert len(store.chunks) >= 4 and all(c.is_cuda and c.dtype == torch.uint8 for c in store.chunks)
    assert store.nbytes == sum(c.numel() for c in store.chunks) + 8 * len(store.chunks)
    host = _jpeg().frame_records(videos, chunk_bytes=fsc.CHUNK_BYTES)
    assert store.records.chunks is None and all(np.array_equal(c.cpu().numpy(), h) for c, h in zip(store.chunks, host.chunks))
    for v in names:
        assert store.has_image(v).tolist() == [n is not None for n in names[v]]


@pytest.mark.parametrize("walk", ["sequential", "parallel", "auto"])
def test_store_decode_equals_pack_and_decode(family, walk):
    jpeg = _jpeg()
    videos, names, store = family
    flat = fsc.flat_names(names, fsc.ITEMS, W)
    packed = jpeg.pack(fsc.flat_files(flat))
    N = len(fsc.ITEMS)
    for order in ("bgr", "rgb"):
        frames, fidx, status = store.decode(fsc.ITEMS, order=order, walk=walk)
        assert frames.dtype == torch.uint8 and frames.device == store.device and tuple(frames.shape) == (N, W, 40, 56, 3)
        assert isinstance(fidx, torch.Tensor) and fidx.dtype == torch.int32 and not fidx.is_cuda and tuple(fidx.shape) == (N, W)
        assert status.dtype == torch.int32 and status.is_cuda and tuple(status.shape) == (N * W,)
        want_frames, want_status = jpeg.decode(packed, order=order, walk=walk)
        assert torch.equal(frames.view(N * W, 40, 56, 3), want_frames) and torch.equal(status, want_status)
        assert np.array_equal(frames.view(N * W, 40, 56, 3).cpu().numpy(), _golden_frames(flat, order)) and not status.any()
        assert np.array_equal(fidx.numpy(), jpeg.plan_frames(store.records, fsc.ITEMS, W).frame_idx)
    out = torch.full((N, W, 40, 56, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    got, _, _, stats = store.decode(fsc.ITEMS, out=out, order="rgb", walk=walk, stats=True)
    assert got is out and np.array_equal(out.view(N * W, 40, 56, 3).cpu().numpy(), _golden_frames(flat, "rgb"))
    _, _, want_stats = jpeg.decode(packed, order="rgb", walk=walk, stats=True)
    assert torch.equal(stats, want_stats) and (stats.any().item() == (walk == "parallel"))


def test_store_decode_edges(family):
    jpeg = _jpeg()
    from m3t import _lib
    videos, names, store = family
    out = torch.full((2, W, 40, 56, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    frames, fidx, status, stats = store.decode([("b", 0), ("b", 1, 2)], out=out, stats=True)     # nothing to decode: zeros, no launch
    assert frames is out and not out.any() and (fidx == -1).all() and status.tolist() == [0] * (2 * W) and tuple(stats.shape) == (0, 2)
    frames, fidx, status = store.decode([("b", 0)])
    assert tuple(frames.shape) == (1, W, 40, 56, 3) and not frames.any()
    side = torch.cuda.Stream(DEV)                                                  # on a side stream: the same bits
    with torch.cuda.stream(side):
        a = store.decode(fsc.ITEMS)
    side.synchronize()
    b = store.decode(fsc.ITEMS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    got = list(store.batches(fsc.ITEMS, 3))
    assert [tuple(g[0].shape[:2]) for g in got] == [(3, W), (3, W), (1, W)]
    assert torch.equal(torch.cat([g[0] for g in got]), b[0]) and torch.equal(torch.cat([g[1] for g in got]), b[1])
    with pytest.raises(ValueError):
        store.decode(fsc.ITEMS, out=out)                                          # the wrong shape
    with pytest.raises(ValueError):
        store.decode([("a", 4)])
    with pytest.raises(ValueError):
        store.decode(fsc.ITEMS, walk="fast")
    with pytest.raises(ValueError):
        list(store.batches(fsc.ITEMS, 0))
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1), pytest.raises(_lib.M3THipError):
            store.decode(fsc.ITEMS)


def test_damaged_store_equals_pack_and_decode():
    jpeg = _jpeg()
    videos, names = fsc.damaged_video()
    n = len(names)
    store = jpeg.FrameStore(videos, n, chunk_bytes=1 << 16)
    assert len(store.chunks) > 1
    packed = jpeg.pack(videos["damaged"])
    for walk in ("sequential", "parallel", "auto"):
        frames, fidx, status = store.decode([("damaged", 0)], order="rgb", walk=walk)
        want_frames, want_status = jpeg.decode(packed, order="rgb", walk=walk)
        assert torch.equal(frames[0], want_frames) and torch.equal(status, want_status), walk
        count = jpeg_cases.check_damaged_result(names, frames[0].cpu().numpy(), status.cpu().numpy())
        assert count["flagged"] >= 22 and count["neighbour"] >= 28
    assert fidx[0].tolist() == list(range(n))


def test_large_segments_travel_through_the_gather():
    """walk="auto": the fixtures of tests/golden/jpeg_par_cases.npz, those that share a size in one store (with the 45 KB frame of
    jpeg_cases beside the 256 x 256 one), the others in a store each"""
    jpeg = _jpeg()
    cases = dict(_par_cases())
    cases["full_256_q95"] = CASES["full_256_q95"]
    by_size = {}
    for name in sorted(cases):
        by_size.setdefault(cases[name][1].shape[:2], []).append(name)
    assert sorted(len(v) for v in by_size.values()) == [1, 1, 1, 2, 2]
    above = 0
    for size, group in sorted(by_size.items()):
        row = [group[0], None] + group[::-1] + group                              # every frame twice, in two orders
        store = jpeg.FrameStore({"v": [None if n is None else cases[n][0] for n in row]}, len(row), chunk_bytes=1 << 16)
        above += int((store.records.segs[:, 1] >= jpeg.AUTO_MIN_BYTES).sum())
        items = [("v", 0), ("v", 1, len(row) - 1)]
        frames, fidx, status = store.decode(items, order="rgb", walk="auto")
        flat = fsc.flat_names({"v": row}, items, len(row))
        assert not status.any() and np.array_equal(frames.view((-1,) + size + (3,)).cpu().numpy(), _golden_frames(flat, "rgb", cases)), group
    assert above >= 4                                                             # (the 45 KB frame and the 4 KB noise frame, three times each)


def test_store_feeds_the_ingest(tmp_path):
    """the ingest of a store-built batch has the bits of the ingest of jpeg.load_clips of the same windows (256 x 256 tracks: crop 224,
    halve to 112)"""
    jpeg = _jpeg()
    from m3t import video
    full, flat_ = CASES["full_256_q95"][0], _par_cases()["p_flat_420_q30"][0]
    path = str(tmp_path / "00002.jpg")
    with open(path, "wb") as f:
        f.write(flat_)
    videos = {"x": [None, full, path, str(tmp_path / "missing.jpg"), flat_, full], "y": [full, None, None, flat_]}
    store = jpeg.FrameStore(videos, W)
    items = [("x", 0), ("y", 0), ("x", 2, 4), ("y", 1, 2), ("x", 3, 3)]
    frames, fidx, status = store.decode(items)
    assert not status.any()
    clips, tls = [], []
    for v, start, *tl in items:
        tl = tl[0] if tl else W
        clips.append([videos[v][start + t] if t < tl else None for t in range(W)])
        tls.append(tl)
    host_frames, present, _ = jpeg.load_clips(clips)
    want_idx = np.stack([video.frame_index(present[n][:tl], 0, tl, W) for n, tl in enumerate(tls)])
    assert torch.equal(frames, host_frames) and np.array_equal(fidx.numpy(), want_idx)
    assert fidx.tolist() == [[-1, 1, 2, 2], [0, 0, 0, 3], [0, 0, 2, 3], [-1, -1, -1, -1], [-1, 1, 2, 2]]
    random.seed(5)
    np.random.seed(5)
    aug = [video.draw_affwild(256, True, True, True, mirror=bool(n % 2), resize=True) for n in range(len(items))]
    got = video.ingest(frames, aug, fidx, "planes")
    want = video.ingest(host_frames, aug, want_idx, "planes")
    assert tuple(got.shape) == (len(items), 3, W, 112, 112) and torch.equal(got, want)


def test_store_agrees_with_the_track_store(family):
    from m3t import dataset
    videos, names, store = family
    tracks = dataset.TrackStore({v: {"nb_frames": len(names[v]), "fps": 30.0, "se": np.zeros((len(names[v]), 4), np.float32),
                                     "has_image": store.has_image(v)} for v in names}, W, "test", se_dim=4)
    batch = tracks.collate(fsc.ITEMS)
    _, fidx, _ = store.decode(fsc.ITEMS)
    assert batch["video_frame_idx"].dtype == fidx.dtype and torch.equal(batch["video_frame_idx"], fidx)
    assert batch["vid_name"] == [it[0] if isinstance(it[0], str) else store.names[it[0]] for it in fsc.ITEMS]
