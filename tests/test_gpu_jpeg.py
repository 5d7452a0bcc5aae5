"""The batched JPEG decode on the MI355X (csrc/jpeg.hip: m3t_jpeg_decode; m3t/jpeg.py): every comparison here is exact.  The kernels run
libjpeg's integer rules, so the frames must have the bits Pillow (libjpeg-turbo) decoded into tests/golden/jpeg_cases.npz, damaged streams
must say so in their status word without touching a neighbour, and the video ingest of decoded frames must equal the ingest of the
frames the host decoder made."""
import random

import numpy as np
import pytest
import torch

import jpeg_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES, _ = jpeg_cases.load()


def _jpeg():
    from m3t import jpeg
    return jpeg


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_golden_in_both_orders(name):
    jpeg = _jpeg()
    data, rgb = CASES[name]
    b = jpeg.pack([data])
    for order, want in (("bgr", rgb[..., ::-1]), ("rgb", rgb)):
        frames, status = jpeg.decode(b, order=order)
        assert frames.dtype == torch.uint8 and frames.is_cuda and tuple(frames.shape) == (1,) + rgb.shape
        assert status.dtype == torch.int32 and status.is_cuda and status.tolist() == [0]
        assert np.array_equal(frames[0].cpu().numpy(), want), order
    frames, _ = jpeg.decode(b)
    assert np.array_equal(frames[0].cpu().numpy(), rgb[..., ::-1])               # the default is cv2.imread's order


def test_family_batch_into_scattered_slots_on_two_streams():
    jpeg = _jpeg()
    names = jpeg_cases.FAMILY
    b = jpeg.pack([CASES[n][0] for n in names])
    slots = [(2, 3), (0, 0), (1, 2), (0, 3), (2, 0), (1, 1), (0, 1), (2, 2)]
    results = []
    for stream in (None, torch.cuda.Stream(DEV)):
        out = torch.full((3, 4, 40, 56, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        if stream is None:
            frames, status = jpeg.decode(b, out=out, slots=slots, order="rgb")
        else:
            with torch.cuda.stream(stream):
                frames, status = jpeg.decode(b, out=out, slots=slots, order="rgb")
            stream.synchronize()
        assert frames is out and status.tolist() == [0] * 8
        got = out.cpu().numpy()
        for n, (c, t) in zip(names, slots):
            assert np.array_equal(got[c, t], CASES[n][1]), n
        for c in range(3):
            for t in range(4):
                if (c, t) not in slots:
                    assert (got[c, t] == jpeg_cases.CANARY).all(), (c, t)
        results.append(got)
    assert np.array_equal(results[0], results[1])
    with pytest.raises(ValueError):
        jpeg.decode(b, out=out, slots=slots[:-1] + [slots[0]])
    with pytest.raises(ValueError):
        jpeg.decode(b, out=out, slots=slots[:-1] + [(3, 0)])
    with pytest.raises(ValueError):
        jpeg.decode(b, out=out[..., :2].contiguous(), slots=slots)


def test_load_clips_feeds_the_ingest(tmp_path):
    """None entries and a path that does not exist are the reference's `img is None`; the ingest of the decoded frames has the bits of the
    ingest of the host-decoded ones (256 x 256 tracks: crop 224, halve to 112)"""
    jpeg = _jpeg()
    from m3t import video
    data, rgb = CASES["full_256_q95"]
    path = str(tmp_path / "00001.jpg")
    with open(path, "wb") as f:
        f.write(data)
    clips = [[None, data, path, str(tmp_path / "missing.jpg")], [path, None, None, data]]
    frames, present, status = jpeg.load_clips(clips)
    assert tuple(frames.shape) == (2, 4, 256, 256, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    assert present.tolist() == [[False, True, True, False], [True, False, False, True]] and status.tolist() == [0] * 8
    host = np.zeros((2, 4, 256, 256, 3), np.uint8)
    host[present] = rgb[..., ::-1]                                                # cv2.imread's order
    assert np.array_equal(frames.cpu().numpy(), host)
    fidx = np.stack([video.frame_index(present[n], 0, 4, 6) for n in range(2)])
    assert fidx.tolist() == [[-1, 1, 2, 2, 2, 2], [0, 0, 0, 3, 3, 3]]            # dataset.py:64-68 and :312
    random.seed(5)
    np.random.seed(5)
    aug = [video.draw_affwild(256, True, True, True, mirror=bool(n), resize=True) for n in range(2)]
    got = video.ingest(frames, aug, fidx, "planes")
    want = video.ingest(torch.from_numpy(host), aug, fidx, "planes")
    assert tuple(got.shape) == (2, 3, 6, 112, 112) and torch.equal(got, want)


def test_damaged_streams_keep_to_themselves():
    jpeg = _jpeg()
    items, names = jpeg_cases.damaged_batch()
    b = jpeg.pack(items)
    n = b.n
    out = torch.full((n, 2, 40, 56, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    frames, status = jpeg.decode(b, out=out, slots=[(i, 1) for i in range(n)], order="rgb")
    got = out.cpu().numpy()
    assert (got[:, 0] == jpeg_cases.CANARY).all()
    count = jpeg_cases.check_damaged_result(names, got[:, 1], status.cpu().numpy())
    print(count)
    assert count["flagged"] >= 22 and count["neighbour"] >= 28                   # (20 truncations + 2 restart cases at the least)


def test_raw_abi_misuse_is_einval():
    jpeg = _jpeg()
    from m3t import _lib
    lib = _lib.load()
    b = jpeg.pack([CASES["f_420_q95"][0], CASES["f_rst_blocks2"][0]])
    n, H, W = b.n, b.height, b.width
    s_d = b.stream.to(DEV)
    out = torch.full((n, H, W, 3), jpeg_cases.CANARY, dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.m3t_jpeg_workspace_bytes(n, H, W)), dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(tables, n_=n, stream_bytes=None, ws_bytes=None):
        t = np.ascontiguousarray(tables, np.int32)
        t_d = torch.from_numpy(t).to(DEV)
        return lib.m3t_jpeg_decode(s_d.data_ptr(), s_d.numel() if stream_bytes is None else stream_bytes, t.ctypes.data, t_d.data_ptr(), n_,
                                   b.n_segs, b.n_quant, b.n_huff, H, W, out.data_ptr(), n, 0, ws.data_ptr(),
                                   ws.numel() if ws_bytes is None else ws_bytes, status.data_ptr(), st)

    outside = b.tables.copy()
    outside[n * jpeg.IMG_COLS + 1] = s_d.numel() - 8                              # the first segment now ends past the stream buffer
    slot = b.tables.copy()
    slot[n * jpeg.IMG_COLS + b.n_segs * jpeg.SEG_COLS] = n
    for rc in (call(outside), call(b.tables, n_=0), call(b.tables, n_=-1), call(slot), call(b.tables, ws_bytes=ws.numel() - 1),
               call(b.tables, stream_bytes=s_d.numel() - 16 * 200)):
        assert rc == _lib.M3T_EINVAL
    torch.cuda.synchronize()
    assert (out == jpeg_cases.CANARY).all() and status.tolist() == [-1] * n       # refused before anything was launched
    assert call(b.tables) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and np.array_equal(out[0].cpu().numpy(), CASES["f_420_q95"][1][..., ::-1])
