"""The halving video ingest on the MI355X (csrc/ingest.hip: m3t_video_ingest_half; m3t/video.py: draws with "scale": 2): every comparison
here is exact.  The kernel averages 2 x 2 blocks in integers, (a + b + c + d + 2) >> 2, and gathers from 256-entry tables, so its output
must have the bits of the reference's loader at input_size 256 followed by float32 `(x - 127.5) / 127.5` (tests/golden/ingest_resize.npz,
whose cv2.resize is that rule), of the numpy restatement (tests/ingest_resize_ref.py) at the shapes where the kernel can go wrong, and --
through a model -- of the float32 route on the same frames and draws."""
import argparse
import copy
import random

import numpy as np
import pytest
import torch

import ingest_resize_ref as R
from golden.recipe import fill_module, draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.load_golden()
IDS = [c["name"] for c in CASES]


def _video():
    from m3t import video
    return video


def _planes(v):
    """a VideoCL's three real channels as [N, 3, T, H, W], and its fourth channel"""
    d = v.data.view(v.N, v.T, v.H, v.W, 4)
    return d[..., :3].permute(0, 4, 1, 2, 3).contiguous(), d[..., 3]


def _slot_ok(v):
    """the raised slot holds the bits of max |out| (epoch 0)"""
    want = int(np.float32(float(v.data.abs().max())).view(np.uint32))
    assert int(v.slot.item()) == want, (hex(int(v.slot.item())), hex(want))


def _both_layouts(frames, aug, fidx, want, norm=None):
    """frames (array or tensor) through m3t.video.ingest in both layouts against `want` [N, 3, T, H, W] (numpy)"""
    from m3t import ops
    video = _video()
    assert video.batch_scale(aug) == 2
    fr = torch.from_numpy(frames) if isinstance(frames, np.ndarray) else frames
    want = torch.from_numpy(want).to(DEV)
    p = video.ingest(fr, aug, fidx, "planes", norm)
    assert p.dtype == torch.float32 and p.shape == want.shape and torch.equal(p, want)
    v = video.ingest(fr, aug, fidx, "cl", norm)
    assert isinstance(v, ops.VideoCL) and v.C == 4 and (v.N, v.T, v.H, v.W) == (want.shape[0],) + tuple(want.shape[2:])
    rgb, fourth = _planes(v)
    assert torch.equal(rgb, want)
    assert torch.equal(fourth, torch.zeros_like(fourth)) and not bool(torch.signbit(fourth).any())
    _slot_ok(v)
    assert torch.equal(v.planes(), want)
    return v


def _aug(cy=0, cx=0, size=70, mirror=False, cutout=None, table=None):
    return {"cy": cy, "cx": cx, "size": size, "mirror": mirror, "cutout": cutout, "table": table, "scale": 2}


# ------------------------------------------------------------------ operator
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_golden_cases_in_both_layouts(c):
    video = _video()
    aug, fidx = R.case_params(video, c)
    v = _both_layouts(c["frames"][None], [aug], fidx[None], c["out"][None])
    assert (v.H, v.W) == (112, 112)


@pytest.mark.parametrize("cx", [0, 1, 2, 3, 4, 5, 6, 7])
def test_odd_width_and_every_granule_alignment(cx):
    """output 35 x 35 (odd; three row tiles of 16, 16, 3) from a 70 x 70 window in 80 x 81 frames: 6 cx mod 16 takes its eight values (and the
    odd row pitch of 243 bytes moves every row's floor); two clips with different windows, mirrors and cutouts, T = 3"""
    video = _video()
    rs = np.random.RandomState(200 + cx)
    frames = rs.randint(0, 256, (2, 3, 80, 81, 3)).astype(np.uint8)
    aug = [_aug(cy=5, cx=cx, mirror=bool(cx & 1), cutout=(3, 20, 0, 17)), _aug(cy=10, cx=11 - cx, mirror=not (cx & 1), cutout=(30, 35, 9, 35))]
    _both_layouts(frames, aug, None, R.batch_ref(video, frames, aug))


@pytest.mark.parametrize("mirror", [False, True])
def test_last_row_ends_at_the_final_byte_of_an_odd_sized_buffer(mirror):
    """N = T = 1, 7 x 7 frames (147 bytes: no multiple of 4), the 6 x 6 window in the last corner, a 3 x 3 output"""
    video = _video()
    frames = np.random.RandomState(7).randint(0, 256, (1, 1, 7, 7, 3)).astype(np.uint8)
    aug = [_aug(cy=1, cx=1, size=6, mirror=mirror)]
    want = R.batch_ref(video, frames, aug)
    assert want.shape == (1, 3, 1, 3, 3)
    _both_layouts(frames, aug, None, want)
    # the same bytes as the tail of a tensor whose storage ends with them
    buf = torch.zeros(5 * 147, dtype=torch.uint8)
    buf[-147:] = torch.from_numpy(frames.reshape(-1))
    _both_layouts(buf[-147:].view(1, 1, 7, 7, 3).to(DEV), aug, None, want)


def test_rounding_of_every_residue_and_the_extremes():
    """the hand-built frame of tests/ingest_resize_ref.py: block sums of every residue mod 4; four 255s give 255, 0 0 0 1 gives 0 and a
    sum of 2 rounds up to 1.  The identity table (raw pixel values) shows the averaged bytes themselves."""
    from m3t import ops
    video = _video()
    img, want = R.rounding_image()
    frames = img[None, None]
    aug = [_aug(size=8)]
    ref = R.batch_ref(video, frames, aug, norm=np.arange(256, dtype=np.float32))
    assert np.array_equal(ref[0, :, 0], want.transpose(2, 0, 1).astype(np.float32))
    assert ref[0, 0, 0, 0, 0] == 255.0 and ref[0, 0, 0, 0, 1] == 0.0 and ref[0, 0, 0, 0, 2] == 1.0
    _both_layouts(frames, aug, None, ref, norm=np.arange(256, dtype=np.float32))
    _both_layouts(frames, [_aug(size=8, mirror=True)], None, ref[..., ::-1].copy(), norm=np.arange(256, dtype=np.float32))
    _both_layouts(frames, aug, None, R.batch_ref(video, frames, aug))


def test_jitter_tables_follow_the_average_and_one_shared_table():
    from m3t import ops
    video = _video()
    rs = np.random.RandomState(9)
    frames = rs.randint(0, 256, (3, 2, 80, 80, 3)).astype(np.uint8)
    tabs = [video.jitter_table(0.93, 1.07), None, video.jitter_table(1.09, 0.91)]
    aug = [_aug(cy=n, cx=n + 1, table=tabs[n]) for n in range(3)]
    want = R.batch_ref(video, frames, aug)
    # the table is applied to the averaged byte, not to the four source bytes
    first = video.norm_lut()[tabs[0]][R.halve(frames[0, 0, 0:70, 1:71])]
    assert np.array_equal(want[0, :, 0], first.transpose(2, 0, 1))
    _both_layouts(frames, aug, None, want)
    # one table for all clips = the same table once per clip
    fr = torch.from_numpy(frames).to(DEV)
    geom = torch.zeros(3, 8, dtype=torch.int32, device=DEV)
    lut = torch.from_numpy(video.jitter_lut(1.05, 0.95)).to(DEV)
    for layout in ("cl", "planes"):
        a = ops.video_ingest_half(fr, None, 2, geom, lut, 40, 40, layout)
        b = ops.video_ingest_half(fr, None, 2, geom, lut.repeat(3, 1).contiguous(), 40, 40, layout)
        if layout == "cl":
            assert int(a.slot.item()) == int(b.slot.item())
            a, b = a.data, b.data
        assert torch.equal(a, b)
    want = R.ingest_half_ref(frames, np.zeros((3, 8), np.int32), None, video.jitter_lut(1.05, 0.95), 40, 40)
    assert torch.equal(b, torch.from_numpy(want).to(DEV))


def test_frame_indices_blank_rows_repeats_and_more_frames_than_stored():
    video = _video()
    rs = np.random.RandomState(10)
    frames = rs.randint(0, 256, (3, 2, 80, 80, 3)).astype(np.uint8)
    fidx = np.array([[-1, -1, -1, -1, -1], [1, 0, 0, 1, 1], [-1, 0, 0, 1, 1]], np.int32)          # T = 5 > Ts = 2; clip 0 has no frame at all
    aug = [_aug(cy=1, cx=1, cutout=(0, 9, 0, 9)), _aug(cy=2, cx=3, mirror=True), _aug(cy=10, cx=0)]
    want = R.batch_ref(video, frames, aug, fidx)
    assert np.array_equal(want[0, :, :, 20, 20], np.full((3, 5), -1.0, np.float32))                # (zeros normalise to -1)
    _both_layouts(frames, aug, fidx, want)


def test_c_abi_argument_checks():
    from m3t import _lib, ops
    lib, st = ops.lib(), ops._stream()
    fr = torch.zeros(1, 2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    geom = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    lut = torch.zeros(256, dtype=torch.float32, device=DEV)
    out = torch.full((2 * 8 * 8 * 4 + 4,), 5.0, dtype=torch.float32, device=DEV)
    p = lambda t: t.data_ptr()
    call = lambda *a: lib.m3t_video_ingest_half(*a, st)
    E = _lib.M3T_EINVAL
    assert call(None, 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == E               # null pointers
    assert call(p(fr), 1, 2, 16, 16, None, 2, None, p(lut), 0, 8, 8, 0, p(out)) == E
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), None, 0, 8, 8, 0, p(out)) == E
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, None) == E
    assert call(p(fr) + 4, 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == E          # misaligned frames / out / tables
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out) + 4) == E
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom) + 2, p(lut), 0, 8, 8, 0, p(out)) == E
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut) + 1, 0, 8, 8, 0, p(out)) == E
    for bad in ((1, 2, 15, 16, 2, 8, 8), (1, 2, 16, 15, 2, 8, 8), (1, 2, 16, 16, 2, 9, 8), (1, 2, 16, 16, 2, 8, 9),      # 2H > Hs, 2W > Ws
                (1, 2, 16, 16, 2, 16, 8), (1, 2, 16, 16, 2, 8, 16), (1, 2, 16, 16, 2, 8, 1 << 30), (1, 2, 16, 16, 2, 1 << 30, 8),
                (1, 0, 16, 16, 2, 8, 8), (1, 2, 0, 16, 2, 8, 8), (1, 2, 16, -1, 2, 8, 8), (1, 2, 16, 16, 2, 0, 8), (1, 2, 16, 16, 2, 8, 0),
                (-1, 2, 16, 16, 2, 8, 8), (1, 2, 16, 16, -2, 8, 8), (1, 2, 16, 16, 3, 8, 8)):
        N, Ts, Hs, Ws, T, H, W = bad                                                                 # ... non-positive sizes, T > Ts without indices
        assert call(p(fr), N, Ts, Hs, Ws, None, T, p(geom), p(lut), 0, H, W, 0, p(out)) == E, bad
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut), 128, 8, 8, 0, p(out)) == E            # table stride, layout
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 2, p(out)) == E
    assert call(p(fr), 0, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0              # nothing to do
    assert call(p(fr), 1, 2, 16, 16, None, 0, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0
    assert bool((out == 5.0).all()), "a refused or empty call wrote"
    # a refused call still consumes an armed slot: the next producer does not raise it
    slot = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.amax_out(slot.data_ptr())
    assert call(None, 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == E
    lut.fill_(3.0)
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0
    assert int(slot.item()) == 0 and bool((out[:-4].view(-1, 4)[:, :3] == 3.0).all()) and bool((out[-4:] == 5.0).all())
    # a window the device-side table puts outside the frame is clamped into it: the call reads nothing else and writes its 8 x 8 output
    geom[0, 0], geom[0, 1] = 1000, -1000
    assert call(p(fr), 1, 2, 16, 16, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0
    torch.cuda.synchronize()
    assert bool((out[-4:] == 5.0).all())


# ------------------------------------------------------------------ modules
def _hp(cls, **kw):
    ns = cls.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def test_affwild_uint8_256_batch_equals_float32_batch():
    """AffWild2VA (visual, v2p_split, window 2, one clip): a uint8 batch of 256 x 256 frames with resize=True draws and frame indices against
    the float32 112 x 112 batch the reference's loader makes of the same frames -- equal output and equal loss, bit for bit, in train mode"""
    from m3t import ops
    from models.model import AffWild2VA
    video = _video()
    B, T = 1, 2
    hp = _hp(AffWild2VA, modality="visual", backbone="v2p_split", window=T, learning_rate=1e-3)
    model = fill_module(AffWild2VA(hp), 31).to(DEV).train()
    rs = np.random.RandomState(52)
    frames = rs.randint(0, 256, (B, 3, 256, 256, 3)).astype(np.uint8)
    random.seed(54)
    np.random.seed(54)
    aug = [video.draw_affwild(256, True, True, True, random.random() > 0.5, resize=True) for _ in range(B)]
    assert aug[0]["scale"] == 2 and aug[0]["cutout"] is not None
    fidx = np.stack([video.frame_index([0, 1, 1], 0, 2, T)])                   # a blank first frame
    dev = lambda a: torch.from_numpy(a).to(DEV)
    rest = {"se_features": dev(draw(rs, (B, 512, T))), "label_valence": dev(draw(rs, (B, T), "uniform_pm1")),
            "label_arousal": dev(draw(rs, (B, T), "uniform_pm1")), "class_expr": dev(rs.randint(0, 7, (B, T)).astype(np.int64)),
            "expr_valid": dev(rs.uniform(size=(B, T)) < 0.7)}
    b32 = dict(rest, video=dev(R.batch_ref(video, frames, aug, fidx, raw=True)))
    b8 = dict(rest, video=torch.from_numpy(frames), video_aug=aug, video_frame_idx=fidx)
    assert b32["video"].shape == (B, 3, T, 112, 112) and float(b32["video"].max()) <= 255.0
    x8 = video.ingest_for(model.visual, b8["video"], aug, fidx)
    assert (x8.H, x8.W) == (112, 112) if isinstance(x8, ops.VideoCL) else tuple(x8.shape) == (B, 3, T, 112, 112)

    def run(batch):
        m = copy.deepcopy(model)
        y = m(batch).detach().clone()
        loss = copy.deepcopy(model).training_step(batch, 0)["loss"].detach().clone()
        torch.cuda.synchronize()
        return y, loss

    y_a, l_a = run(b32)
    y_b, l_b = run(b32)
    assert torch.equal(y_a, y_b) and torch.equal(l_a, l_b), "the float32 route does not reproduce itself"
    y_c, l_c = run(b8)
    assert bool(torch.isfinite(y_c).all()) and torch.equal(y_c, y_a), "output"
    assert torch.equal(l_c, l_a), (float(l_c), float(l_a))
