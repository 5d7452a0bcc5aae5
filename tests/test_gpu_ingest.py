"""The video ingest on the MI355X (csrc/ingest.hip, m3t/video.py): every comparison here is exact.  The kernel only gathers from 256-entry
tables, so its output must have the bits of the reference's loaders followed by float32 `(x - 127.5) / 127.5` (tests/golden/ingest.npz), of
the numpy restatement (tests/ingest_ref.py) at the shapes where the kernel can go wrong, and -- through the models -- of the float32 route
on the same frames and draws."""
import argparse
import copy
import ctypes
import random

import numpy as np
import pytest
import torch

import ingest_ref
from golden.recipe import fill_module, draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ingest_ref.load_golden()
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
    video = _video()
    fr = torch.from_numpy(frames) if isinstance(frames, np.ndarray) else frames
    want = torch.from_numpy(want).to(DEV)
    p = video.ingest(fr, aug, fidx, "planes", norm)
    assert p.dtype == torch.float32 and p.shape == want.shape and torch.equal(p, want)
    v = video.ingest(fr, aug, fidx, "cl", norm)
    from m3t import ops
    assert isinstance(v, ops.VideoCL) and v.C == 4 and (v.N, v.T, v.H, v.W) == (want.shape[0],) + tuple(want.shape[2:])
    rgb, fourth = _planes(v)
    assert torch.equal(rgb, want)
    assert torch.equal(fourth, torch.zeros_like(fourth)) and not bool(torch.signbit(fourth).any())
    _slot_ok(v)
    assert torch.equal(v.planes(), want)
    return v


def _aug(cy=0, cx=0, size=35, mirror=False, cutout=None, table=None):
    return {"cy": cy, "cx": cx, "size": size, "mirror": mirror, "cutout": cutout, "table": table}


# ------------------------------------------------------------------ operator
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_golden_cases_in_both_layouts(c):
    video = _video()
    aug, fidx = ingest_ref.case_params(video, c)
    _both_layouts(c["frames"][None], [aug], fidx[None], c["out"][None])


@pytest.mark.parametrize("cx", [0, 1, 2, 3, 4, 5])
def test_odd_width_and_every_byte_alignment(cx):
    """W = 35 (odd, no multiple of 4), 3 cx mod 4 in {0, 3, 2, 1, 0, 3}; three row tiles per frame, two clips with different windows"""
    video = _video()
    rs = np.random.RandomState(100 + cx)
    frames = rs.randint(0, 256, (2, 3, 40, 41, 3)).astype(np.uint8)
    aug = [_aug(cy=5, cx=cx, mirror=bool(cx & 1), cutout=(3, 20, 0, 17)), _aug(cy=0, cx=5 - cx, mirror=not (cx & 1), cutout=(30, 35, 9, 35))]
    _both_layouts(frames, aug, None, ingest_ref.batch_ref(video, frames, aug))


@pytest.mark.parametrize("mirror", [False, True])
def test_last_row_ends_at_the_final_byte_of_an_odd_sized_buffer(mirror):
    """N = T = 1, 5 x 5 frames (75 bytes: no multiple of 4), the 3 x 3 window in the last corner"""
    video = _video()
    frames = np.random.RandomState(7).randint(0, 256, (1, 1, 5, 5, 3)).astype(np.uint8)
    aug = [_aug(cy=2, cx=2, size=3, mirror=mirror)]
    _both_layouts(frames, aug, None, ingest_ref.batch_ref(video, frames, aug))
    # the same bytes as the tail of a tensor whose storage ends with them
    buf = torch.zeros(5 * 75, dtype=torch.uint8)
    buf[-75:] = torch.from_numpy(frames.reshape(-1))
    _both_layouts(buf[-75:].view(1, 1, 5, 5, 3).to(DEV), aug, None, ingest_ref.batch_ref(video, frames, aug))


def test_one_clip_one_frame_no_draws():
    video = _video()
    frames = np.random.RandomState(8).randint(0, 256, (1, 1, 9, 11, 3)).astype(np.uint8)
    v = _both_layouts(frames, None, None, ingest_ref.batch_ref(video, frames))
    assert (v.H, v.W) == (9, 11)


def test_shared_table_against_per_clip_tables():
    from m3t import ops
    video = _video()
    rs = np.random.RandomState(9)
    frames = rs.randint(0, 256, (3, 2, 40, 40, 3)).astype(np.uint8)
    tabs = [video.jitter_table(0.93, 1.07), None, video.jitter_table(1.09, 0.91)]
    aug = [_aug(cy=n, cx=n + 1, table=tabs[n]) for n in range(3)]
    _both_layouts(frames, aug, None, ingest_ref.batch_ref(video, frames, aug))
    # one table for all clips = the same table once per clip
    fr = torch.from_numpy(frames).to(DEV)
    geom = torch.zeros(3, 8, dtype=torch.int32, device=DEV)
    lut = torch.from_numpy(video.jitter_lut(1.05, 0.95)).to(DEV)
    for layout in ("cl", "planes"):
        a = ops.video_ingest(fr, None, 2, geom, lut, 40, 40, layout)
        b = ops.video_ingest(fr, None, 2, geom, lut.repeat(3, 1).contiguous(), 40, 40, layout)
        if layout == "cl":
            assert int(a.slot.item()) == int(b.slot.item())
            a, b = a.data, b.data
        assert torch.equal(a, b)
    want = ingest_ref.ingest_ref(frames, np.zeros((3, 8), np.int32), None, video.jitter_lut(1.05, 0.95), 40, 40)
    assert torch.equal(b, torch.from_numpy(want).to(DEV))


def test_frame_indices_blank_rows_repeats_and_more_frames_than_stored():
    video = _video()
    rs = np.random.RandomState(10)
    frames = rs.randint(0, 256, (3, 2, 40, 40, 3)).astype(np.uint8)
    fidx = np.array([[-1, -1, -1, -1, -1], [1, 0, 0, 1, 1], [-1, 0, 0, 1, 1]], np.int32)          # T = 5 > Ts = 2; clip 0 has no frame at all
    aug = [_aug(cy=1, cx=1, cutout=(0, 9, 0, 9)), _aug(cy=2, cx=3, mirror=True), _aug(cy=5, cx=0)]
    want = ingest_ref.batch_ref(video, frames, aug, fidx)
    assert np.array_equal(want[0, :, :, 20, 20], np.full((3, 5), -1.0, np.float32))                # (zeros normalise to -1)
    _both_layouts(frames, aug, fidx, want)
    _both_layouts(frames, aug, torch.from_numpy(fidx).long(), want)


def test_empty_cutout_and_cutout_over_the_whole_frame():
    video = _video()
    frames = np.random.RandomState(11).randint(0, 256, (2, 2, 40, 40, 3)).astype(np.uint8)
    aug = [_aug(cy=1, cx=2, cutout=(7, 7, 3, 30)), _aug(cy=4, cx=3, cutout=(0, 35, 0, 35))]
    want = ingest_ref.batch_ref(video, frames, aug)
    assert not want[1].any() and np.abs(want[0]).max() == 1.0
    v = _both_layouts(frames, aug, None, want)
    whole = video.ingest(torch.from_numpy(frames[1:]), aug[1:], None, "cl")                         # nothing but the hole: the slot stays 0
    assert int(whole.slot.item()) == 0 and not bool(whole.data.any())
    assert int(v.slot.item()) == int(np.float32(1.0).view(np.uint32))


def test_non_contiguous_and_misaligned_inputs_are_made_contiguous():
    video = _video()
    rs = np.random.RandomState(12)
    big = rs.randint(0, 256, (2, 4, 40, 44, 3)).astype(np.uint8)
    aug = [_aug(cy=2, cx=1), _aug(cy=0, cx=4, mirror=True)]
    view = torch.from_numpy(big).to(DEV)[:, ::2, :, 2:42]                                          # every other frame, a column window
    assert not view.is_contiguous()
    frames = np.ascontiguousarray(big[:, ::2, :, 2:42])
    want = ingest_ref.batch_ref(video, frames, aug)
    _both_layouts(view, aug, None, want)
    _both_layouts(torch.from_numpy(big)[:, ::2, :, 2:42], aug, None, want)                         # the same view of a host tensor
    buf = torch.zeros(frames.size + 16, dtype=torch.uint8, device=DEV)
    off = next(o for o in range(1, 16) if (buf.data_ptr() + o) % 16 == 1)
    buf[off:off + frames.size] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    mis = buf[off:off + frames.size].view(frames.shape)
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 1
    _both_layouts(mis, aug, None, want)


def test_c_abi_argument_checks():
    from m3t import _lib, ops
    lib, st = ops.lib(), ops._stream()
    fr = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    geom = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    lut = torch.zeros(256, dtype=torch.float32, device=DEV)
    out = torch.full((2 * 8 * 8 * 4 + 4,), 5.0, dtype=torch.float32, device=DEV)
    p = lambda t: t.data_ptr()
    call = lambda *a: lib.m3t_video_ingest(*a, st)
    E = _lib.M3T_EINVAL
    assert call(None, 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == E                 # null pointers
    assert call(p(fr), 1, 2, 8, 8, None, 2, None, p(lut), 0, 8, 8, 0, p(out)) == E
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), None, 0, 8, 8, 0, p(out)) == E
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, None) == E
    assert call(p(fr) + 4, 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == E            # misaligned frames / out / tables
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out) + 4) == E
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom) + 2, p(lut), 0, 8, 8, 0, p(out)) == E
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), p(lut) + 1, 0, 8, 8, 0, p(out)) == E
    for bad in ((1, 0, 8, 8, 2, 8, 8), (1, 2, 0, 8, 2, 8, 8), (1, 2, 8, -1, 2, 8, 8), (1, 2, 8, 8, 2, 0, 8), (1, 2, 8, 8, 2, 8, 0),
                (-1, 2, 8, 8, 2, 8, 8), (1, 2, 8, 8, -2, 8, 8), (1, 2, 8, 8, 2, 9, 8), (1, 2, 8, 8, 2, 8, 9), (1, 2, 8, 8, 3, 8, 8)):
        N, Ts, Hs, Ws, T, H, W = bad                                                                 # non-positive sizes, window > frame, T > Ts without indices
        assert call(p(fr), N, Ts, Hs, Ws, None, T, p(geom), p(lut), 0, H, W, 0, p(out)) == E, bad
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), p(lut), 128, 8, 8, 0, p(out)) == E              # table stride, layout
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 2, p(out)) == E
    assert call(p(fr), 0, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0                # nothing to do
    assert call(p(fr), 1, 2, 8, 8, None, 0, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0
    assert bool((out == 5.0).all()), "a refused or empty call wrote"
    # a refused call still consumes an armed slot: the next producer does not raise it
    slot = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.amax_out(slot.data_ptr())
    assert call(None, 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == E
    lut.fill_(3.0)
    assert call(p(fr), 1, 2, 8, 8, None, 2, p(geom), p(lut), 0, 8, 8, 0, p(out)) == 0
    assert int(slot.item()) == 0 and bool((out[:-4].view(-1, 4)[:, :3] == 3.0).all()) and bool((out[-4:] == 5.0).all())


# ------------------------------------------------------------------ chain
def _clips(seed, N, Ts, size):
    return np.random.RandomState(seed).randint(0, 256, (N, Ts, size, size, 3)).astype(np.uint8)


def _aff_draws(seed, N, size=128, cutout=True):
    video = _video()
    random.seed(seed)
    np.random.seed(seed)
    return [video.draw_affwild(size, True, True, cutout, random.random() > 0.5) for _ in range(N)]


def _run_stem(model, x, extra, ct):
    """(output, gradient of the first convolution's weight) of a fresh copy of `model` (train mode moves the BatchNorm buffers)"""
    m = copy.deepcopy(model)
    y = m(x, *extra)
    (y * ct).sum().backward()
    first = next(mod for mod in m.modules() if isinstance(mod, torch.nn.Conv3d))
    torch.cuda.synchronize()
    return y.detach(), first.weight.grad.detach().clone()


@pytest.mark.parametrize("which", ["vggm_split", "resnet3d"])
def test_first_convolution_takes_the_ingest_output(which):
    """VA_3DVGGM_Split (defaults; the channels-last chain) at N = 2, T = 4 and VA_3DResNet (planes) at N = 1, T = 4, 128 -> 112, train mode:
    output and first-layer weight gradient of the uint8 route equal the float32 route's on the reference-style input, bit for bit."""
    from m3t import ops
    from models.backbone import VA_3DVGGM_Split, VA_3DResNet
    video = _video()
    N, T = (2, 4) if which == "vggm_split" else (1, 4)
    rs = np.random.RandomState(21)
    frames = _clips(22, N, T, 128)
    aug = _aff_draws(23, N)
    fidx = np.stack([video.frame_index([1, 1, 0, 1], 0, 4, 4), video.frame_index([0, 1, 1, 1], 0, 4, 4)][:N])
    x32 = torch.from_numpy(ingest_ref.batch_ref(video, frames, aug, fidx)).to(DEV)                  # the reference's output for these frames and draws
    if which == "vggm_split":
        model = fill_module(VA_3DVGGM_Split(frameLen=T), 24).to(DEV).train()
        extra = (torch.from_numpy(draw(rs, (N, 512, T))).to(DEV), torch.from_numpy(draw(rs, (N, 512, T))).to(DEV))
        layout = "cl"
        assert model.shared[0].cl_chain and ops.conv3d_cl_ok(x32, model.shared[0].weight, (1, 2, 2), (1, 0, 0), 1, (1, 1, 1), "zeros")
    else:
        model = fill_module(VA_3DResNet(frameLen=T), 24).to(DEV).train()
        extra, layout = (), "planes"
        assert not model.c3d[0].cl_chain
    with torch.no_grad():
        shape = copy.deepcopy(model)(x32, *extra).shape
    ct = torch.from_numpy(draw(rs, tuple(shape))).to(DEV)
    y_a, g_a = _run_stem(model, x32, extra, ct)
    y_b, g_b = _run_stem(model, x32, extra, ct)
    assert torch.equal(y_a, y_b) and torch.equal(g_a, g_b), "the float32 route does not reproduce itself"
    walks = ops.CONV3D_CALLS["walk"]
    x8 = video.ingest(torch.from_numpy(frames), aug, fidx, layout)
    assert isinstance(x8, ops.VideoCL) == (layout == "cl")
    y_c, g_c = _run_stem(model, x8, extra, ct)
    assert torch.equal(y_c, y_a), "output"
    assert torch.equal(g_c, g_a), "gradient of the first convolution's weight"
    if layout == "cl":
        assert ops.CONV3D_CALLS["walk"] > walks          # (the chain took the VideoCL: no fall-back to its planes)


# ------------------------------------------------------------------ modules
def _hp(cls, **kw):
    ns = cls.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _step_and_params(model, hp, batch):
    """loss of training_step on one copy, parameters after one Trainer.step on another"""
    from m3t.trainer import Trainer
    loss = copy.deepcopy(model).training_step(batch, 0)["loss"].detach().clone()
    m = copy.deepcopy(model)
    tr = Trainer.from_hparams(m, hp, checkpoint_path=None)
    out = tr.step(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"]))
    return loss, [p.detach().clone() for p in m.parameters()], out["loss"].detach().clone()


def _same_steps(model, hp, b32, b8):
    l_a, p_a, s_a = _step_and_params(model, hp, b32)
    l_b, p_b, s_b = _step_and_params(model, hp, b32)
    assert torch.equal(l_a, l_b) and torch.equal(s_a, s_b) and all(torch.equal(a, b) for a, b in zip(p_a, p_b)), \
        "the float32 route does not reproduce itself"
    l_c, p_c, s_c = _step_and_params(model, hp, b8)
    assert torch.equal(l_c, l_a) and torch.equal(s_c, s_a), (float(l_c), float(l_a))
    moved = sum(not torch.equal(a, b) for a, b in zip(p_a, model.parameters()))
    assert moved > 0
    for (n, _), a, c in zip(model.named_parameters(), p_a, p_c):
        assert torch.equal(a, c), n


def test_affwild_uint8_batch_equals_float32_batch():
    """AffWild2VA (visual, v2p_split, window 4): a uint8 batch with draws and frame indices against the float32 batch the reference's loader
    makes of the same frames -- equal loss, equal parameters after one Trainer.step"""
    from models.model import AffWild2VA
    video = _video()
    B, T = 2, 4
    hp = _hp(AffWild2VA, modality="visual", backbone="v2p_split", window=T, learning_rate=1e-3)
    model = fill_module(AffWild2VA(hp), 31).to(DEV).train()
    rs = np.random.RandomState(32)
    frames = _clips(33, B, 3, 128)
    aug = _aff_draws(34, B)
    fidx = np.stack([video.frame_index([1, 0, 1], 0, 3, T), video.frame_index([0, 1, 1], 0, 3, T)])      # repeats, a blank first frame, edge padding
    dev = lambda a: torch.from_numpy(a).to(DEV)
    rest = {"se_features": dev(draw(rs, (B, 512, T))), "label_valence": dev(draw(rs, (B, T), "uniform_pm1")),
            "label_arousal": dev(draw(rs, (B, T), "uniform_pm1")), "class_expr": dev(rs.randint(0, 7, (B, T)).astype(np.int64)),
            "expr_valid": dev(rs.uniform(size=(B, T)) < 0.7)}
    b32 = dict(rest, video=dev(ingest_ref.batch_ref(video, frames, aug, fidx, raw=True)))
    b8 = dict(rest, video=torch.from_numpy(frames), video_aug=aug, video_frame_idx=fidx)
    assert b32["video"].shape == (B, 3, T, 112, 112) and float(b32["video"].max()) == 255.0
    _same_steps(model, hp, b32, b8)


def test_vox2_uint8_batch_with_jitter_equals_float32_batch():
    from models.vox2_model import VoxCeleb2_1k
    video = _video()
    B, T = 2, 3
    hp = _hp(VoxCeleb2_1k, window=T, learning_rate=1e-3)
    model = fill_module(VoxCeleb2_1k(hp), 41).to(DEV).train()
    frames = _clips(42, B, T, 128)
    random.seed(43)
    aug = [video.draw_vox2(128, True, True) for _ in range(B)]
    assert all(a["table"] is not None for a in aug)
    label = torch.from_numpy(np.random.RandomState(44).randint(0, 1000, (B,)).astype(np.int64)).to(DEV)
    b32 = {"video": torch.from_numpy(ingest_ref.batch_ref(video, frames, aug, raw=True)).to(DEV), "label": label}
    b8 = {"video": torch.from_numpy(frames).to(DEV), "label": label, "video_aug": aug}
    _same_steps(model, hp, b32, b8)
    # forward() takes the frames too
    m = copy.deepcopy(model).eval()
    with torch.no_grad():
        assert torch.equal(m(b8["video"], aug), m(b32["video"]))
