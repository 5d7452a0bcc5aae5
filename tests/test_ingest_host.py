"""CPU-side checks of the video ingest (m3t/video.py): its draws, frame indices and tables reproduce the parameters the reference's two
`load_video` functions used under the same seeds, the numpy restatement of the operator (tests/ingest_ref.py) reproduces every golden
output bit for bit, and the wrapper validates on the host before anything touches a device.  No GPU here."""
import random

import numpy as np
import pytest
import torch

import ingest_ref
from m3t import video

CASES = ingest_ref.load_golden()
IDS = [c["name"] for c in CASES]


def test_golden_covers_the_issues_cases():
    draws = {c["name"]: ingest_ref.case_params(video, c) for c in CASES}
    train = [a for n, (a, _) in draws.items() if "eval" not in n]
    assert {a["mirror"] for a in train} == {True, False}
    assert {a["cx"] % 2 for a in train} == {0, 1}
    cuts = [a["cutout"] for a in train if a["cutout"] is not None]
    assert any(c[1] - c[0] == 34 and c[3] - c[2] == 34 for c in cuts), "a cutout that no border clips"
    assert any(c[1] - c[0] < 34 or c[3] - c[2] < 34 for c in cuts), "a cutout clipped at a border"
    assert sum(a["table"] is not None for a in train) == 3, "three jitter draws"
    assert draws["aff_128_first"][1].tolist() == [-1, 1]                    # missing first frame: zeros
    assert draws["aff_40_middle"][1].tolist() == [1, 2, 2, 4]               # missing middle frame: the previous one
    assert draws["aff_40_last_pad"][1].tolist() == [0, 1, 2, 2, 2, 2]       # missing last frame, then edge padding
    for n in ("aff_40_eval", "vox_40_eval"):                                # eval: centred crop, nothing else
        a = draws[n][0]
        assert (a["cy"], a["cx"], a["mirror"], a["cutout"], a["table"]) == (40 // 16, 40 // 16, False, None, None)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_reproduces_the_reference_bit_for_bit(c):
    aug, fidx = ingest_ref.case_params(video, c)
    geom, fi, lut = ingest_ref.case_tables(video, aug, fidx)
    out = ingest_ref.ingest_ref(c["frames"][None], geom, fi, lut, aug["size"], aug["size"])
    assert out.shape[1:] == c["out"].shape and out.dtype == np.float32
    assert np.array_equal(out[0].view(np.uint32), c["out"].view(np.uint32))


def test_plan_packs_what_the_restatement_takes():
    c = CASES[1]
    aug, fidx = ingest_ref.case_params(video, c)
    T, H, W, geom, fi, tables = video.plan((1,) + c["frames"].shape, torch.uint8, [aug], fidx[None])
    g_ref, fi_ref, _ = ingest_ref.case_tables(video, aug, fidx)
    assert (T, H, W) == (c["window"], 35, 35) and np.array_equal(geom, g_ref) and np.array_equal(fi, fi_ref) and tables == [None]
    assert geom.dtype == np.int32 and fi.dtype == np.int32


def test_norm_and_jitter_tables():
    n = video.norm_lut()
    assert n.dtype == np.float32 and n.shape == (256,)
    assert np.array_equal(n, ((torch.arange(256, dtype=torch.float32) - 127.5) / 127.5).numpy())          # torch's float32 on the host
    assert np.array_equal(video.norm_lut("cpu"), n)
    # cv_augment.py:16,33 restated independently: python floats, clip, astype('uint8') (truncation)
    b, k = 1.0831, 0.9127
    bt = [min(max(int(i * b), 0), 255) for i in range(256)]
    ct = [min(max(int((i - 74) * k + 74), 0), 255) for i in range(256)]
    want = np.array([n[ct[bt[i]]] for i in range(256)], np.float32)
    assert np.array_equal(video.jitter_lut(b, k), want)
    assert np.array_equal(video.jitter_lut(1.0, 1.0), n)


def test_draws_consume_the_generators_in_the_references_order():
    random.seed(11)
    np.random.seed(11)
    a = video.draw_affwild(128, True, True, True, mirror=True)
    random.seed(11)
    np.random.seed(11)
    cx, cy = random.randint(0, 16), random.randint(0, 16)
    y, x = np.random.randint(112), np.random.randint(112)
    assert (a["cx"], a["cy"], a["size"]) == (cx, cy, 112)
    assert a["cutout"] == (max(y - 56, 0), min(y + 56, 112), max(x - 56, 0), min(x + 56, 112))
    random.seed(12)
    v = video.draw_vox2(128, True, True)
    random.seed(12)
    m, cx, cy = random.random() > 0.5, random.randint(0, 16), random.randint(0, 16)
    bf, cf = random.uniform(0.9, 1.1), random.uniform(0.9, 1.1)
    assert (v["mirror"], v["cx"], v["cy"]) == (m, cx, cy) and np.array_equal(v["table"], video.jitter_table(bf, cf))
    # eval mode: no crop or cutout draw is made; the VoxCeleb2 call site's mirror draw is
    random.seed(13)
    s0 = random.getstate()
    video.draw_affwild(128, False, True, True, mirror=True)
    assert random.getstate() == s0
    video.draw_vox2(128, False, True)
    s1 = random.getstate()
    random.seed(13)
    random.random()
    assert random.getstate() == s1
    e = video.draw_affwild(128, False, False, True)
    assert (e["cy"], e["cx"], e["size"], e["cutout"]) == (0, 0, 128, None)


def test_frame_index():
    assert video.frame_index([1, 1, 1], 0, 3, 3).tolist() == [0, 1, 2]
    assert video.frame_index([0, 0, 1, 0], 0, 4, 4).tolist() == [-1, -1, 2, 2]
    assert video.frame_index([1, 0, 1, 1], 1, 2, 4).tolist() == [-1, 2, 2, 2]       # a frame before `start` does not fill in
    assert video.frame_index([0, 0], 0, 2, 3).tolist() == [-1, -1, -1]
    assert video.frame_index([1, 1], 0, 2, 2).dtype == np.int32
    with pytest.raises(ValueError):
        video.frame_index([1, 1], 1, 2, 2)
    with pytest.raises(ValueError):
        video.frame_index([1, 1, 1], 0, 3, 2)


def _aug(cy=0, cx=0, size=35, mirror=False, cutout=None, table=None):
    return {"cy": cy, "cx": cx, "size": size, "mirror": mirror, "cutout": cutout, "table": table}


@pytest.mark.parametrize("frames,aug,fidx", [
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), [_aug(cy=6)], None),                       # crop window below the frame
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), [_aug(cx=-1)], None),
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), [_aug(size=41)], None),
    (torch.zeros(2, 2, 40, 40, 3, dtype=torch.uint8), [_aug(), _aug(size=34)], None),            # two output sizes in one batch
    (torch.zeros(2, 2, 40, 40, 3, dtype=torch.uint8), [_aug()], None),                           # one draw for two clips
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), [_aug(cutout=(0, 36, 0, 3))], None),       # cutout outside the output
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), None, [[0, 2]]),                           # frame index >= Ts
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), None, [[-2, 0]]),
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), None, [[0.0, 1.0]]),
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), None, [0, 1]),
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.float32), None, None),                             # wrong dtype
    (torch.zeros(1, 3, 2, 40, 40, dtype=torch.uint8), None, None),                               # planes, not frames as decoded
    (torch.zeros(2, 40, 40, 3, dtype=torch.uint8), None, None),
    (np.zeros((1, 2, 40, 40, 3), np.int8), None, None),
    (torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), [_aug(table=np.zeros(256, np.float32))], None),
])
def test_ingest_validates_on_the_host(frames, aug, fidx, monkeypatch):
    """ValueError before any device is touched: neither the availability query nor the library call is reached"""
    def touched(*a, **k):
        raise AssertionError("the wrapper reached the device before validating")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(video, "video_ingest", touched)
    for layout in ("cl", "planes"):
        with pytest.raises(ValueError):
            video.ingest(frames, aug, fidx, layout)


def test_resize_branch_and_layout_raise():
    for draw in (lambda: video.draw_affwild(256, True, True, False), lambda: video.draw_affwild(256, False, True, False),
                 lambda: video.draw_vox2(129, True, True)):
        with pytest.raises(ValueError):
            draw()
    with pytest.raises(ValueError):
        video.ingest(torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8), layout="nchw")


def test_valid_call_without_a_gpu_fails_loudly(monkeypatch):
    from m3t.ops import M3THipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(M3THipError):
        video.ingest(torch.zeros(1, 2, 40, 40, 3, dtype=torch.uint8))
