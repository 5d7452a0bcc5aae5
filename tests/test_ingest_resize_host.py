"""CPU-side checks of the 256-pixel branch of the video ingest (m3t/video.py: draw_affwild(..., resize=True), draws with "scale": 2): the
draws and frame indices reproduce what the reference's `load_video` did at input_size 256 under the same seeds -- through the numpy
restatement of m3t_video_ingest_half (tests/ingest_resize_ref.py), bit for bit, and in the state both random generators are left in --
and plan() rejects what the halving kernel cannot take before anything touches a device.  The fixture's `cv2.resize` is the 2 x 2 rule
(a + b + c + d + 2) >> 2 taken from OpenCV's source, not a run of OpenCV; the last test checks the rule against the real one where it exists.
No GPU here."""
import random

import numpy as np
import pytest
import torch

import ingest_resize_ref as R
from m3t import video

CASES = R.load_golden()
IDS = [c["name"] for c in CASES]


def test_golden_covers_the_issues_cases():
    draws = {c["name"]: R.case_params(video, c) for c in CASES}
    assert all(c["input_size"] == 256 for c in CASES)
    a, fa = draws["train_mirror_cut"]
    assert a["mirror"] and (a["size"], a["scale"]) == (224, 2) and a["cy"] + 224 == 256 and a["cx"] % 2 == 1
    cut = a["cutout"]
    assert 0 < cut[1] - cut[0] < 112 and cut[1] == 112, "a cutout clipped at a border"
    b, fb = draws["train_missing_pad"]
    assert fb.tolist() == [-1, 1, 1, 3, 3, 3]                # missing first: zeros; missing middle: the previous one; then edge padding
    assert not b["mirror"] and b["cutout"] is not None
    e, _ = draws["eval"]                                     # eval: centred crop, nothing else
    assert (e["cy"], e["cx"], e["size"], e["scale"], e["mirror"], e["cutout"], e["table"]) == (16, 16, 224, 2, False, None, None)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_draws_and_restatement_reproduce_the_reference_bit_for_bit(c):
    aug, fidx = R.case_params(video, c)
    T, H, W, geom, fi, tables = video.plan((1,) + c["frames"].shape, torch.uint8, [aug], fidx[None])
    assert (T, H, W) == (c["window"], 112, 112) and tables == [None] and geom[0, 7] == 0
    out = R.ingest_half_ref(c["frames"][None], geom, fi, video.norm_lut(), H, W)
    assert out.shape[1:] == c["out"].shape and out.dtype == np.float32
    assert np.array_equal(out[0].view(np.uint32), c["out"].view(np.uint32))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_draws_leave_the_generators_where_the_reference_does(c):
    """the state of `random` and `np.random` after the draws equals the state after the reference's load_video (recorded by the fixture's
    generator under the same seed): as many values drawn, from the same generator, in every mode"""
    R.case_params(video, c)
    py, nps = R.rng_state()
    assert np.array_equal(py, c["rng_py"]) and np.array_equal(nps, c["rng_np"])


def test_resize_draw_consumes_the_generators_in_the_references_order():
    random.seed(11)
    np.random.seed(11)
    a = video.draw_affwild(256, True, True, True, mirror=True, resize=True)
    s_py, s_np = R.rng_state()
    random.seed(11)
    np.random.seed(11)
    cx, cy = random.randint(0, 32), random.randint(0, 32)    # dataset.py:56-57, crop_x first
    y, x = np.random.randint(112), np.random.randint(112)    # sequence_cutout sees the resized clip: h = w = 112, length 56
    r_py, r_np = R.rng_state()
    assert np.array_equal(s_py, r_py) and np.array_equal(s_np, r_np)
    assert (a["cx"], a["cy"], a["size"], a["scale"], a["mirror"], a["table"]) == (cx, cy, 224, 2, True, None)
    assert a["cutout"] == (max(y - 56, 0), min(y + 56, 112), max(x - 56, 0), min(x + 56, 112))
    # eval mode: a centred window, no draw from either generator
    random.seed(13)
    np.random.seed(13)
    s0, n0 = R.rng_state()
    e = video.draw_affwild(256, False, True, True, mirror=True, resize=True)
    s1, n1 = R.rng_state()
    assert np.array_equal(s0, s1) and np.array_equal(n0, n1)
    assert (e["cx"], e["cy"], e["size"], e["scale"], e["mirror"], e["cutout"]) == (16, 16, 224, 2, False, None)


def test_what_the_keyword_does_not_change():
    for draw in (lambda: video.draw_affwild(200, True, True, False, resize=True),        # a 175-pixel crop: no factor of 2
                 lambda: video.draw_affwild(200, False, True, False, resize=True),
                 lambda: video.draw_affwild(512, True, True, False, resize=True),
                 lambda: video.draw_affwild(256, True, True, True),                      # not asked for
                 lambda: video.draw_affwild(256, True, True, True, resize=False)):
        s0 = random.getstate()
        with pytest.raises(ValueError):
            draw()
        assert random.getstate() == s0, "a refused draw consumed the generator"
    with pytest.raises(ValueError, match="resize=True"):
        video.draw_affwild(256, True, True, False)
    # at or below 128, and without a crop, the keyword changes nothing: no "scale", the reference does not resize there
    for args in ((128, True, True, True), (40, False, True, True), (256, True, False, True), (256, False, False, False)):
        random.seed(5)
        np.random.seed(5)
        a = video.draw_affwild(*args, mirror=True)
        random.seed(5)
        np.random.seed(5)
        b = video.draw_affwild(*args, mirror=True, resize=True)
        assert a == b and "scale" not in b


def _aug(cy=0, cx=0, size=70, mirror=False, cutout=None, table=None, scale=2):
    d = {"cy": cy, "cx": cx, "size": size, "mirror": mirror, "cutout": cutout, "table": table}
    if scale is not None:
        d["scale"] = scale
    return d


def test_plan_halves_the_window():
    T, H, W, geom, fi, tables = video.plan((2, 3, 80, 81, 3), torch.uint8,
                                           [_aug(cy=10, cx=11, mirror=True, cutout=(0, 35, 30, 35)), _aug(cy=0, cx=0)], None)
    assert (T, H, W) == (3, 35, 35) and fi is None and tables == [None, None]
    assert geom.tolist() == [[10, 11, 1, 0, 35, 30, 35, 0], [0, 0, 0, 0, 0, 0, 0, 0]]
    assert video.batch_scale([_aug(), _aug()]) == 2 and video.batch_scale([_aug(scale=None), _aug(scale=1)]) == 1
    assert video.batch_scale(None) == 1


@pytest.mark.parametrize("shape,aug", [
    ((1, 2, 80, 80, 3), [_aug(size=71)]),                                # an odd window with scale 2
    ((2, 2, 80, 80, 3), [_aug(), _aug(scale=None)]),                     # mixed scales in a batch
    ((2, 2, 80, 80, 3), [_aug(scale=1), _aug()]),
    ((1, 2, 80, 80, 3), [_aug(scale=3, size=72)]),                       # no such kernel
    ((1, 2, 80, 80, 3), [_aug(cy=11)]),                                  # window cy + size > Hs (its output, 35 rows, would fit)
    ((1, 2, 80, 80, 3), [_aug(cx=11)]),
    ((1, 2, 69, 80, 3), [_aug()]),
    ((1, 2, 256, 256, 3), [_aug(size=224, cy=33)]),
    ((1, 2, 80, 80, 3), [_aug(cutout=(0, 36, 0, 3))]),                   # cutout beyond the 35 x 35 output (inside the 70 x 70 window)
    ((1, 2, 256, 256, 3), [_aug(size=224, cutout=(0, 112, 50, 113))]),   # cutout beyond 112
])
def test_ingest_validates_on_the_host(shape, aug, monkeypatch):
    """ValueError before any device is touched: neither the availability query nor either library call is reached"""
    def touched(*a, **k):
        raise AssertionError("the wrapper reached the device before validating")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(video, "video_ingest", touched)
    monkeypatch.setattr(video, "video_ingest_half", touched)
    with pytest.raises(ValueError):
        video.plan(shape, torch.uint8, aug, None)
    for layout in ("cl", "planes"):
        with pytest.raises(ValueError):
            video.ingest(torch.zeros(shape, dtype=torch.uint8), aug, None, layout)


def test_ingest_dispatches_on_the_scale(monkeypatch):
    """a valid batch reaches exactly one entry point, chosen by the draws' scale, with the OUTPUT size"""
    calls = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(video, "video_ingest", lambda fr, f, T, g, l, H, W, layout: calls.append(("full", T, H, W)))
    monkeypatch.setattr(video, "video_ingest_half", lambda fr, f, T, g, l, H, W, layout: calls.append(("half", T, H, W)))
    fr = torch.zeros(1, 2, 80, 80, 3, dtype=torch.uint8)
    video.ingest(fr, [_aug(cy=10, cx=10)], None, "planes")
    video.ingest(fr, [_aug(cy=10, cx=10, scale=None)], None, "planes")
    video.ingest(fr, None, None, "planes")
    assert calls == [("half", 2, 35, 35), ("full", 2, 70, 70), ("full", 2, 80, 80)]


def test_valid_call_without_a_gpu_fails_loudly(monkeypatch):
    from m3t.ops import M3THipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(M3THipError):
        video.ingest(torch.zeros(1, 2, 80, 80, 3, dtype=torch.uint8), [_aug()])


def test_rounding_image_covers_every_residue():
    img, want = R.rounding_image()
    s = img.astype(np.int64)
    s = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
    assert set(np.unique(s % 4)) == {0, 1, 2, 3} and s.max() == 1020 and s.min() == 0 and (s == 1).any()
    assert np.array_equal(R.halve(img), want)
    assert want[0, 0, 0] == 255 and want[0, 1, 0] == 0 and want[0, 2, 0] == 1


def test_the_rule_against_the_real_cv2():
    """The check nobody on this project could run: OpenCV's own resize on a 224 x 224 x 3 uint8 image (and on the rounding image tiled to
    that size) must equal (a + b + c + d + 2) >> 2 exactly.  Skipped where cv2 is not installed."""
    cv2 = pytest.importorskip("cv2")
    rnd = np.random.RandomState(0).randint(0, 256, (224, 224, 3)).astype(np.uint8)
    small, _ = R.rounding_image()
    tiled = np.tile(small, (28, 28, 1))
    for img in (rnd, tiled):
        assert img.shape == (224, 224, 3)
        got = cv2.resize(img, (112, 112))
        assert got.dtype == np.uint8 and np.array_equal(got, R.halve(img))
    got = cv2.resize(small, (4, 4))
    assert np.array_equal(got, R.halve(small))
