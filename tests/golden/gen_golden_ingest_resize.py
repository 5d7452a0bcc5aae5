#!/usr/bin/env python3
"""Generate tests/golden/ingest_resize.npz: the reference's `load_video` (models/dataset.py:46-80) at input_size 256 -- its default, the
branch that crops 224 x 224 and calls `cv2.resize(img, (112, 112))` (dataset.py:61,73) -- run by the REFERENCE itself, imported read-only,
on seeded random uint8 frames, followed by the task modules' normalisation `(x - 127.5) / 127.5` (models/model.py:106) in torch float32 on
the host.  cv2 is absent here: gen_golden_ingest.py's in-memory stub (`imread`, `flip`) serves, plus

    cv2.resize = every output channel (a + b + c + d + 2) >> 2 over its 2 x 2 source block

which is what OpenCV's `resize` computes for an 8-bit image at an exact factor of 2 on both axes (it replaces INTER_LINEAR by its integer
INTER_AREA path there) ACCORDING TO ITS PUBLISHED SOURCE; no run of OpenCV stands behind this fixture.  The stub refuses anything but a
224 x 224 x 3 uint8 image and the target (112, 112).  tests/test_ingest_resize_host.py checks the rule against the real cv2 where it exists.

The fixture is data: frames (zeros for the missing ones), presence masks, the cases' flags and seeds, the reference's output, and the state
of `random` and `np.random` after the reference's call (the draws of m3t.video must leave both generators in the same state).

Three cases: training with mirror and a cutout clipped at a border (the crop window ends on the frame's last row); training with a missing
first and a missing middle frame and a window longer than the clip (dataset.py:312's edge padding applied to load_video's result); eval
mode.  main() asserts that coverage.  Frames are 196 608 bytes each and random, so a case stores one or two; the second case draws its
pixels from 32 random levels, which deflate packs in 5 bits each (every sum residue mod 4 still occurs).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ingest_resize.py
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as G                                       # noqa: E402  (the reference import path and the cv2 / Lightning stubs)
import gen_golden_ingest as GI                               # noqa: E402  (the in-memory decoder: imread, flip; the reference's dataset module)

cv2 = sys.modules["cv2"]
RESIZES = [0]


def _resize(img, dsize):
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (224, 224, 3), (img.dtype, img.shape)
    assert tuple(dsize) == (112, 112), dsize
    RESIZES[0] += 1
    a = img.astype(np.int64)
    s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint8)


cv2.resize = _resize

#        name             training crop cutout start length window seed levels present (over the stored frames)
CASES = [("train_mirror_cut",    1, 1, 1, 0, 1, 1, 19, 256, [1]),
         ("train_missing_pad",   1, 1, 1, 0, 4, 6, 9,  32,  [0, 1, 0, 1]),
         ("eval",                0, 1, 1, 0, 1, 1, 2,  256, [1])]
INPUT = 256


def rng_state():
    py = random.getstate()
    nps = np.random.get_state()
    assert py[0] == 3 and py[2] is None and nps[0] == "MT19937" and nps[3] == 0
    return np.array(py[1], np.int64), np.concatenate([np.asarray(nps[1], np.int64), [int(nps[2])]])


def run_case(name, training, crop, cutout, start, length, window, seed, levels, present):
    rs = np.random.RandomState(2000 + seed)
    palette = np.arange(256, dtype=np.uint8) if levels == 256 else np.sort(rs.choice(256, levels, replace=False)).astype(np.uint8)
    frames = palette[rs.randint(0, levels, (len(present), INPUT, INPUT, 3))]
    frames[~np.array(present, bool)] = 0                     # (never read: a missing frame has no file)
    GI._CLIP["frames"] = frames
    GI._CLIP["present"] = np.array(present, bool)
    random.seed(seed)
    np.random.seed(seed)
    n0 = RESIZES[0]
    # the call site, dataset.py:256-261: the mirror draw is an argument, evaluated before load_video runs
    seq = GI.aff_dataset.load_video("clip", start, length, bool(training), random.random() > 0.5, bool(crop), bool(cutout), INPUT)
    py, nps = rng_state()
    assert RESIZES[0] - n0 == int(np.sum(present[start:start + length])), "every present frame goes through cv2.resize once"
    if window > length:
        seq = np.pad(seq, ((0, 0), (0, window - length), (0, 0), (0, 0)), 'edge')      # dataset.py:312
    assert seq.shape == (3, window, 112, 112) and seq.dtype == np.float32
    x = torch.from_numpy(np.ascontiguousarray(seq))
    out = ((x - 127.5) / 127.5).numpy()                      # models/model.py:106
    return {"%s.frames" % name: frames, "%s.present" % name: GI._CLIP["present"], "%s.out" % name: out,
            "%s.rng_py" % name: py, "%s.rng_np" % name: nps,
            "%s.args" % name: np.array([INPUT, training, crop, cutout, start, length, window, seed], np.int64)}


def main():
    arrs = {"names": np.array([c[0] for c in CASES])}
    for c in CASES:
        arrs.update(run_case(*c))
    G.save("ingest_resize", **arrs)
    # coverage of the chosen seeds, from the project's own draws (tests/test_ingest_resize_host.py checks them against the outputs above)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "m3f.pytorch_amd"))
    sys.path.insert(0, os.path.dirname(HERE))
    import ingest_resize_ref as R
    from m3t import video
    draws = {c["name"]: R.case_params(video, c) for c in R.load_golden()}
    a, _ = draws["train_mirror_cut"]
    assert a["mirror"] and a["scale"] == 2 and a["size"] == 224 and a["cx"] % 2 == 1 and a["cy"] + 224 == INPUT
    cut = a["cutout"]
    assert (cut[1] - cut[0] < 112 or cut[3] - cut[2] < 112) and (cut[1] == 112 or cut[0] == 0) and cut[1] - cut[0] > 0
    b, fidx = draws["train_missing_pad"]
    assert not b["mirror"] and b["cutout"] is not None and fidx.tolist() == [-1, 1, 1, 3, 3, 3]
    e, _ = draws["eval"]
    assert (e["cy"], e["cx"], e["size"], e["scale"], e["mirror"], e["cutout"]) == (16, 16, 224, 2, False, None)
    z = np.load(os.path.join(HERE, "ingest_resize.npz"))
    fr = z["train_missing_pad.frames"][1].astype(np.int64)
    s = fr[0::2, 0::2] + fr[0::2, 1::2] + fr[1::2, 0::2] + fr[1::2, 1::2]
    assert set(np.unique(s % 4)) == {0, 1, 2, 3}
    assert os.path.getsize(os.path.join(HERE, "ingest_resize.npz")) < 1000 * 1024     # (the issue's 1.5 MB, and the 1 MiB a committed file may have)


if __name__ == "__main__":
    main()
