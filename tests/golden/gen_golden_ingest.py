#!/usr/bin/env python3
"""Generate tests/golden/ingest.npz: the reference's two `load_video` functions (models/dataset.py:46-80, models/vox2_dataset.py:14-50)
run by the REFERENCE itself, imported read-only, on seeded random uint8 frames, followed by the task modules' normalisation
`(x - 127.5) / 127.5` (models/model.py:106) in torch float32 on the host.  cv2 is absent here: the stub gen_golden.py installs gets an
in-memory `imread`, `flip`, `LUT` and `VideoCapture` (exact by definition: a file read, a reversal, a table look-up).  The fixture is
data: frames, presence masks, the cases' flags and seeds, the reference's output.

A window shorter than the dataset's window length is edge-padded in time by the dataset's __getitem__ (dataset.py:312); the one case that
covers it applies that line's np.pad to load_video's result.

The seeds are chosen so that the cases cover both mirror values, a cutout clipped at a border and one that is not, odd and even crop_x, a
missing first, middle and last frame, eval mode and three jitter draws; main() asserts it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ingest.py
"""
import os
import random
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as G                                       # noqa: E402  (sets up the reference import path and the cv2 / Lightning stubs)

cv2 = sys.modules["cv2"]
_CLIP = {}                                                   # the clip the stubbed decoder serves: frames [Ts, Hs, Ws, 3], present [Ts]


def _imread(path):
    i = int(re.search(r"(\d+)\.jpg$", path).group(1)) - 1    # (file names count from 1, dataset.py:64)
    return _CLIP["frames"][i].copy() if _CLIP["present"][i] else None


class _Capture:
    def __init__(self, path):
        self.pos = 0

    def isOpened(self):
        return True

    def set(self, prop, value):
        assert prop == 1
        self.pos = int(value)

    def read(self):
        i, self.pos = self.pos, self.pos + 1
        if i < len(_CLIP["frames"]) and _CLIP["present"][i]:
            return True, _CLIP["frames"][i].copy()
        return False, None

    def release(self):
        pass


cv2.imread = _imread
cv2.flip = lambda img, code: {1: img[:, ::-1]}[code]
cv2.LUT = lambda img, table: table[img]
cv2.VideoCapture = _Capture

from models import dataset as aff_dataset                    # noqa: E402  (reference)
from models import vox2_dataset                              # noqa: E402  (reference)

#        name             input training crop cutout start length window seed  present (over the stored frames)
CASES = [("aff_128_first",   128, 1, 1, 0, 0, 2, 2, 5,   [0, 1]),
         ("aff_40_middle",    40, 1, 1, 1, 1, 4, 4, 398, [1, 1, 1, 0, 1]),
         ("aff_40_last_pad",  40, 1, 1, 1, 0, 4, 6, 1,   [1, 1, 1, 0]),
         ("aff_40_eval",      40, 0, 1, 1, 0, 3, 3, 2,   [1, 1, 1]),
         ("vox_40_j0",        40, 1, 1, 0, 1, 3, 3, 0,   [1, 1, 1, 1]),
         ("vox_40_j1",        40, 1, 1, 0, 0, 3, 3, 3,   [1, 1, 1]),
         ("vox_40_j2",        40, 1, 1, 0, 0, 2, 2, 7,   [1, 1]),
         ("vox_40_eval",      40, 0, 1, 0, 0, 2, 2, 4,   [1, 1])]


def run_case(name, input_size, training, crop, cutout, start, length, window, seed, present):
    rs = np.random.RandomState(1000 + seed)
    _CLIP["frames"] = rs.randint(0, 256, (len(present), input_size, input_size, 3)).astype(np.uint8)
    _CLIP["present"] = np.array(present, bool)
    random.seed(seed)
    np.random.seed(seed)
    if name.startswith("aff"):
        # the call site, dataset.py:256-261: the mirror draw is an argument, evaluated before load_video runs
        seq = aff_dataset.load_video("clip", start, length, bool(training), random.random() > 0.5, bool(crop), bool(cutout), input_size)
        if window > length:
            seq = np.pad(seq, ((0, 0), (0, window - length), (0, 0), (0, 0)), 'edge')      # dataset.py:312
    else:
        seq = vox2_dataset.load_video("clip", start, length, bool(training), random.random() > 0.5, bool(crop), input_size)
    x = torch.from_numpy(np.ascontiguousarray(seq))
    out = ((x - 127.5) / 127.5).numpy()                      # models/model.py:106, vox2_model.py:55
    return {"%s.frames" % name: _CLIP["frames"], "%s.present" % name: _CLIP["present"], "%s.out" % name: out,
            "%s.args" % name: np.array([input_size, training, crop, cutout, start, length, window, seed], np.int64)}


def main():
    arrs = {"names": np.array([c[0] for c in CASES])}
    for c in CASES:
        arrs.update(run_case(*c))
    G.save("ingest", **arrs)
    # coverage of the chosen seeds, from the project's own draws (tests/test_ingest_host.py checks them against the outputs above)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "m3f.pytorch_amd"))
    sys.path.insert(0, os.path.dirname(HERE))
    import ingest_ref
    from m3t import video
    draws = {c["name"]: ingest_ref.case_params(video, c)[0] for c in ingest_ref.load_golden()}
    train = [d for n, d in draws.items() if "eval" not in n]
    assert {d["mirror"] for d in train} == {True, False}
    assert {d["cx"] % 2 for d in train} == {0, 1}
    cuts = [d["cutout"] for d in train if d["cutout"] is not None]
    assert any(c[1] - c[0] == 34 and c[3] - c[2] == 34 for c in cuts) and any(c[1] - c[0] < 34 or c[3] - c[2] < 34 for c in cuts)
    assert sum(d["table"] is not None for d in train) == 3
    assert os.path.getsize(os.path.join(HERE, "ingest.npz")) < 600 * 1024


if __name__ == "__main__":
    main()
