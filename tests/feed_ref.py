"""What tests/test_feed_host.py and tests/test_gpu_feed.py share: the synthetic Aff-Wild2 tree and the reference loader's record of it
(tests/golden/feed_cases.npz, written by tests/golden/gen_golden_feed.py), rebuilt on disk; the six recorded configurations; the per-item
draws read off the recorded transcript; a replay of the transcript against `random` / `np.random`.  Shares no code with m3t/feed.py."""
import functools
import os
import random
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from conftest import load_golden


@functools.lru_cache(None)
def golden():
    return load_golden("feed_cases")


def configs():
    return [str(c) for c in golden()["configs"]]


def config(name):
    g = golden()
    window, cutout, resample, input_size, stride, seed, wpe, batch, n_batches = (int(v) for v in g[name + ".args"])
    split, modality, run = (str(s) for s in g[name + ".strs"])
    return SimpleNamespace(name=name, window=window, cutout=bool(cutout), resample=bool(resample), input_size=input_size, stride=stride, seed=seed,
                           windows_per_epoch=wpe, batch=batch, n_batches=n_batches, split=split, modality=modality, run=run,
                           visual="visual" in modality, training=split == "train")


def write_tree(root):
    """the golden's files under `root` (data/..., run128/splits/..., run256/splits/...) -> str(root)"""
    root = str(root)
    for k, v in golden().items():
        if k.startswith("tree/"):
            p = os.path.join(root, k[len("tree/"):])
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(v.tobytes())
    return root


def seed(c):
    random.seed(c.seed)
    np.random.seed(c.seed)
    torch.manual_seed(c.seed)


def scan(root, c, **kw):
    from m3t import feed
    args = dict(release="vipl", input_size=c.input_size, splits_dir=os.path.join(root, c.run, "splits"), resample=c.resample, window=c.window)
    args.update(kw)
    return feed.scan_affwild(os.path.join(root, "data"), c.split, c.modality, **args)


def make_feed(root, c, corpus=None, reseed=True, **kw):
    """the feed of a recorded configuration, seeded as the generator seeded the reference (the seeds come before construction: the training
    split shuffles there)"""
    from m3t import feed
    corpus = scan(root, c) if corpus is None else corpus
    if reseed:
        seed(c)
    args = dict(cutout=c.cutout, input_size=c.input_size, release="vipl", windows_per_epoch=c.windows_per_epoch, inv_test_stride=c.stride)
    args.update(kw)
    return feed.AffWild2Feed(corpus, c.window, c.batch, c.split, c.modality, **args)


def items(name):
    g = golden()
    return [(str(n), int(s), int(l)) for n, s, l in zip(g[name + ".vid_name"], g[name + ".start"], g[name + ".length"])]


def transcript(name):
    g = golden()
    return [(str(k), int(a), float(v)) for k, a, v in zip(g[name + ".tr_kind"], g[name + ".tr_arg"], g[name + ".tr_val"])]


def draws(name):
    """per item, read off the transcript in the reference's order (dataset.py:246, :258, :56-57, :22-23): dict of 'start' (training), 'mirror'
    (the draw `random.random() > 0.5` AND training, what load_video applies), 'cx', 'cy', 'cutout' (y1, y2, x1, x2 on the 112 x 112 output)"""
    c = config(name)
    tr = [t for t in transcript(name) if t[0] != "shuffle"]
    out, p = [], 0
    for _ in items(name):
        d = {"start": None, "mirror": False, "cx": c.input_size // 16, "cy": c.input_size // 16, "cutout": None}
        if c.training:
            assert tr[p][0] == "choice"
            d["start"] = int(tr[p][2])
            p += 1
        if c.visual:
            assert tr[p][0] == "random"
            d["mirror"] = tr[p][2] > 0.5 and c.training
            p += 1
            if c.training:
                assert tr[p][0] == tr[p + 1][0] == "randint" and tr[p][1] == c.input_size // 8
                d["cx"], d["cy"] = int(tr[p][2]), int(tr[p + 1][2])
                p += 2
                if c.cutout:
                    assert tr[p][0] == tr[p + 1][0] == "np_randint" and tr[p][1] == 112
                    y, x = int(tr[p][2]), int(tr[p + 1][2])
                    p += 2
                    d["cutout"] = (max(y - 56, 0), min(y + 56, 112), max(x - 56, 0), min(x + 56, 112))
        out.append(d)
    assert p == len(tr)
    return out


def replay(name):
    """seed as the generator did, then make the transcript's calls against the real `random` / `np.random`, checking every recorded value;
    afterwards the two generators are in the state the reference left them in"""
    c = config(name)
    seed(c)
    for kind, arg, val in transcript(name):
        if kind == "shuffle":
            x = list(range(arg))
            random.shuffle(x)
        elif kind == "choice":
            random.choice(range(arg))
        elif kind == "random":
            assert random.random() == val
        elif kind == "randint":
            assert random.randint(0, arg) == val
        else:
            assert kind == "np_randint" and np.random.randint(arg) == val


def np_state_key():
    s = np.random.get_state()
    return (s[0], s[1].tobytes(), s[2], s[3], s[4])


def torch_state_crc():
    return zlib.crc32(torch.get_rng_state().numpy().tobytes())


def batch_arrays(name, b):
    """the non-video arrays of recorded batch b: key -> array"""
    pre = "%s.b%d." % (name, b)
    return {k[len(pre):]: v for k, v in golden().items() if k.startswith(pre)}


def frame_crcs(planes):
    """planes float32 [N, 3, T, H, W] (numpy) -> uint32 [N, T]: the CRC32 of every frame [3, H, W], as the generator took them"""
    return np.array([[zlib.crc32(np.ascontiguousarray(planes[n, :, t]).tobytes()) for t in range(planes.shape[2])] for n in range(planes.shape[0])],
                    np.uint32)
