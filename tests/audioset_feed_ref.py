"""What tests/test_audioset_feed_host.py and tests/test_gpu_audioset_feed.py share: the synthetic AudioSet tree and the reference loader's
record of it (tests/golden/audioset_feed_cases.npz, written by tests/golden/gen_golden_audioset_feed.py), rebuilt on disk; the recorded
configurations; the per-item draws read off the recorded transcript.  Shares no code with m3t/audioset.py."""
import functools
import os
import random
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from conftest import load_golden

FPS_VALUES = [15.0, 17.0, 19.0, 22.0, 23.976, 24.0, 25.0, 29.97, 30.0]      # audioset_dataset.py:13


@functools.lru_cache(None)
def golden():
    return load_golden("audioset_feed_cases")


def configs():
    return [str(c) for c in golden()["configs"]]


def config(name):
    g = golden()
    window, batch, seed, epochs, world, rank = (int(v) for v in g[name + ".args"])
    split = str(g[name + ".split"][0])
    return SimpleNamespace(name=name, window=window, batch=batch, seed=seed, epochs=epochs, world=world, rank=rank, split=split,
                           training=split == "train")


def write_tree(root):
    """the golden's files under `root` -> str(root)"""
    root = str(root)
    for k, v in golden().items():
        if k.startswith("tree/"):
            p = os.path.join(root, k[len("tree/"):])
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(v.tobytes())
    return root


def clip(rel):
    """the int16 samples of a clip of the tree, cut out of the golden's file bytes by hand: the generator wrote them with Python's `wave`
    module, whose header is the canonical 44 bytes"""
    data = golden()["tree/" + rel].tobytes()
    assert data[:4] == b"RIFF" and data[36:40] == b"data"
    return np.frombuffer(data, "<i2", offset=44).astype(np.int16)


def seed(c):
    random.seed(c.seed)
    np.random.seed(c.seed)
    torch.manual_seed(c.seed)


def make_feed(root, c, reseed=True, **kw):
    """the feed of a recorded configuration, seeded as the generator seeded the reference"""
    from m3t import audioset
    scan = audioset.scan_audioset(root, c.split)
    if reseed:
        seed(c)
    args = dict(rank=c.rank, world=c.world)
    args.update(kw)
    return audioset.AudioSetFeed(scan, c.window, c.batch, c.split, **args)


def items(name, epoch):
    return golden()["%s.e%d.items" % (name, epoch)].tolist()


def n_batches(name, epoch):
    return int(golden()["%s.e%d.n_batches" % (name, epoch)][0])


def draws(name, epoch, lengths):
    """per item of the epoch, read off the transcript in the reference's order (audioset_dataset.py:60-69): dicts of fps, hop, start,
    nsamples; `lengths`: the samples of every clip of the split"""
    g, c = golden(), config(name)
    pre = "%s.e%d." % (name, epoch)
    tr = [(str(k), int(a), float(v)) for k, a, v in zip(g[pre + "tr_kind"], g[pre + "tr_arg"], g[pre + "tr_val"])]
    out, p = [], 0
    for i in items(name, epoch):
        tot = int(lengths[i])
        if c.training:
            assert tr[p][0] == "choice" and tr[p][1] == len(FPS_VALUES) and tr[p + 1][0] == "randint"
            fps = tr[p][2]
            ns = int(c.window / fps * 16000)
            if ns > tot:
                tot = ns + 5
            assert tr[p + 1][1] == tot - ns
            start = int(tr[p + 1][2])
            p += 2
        else:
            fps = 30.0
            ns = int(c.window / fps * 16000)
            if ns > tot:
                tot = ns + 5
            start = (tot - ns) // 2
        out.append({"fps": fps, "hop": int(1 / 3 * 1 / fps * 16000), "start": start, "nsamples": ns})
    assert p == len(tr)
    return out


def random_crc():
    return zlib.crc32(repr(random.getstate()).encode())


def torch_crc():
    return zlib.crc32(torch.get_rng_state().numpy().tobytes())


def state_crcs(name, epoch):
    g = golden()
    return int(g["%s.e%d.random_crc" % (name, epoch)][0]), int(g["%s.e%d.torch_crc" % (name, epoch)][0])


def batch(name, epoch, b):
    g = golden()
    return g["%s.e%d.b%d.audio" % (name, epoch, b)], g["%s.e%d.b%d.label" % (name, epoch, b)]
