"""The host half of the AffWild2 epoch feed (m3t/feed.py) against the reference loader's record of a small synthetic tree
(tests/golden/feed_cases.npz): the folder scan, the epoch plan -- items, order and every draw -- the sharding, the cache files and the
resume state.  No GPU: nothing here may touch one."""
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import collate_ref
import feed_ref as F

CONFIGS = F.configs()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.write_tree(tmp_path_factory.mktemp("affwild"))


def test_the_golden_holds_the_six_configurations():
    assert CONFIGS == ["train_av_cutout", "train_v_resample", "train_audio", "val_av", "test_av", "train_v_256"]
    assert all(F.config(n).batch == 2 for n in CONFIGS)


# ---------------------------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("name", CONFIGS)
def test_scan_gives_the_reference_s_corpus(tree, name):
    g, c = F.golden(), F.config(name)
    corpus = F.scan(tree, c)
    assert corpus.names == list(corpus.videos) == [str(f) for f in g[name + ".files"]]
    assert corpus.nb_frames == g[name + ".nb_frames"].tolist()
    base = os.path.join(tree, "data", "face_%d" % c.input_size)
    for v in corpus.names:
        d = corpus.videos[v]
        if c.split == "test":
            assert "va" not in d and "expr" not in d
        else:
            want = g["%s.va.%s" % (name, v)]
            assert d["va"].dtype == np.float32 and d["va"].tobytes() == want.tobytes() and d["va"].shape == want.shape
            key = "%s.expr.%s" % (name, v)
            assert ("expr" in d) == (key in g)
            if key in g:
                assert d["expr"].dtype == np.int64 and np.array_equal(d["expr"], g[key])
        if c.visual:
            count = d["nb_frames"] if c.split == "test" else len(d["va"])
            exists = [os.path.exists(os.path.join(base, v, "%05d.jpg" % (i + 1))) for i in range(count)]
            assert d["has_image"].tolist() == exists
            assert [p is not None for p in corpus.frames[v]] == exists and all(p is None or os.path.exists(p) for p in corpus.frames[v])
            assert d["se"].dtype == np.float32 and d["se"].shape[1] == 512 and d["au"].shape == (d["nb_frames"], 268)
        else:
            assert corpus.frames is None and "se" not in d and "has_image" not in d
        if "audio" in c.modality:
            assert ("mel" in d) == (d["fps"] >= 15)
        if c.training:
            assert corpus.avail[v] == g["%s.avail.%s" % (name, v)].tolist()
    if c.visual and "A" in corpus.names:
        assert corpus.videos["A"]["has_image"][:7].tolist() == [False, True, True, True, True, False, True]
    if "B" in corpus.names and c.visual:
        assert corpus.videos["B"]["se"].shape[0] == corpus.videos["B"]["nb_frames"] - 2


def test_the_two_window_plans_differ_and_resample_zeroes_the_unlabelled_rows(tree):
    plain, noisy = F.scan(tree, F.config("train_av_cutout"), window=5), F.scan(tree, F.config("train_v_resample"))
    assert plain.avail["D"] != noisy.avail["D"]
    assert (plain.videos["D"]["va"][5:8] == -5).all() and (noisy.videos["D"]["va"][5:8] == 0).all()


def test_refusals_name_the_video_and_the_file(tree, tmp_path):
    import shutil
    from m3t import feed
    c = F.config("train_av_cutout")
    root = str(tmp_path / "copy")
    shutil.copytree(tree, root)
    va = os.path.join(root, "data", "annotations", "VA_Set", "Training_Set", "B.txt")
    os.rename(va, va + ".away")
    with pytest.raises(ValueError, match=r"video 'B'.*annotation.*B\.txt"):
        F.scan(root, c)
    os.rename(va + ".away", va)
    mel = os.path.join(root, "data", "mel_spec", "D.npy")
    os.rename(mel, mel + ".away")
    with pytest.raises(ValueError, match=r"video 'D'.*log-Mel.*D\.npy"):
        F.scan(root, c)
    F.scan(root, F.config("train_v_resample"))                                  # (no audio: the mel files are not asked for)
    os.rename(mel + ".away", mel)
    with open(os.path.join(root, "run128", "splits", "train.csv"), "a") as f:
        f.write("nobody\n")
    with pytest.raises(ValueError, match=r"video 'nobody'.*train\.csv.*frames_fps\.csv"):
        F.scan(root, c)
    with pytest.raises(ValueError, match="split"):
        feed.scan_affwild(os.path.join(tree, "data"), "dev", "audio")


def test_a_feed_refuses_a_corpus_scanned_for_something_else(tree):
    c = F.config("val_av")
    with pytest.raises(ValueError, match="window"):
        F.make_feed(tree, c, corpus=F.scan(tree, c, window=8))


# ---------------------------------------------------------------------------------------------- the epoch plan
def _flat(plans):
    return [it for p in plans for it in p.items], [a for p in plans for a in (p.aug or [])]


@pytest.mark.parametrize("name", CONFIGS)
def test_plan_epoch_equals_the_reference_s_epoch(tree, name):
    c = F.config(name)
    feed = F.make_feed(tree, c)
    if c.training:
        assert feed.sample_src == F.golden()[name + ".shuffled"].tolist()
    plans = feed.plan_epoch(0)
    got_states = random.getstate(), F.np_state_key(), F.torch_state_crc()
    assert len(plans) == len(feed) == c.n_batches and [p.index for p in plans] == list(range(c.n_batches))
    assert [len(p.items) for p in plans] == [c.batch] * (c.n_batches - 1) + [len(F.items(name)) - c.batch * (c.n_batches - 1)]
    items, aug = _flat(plans)
    assert [(feed.names[v], s, tl) for v, s, tl in items] == F.items(name)      # item order, starts, track_len
    want = F.draws(name)
    if c.training:
        assert [s for _, s, _ in items] == [d["start"] for d in want]
    if not c.visual:
        assert all(p.aug is None for p in plans)
    else:
        assert len(aug) == len(want)
        size = c.input_size * 7 // 8
        for a, d in zip(aug, want):
            assert (a["mirror"], a["cx"], a["cy"], a["cutout"], a["size"], a.get("scale", 1)) == (d["mirror"], d["cx"], d["cy"], d["cutout"], size, size // 112)
    # no extra draw, no missing draw: the generators are where the reference left them
    F.replay(name)
    assert got_states[0] == random.getstate() and got_states[1] == F.np_state_key()
    assert got_states[2] == int(F.golden()[name + ".torch_state_crc"][0])


def test_with_an_identity_sampler_the_audio_plan_is_train_items_and_the_visual_plan_is_not(tree):
    c = F.config("train_audio")
    corpus = F.scan(tree, c)
    feed = F.make_feed(tree, c, corpus=corpus, sampler=lambda ds: range(len(ds)))
    items, _ = _flat(feed.plan_epoch(0))
    avail = [corpus.avail[n] for n in corpus.names]
    want = collate_ref.train_transcript(len(corpus.names), c.windows_per_epoch, avail, c.seed)
    assert [(v, s) for v, s, _ in items] == want and all(tl == c.window for _, _, tl in items)
    c = F.config("train_av_cutout")
    corpus = F.scan(tree, c)
    feed = F.make_feed(tree, c, corpus=corpus, sampler=lambda ds: range(len(ds)))
    items, _ = _flat(feed.plan_epoch(0))
    avail = [corpus.avail[n] for n in corpus.names]
    hand = collate_ref.train_transcript(len(corpus.names), c.windows_per_epoch, avail, c.seed)
    assert [v for v, _, _ in items] == [v for v, _ in hand]                     # the same shuffle ...
    assert [(v, s) for v, s, _ in items] != hand                                # ... but the choices interleave with the clip's draws


@pytest.mark.parametrize("name", ["train_audio", "val_av"])
def test_two_ranks_take_the_distributed_sampler_s_shards(tree, name):
    from torch.utils.data.distributed import DistributedSampler
    c = F.config(name)
    corpus = F.scan(tree, c)
    n = len(F.items(name))
    assert n % 2 == 1                                                            # an odd length: the sampler pads
    for rank in (0, 1):
        feed = F.make_feed(tree, c, corpus=corpus, rank=rank, world=2)
        sampler = DistributedSampler(range(n), num_replicas=2, rank=rank)
        for epoch in (0, 1):
            sampler.set_epoch(epoch)
            want = list(sampler)
            plans = feed.plan_epoch(epoch)
            got = [i for p in plans for i in p.indices]
            assert got == want and len(got) == (n + 1) // 2
            src = feed.sample_src
            assert [it[0] for p in plans for it in p.items] == [src[i] if c.training else src[i][0] for i in want]
    assert list(DistributedSampler(range(n), num_replicas=2, rank=0)) != list(range(0, n, 2))   # (shuffled, as the reference's default)


def test_cache_files_have_the_reference_s_names_and_content(tree, tmp_path):
    g = F.golden()
    for name in ("train_av_cutout", "train_v_resample", "train_audio"):
        c = F.config(name)
        cache = tmp_path / name
        corpus = F.scan(tree, c, cache_dir=str(cache))
        assert os.listdir(cache) == [str(g[name + ".cache_name"][0])]
        with open(cache / os.listdir(cache)[0], "rb") as f:
            held = pickle.load(f)
        assert held == {v: g["%s.avail.%s" % (name, v)].tolist() for v in corpus.names} and list(held) == corpus.names
        # a second scan reads the file: plant a recognisable plan in it
        held["A"] = [1]
        with open(cache / os.listdir(cache)[0], "wb") as f:
            pickle.dump(held, f)
        again = F.scan(tree, c, cache_dir=str(cache))
        assert again.avail["A"] == [1] and again.avail["B"] == corpus.avail["B"]
        assert again.videos["D"]["va"].tobytes() == corpus.videos["D"]["va"].tobytes()
    before = sorted(os.listdir(tmp_path))
    cwd_before = sorted(os.listdir("."))
    F.scan(tree, F.config("train_av_cutout"))
    assert sorted(os.listdir(tmp_path)) == before and sorted(os.listdir(".")) == cwd_before


@pytest.mark.parametrize("name", ["train_av_cutout", "val_av"])
def test_state_dict_resumes_the_next_epoch(tree, name):
    c = F.config(name)
    feed = F.make_feed(tree, c)
    feed.plan_epoch(0)
    state = feed.state_dict()
    want = feed.plan_epoch(1)
    random.seed(999)
    np.random.seed(999)
    torch.manual_seed(999)
    fresh = F.make_feed(tree, c, reseed=False)
    if c.training:
        assert fresh.sample_src != feed.sample_src
    fresh.load_state_dict(state)
    assert fresh.epoch == 0
    got = fresh.plan_epoch(1)
    assert got == want and fresh.epoch == 1
    if c.training:
        assert want != feed.plan_epoch(2)                                        # (the comparison can tell two epochs apart)


def test_the_task_module_builds_the_feeds_from_hparams(tree):
    import argparse
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.modality, ns.window, ns.batch_size, ns.windows_per_epoch, ns.input_size, ns.num_hidden = "audio", 4, 2, 3, 128, 16
    ns.dataset_path, ns.splits_dir = os.path.join(tree, "data"), os.path.join(tree, "run128", "splits")
    m = AffWild2VA(ns)
    train, val, test = m.train_dataloader(), m.val_dataloader(), m.test_dataloader()
    assert (train.split, val.split, test.split) == ("train", "val", "test")
    assert (train.inv_test_stride, val.inv_test_stride, test.inv_test_stride) == (1, 1, 2)
    assert len(train) == 5 and train.windows_per_epoch == 3 and train.names == ["A", "B", "D"]
    ns.test_on_val = True
    val2 = m.test_dataloader()
    assert val2.split == "val" and val2.inv_test_stride == 2
    ns.mode = "frame"
    with pytest.raises(NotImplementedError):
        m.train_dataloader()


def test_planning_does_not_initialise_the_gpu(tree):
    code = ("import sys; sys.path[:0] = %r\n"
            "import torch, feed_ref as F\n"
            "from m3t import feed\n"
            "for name in ('train_av_cutout', 'val_av'):\n"
            "    fd = F.make_feed(%r, F.config(name))\n"
            "    assert len(fd.plan_epoch(0)) == len(fd)\n"
            "    fd.state_dict()\n"
            "assert not torch.cuda.is_initialized()\n"
            "print('planned')\n") % ([p for p in sys.path if p], tree)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "planned" in res.stdout, res.stderr[-2000:]
