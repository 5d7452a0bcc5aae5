"""The host half of the AudioSet epoch feed (m3t/audioset.py) against the reference loader's record of a small synthetic tree
(tests/golden/audioset_feed_cases.npz): the folder scan, the epoch plan -- items, order and every draw -- the generator states, the
sharding and the resume state; the store form of m3t.audio.plan_waves; the task module and the driver's parser.  No GPU: nothing here may
touch one."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import audioset_feed_ref as F

CONFIGS = F.configs()
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m3f.pytorch_amd")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.write_tree(tmp_path_factory.mktemp("audioset"))


def test_the_golden_holds_the_four_configurations():
    assert CONFIGS == ["train", "val", "train_w2r0", "train_w2r1"]
    assert all((F.config(n).window, F.config(n).batch) == (4, 2) for n in CONFIGS) and F.config("train").epochs == 2


# ---------------------------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("split", ["train", "val"])
def test_scan_gives_the_reference_s_files_and_labels(tree, split):
    from m3t import audioset
    g = F.golden()
    scan = audioset.scan_audioset(tree, split)
    assert [os.path.relpath(f, tree) for f in scan.files] == [str(f) for f in g[split + ".files"]]
    assert scan.labels.dtype == np.uint8 and scan.labels.shape == (len(scan.files), 527) and np.array_equal(scan.labels, g[split + ".labels"])
    want = {"train": [16000, 3000, 2133, 9000, 4267], "val": [1000, 2134, 8000]}[split]
    assert scan.lengths().tolist() == want == [len(F.clip(str(f))) for f in g[split + ".files"]]
    if split == "train":
        assert not any("gone" in f for f in scan.files)                          # listed, no file: skipped silently
        assert scan.labels[3, 526] == 1 and scan.labels.sum(1).tolist() == [1, 2, 1, 2, 1]


def _copy(tree, tmp_path, name):
    root = str(tmp_path / name)
    shutil.copytree(tree, root)
    return root


def test_refusals_name_the_file_and_the_line(tree, tmp_path):
    from m3t import audioset
    root = _copy(tree, tmp_path, "four")
    seg = os.path.join(root, "balanced_train_segments.csv")
    lines = open(seg).read().splitlines()
    with open(seg, "w") as f:                                                    # line 6 loses a separator
        f.write("\n".join(lines[:5] + [lines[5].replace(", ", ",", 1)] + lines[6:]) + "\n")
    with pytest.raises(ValueError, match=r"balanced_train_segments\.csv, line 6.*four parts"):
        audioset.scan_audioset(root, "train")
    audioset.scan_audioset(root, "val")
    root = _copy(tree, tmp_path, "mid")
    seg = os.path.join(root, "eval_segments.csv")
    lines = open(seg).read().splitlines()
    with open(seg, "w") as f:
        f.write("\n".join(lines[:4] + [lines[4][:-1] + ',/m/nowhere"'] + lines[5:]) + "\n")
    with pytest.raises(ValueError, match=r"eval_segments\.csv, line 5.*'/m/nowhere'.*'v2'.*class_labels_indices\.csv"):
        audioset.scan_audioset(root, "val")
    # ... but a listed clip WITHOUT a file is skipped before its labels are looked at, as in the reference
    seg = os.path.join(root, "balanced_train_segments.csv")
    text = open(seg).read()
    gone = [l for l in text.splitlines() if l.startswith("gone, ")]
    assert len(gone) == 1
    with open(seg, "w") as f:
        f.write(text.replace(gone[0], gone[0][:-1] + ',/m/nowhere"'))
    assert len(audioset.scan_audioset(root, "train")) == 5
    os.remove(os.path.join(root, "class_labels_indices.csv"))
    with pytest.raises(ValueError, match=r"class list.*class_labels_indices\.csv"):
        audioset.scan_audioset(root, "train")
    with pytest.raises(ValueError, match="split"):
        audioset.scan_audioset(tree, "test")


def test_a_clip_at_another_rate_or_without_samples_is_refused_by_name(tree, tmp_path):
    import wave
    from m3t import audioset
    root = _copy(tree, tmp_path, "rate")
    path = os.path.join(root, "eval_segments", "v2.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(b"\0\0" * 100)
    with pytest.raises(ValueError, match=r"v2\.wav.*44100 Hz"):
        audioset.scan_audioset(root, "val").lengths()
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
    with pytest.raises(ValueError, match=r"v2\.wav.*empty clip"):
        audioset.AudioSetFeed(audioset.scan_audioset(root, "val"), 4, 2, "val")
    with pytest.raises(ValueError, match="scanned for"):
        audioset.AudioSetFeed(audioset.scan_audioset(tree, "val"), 4, 2, "train")


# ---------------------------------------------------------------------------------------------- the epoch plan
@pytest.mark.parametrize("name", CONFIGS)
def test_plan_epoch_equals_the_reference_s_epochs(tree, name):
    c = F.config(name)
    feed = F.make_feed(tree, c)
    for epoch in range(c.epochs):
        plans = feed.plan_epoch(epoch)
        states = F.random_crc(), F.torch_crc()
        want_items, nb = F.items(name, epoch), F.n_batches(name, epoch)
        assert len(plans) == len(feed) == nb and [p.index for p in plans] == list(range(nb))
        assert [len(p.items) for p in plans] == [c.batch] * (nb - 1) + [len(want_items) - c.batch * (nb - 1)]
        assert [i for p in plans for i in p.items] == want_items                  # the order
        got = [a for p in plans for a in p.aug]
        want = F.draws(name, epoch, feed.lengths)
        assert [(a["fps"], a["start"], a["nsamples"], a["hop"]) for a in got] == [(d["fps"], d["start"], d["nsamples"], d["hop"]) for d in want]
        # no extra draw, no missing draw: the generators are where the reference left them
        assert states == F.state_crcs(name, epoch)
    if name == "train":
        assert F.items(name, 0) != F.items(name, 1)


def test_the_two_ranks_shards_are_the_golden_s(tree):
    from torch.utils.data.distributed import DistributedSampler
    shards = []
    for rank in (0, 1):
        c = F.config("train_w2r%d" % rank)
        feed = F.make_feed(tree, c)
        got = [i for p in feed.plan_epoch(0) for i in p.items]
        assert got == F.items(c.name, 0) == list(DistributedSampler(range(5), num_replicas=2, rank=rank))
        shards.append(got)
        sampler = DistributedSampler(range(5), num_replicas=2, rank=rank)
        sampler.set_epoch(1)
        assert [i for p in feed.plan_epoch(1) for i in p.items] == list(sampler)
    assert sorted(set(shards[0] + shards[1])) == [0, 1, 2, 3, 4] and len(shards[0]) == len(shards[1]) == 3     # an odd length: the sampler pads
    c = F.config("val")
    val = F.make_feed(tree, c, world=2, rank=1)                                  # the reference shards validation the same way
    assert [i for p in val.plan_epoch(0) for i in p.items] == list(DistributedSampler(range(3), num_replicas=2, rank=1))


def test_state_dict_in_the_middle_reproduces_the_second_epoch(tree):
    c = F.config("train")
    feed = F.make_feed(tree, c)
    feed.plan_epoch(0)
    state = feed.state_dict()
    want = feed.plan_epoch(1)
    assert [i for p in want for i in p.items] == F.items("train", 1)
    random.seed(999)
    np.random.seed(999)
    torch.manual_seed(999)
    fresh = F.make_feed(tree, c, reseed=False)
    fresh.load_state_dict(state)
    assert fresh.epoch == 0
    got = fresh.plan_epoch(1)
    assert got == want and fresh.epoch == 1
    assert (F.random_crc(), F.torch_crc()) == F.state_crcs("train", 1)
    assert want != feed.plan_epoch(2)                                            # (the comparison can tell two epochs apart)


def test_a_sampler_of_one_s_own_overrides_the_order(tree):
    c = F.config("train")
    feed = F.make_feed(tree, c, sampler=lambda ds: [4, 0, 4])
    plans = feed.plan_epoch(0)
    assert [p.items for p in plans] == [[4, 0], [4]]


# ---------------------------------------------------------------------------------------------- the store form of the ingest's plan
def test_the_store_form_of_plan_waves_gives_the_list_form_s_table_but_for_the_offsets(tree):
    from m3t import audio, audioset
    g = F.golden()
    clips = [F.clip(str(f)) for f in g["train.files"]]
    lens = np.array([len(c) for c in clips], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    flat = torch.from_numpy(np.concatenate(clips))
    items = [4, 0, 4, 2]
    random.seed(5)
    draws = [audio.draw_audioset(int(lens[i]), 4, True) for i in items]
    wave_l, table_l, R_l = audio.plan_waves([clips[i] for i in items], draws, 4)
    wave_s, table_s, R_s = audio.plan_waves(flat, draws, 4, lengths=lens[items], offsets=offs[items])
    assert wave_s.data_ptr() == flat.data_ptr() and wave_s.numel() == flat.numel()          # read in place: no sample is copied
    assert R_s == R_l and np.array_equal(table_s[:, 1:], table_l[:, 1:])
    assert table_s[:, 0].tolist() == offs[items].tolist() and table_l[:, 0].tolist() == [0, 4267, 20267, 24534]
    for n, i in enumerate(items):                                                # the same samples behind either table
        assert np.array_equal(wave_l.numpy()[table_l[n, 0]:table_l[n, 0] + table_l[n, 1]], flat.numpy()[table_s[n, 0]:table_s[n, 0] + table_s[n, 1]])
    got_items, table_b, R_b = audioset.plan_batch(flat, offs, lens, items, draws, 4)
    assert got_items.tolist() == items and np.array_equal(table_b, table_s) and R_b == R_s
    # the evaluation draws when none are given
    _, table_e, _ = audioset.plan_batch(flat, offs, lens, [1], None, 4)
    assert table_e[0, 2:4].tolist() == [(3000 - 2133) // 2, 2133]


def test_the_store_form_refuses_what_leaves_the_buffer(tree):
    from m3t import audio, audioset
    flat = torch.zeros(1000, dtype=torch.int16)
    d = [audio.draw_audioset(100, 4, False)]
    audio.plan_waves(flat, d, 4, lengths=[100], offsets=[900])
    for offs, lens, what in (([901], [100], "outside the buffer"), ([-1], [100], "outside the buffer"), ([0], [1001], "outside the buffer"),
                             ([0], [0], "empty"), ([2 ** 62], [2 ** 62], "outside the buffer")):
        with pytest.raises(ValueError, match=what):
            audio.plan_waves(flat, d, 4, lengths=lens, offsets=offs)
    with pytest.raises(ValueError, match="lengths"):
        audio.plan_waves(flat, d, 4, offsets=[0])
    with pytest.raises(ValueError, match="flat"):
        audio.plan_waves(flat.reshape(10, 100), d, 4, lengths=[100], offsets=[0])
    with pytest.raises(ValueError, match="integers"):
        audio.plan_waves(flat, d, 4, lengths=[100.0], offsets=[0])
    with pytest.raises(ValueError, match="int16 or float32"):
        audio.plan_waves(flat.to(torch.int32), d, 4, lengths=[100], offsets=[0])
    with pytest.raises(ValueError, match="2 draws for 1 clips"):
        audio.plan_waves(flat, d + d, 4, lengths=[100], offsets=[0])
    offs, lens = np.array([0, 400]), np.array([400, 600])
    for items in ([2], [-1], [0, 1, 5]):
        with pytest.raises(ValueError, match=r"clip %d; the store holds 2" % items[-1]):
            audioset.plan_batch(flat, offs, lens, items, None, 4)
    with pytest.raises(ValueError, match="non-empty"):
        audioset.plan_batch(flat, offs, lens, [], None, 4)


# ---------------------------------------------------------------------------------------------- the module and the driver
def test_the_task_module_builds_the_feeds_without_a_gpu(tree):
    code = ("import sys; sys.path[:0] = %r\n"
            "import argparse, torch\n"
            "from models.audioset_model import AudioSet\n"
            "ns = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])\n"
            "ns.dataset_path, ns.window, ns.batch_size, ns.num_hidden = %r, 4, 2, 16\n"
            "m = AudioSet(ns)\n"
            "train, val = m.train_dataloader(), m.val_dataloader()\n"
            "assert (train.split, val.split, len(train), len(val)) == ('train', 'val', 3, 2)\n"
            "assert (train.window, train.batch_size, train.world, train.store) == (4, 2, 1, None)\n"
            "assert len(train.plan_epoch(0)) == 3 and [p.items for p in val.plan_epoch(0)] == [[0, 1], [2]]\n"
            "train.state_dict()\n"
            "assert not torch.cuda.is_initialized()\n"
            "print('planned')\n") % ([p for p in sys.path if p], tree)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "planned" in res.stdout, res.stderr[-2000:]


def test_the_driver_s_parser_has_the_reference_s_flags_and_defaults():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pretrain_audioset", os.path.join(PKG, "pretrain_audioset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ns = mod.make_parser().parse_args([])
    # pretrain_audioset.py:41-46 of the reference
    assert (ns.gpus, ns.nodes, ns.seed, ns.checkpoint) == ("2", 1, 12345, "")
    # models/audioset_model.py:147-175 of the reference
    assert (ns.learning_rate, ns.min_lr, ns.decay_factor, ns.batch_size, ns.optimizer, ns.scheduler) == (0.3, 1e-3, 0.5, 128, "adam", "plateau")
    assert (ns.num_fc_layers, ns.num_hidden, ns.window, ns.workers, ns.max_nb_epochs, ns.checkpoint_path) == (2, 256, 32, 8, 80, "./audioset")
    assert ns.test_lr is False and ns.distributed is False and ns.dataset_path.endswith("AudioSet_16k")
    assert sorted(vars(ns)) == sorted(["gpus", "nodes", "seed", "checkpoint", "learning_rate", "min_lr", "decay_factor", "batch_size", "optimizer",
                                       "scheduler", "test_lr", "num_fc_layers", "num_hidden", "window", "distributed", "dataset_path",
                                       "checkpoint_path", "workers", "max_nb_epochs"])
    ns = mod.make_parser().parse_args(["--test_lr"])
    with pytest.raises(NotImplementedError, match="LR range finder"):
        mod.main(ns)
