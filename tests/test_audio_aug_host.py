"""The host half of the AudioSet feed's augmentation (m3t.audio.draw_spec_augment / plan_aug / pack_tables, m3t.audioset.AudioSetFeed's
spec_augment and mixup_alpha) without a GPU: the mask draws against the reference's own spec_augment as recorded in
tests/golden/spec_augment_cases.npz (zero patterns and both generators' states), the refusals, the order of the draws in a training epoch,
that switched off nothing changes, the resume state, the validation split, the driver's flags, and csrc/audio_aug_core.h as a stand-alone
program under the address and undefined-behaviour sanitizers.  Nothing here may touch a GPU."""
import argparse
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_aug_ref as G
import audioset_feed_ref as F

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m3f.pytorch_amd")
SA = {"F": 20, "T": 8, "n_freq": 2, "n_time": 1}            # the tree's clips are 13 frames long (window 4): T stays below that


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.write_tree(tmp_path_factory.mktemp("audioset"))


# ---------------------------------------------------------------------------------------------- the mask draws against the reference
@pytest.mark.parametrize("case", G.cases(), ids=lambda c: "tau%d-F%g-T%g-%dx%d" % c[1:])
def test_draw_spec_augment_reproduces_the_reference_s_record(case):
    from m3t import audio
    c, tau, Fp, Tp, n_freq, n_time = case
    g = G.golden()
    for seed in G.seeds():
        random.seed(seed)
        np.random.seed(seed)
        key = "c%d.s%d." % (c, seed)
        if g[key + "refused"][0]:
            with pytest.raises(ValueError, match=r"clip 7.*does not fit"):
                audio.draw_spec_augment(tau, Fp, Tp, n_freq, n_time, name="clip 7")
            continue
        d = audio.draw_spec_augment(tau, Fp, Tp, n_freq, n_time)
        assert sorted(d) == ["fmask", "tmask"] and len(d["fmask"]) == n_freq and len(d["tmask"]) == n_time
        assert all(0 <= f0 and f0 + f <= 40 and f >= 0 for f0, f in d["fmask"]) and all(0 <= t0 and t0 + t <= tau and t >= 0 for t0, t in d["tmask"])
        assert np.array_equal(G.zero_pattern(d, tau), g[key + "zero"].astype(bool)), (case, seed, d)
        assert (G.random_crc(), G.numpy_crc()) == (int(g[key + "random_crc"][0]), int(g[key + "numpy_crc"][0])), (case, seed)


def test_the_defaults_are_the_reference_s():
    from m3t import audio
    random.seed(3)
    np.random.seed(3)
    a = audio.draw_spec_augment(97)
    random.seed(3)
    np.random.seed(3)
    assert a == audio.draw_spec_augment(97, 20, 20, 1, 1) and audio.MAX_MASKS == 4


def test_the_cell_rule_on_stacked_rows_is_the_mask_on_the_spectrogram():
    """the oracle's own two statements of the rule agree: zeroing slices of [40, tau] and then stacking, against mask_rows on the stack"""
    rs = np.random.RandomState(0)
    for tau, T in ((13, 4), (97, 32), (8, 4)):
        spec = (1 + np.arange(40 * tau, dtype=np.float32)).reshape(40, tau)
        d = {"fmask": [(int(rs.randint(0, 30)), int(rs.randint(0, 11))), (37, 3)], "tmask": [(int(rs.randint(0, tau - 4)), 4), (tau - 2, 2)]}
        masked = np.where(G.zero_pattern(d, tau), np.float32(0), spec)
        stack = lambda s: np.stack([np.concatenate([s[:, 3 * i + k] if 3 * i + k < tau else np.zeros(40, np.float32) for k in range(5)]) for i in range(T)])
        assert np.array_equal(G.mask_rows(stack(spec), d), stack(masked))


# ---------------------------------------------------------------------------------------------- the refusals
def test_refusals():
    from m3t import audio
    with pytest.raises(ValueError, match=r"5 frequency and 1 time masks"):
        audio.draw_spec_augment(97, n_freq=5)
    with pytest.raises(ValueError, match=r"0 .. 4"):
        audio.draw_spec_augment(97, n_time=-1)
    random.seed(0)
    np.random.seed(0)
    with pytest.raises(ValueError, match=r"b\.wav.*time mask of \d+ frames does not fit the 2"):
        for _ in range(50):
            audio.draw_spec_augment(2, 20, 20, 1, 1, name="b.wav")
    with pytest.raises(ValueError, match=r"b\.wav.*frequency mask of \d+ bands does not fit the 40"):
        for _ in range(50):
            audio.draw_spec_augment(97, 400, 20, 1, 1, name="b.wav")
    # plan_aug: the tables of a launch, validated before it
    table = np.zeros((3, 8), np.int64)
    table[:, 5] = (13, 13, 7)
    plain = [{"fps": 30.0}] * 3
    assert audio.plan_aug(plain, table) is None and audio.plan_aug(None, table) is None
    ok = [dict(fmask=[(0, 40)], tmask=[(0, 13)]), dict(fmask=[], tmask=[(13, 0)]), dict(tmask=[(3, 4)] * 4)]
    ints, w = audio.plan_aug(ok, table, ([2, 1, 0], [1.0, 0.25, 0.0]))
    assert ints.dtype == np.int32 and ints.shape == (3, 20) and w.dtype == np.float32 and w.shape == (3, 2)
    assert ints[:, :4].tolist() == [[1, 1, 2, 0], [0, 1, 1, 0], [0, 4, 0, 0]] and ints[0, 4:6].tolist() == [0, 40] and ints[2, 12:].tolist() == [3, 4] * 4
    assert w.tolist() == [[1.0, 0.0], [0.25, 0.75], [0.0, 1.0]]
    ints, w = audio.plan_aug(ok, table)
    assert ints[:, 2].tolist() == [-1, -1, -1] and w.tolist() == [[1.0, 0.0]] * 3
    ints, w = audio.plan_aug(plain, table, ([0, 1, 2], [0.3, 0.3, 0.3]))               # mixup alone
    assert ints[:, :3].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 2]] and w[0, 0] == np.float32(0.3) and w[0, 1] == np.float32(1) - np.float32(0.3)
    for bad, what in (([dict(fmask=[(1, 40)])] + plain[1:], r"clip 0: mask bands 1 \.\. 41 lies outside the clip's 40"),
                      (plain[:2] + [dict(tmask=[(4, 4)])], r"clip 2: mask frames 4 \.\. 8 lies outside the clip's 7"),
                      ([dict(tmask=[(-1, 2)])] + plain[1:], r"clip 0: mask frames -1"),
                      ([dict(fmask=[(0, 1)] * 5)] + plain[1:], r"clip 0: 5 masks under 'fmask'; at most 4")):
        with pytest.raises(ValueError, match=what):
            audio.plan_aug(bad, table)
    for mix, what in ((([0, 3, 1], [0.5] * 3), r"clip 1: its partner 3 is outside the batch of 3"), (([0, -1, 1], [0.5] * 3), r"partner -1"),
                      (([0, 1, 2], [0.5, 1.5, 0.5]), r"clip 1: lam 1\.5"), (([0, 1, 2], [0.5, float("nan"), 0.5]), r"clip 1: lam nan"),
                      (([0, 1], [0.5, 0.5]), r"mix needs"), (([0.0, 1.0, 2.0], [0.5] * 3), r"mix needs")):
        with pytest.raises(ValueError, match=what):
            audio.plan_aug(plain, table, mix)
    with pytest.raises(ValueError, match=r"aug=None"):
        audio.plan_aug(None, table, ([0, 1, 2], [0.5] * 3))
    # ... and through ingest, before any device is looked for
    y = [np.zeros(3000, np.int16)]
    d = audio.draw_audioset(3000, 4, False)
    with pytest.raises(ValueError, match=r"clip 0: mask frames 10 \.\. 14 lies outside the clip's 13"):
        audio.ingest(y, [dict(d, tmask=[(10, 4)])], 4)
    with pytest.raises(ValueError, match=r"partner 1 is outside the batch of 1"):
        audio.ingest(y, [d], 4, mix=([1], [0.5]))
    with pytest.raises(ValueError, match=r"aug=None"):
        audio.ingest(y, None, 4, mix=([0], [0.5]))


def test_one_copy_carries_every_table():
    from m3t import audio
    table = np.arange(24, dtype=np.int64).reshape(3, 8)
    table[:, 5] = 13
    ints, w = audio.plan_aug([dict(fmask=[(1, 2)], tmask=[(3, 4)])] * 3, table, ([1, 2, 0], [0.25, 0.5, 1.0]))
    flat, split = audio.pack_tables(table, (ints, w), [7, 8, 9])
    assert flat.dtype == np.int64 and flat.shape == (3 * 8 + 3 * 10 + 3 + 3,)
    tab, (ai, af), tail = split(torch.from_numpy(flat))
    assert tab.tolist() == table.reshape(-1).tolist() and tail.tolist() == [7, 8, 9]
    assert ai.dtype == torch.int32 and ai.tolist() == ints.reshape(-1).tolist() and af.dtype == torch.float32 and af.tolist() == w.reshape(-1).tolist()
    assert ai.data_ptr() == tab.data_ptr() + 8 * 24 and af.data_ptr() == ai.data_ptr() + 4 * 60          # views of the one buffer
    flat, split = audio.pack_tables(table, None, [7])
    tab, none, tail = split(torch.from_numpy(flat))
    assert none is None and tab.numel() == 24 and tail.tolist() == [7]


# ---------------------------------------------------------------------------------------------- the feed
class Transcript:
    """wraps the generator calls the feed may make; every call is recorded as (name, argument, result)"""
    NAMES = (("random", "choice"), ("random", "randint"), ("np.random", "uniform"), ("np.random", "beta"), ("np.random", "permutation"))

    def __enter__(self):
        self.calls, self.orig = [], {}
        for mod, fn in self.NAMES:
            owner = random if mod == "random" else np.random
            self.orig[(mod, fn)] = getattr(owner, fn)
            setattr(owner, fn, self._wrap(fn, self.orig[(mod, fn)]))
        return self

    def _wrap(self, name, fn):
        def call(*a, **kw):
            v = fn(*a, **kw)
            self.calls.append((name, None if name == "choice" else kw.get("high", kw.get("size", a[-1] if a else None)), v))
            return v
        return call

    def __exit__(self, *exc):
        for (mod, fn), f in self.orig.items():
            setattr(random if mod == "random" else np.random, fn, f)


def test_a_training_epoch_draws_the_parent_s_draws_first_and_the_masks_after_them(tree):
    c = F.config("train")
    plain = F.make_feed(tree, c)
    base = plain.plan_epoch(0)
    feed = F.make_feed(tree, c, spec_augment=SA, mixup_alpha=0.4)
    with Transcript() as tr:
        plans = feed.plan_epoch(0)
    assert [p.items for p in plans] == [p.items for p in base] == [F.items("train", 0)[i:i + 2] for i in (0, 2, 4)]
    calls = list(tr.calls)
    for p in plans:
        for i, a in zip(p.items, p.aug):
            tau = 1 + a["nsamples"] // a["hop"]
            tot = max(int(feed.lengths[i]), a["nsamples"] + 5) if a["nsamples"] > feed.lengths[i] else int(feed.lengths[i])
            want = [("choice", None, a["fps"]), ("randint", tot - a["nsamples"], a["start"])]
            for f0, f in a["fmask"]:
                want += [("uniform", 20, None), ("randint", 40 - f, f0)]
            for t0, t in a["tmask"]:
                want += [("uniform", 8, None), ("randint", tau - t, t0)]
            got, calls = calls[:len(want)], calls[len(want):]
            assert [g[0] for g in got] == [w[0] for w in want], (i, got)
            assert all(g[1] == w[1] for g, w in zip(got, want) if w[0] != "choice") and all(g[2] == w[2] for g, w in zip(got, want) if w[2] is not None)
            assert [int(g[2]) for g in got if g[0] == "uniform"] == [f for _, f in a["fmask"]] + [t for _, t in a["tmask"]]
            assert len(a["fmask"]) == 2 and len(a["tmask"]) == 1 and tau == 13
        # then the batch's mix: the weights, then the partners
        (k1, n1, lam), (k2, n2, perm) = calls[:2]
        calls = calls[2:]
        N = len(p.items)
        assert (k1, n1, k2, n2) == ("beta", N, "permutation", N)
        assert p.mix == (list(perm), list(lam)) and sorted(p.mix[0]) == list(range(N)) and all(0.0 <= v <= 1.0 for v in p.mix[1])
    assert not calls
    # the items' own draws differ from the plain feed's only by what the extra draws did to `random`: the first item's are the same
    first = {k: plans[0].aug[0][k] for k in ("fps", "hop", "start", "nsamples")}
    assert first == base[0].aug[0] and sorted(plans[0].aug[0]) == ["fmask", "fps", "hop", "nsamples", "start", "tmask"]
    # masks alone, mixup alone
    only_masks = F.make_feed(tree, c, spec_augment=True).plan_epoch
    with pytest.raises(ValueError, match=r"balanced_train_segments.*\.wav: a time mask of \d+ frames does not fit the 13"):
        for e in range(20):                       # the defaults' T = 20 reaches past these 13-frame clips: refused with the file named
            only_masks(e)
    mixed = F.make_feed(tree, c, mixup_alpha=1.0).plan_epoch(0)
    assert [p.aug for p in mixed] == [p.aug for p in base] and all(p.mix is not None for p in mixed) and all(p.mix is None for p in base)
    assert mixed != base


def test_switched_off_nothing_changes(tree):
    from m3t import audioset
    for name in ("train", "val"):
        c = F.config(name)
        a = F.make_feed(tree, c)
        pa = [a.plan_epoch(e) for e in range(2)]
        sa = (F.random_crc(), G.numpy_crc(), F.torch_crc())
        b = F.make_feed(tree, c, spec_augment=None, mixup_alpha=0.0)
        pb = [b.plan_epoch(e) for e in range(2)]
        assert pa == pb and sa == (F.random_crc(), G.numpy_crc(), F.torch_crc())
        assert all(p.mix is None and all(sorted(d) == ["fps", "hop", "nsamples", "start"] for d in p.aug) for e in pb for p in e)
        assert b.spec_augment is None and b.mixup_alpha == 0.0
        assert repr(pb[0][0]) == "BatchPlan(index=0, items=%r, aug=%r)" % (pb[0][0].items, pb[0][0].aug)
    assert audioset.BatchPlan([1], [{}], 0) == audioset.BatchPlan([1], [{}], 0, None) != audioset.BatchPlan([1], [{}], 0, ([0], [0.5]))
    with pytest.raises(ValueError, match="spec_augment takes"):
        F.make_feed(tree, F.config("train"), spec_augment={"freq": 3})
    with pytest.raises(ValueError, match=r"0 \.\. 4 masks"):
        F.make_feed(tree, F.config("train"), spec_augment={"n_time": 5})
    with pytest.raises(ValueError, match="mixup_alpha must be positive"):
        F.make_feed(tree, F.config("train"), mixup_alpha=-1.0)


def test_the_validation_split_ignores_the_options(tree):
    c = F.config("val")
    plain = F.make_feed(tree, c).plan_epoch(0)
    feed = F.make_feed(tree, c, spec_augment=SA, mixup_alpha=0.4)
    before = (F.random_crc(), G.numpy_crc())
    with Transcript() as tr:
        plans = feed.plan_epoch(0)
    assert plans == plain and not tr.calls and before == (F.random_crc(), G.numpy_crc())
    assert feed.spec_augment is None and feed.mixup_alpha == 0.0 and all(p.mix is None for p in plans)
    assert (F.random_crc(), F.torch_crc()) == F.state_crcs("val", 0)


def test_state_dict_resumes_the_augmented_plan(tree):
    c = F.config("train")
    feed = F.make_feed(tree, c, spec_augment=SA, mixup_alpha=0.4)
    feed.plan_epoch(0)
    state = feed.state_dict()
    want = feed.plan_epoch(1)
    random.seed(999)
    np.random.seed(999)
    torch.manual_seed(999)
    fresh = F.make_feed(tree, c, reseed=False, spec_augment=SA, mixup_alpha=0.4)
    fresh.load_state_dict(state)
    got = fresh.plan_epoch(1)
    assert got == want and all(p.mix is not None and "tmask" in p.aug[0] for p in got)
    assert want != feed.plan_epoch(2)                                            # (the comparison can tell two epochs apart)
    np.random.seed(5)                                                            # ... and it is numpy's generator the mix hangs on
    fresh.load_state_dict(state)
    np.random.seed(6)
    assert [p.mix for p in fresh.plan_epoch(1)] != [p.mix for p in want]


# ---------------------------------------------------------------------------------------------- the driver and the module
def test_the_driver_s_flags_are_absent_unless_given(tree):
    from m3t import audioset
    sys.path.insert(0, PKG)
    import pretrain_audioset as P
    ns = P.make_parser().parse_args([])
    flags = ("spec_augment", "freq_mask_para", "time_mask_para", "freq_mask_num", "time_mask_num", "mixup_alpha")
    assert not any(hasattr(ns, f) for f in flags)
    from models.audioset_model import AudioSet
    model_ns = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    assert not any(hasattr(model_ns, f) for f in flags)                           # the driver's flags, not the model's
    ns = P.make_parser().parse_args(["--spec_augment", "--time_mask_para", "8", "--freq_mask_num", "2", "--mixup_alpha", "0.4",
                                     "--dataset_path", tree, "--window", "4", "--batch_size", "2"])
    assert ns.spec_augment is True and ns.time_mask_para == 8.0 and ns.freq_mask_num == 2 and ns.mixup_alpha == 0.4
    train, val = audioset.feed_from_hparams(ns, "train"), audioset.feed_from_hparams(ns, "val")
    assert train.spec_augment == {"F": 20, "T": 8.0, "n_freq": 2, "n_time": 1} and train.mixup_alpha == 0.4
    assert val.spec_augment is None and val.mixup_alpha == 0.0
    ns = P.make_parser().parse_args(["--time_mask_para", "8", "--dataset_path", tree, "--window", "4", "--batch_size", "2"])
    plain = audioset.feed_from_hparams(ns, "train")                               # a parameter without --spec_augment switches nothing on
    assert plain.spec_augment is None and plain.mixup_alpha == 0.0


def test_the_task_module_hands_the_mix_to_the_ingest(monkeypatch):
    from m3t import audio
    from models.audioset_model import AudioSet
    ns = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.window, ns.num_hidden = 4, 16
    seen = []
    monkeypatch.setattr(audio, "ingest", lambda x, aug, length, lengths, mix=None: seen.append((aug, length, lengths, mix)) or "rows")
    m = AudioSet(ns)
    pcm = torch.zeros(2, 3000, dtype=torch.int16)
    assert m._features(pcm, ["d", "d"], None, ([1, 0], [0.5, 0.5])) == "rows" and m._features(pcm) == "rows"
    assert seen == [(["d", "d"], 4, None, ([1, 0], [0.5, 0.5])), (None, 4, None, None)]
    rows = torch.zeros(2, 4, 200)
    assert m._features(rows, None, None, ([1, 0], [0.5, 0.5])) is rows            # ready rows are left alone


# ---------------------------------------------------------------------------------------------- the cell rule under sanitizers
def test_cell_rule_on_the_host_under_sanitizers(tmp_path):
    """csrc/audio_aug_core.h -- the text m3t_audio_db_stack_aug compiles -- as a stand-alone program with its own main, built with the
    address and undefined-behaviour sanitizers: every cell of every (T, nf, masks) case agrees with masking the spectrogram and then
    stacking it, and no read leaves the 20-int table."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "audio_aug_host_check")
    src = os.path.join(PKG, "csrc", "audio_aug_host_check.cpp")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    b = subprocess.run([cxx] + flags + [src, "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and ("sanitize" in b.stderr + b.stdout or "asan" in (b.stderr + b.stdout).lower()):
        b = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], capture_output=True, text=True)      # no sanitizer runtime installed
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cases agree" in r.stdout
