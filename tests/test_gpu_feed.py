"""The AffWild2 epoch feed (m3t/feed.py) on the GPU against the reference loader's record of the synthetic tree
(tests/golden/feed_cases.npz): every batch bit for bit, the by-hand composition of the stores, the stream, a damaged frame, the task module
and the trainer fed by it, and the two drivers as child processes."""
import argparse
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import feed_ref as F

pytestmark = pytest.mark.gpu
CONFIGS = F.configs()
IDENTITY = np.arange(256, dtype=np.float32)
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m3f.pytorch_amd")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = F.write_tree(tmp_path_factory.mktemp("affwild"))
    os.makedirs(os.path.join(root, "runA", "splits"))                           # a split of A alone: the one video with 8-frame windows
    for f in ("frames_fps.csv", "expr.csv"):
        with open(os.path.join(root, "run128", "splits", f)) as src, open(os.path.join(root, "runA", "splits", f), "w") as dst:
            dst.write(src.read())
    with open(os.path.join(root, "runA", "splits", "train.csv"), "w") as f:
        f.write("A\n")
    return root


def _same_bits(got, ref, what):
    assert tuple(got.shape) == ref.shape and got.cpu().numpy().dtype == ref.dtype, (what, got.dtype, tuple(got.shape), ref.dtype, ref.shape)
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(ref).tobytes(), what


def _planes(batch):
    """the clip the reference hands the model before normalisation, as the ingest expresses it: the identity table, so a pixel is its own
    value; the ingest writes the cutout's fill AFTER normalisation (0.0), the reference's 127.5 goes into the drawn boxes here"""
    from m3t import video
    raw = video.ingest(batch["video"], batch["video_aug"], batch["video_frame_idx"], layout="planes", norm=IDENTITY).cpu().numpy()
    filled = raw.copy()
    for n, a in enumerate(batch["video_aug"]):
        if a["cutout"]:
            y1, y2, x1, x2 = a["cutout"]
            filled[n, :, :, y1:y2, x1:x2] = 127.5
    return raw, filled


# ---------------------------------------------------------------------------------------------- every batch against the reference
@pytest.mark.parametrize("name", CONFIGS)
def test_every_batch_equals_the_reference_s(tree, name):
    g, c = F.golden(), F.config(name)
    feed = F.make_feed(tree, c)
    want_items = F.items(name)
    crcs, seen = [], 0
    for b, batch in enumerate(feed):
        ref = F.batch_arrays(name, b)
        n = len(batch["vid_name"])
        assert list(zip(batch["vid_name"], batch["start"].tolist(), batch["length"].tolist())) == want_items[seen:seen + n]
        seen += n
        extra = {"vid_name", "start", "length"} | ({"video", "video_aug", "video_frame_idx"} if c.visual else set())
        assert sorted(set(batch) - extra) == sorted(ref), (sorted(batch), sorted(ref))
        for k, v in ref.items():
            assert batch[k].is_cuda
            _same_bits(batch[k], v, (b, k))
        if c.visual:
            assert batch["video"].dtype == torch.uint8 and tuple(batch["video"].shape) == (n, c.window, c.input_size, c.input_size, 3)
            raw, filled = _planes(batch)
            crcs.append(F.frame_crcs(filled))
            if b == 0:
                assert np.array_equal(raw, g[name + ".video0"].astype(np.float32))
    assert b == c.n_batches - 1 and seen == len(want_items) and feed.decode_errors == []
    if c.visual:
        assert np.array_equal(np.concatenate(crcs), g[name + ".crc"])


@pytest.mark.parametrize("name", CONFIGS)
def test_every_batch_equals_the_stores_driven_by_hand(tree, name):
    from collections import OrderedDict
    from m3t import dataset, jpeg
    c = F.config(name)
    corpus = F.scan(tree, c)
    got = list(F.make_feed(tree, c, corpus=corpus))
    plans = F.make_feed(tree, c, corpus=corpus).plan_epoch(0)
    videos, frames = corpus.videos, None
    if c.visual:
        frames = jpeg.FrameStore(corpus.frames, c.window)
        videos = OrderedDict((n, dict(corpus.videos[n], has_image=frames.has_image(n))) for n in corpus.names)
    tracks = dataset.TrackStore(videos, c.window, c.split)
    assert len(plans) == len(got)
    for plan, batch in zip(plans, got):
        hand = tracks.collate(plan.items)
        if c.visual:
            hand["video"], hand["video_frame_idx"], _ = frames.decode(plan.items)
            hand["video_aug"] = plan.aug
        assert sorted(hand) == sorted(batch)
        for k, v in hand.items():
            assert torch.equal(v, batch[k]) if isinstance(v, torch.Tensor) else v == batch[k], (plan.index, k)


def test_the_feed_runs_on_the_current_stream(tree):
    c = F.config("val_av")
    corpus = F.scan(tree, c)
    want = list(F.make_feed(tree, c, corpus=corpus))
    feed = F.make_feed(tree, c, corpus=corpus).build_stores()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = list(feed)
    st.synchronize()
    assert len(got) == len(want) == c.n_batches
    for a, b in zip(got, want):
        for k, v in b.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(a[k], v), k


# ---------------------------------------------------------------------------------------------- a damaged frame
def test_a_damaged_frame_is_reported_once_when_the_epoch_ends(tmp_path):
    """The damaged streams of jpeg_cases are 40 x 56 and the frames of a store share one size, so they cannot go among the tree's 128-pixel
    frames: they get a folder of their own -- release 'ibug' (no crop), input_size 40, the test split, one video made of the first frames
    of jpeg_cases.damaged_batch(): an undamaged neighbour, eight truncated streams, a neighbour, two more."""
    import jpeg_cases
    from m3t import feed as feed_mod
    streams, names = jpeg_cases.damaged_batch()
    streams, names = streams[:12], names[:12]
    kinds = {d[0]: d[1] for d in jpeg_cases.damaged()}
    root = str(tmp_path)
    for sub in ("cropped_aligned/dmg", "se101_feats", "AU_feats", "splits"):
        os.makedirs(os.path.join(root, sub))
    for i, data in enumerate(streams):
        with open(os.path.join(root, "cropped_aligned", "dmg", "%05d.jpg" % (i + 1)), "wb") as f:
            f.write(data)
    np.save(os.path.join(root, "se101_feats", "dmg.npy"), np.zeros((12, 512), np.float32))
    np.save(os.path.join(root, "AU_feats", "dmg.npy"), np.zeros((12, 268), np.float32))
    for f, text in (("frames_fps.csv", "dmg,12,30.0\n"), ("test.csv", "dmg\n")):
        with open(os.path.join(root, "splits", f), "w") as out:
            out.write(text)
    corpus = feed_mod.scan_affwild(root, "test", "visual", release="ibug", input_size=40, splits_dir=os.path.join(root, "splits"), window=4)
    fd = feed_mod.AffWild2Feed(corpus, 4, 2, "test", "visual", input_size=40, release="ibug", inv_test_stride=2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        batches = list(fd)
    assert len(batches) == len(fd) == 3                                          # the epoch ran to its end
    ours = [w for w in caught if "did not decode cleanly" in str(w.message)]
    assert len(ours) == 1 and "dmg frame 1 " in str(ours[0].message)
    reported = {(v, f) for v, f, _ in fd.decode_errors}
    assert len(reported) == len(fd.decode_errors) and all(s != 0 for _, _, s in fd.decode_errors)
    assert reported >= {("dmg", i) for i, n in enumerate(names) if kinds.get(n) == "trunc"} and len(reported) >= 8
    assert not reported & {("dmg", i) for i, n in enumerate(names) if n not in kinds}
    with warnings.catch_warnings(record=True) as caught:                          # the next epoch reports again, once
        warnings.simplefilter("always")
        list(fd)
    assert len([w for w in caught if "did not decode cleanly" in str(w.message)]) == 1 and len(fd.decode_errors) == len(reported)


# ---------------------------------------------------------------------------------------------- through the model and the trainer
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _two_steps(model, feed):
    from m3t import ops
    from m3t.trainer import Trainer
    tr = Trainer.from_hparams(model, model.hparams, gradient_clip_val=1.0)
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    stock = dict(ops.STOCK_FALLBACKS)
    losses = []
    for batch in feed:
        losses.append(float(tr.step(batch)["loss"].detach()))
        if len(losses) == 2:
            break
    assert len(losses) == 2 and all(np.isfinite(l) for l in losses), losses
    after = model.state_dict()
    assert any(not torch.equal(v, after[k]) for k, v in before.items())
    assert dict(ops.STOCK_FALLBACKS) == stock


def test_the_audio_model_steps_straight_from_the_feed(tree):
    from models.model import AffWild2VA
    hp = _hp(modality="audio", window=4, batch_size=2, windows_per_epoch=3, input_size=128, dataset_path=os.path.join(tree, "data"),
             splits_dir=os.path.join(tree, "run128", "splits"), scheduler="none")
    torch.manual_seed(3)
    model = AffWild2VA(hp).cuda()
    _two_steps(model, model.train_dataloader())


def test_the_audiovisual_model_steps_straight_from_the_feed(tree):
    """2 clips x 8 frames of 128 -> 112, v2p_split, cutout and mirror drawn by the feed; A alone has windows of 8 (with resample)"""
    from models.model import AffWild2VA
    hp = _hp(modality="audiovisual", backbone="v2p_split", window=8, batch_size=2, windows_per_epoch=4, input_size=128, cutout=True, resample=True,
             dataset_path=os.path.join(tree, "data"), splits_dir=os.path.join(tree, "runA", "splits"), scheduler="none")
    torch.manual_seed(4)
    model = AffWild2VA(hp).cuda()
    feed = model.train_dataloader()
    assert len(feed) == 2 and feed.model_visual is model.visual
    _two_steps(model, feed)


def test_evaluate_over_the_feed_equals_evaluate_over_batches_built_by_hand(tree, tmp_path, monkeypatch):
    from m3t import dataset
    from m3t.trainer import Trainer
    from models.model import AffWild2VA
    monkeypatch.chdir(tmp_path)
    hp = _hp(modality="audio", window=4, batch_size=2, input_size=128, dataset_path=os.path.join(tree, "data"),
             splits_dir=os.path.join(tree, "run128", "splits"))
    torch.manual_seed(5)
    model = AffWild2VA(hp).cuda()
    tr = Trainer.from_hparams(model, hp)
    feed = model.val_dataloader()
    assert feed.names == ["A", "E", "D"]                                         # (C has 12 fps: dropped for modality 'audio')
    store = dataset.TrackStore(feed.corpus.videos, 4, "val")
    items = dataset.eval_items(feed.corpus.nb_frames, 4, 1)
    want = tr.evaluate(list(store.batches(items, 2)))
    want_file = torch.load("predictions_val.pt")
    os.remove("predictions_val.pt")
    got = tr.evaluate(feed)
    got_file = torch.load("predictions_val.pt")
    assert got == want and set(got["log"]) >= {"val_ccc_v", "val_ccc_a", "val_loss"}
    assert list(got_file) == list(want_file)
    for k in want_file:
        assert list(got_file[k]) == list(want_file[k]) == ["A", "E", "D"]
        for vid in want_file[k]:
            assert torch.equal(got_file[k][vid], want_file[k][vid]), (k, vid)


# ---------------------------------------------------------------------------------------------- the drivers
def _driver_args(tree):
    return ["--modality", "audio", "--window", "4", "--batch_size", "2", "--windows_per_epoch", "2", "--input_size", "128",
            "--dataset_path", os.path.join(tree, "data"), "--splits_dir", os.path.join(tree, "run128", "splits")]


def test_train_py_scores_the_epoch_on_the_device_on_request(tree, tmp_path):
    ck = str(tmp_path / "ck")
    res = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--max_nb_epochs", "1", "--checkpoint_path", ck, "--eval_on_device"]
                         + _driver_args(tree), cwd=str(tmp_path), env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    assert os.path.exists(os.path.join(ck, "best.ckpt")) and "epoch 0:" in res.stdout and "(improved)" in res.stdout
    val = torch.load(tmp_path / "predictions_val.pt")
    assert list(val["valence_pred"]) == ["A", "E", "D"] and tuple(val["valence_gt"]["A"].shape) == (11,)


def test_train_py_and_eval_py_run_on_the_tree(tree, tmp_path):
    common = _driver_args(tree)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    ck = str(tmp_path / "ck")
    res = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--max_nb_epochs", "1", "--checkpoint_path", ck, "--seed", "7"] + common,
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]                               # (nothing is started after a failure)
    best = os.path.join(ck, "best.ckpt")
    assert os.path.exists(best) and "Loaded partition train: 3 files, 6 windows" in res.stdout
    assert os.path.exists(tmp_path / "predictions_val.pt")
    res = subprocess.run([sys.executable, os.path.join(PKG, "eval.py"), "--checkpoint", best] + common,
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "Loaded pretrained weights" in res.stdout
    pred = torch.load(tmp_path / "predictions_test.pt")
    frames = {"A": 11, "E": 3}                                                   # the test split's videos at 15 fps and above
    for k in ("valence_pred", "arousal_pred"):
        assert list(pred[k]) == ["A", "E"]
        for vid, n in frames.items():
            assert tuple(pred[k][vid].shape) == (n,) and bool(torch.isfinite(pred[k][vid]).all())
