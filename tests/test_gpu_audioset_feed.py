"""The AudioSet epoch feed (m3t/audioset.py) on the GPU against the reference loader's record of the synthetic tree
(tests/golden/audioset_feed_cases.npz): every batch of every configuration, the store's addressing against the list form of the ingest, the
label launch, the task module and the trainer fed by it, and the driver as a child process.

Bounds.  `label` is a copy: bit-equal.  `audio` is held to tests/audio_ingest_ref.TOL_DB (2e-3 dB), the project's bound of the fp32 DFT by
GEMM against the float64 oracle: the golden's audio IS that oracle, run by the reference's own loader code through a stub librosa (the
generator's header: a restatement of librosa, not a run of it).  Feed against list form, and validation_step against validation_step: the
same kernels on the same samples, so bit-equal."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_ingest_ref as A
import audioset_feed_ref as F

pytestmark = pytest.mark.gpu
CONFIGS = F.configs()
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m3f.pytorch_amd")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.write_tree(tmp_path_factory.mktemp("audioset"))


@pytest.fixture(scope="module")
def clips():
    g = F.golden()
    return {split: [F.clip(str(f)) for f in g[split + ".files"]] for split in ("train", "val")}


def _epochs(tree, name):
    """[(epoch, batches, generator states after it)] of a recorded configuration, iterated as a training loop does"""
    c = F.config(name)
    feed = F.make_feed(tree, c)
    out = []
    for epoch in range(c.epochs):
        feed.set_epoch(epoch)
        batches = list(feed)
        out.append((epoch, batches, (F.random_crc(), F.torch_crc())))
    return c, feed, out


# ---------------------------------------------------------------------------------------------- every batch against the reference
@pytest.mark.parametrize("name", CONFIGS)
def test_every_batch_equals_the_reference_s(tree, name):
    c, feed, epochs = _epochs(tree, name)
    worst = 0.0
    for epoch, batches, states in epochs:
        assert len(batches) == F.n_batches(name, epoch)
        for b, batch in enumerate(batches):
            ref_audio, ref_label = F.batch(name, epoch, b)
            assert sorted(batch) == ["audio", "label"] and batch["audio"].is_cuda and batch["label"].is_cuda
            assert batch["audio"].dtype == torch.float32 and tuple(batch["audio"].shape) == ref_audio.shape == (ref_label.shape[0], 4, 200)
            assert batch["label"].dtype == torch.float32 and tuple(batch["label"].shape) == ref_label.shape
            assert batch["label"].cpu().numpy().tobytes() == ref_label.tobytes(), (epoch, b)
            err = A.max_err(batch["audio"], ref_audio.astype(np.float64), "%s e%d b%d" % (name, epoch, b))
            worst = max(worst, err)
            assert err < A.TOL_DB, (epoch, b, err)
        assert states == F.state_crcs(name, epoch)
    print("%s: worst |feed - reference| = %.3e dB over %d epochs, store %d bytes" % (name, worst, c.epochs, feed.store.nbytes))
    assert feed.store.wave.dtype == torch.int16 and feed.store.wave.dim() == 1 and len(feed.store) == len(feed.files)
    assert feed.store.nbytes == 2 * int(feed.lengths.sum()) + 527 * len(feed.files)


# ---------------------------------------------------------------------------------------------- the store's addressing
@pytest.mark.parametrize("name", ["train", "val", "train_w2r1"])
def test_the_feed_s_audio_is_the_list_form_s_bit_for_bit(tree, clips, name):
    """same kernels, other offsets: the clips of a batch handed to m3t.audio.ingest as a list (copied, packed from offset 0) against the same
    clips read in place out of the store"""
    from m3t import audio
    c = F.config(name)
    feed = F.make_feed(tree, c)
    plans = feed.plan_epoch(0)
    assert [i for p in plans for i in p.items] == F.items(name, 0)
    for plan in plans:
        got = feed.batch(plan)["audio"]
        want = audio.ingest([clips[c.split][i] for i in plan.items], plan.aug, c.window)
        assert torch.equal(got, want), plan
    # a hand-made batch out of the store: a repeat, the last clip first, evaluation draws
    store = feed.store
    got = store.batch([len(store) - 1, 0, len(store) - 1], None, c.window)["audio"]
    want = audio.ingest([clips[c.split][i] for i in (len(store) - 1, 0, len(store) - 1)], None, c.window)
    assert torch.equal(got, want) and torch.equal(got[0], got[2])
    for pad_mode in ("reflect",):
        got = store.batch([1, 0], None, c.window, pad_mode=pad_mode)["audio"]
        assert torch.equal(got, audio.ingest([clips[c.split][1], clips[c.split][0]], None, c.window, pad_mode=pad_mode))


def test_the_store_is_staged_through_a_bounded_host_buffer(tree, clips):
    """a stage of 6 000 samples: clip a (16 000) goes on its own, b and c share the buffer, d (9 000) flushes it and goes on its own, e is
    flushed at the end"""
    from m3t import audioset
    scan = audioset.scan_audioset(tree, "train")
    small = audioset.WaveStore(scan.files, scan.labels, chunk_bytes=12000)
    whole = audioset.WaveStore(scan.files, scan.labels)
    want = np.concatenate(clips["train"])
    assert small.wave.cpu().numpy().tobytes() == whole.wave.cpu().numpy().tobytes() == want.tobytes()
    assert small.offsets.tolist() == [0, 16000, 19000, 21133, 30133] and small.lengths.tolist() == [16000, 3000, 2133, 9000, 4267]
    assert small.offsets.dtype == small.lengths.dtype == np.int64 and len(small) == 5
    assert small.label_table.dtype == torch.uint8 and small.label_table.is_cuda and small.nbytes == 2 * 34400 + 5 * 527
    with pytest.raises(ValueError, match=r"clip 5; the store holds 5"):
        small.batch([0, 5], None, 4)


# ---------------------------------------------------------------------------------------------- the label launch
def test_label_rows_against_numpy(tree):
    from m3t import _lib, audioset
    scan = audioset.scan_audioset(tree, "train")
    store = audioset.WaveStore(scan.files, scan.labels)
    items = [4, 0, 4]                                                            # a repeat; 3 x 527 cells: the last row ends at an odd address
    got = store.label_rows(torch.tensor(items, dtype=torch.int64, device="cuda"), 3)
    want = scan.labels[items].astype(np.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 527) and got.cpu().numpy().tobytes() == want.tobytes()
    assert want.sum(1).tolist() == [1, 1, 1] and want[0, 300] == 1
    d = store.batch([3], None, 4)["label"]                                       # class 526: the last column
    assert d[0, 526] == 1 and float(d.sum()) == 2
    # an item outside the table leaves its row untouched and reads nothing (the host refuses it first; the raw entry point is checked here)
    out = torch.full((3, 527), 7.0, device="cuda")
    bad = torch.tensor([1, 5, -1], dtype=torch.int64, device="cuda")
    lib = _lib.load()
    assert lib.m3t_label_rows(store.label_table.data_ptr(), 5, 527, bad.data_ptr(), 3, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tobytes() == scan.labels[1].astype(np.float32).tobytes() and bool((out[1:] == 7.0).all())
    assert lib.m3t_label_rows(store.label_table.data_ptr(), 5, 527, bad.data_ptr(), 0, out.data_ptr(), None) == 0
    assert lib.m3t_label_rows(store.label_table.data_ptr(), 5, 0, bad.data_ptr(), 3, out.data_ptr(), None) == _lib.M3T_EINVAL
    assert lib.m3t_label_rows(None, 5, 527, bad.data_ptr(), 3, out.data_ptr(), None) == _lib.M3T_EINVAL
    assert lib.m3t_label_rows(store.label_table.data_ptr(), 5, 527, bad.data_ptr() + 4, 2, out.data_ptr(), None) == _lib.M3T_EINVAL


# ---------------------------------------------------------------------------------------------- through the model and the trainer
def _hp(tree, **kw):
    from models.audioset_model import AudioSet
    ns = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.dataset_path, ns.window, ns.batch_size, ns.checkpoint_path = tree, 4, 2, None
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def test_validation_step_on_a_feed_batch_equals_the_hand_built_batch(tree, clips):
    from m3t import audio
    from models.audioset_model import AudioSet
    torch.manual_seed(6)
    model = AudioSet(_hp(tree)).cuda().eval()
    feed = model.val_dataloader()
    labels = F.golden()["val.labels"]
    plans = feed.plan_epoch(0)
    for b, batch in enumerate(feed):
        items = plans[b].items
        hand = {"audio": audio.ingest([clips["val"][i] for i in items], None, 4),
                "label": torch.from_numpy(labels[items].astype(np.float32)).cuda()}
        got, want = model.validation_step(batch, b), model.validation_step(hand, b)
        assert sorted(got) == ["correct", "val_loss"]
        assert torch.equal(got["val_loss"], want["val_loss"]) and torch.equal(got["correct"], want["correct"])
        assert bool(torch.isfinite(got["val_loss"]))
    assert b == 1


def test_two_trainer_steps_from_train_dataloader(tree):
    from m3t import ops
    from m3t.trainer import Trainer
    from models.audioset_model import AudioSet
    torch.manual_seed(7)
    F.seed(F.config("train"))
    model = AudioSet(_hp(tree, learning_rate=1e-3, scheduler="none")).cuda()
    tr = Trainer.from_hparams(model, model.hparams, gradient_clip_val=1.0)
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    stock = dict(ops.STOCK_FALLBACKS)
    losses = []
    for batch in model.train_dataloader():
        losses.append(float(tr.step(batch)["loss"].detach()))
        if len(losses) == 2:
            break
    assert len(losses) == 2 and all(np.isfinite(l) for l in losses), losses
    after = model.state_dict()
    assert any(not torch.equal(v, after[k]) for k, v in before.items())
    assert dict(ops.STOCK_FALLBACKS) == stock


# ---------------------------------------------------------------------------------------------- the other forms keep their bits
def test_the_list_and_the_rows_forms_agree_with_the_store_form_and_are_left_alone_by_it():
    """The ragged batch of tests/test_gpu_audio_ingest.py (its table, its signals): the list form, the [N, S] form with lengths and the store
    form over one flat buffer give the same bits, and the two older forms give those bits again after the store form has run (the
    constants and the workspace it shares with them are left as they were).  Against the float64 oracle the bound is TOL_DB as there."""
    from m3t import audio
    rows = [(15.0, 6000, 0), (23.976, 2669, 0), (30.0, 1500, 3), (30.0, 9000, 3111)]
    sig = [A.signal(n, 10 + i) for i, (_, n, _) in enumerate(rows)]
    draws = [A.draw(fps, start, 4) for fps, _, start in rows]
    S = max(len(c) for c in sig)
    packed = np.full((4, S), 7.0, np.float32)
    for n, c in enumerate(sig):
        packed[n, :len(c)] = c
    lens = [len(c) for c in sig]
    for pad_mode in ("constant", "reflect"):
        listed = audio.ingest(sig, draws, 4, pad_mode=pad_mode)
        in_rows = audio.ingest(torch.from_numpy(packed), draws, 4, lengths=lens, pad_mode=pad_mode)
        assert A.max_err(listed, A.reference(sig, draws, 4, pad_mode), "list form/" + pad_mode) < A.TOL_DB
        # the store form: the clips in another order in one device buffer, a gap between them
        order = [2, 0, 3, 1]
        flat, offs = [], {}
        for i in order:
            flat.append(np.full(3, 9.0, np.float32))
            offs[i] = sum(len(x) for x in flat)
            flat.append(sig[i])
        buf = torch.from_numpy(np.concatenate(flat)).cuda()
        stored = audio.ingest(buf, draws, 4, lengths=lens, offsets=[offs[i] for i in range(4)], pad_mode=pad_mode)
        assert torch.equal(listed, in_rows) and torch.equal(listed, stored)
        assert torch.equal(audio.ingest(sig, draws, 4, pad_mode=pad_mode), listed)
        assert torch.equal(audio.ingest(packed, draws, 4, lengths=lens, pad_mode=pad_mode), listed)


# ---------------------------------------------------------------------------------------------- the driver
def test_pretrain_audioset_py_runs_an_epoch_on_the_tree(tree, tmp_path):
    ck = str(tmp_path / "ck")
    res = subprocess.run([sys.executable, os.path.join(PKG, "pretrain_audioset.py"), "--dataset_path", tree, "--window", "4", "--batch_size", "2",
                          "--max_nb_epochs", "1", "--checkpoint_path", ck, "--learning_rate", "0.001"],
                         cwd=str(tmp_path), env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "Loaded partition train: 5 samples" in res.stdout and "Loaded partition val: 3 samples" in res.stdout
    assert "epoch 0:" in res.stdout and "(improved)" in res.stdout
    best = torch.load(os.path.join(ck, "best.ckpt"), map_location="cpu")
    assert any(k.startswith("audio.gru.") for k in best["state_dict"]) and any(k.startswith("audio.fc.3.") for k in best["state_dict"])
