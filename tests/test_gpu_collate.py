"""The GPU-resident track store on the MI355X (m3t.dataset.TrackStore over csrc/collate.hip, m3t_window_collate) against the numpy
restatement of the reference loader's __getitem__ + default collate (tests/collate_ref.py).  Every output is a copy, so every comparison is
bit for bit, in dtype and shape too.  The fixture: four videos, n_mels 40 (collate_ref.fixture); each store is built once per module."""
import argparse
import functools
import random

import numpy as np
import pytest
import torch

import collate_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.bool_): torch.bool}


@functools.lru_cache(maxsize=None)
def _videos(se_width=512, au_width=268, au=True, se=True):
    return R.fixture(se_width=se_width, au_width=au_width, au=au, se=se)


@functools.lru_cache(maxsize=None)
def _store(window, split, se_dim=512, au_dim=256, se_width=512, au_width=268, au=True, se=True):
    from m3t.dataset import TrackStore
    return TrackStore(_videos(se_width, au_width, au, se), window, split, se_dim=se_dim, au_dim=au_dim)


def _named(store, items):
    """(index | name, start[, track_len]) -> the restatement's (name, start, track_len)"""
    return [(it[0] if isinstance(it[0], str) else store.names[it[0]], it[1], it[2] if len(it) == 3 else store.window) for it in items]


def _same_bits(got, ref, what):
    assert isinstance(got, torch.Tensor) and got.dtype == TORCH[ref.dtype] and tuple(got.shape) == ref.shape, (what, got.dtype, tuple(got.shape), ref.shape)
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(ref).tobytes(), what


def _check(store, items, videos, **kw):
    got = store.collate(items)
    ref = R.batch(videos, _named(store, items), store.window, store.split, se_dim=store.se_dim, au_dim=store.au_dim, **kw)
    assert sorted(k for k in got if k != "video_frame_idx") == sorted(ref), (sorted(got), sorted(ref))
    assert got["vid_name"] == ref["vid_name"]
    for k in ("start", "length"):
        assert not got[k].is_cuda
        _same_bits(got[k], ref[k], k)
    for k in ref:
        if k in R.DTYPES:
            assert got[k].is_cuda and got[k].is_contiguous() and ref[k].dtype == R.DTYPES[k]
            _same_bits(got[k], ref[k], k)
    return got, ref


def _eval_items(store, skip=()):
    from m3t.dataset import eval_items
    return [it for it in eval_items([m["nb_frames"] for m in store.meta], store.window, 2) if it not in skip]


def test_eval_windows_down_to_one_frame():
    """window 8, inv_test_stride 2: tails of 7, 5, 3 and 1 frames.  B's feature track has 15 rows for 17 frames: its window at 16 is a
    ValueError on a store with feature tracks, as in the reference (np.pad 'edge' of an empty slice), and collates on the audio store"""
    store = _store(8, "val")
    items = _eval_items(store)
    assert len(items) == 18 and (1, 16, 1) in items and (2, 8, 1) in items
    with pytest.raises(ValueError, match="se track"):
        store.collate(items)
    got, ref = _check(store, [it for it in items if it != (1, 16, 1)], _videos())
    assert got["se_features"].shape == (17, 512, 8) and got["au_features"].shape == (17, 256, 8) and got["audio"].shape == (17, 8, 200)
    assert got["length"].tolist()[-4:] == [8, 8, 8, 4] and 1 in got["length"].tolist()
    assert not ref["audio"][12].any() and ref["audio"][0].any()                 # C: 12 fps
    assert not ref["expr_valid"].all() and ref["expr_valid"].any() and ref["class_expr"].max() == 6
    audio_store = _store(8, "val", au=False, se=False)
    got, _ = _check(audio_store, items, _videos(au=False, se=False))
    assert sorted(got) == ["audio", "class_expr", "expr_valid", "label_arousal", "label_valence", "length", "start", "vid_name", "video_frame_idx"]
    assert got["length"].tolist()[10] == 1 and got["vid_name"][10] == "B"


@pytest.mark.parametrize("N", [1, 19])
def test_train_windows(N):
    """track_len = window, several windows of one video in a batch, (video, start) pairs; N = 1 and N = 19"""
    from m3t.dataset import available_windows, train_items
    store = _store(8, "train")
    vids = _videos()
    avail = [available_windows(None, np.ones(v["nb_frames"], bool), 8, "audio") for v in vids.values()]
    items = train_items(4, 5, avail, random.Random(N))[:N]
    if N == 19:
        items[-1] = (1, 9)                                                       # B's 15 feature rows end inside this full window
    assert len(items) == N and all(len(it) == 2 for it in items)
    got, _ = _check(store, items, vids)
    assert got["length"].tolist() == [8] * N
    if N == 19:
        assert max(got["vid_name"].count(n) for n in "ABCD") >= 2
        assert any(v == 1 and s > 7 for v, s in items)                           # B's short feature track pads inside a full window


def test_window_5_and_names():
    store = _store(5, "val")
    items = [("A", 18, 5), ("B", 14, 3), ("C", 8, 1), ("D", 0, 5), ("A", 0, 5), ("B", 10, 5), ("D", 11, 5)]
    _check(store, items, _videos())


def test_ragged_time_tile_window_37():
    """one 80-frame video at window 37: a second, ragged tile along T; se_dim 512 = four channel tiles"""
    from m3t.dataset import TrackStore, eval_items
    rs = np.random.RandomState(37)
    vid = {"nb_frames": 80, "fps": 30.0, "se": rs.standard_normal((80, 512)).astype(np.float32),
           "au": rs.standard_normal((80, 268)).astype(np.float32), "mel": rs.standard_normal((200, 40)).astype(np.float32),
           "va": rs.uniform(-1, 1, (80, 2)).astype(np.float32), "expr": rs.randint(-1, 9, 80).astype(np.int64)}
    store = TrackStore({"long": vid}, 37, "val")
    items = eval_items([80], 37) + [(0, 43, 37), (0, 79, 1)]
    assert items[:3] == [(0, 0, 37), (0, 37, 37), (0, 74, 6)]
    _check(store, items, {"long": vid})


@pytest.mark.parametrize("se_width,se_dim,au_width,au_dim", [(24, 24, 11, 6), (30, 24, 268, 256), (512, 24, 12, 6)])
def test_narrow_and_cut_feature_rows(se_width, se_dim, au_width, au_dim):
    """se_dim 24 of rows 24, 30 (no 16-byte rows) and 512 wide; au 268 cut to 256 and 11 (and 12) cut to 6: column counts below the
    row stride and no multiple of the tile"""
    store = _store(8, "val", se_dim, au_dim, se_width, au_width)
    vids = _videos(se_width, au_width)
    got, _ = _check(store, _eval_items(store, skip=[(1, 16, 1)]), vids)
    assert got["se_features"].shape == (17, se_dim, 8) and got["au_features"].shape == (17, au_dim, 8)


def test_mel_rows_that_are_no_multiple_of_16_bytes():
    """n_mels 10: the audio rows are gathered by the float (the 16-byte cells need n_mels % 4 == 0)"""
    from m3t.dataset import TrackStore
    vids = R.fixture(n_mels=10, au=False, se=False)
    store = TrackStore(vids, 8, "val")
    got, _ = _check(store, _eval_items(store), vids, n_mels=10)
    assert got["audio"].shape == (18, 8, 50)


def test_test_split_has_no_labels():
    store = _store(8, "test")
    got, _ = _check(store, _eval_items(store, skip=[(1, 16, 1)]), _videos())
    assert sorted(k for k in got) == ["au_features", "audio", "length", "se_features", "start", "vid_name", "video_frame_idx"]


def test_store_without_au():
    store = _store(8, "val", au=False)
    got, _ = _check(store, _eval_items(store, skip=[(1, 16, 1)]), _videos(au=False))
    assert "au_features" not in got and "se_features" in got


def test_audio_equals_load_audio_batch():
    from m3t import audio
    store = _store(8, "val", au=False, se=False)
    vids = _videos(au=False, se=False)
    items = _eval_items(store)
    got = store.collate(items)["audio"]
    names = list(vids)
    want = audio.load_audio_batch([vids[names[v]]["mel"] for v, _, _ in items], [s for _, s, _ in items], [t for _, _, t in items], 8,
                                  valid=[vids[names[v]]["fps"] >= 15 for v, _, _ in items])
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def test_frame_index_rows_nbytes_and_batches():
    from m3t import video
    store = _store(8, "val")
    vids = _videos()
    assert store.nbytes == sum(a.nbytes for v in vids.values() for k, a in v.items() if k in ("se", "au", "mel", "va", "expr")) + 4 * 12 * 8
    items = _eval_items(store, skip=[(1, 16, 1)])
    batches = list(store.batches(items, 4))
    assert [len(b["vid_name"]) for b in batches] == [4, 4, 4, 4, 1]
    whole = store.collate(items)
    for k in ("se_features", "audio", "class_expr", "expr_valid", "label_arousal"):
        assert torch.equal(torch.cat([b[k] for b in batches]), whole[k]), k
    fidx = whole["video_frame_idx"]
    assert fidx.dtype == torch.int32 and tuple(fidx.shape) == (17, 8) and not fidx.is_cuda
    for n, (v, s, tl) in enumerate(items):
        present = vids[store.names[v]]["has_image"][s:s + tl]
        assert np.array_equal(fidx[n].numpy(), video.frame_index(present, 0, tl, 8))
    assert store.collate([])["vid_name"] == []


def test_collate_runs_on_the_current_stream():
    store = _store(8, "val")
    items = _eval_items(store, skip=[(1, 16, 1)])
    want = store.collate(items)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = store.collate(items)
    st.synchronize()
    for k in R.DTYPES:
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------- through the model and the trainer
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _uploaded(ref):
    """the restatement's batch as the DataLoader hands it over and the training loop uploads it"""
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if k in R.DTYPES else (torch.from_numpy(v) if isinstance(v, np.ndarray) else v))
            for k, v in ref.items()}


def test_audio_model_fed_by_the_store(tmp_path, monkeypatch):
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    store = _store(8, "val", au=False, se=False)
    vids = _videos(au=False, se=False)
    items = _eval_items(store)
    host = [_uploaded(R.batch(vids, _named(store, items[i:i + 4]), 8, "val")) for i in range(0, len(items), 4)]
    torch.manual_seed(5)
    model = AffWild2VA(_hp(modality="audio", loss="ccc_mtl", window=8, test_on_val=True)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    want = tr.evaluate(host)
    want_file = torch.load("predictions_val.pt")
    got = tr.evaluate(store.batches(items, 4))
    got_file = torch.load("predictions_val.pt")
    assert got == want and set(got["log"]) >= {"val_ccc_v", "val_ccc_a", "val_loss"}
    assert list(got_file) == list(want_file)
    for k in want_file:
        assert list(got_file[k]) == list(want_file[k]) == ["A", "B", "C", "D"]
        for vid in want_file[k]:
            assert torch.equal(got_file[k][vid], want_file[k][vid]), (k, vid)
    # one training step: the same loss bits from the two feeds
    model.train()
    torch.manual_seed(6)
    a = model.training_step(host[0], 0)["loss"]
    torch.manual_seed(6)
    b = model.training_step(store.collate(items[:4]), 0)["loss"]
    assert np.isfinite(float(a)) and torch.equal(a, b)
