"""Host side of the GPU-resident track store (m3t/dataset.py): the window plans against hand-worked cases, brute force and a direct
`random` transcript, plan()'s ValueErrors, and the tables of the collate fixture.  No device."""
import random

import numpy as np
import pytest
import torch

import collate_ref as R
from m3t import dataset as D
from m3t._lib import M3THipError


def test_one_runs():
    assert D.one_runs([0, 1, 1, 0, 1]).tolist() == [[1, 3], [4, 5]]
    assert D.one_runs([1, 1]).tolist() == [[0, 2]]
    assert D.one_runs(np.zeros(4, bool)).shape == (0, 2)
    assert D.one_runs(np.array([True, False, True, True])).tolist() == [[0, 1], [2, 4]]


def test_available_windows_hand_worked():
    img = [1, 1, 1, 0, 1, 1, 1, 1]
    lab = [1, 1, 1, 1, 1, 1, 0, 1]
    assert D.available_windows(img, lab, 2, "visual") == [0, 1, 4]               # runs [0,3) [4,6) [7,8)
    assert D.available_windows(img, lab, 2, "audiovisual") == [0, 1, 4]
    assert D.available_windows(None, lab, 2, "audio") == [0, 1, 2, 3, 4]         # runs [0,6) [7,8): images do not count
    assert D.available_windows(None, [1, 0, 1], 2, "audio") == []                # the reference asserts for the visual modalities only
    with pytest.raises(ValueError):
        D.available_windows([1, 0, 1], [1, 1, 1], 2, "visual")


@pytest.mark.parametrize("window", [1, 3, 8])
def test_available_windows_brute_force(window):
    rs = np.random.RandomState(window)
    img, lab = rs.uniform(size=200) < 0.9, rs.uniform(size=200) < 0.9
    ok = img & lab
    want = [s for s in range(200 - window + 1) if ok[s:s + window].all()]
    assert D.available_windows(img, lab, window, "visual") == want
    want_a = [s for s in range(200 - window + 1) if lab[s:s + window].all()]
    assert D.available_windows(img, lab, window, "audio") == want_a


def test_has_label():
    va = np.array([[0.5, -1.0], [1.0, 1.0], [-5.0, -5.0], [0.2, 1.5]], np.float32)
    assert D.has_label(va).tolist() == [True, True, False, False]


def test_noisy_balanced_windows_visual_hand_worked():
    va = np.array([[0.5, 0], [-0.9, 0], [-0.9, 0], [2.0, 0.3], [0.1, 0]], np.float32)
    keep = va.copy()
    # window 4: both starts miss one label of four (25 %: allowed) and have a negative mean valence once row 3 is zeroed: each twice
    starts, out = D.noisy_balanced_windows(va, np.ones(5, bool), 4, "visual")
    assert starts == [0, 0, 1, 1]
    assert np.array_equal(va, keep) and out is not va                            # returned, not mutated
    assert out[3].tolist() == [0.0, 0.0] and np.array_equal(out[[0, 1, 2, 4]], keep[[0, 1, 2, 4]])
    # start 0 also misses two images of four: dropped
    starts, _ = D.noisy_balanced_windows(va, [0, 0, 1, 1, 1], 4, "audiovisual")
    assert starts == [1, 1]
    va[:, 0] = [0.5, 0.9, 0.9, 2.0, 0.1]                                         # positive means: once each
    assert D.noisy_balanced_windows(va, np.ones(5, bool), 4, "visual")[0] == [0, 1]
    with pytest.raises(ValueError):
        D.noisy_balanced_windows(va, np.zeros(5, bool), 4, "visual")


def test_noisy_balanced_windows_audio_hand_worked():
    va = np.zeros((10, 2), np.float32)
    va[:, 0] = [0.5, 0.5, 0.1, 0.1, 0.1, 0.1, -7.0, -0.5, -0.3, 0.2]
    keep = va.copy()
    # runs [0,6) [7,10), window 2: starts 0..4, 7, 8.  The reference pairs start k with run k: (0, mean va[0:2]) = 0.5, (1, mean va[7:9]) = -0.4;
    # the pair with a negative score repeats ITS start, 1
    starts, out = D.noisy_balanced_windows(va, None, 2, "audio")
    assert starts == [0, 1, 2, 3, 4, 7, 8, 1]
    assert np.array_equal(out, keep)                                             # the audio branch leaves the labels alone


def test_eval_items():
    items = D.eval_items([23, 17, 9, 16], 8, 2)
    want = []
    for v, n in enumerate([23, 17, 9, 16]):
        for s in range(0, n, 4):
            want.append((v, s, min(8, n - s)))
    assert items == want and len(items) == 6 + 5 + 3 + 4
    assert (1, 16, 1) in items and (0, 20, 3) in items and items[0] == (0, 0, 8)
    assert D.eval_items([5], 8) == [(0, 0, 5)]
    assert D.eval_items([16], 8) == [(0, 0, 8), (0, 8, 8)]
    with pytest.raises(ValueError):
        D.eval_items([5], 2, 4)


@pytest.mark.parametrize("seed", [0, 7])
def test_train_items_follow_the_references_draws(seed):
    avail = [list(range(3, 40)), [0], list(range(100, 110)), [5, 5, 6]]
    want = R.train_transcript(4, 5, avail, seed)
    got = D.train_items(4, 5, avail, random.Random(seed))
    assert got == want and len(got) == 20 and sorted(v for v, _ in got) == sorted(list(range(4)) * 5)
    random.seed(seed)                                                            # the module itself works as rng, like the reference
    assert D.train_items(4, 5, avail, random) == want


def _meta():
    return D.layout(R.fixture(), "val")[0]


def test_plan_tables_and_names():
    meta = _meta()
    tab = D.plan(meta, [("B", 14, 3), (0, 3), (3, 8, 8), ("C", 8, 1)], 8, "val")
    assert tab.dtype == np.int32 and tab.tolist() == [[1, 14, 3], [0, 3, 8], [3, 8, 8], [2, 8, 1]]
    assert D.plan(meta, [], 8, "val").shape == (0, 3)
    nb = [m["nb_frames"] for m in meta]
    assert nb == [23, 17, 9, 16]
    items = D.eval_items(nb, 8, 2)
    # B's feature track has 15 rows for 17 frames: the window at 16 starts past it, as np.pad 'edge' of the reference's empty slice
    with pytest.raises(ValueError, match="se track"):
        D.plan(meta, items, 8, "val")
    ok = [it for it in items if it != (1, 16, 1)]
    assert D.plan(meta, ok, 8, "val").tolist() == [list(it) for it in ok]


@pytest.mark.parametrize("item,split,what", [
    (("B", 15, 1), "val", "se track"),                   # start >= Lse (15 rows)
    (("A", 23, 1), "test", "se track"),
    (("A", 16, 8), "val", "va labels"),                  # start + track_len > Lva = 23
    (("D", 9, 8), "train", "va labels"),
    (("A", 0, 0), "val", "track_len"),
    (("A", 0, 9), "val", "track_len"),
    (("A", -1, 4), "val", "negative"),
    (("E", 0, 4), "val", "unknown video"),
    ((4, 0, 4), "val", "unknown video"),
    ((-1, 0, 4), "val", "unknown video"),
    (("A", 0, 4, 4), "val", "expected"),
])
def test_plan_value_errors(item, split, what):
    with pytest.raises(ValueError, match=what):
        D.plan(_meta(), [("A", 0, 8), item], 8, split)


def test_plan_checks_expr_labels_and_skips_labels_on_test():
    vids = R.fixture()
    vids["D"]["expr"] = vids["D"]["expr"][:12]           # expression labels shorter than the valence / arousal track
    meta = D.layout(vids, "val")[0]
    D.plan(meta, [("D", 4, 8)], 8, "val")
    with pytest.raises(ValueError, match="expr labels"):
        D.plan(meta, [("D", 5, 8)], 8, "val")
    D.plan(D.layout(vids, "test")[0], [("D", 5, 8), ("A", 20, 8)], 8, "test")      # no labels, nothing to run past
    with pytest.raises(ValueError):
        D.plan(meta, [("A", 0, 4)], 0, "val")


def test_layout_tables_of_the_fixture():
    vids = R.fixture()
    meta, table, flat = D.layout(vids, "val")
    assert table.dtype == np.int64 and table.shape == (4, D.TABLE_COLS)
    assert table.tolist() == [
        # se       au       mel       va       expr    flags
        [0, 23,   0, 23,   0, 71,    0, 23,   0, 23,   3, 0],
        [23, 15,  23, 17,  71, 40,   23, 17,  0, 0,    2, 0],         # B: no expr labels
        [38, 9,   40, 9,   111, 9,   40, 9,   23, 9,   1, 0],         # C: 12 fps, audio invalid
        [47, 16,  49, 16,  120, 50,  49, 16,  32, 16,  3, 0]]
    assert {k: (a.shape, a.dtype) for k, a in flat.items()} == {
        "se": ((63, 512), np.float32), "au": ((65, 268), np.float32), "mel": ((170, 40), np.float32), "va": ((65, 2), np.float32),
        "expr": ((48,), np.int64)}
    assert flat["se"][23:38].tobytes() == vids["B"]["se"].tobytes()              # float32 exactly as given
    assert np.array_equal(flat["expr"][23:32], vids["C"]["expr"])
    assert [(m["name"], m["se"], m["au"], m["va"], m["expr"]) for m in meta] == [
        ("A", 23, 23, 23, 23), ("B", 15, 17, 17, None), ("C", 9, 9, 9, 9), ("D", 16, 16, 16, 16)]
    # the test split stores no labels
    _, table_t, flat_t = D.layout(vids, "test")
    assert sorted(flat_t) == ["au", "mel", "se"] and not table_t[:, 6:10].any() and table_t[:, 10].tolist() == [2, 2, 0, 2]
    # a low-fps video may come without a mel track; any other may not
    del vids["C"]["mel"]
    assert D.layout(vids, "val")[1][2, 4:6].tolist() == [0, 0]
    del vids["D"]["mel"]
    with pytest.raises(ValueError, match="mel"):
        D.layout(vids, "val")


def test_layout_value_errors():
    with pytest.raises(ValueError):
        D.layout({}, "val")
    for kind, bad in (("se", lambda a: a.astype(np.float64)), ("se", lambda a: a[:, :100]), ("au", lambda a: a[:, :200]),
                      ("va", lambda a: a[:, :1]), ("expr", lambda a: a.astype(np.float32)), ("se", lambda a: a[0])):
        vids = R.fixture()
        vids["D"][kind] = bad(vids["D"][kind])
        with pytest.raises(ValueError):
            D.layout(vids, "val")
    vids = R.fixture()
    del vids["B"]["va"]
    with pytest.raises(ValueError, match="va"):
        D.layout(vids, "val")
    D.layout(vids, "test")
    del vids["C"]["au"]                                                          # a feature kind is stored for every video or none
    with pytest.raises(ValueError, match="au"):
        D.layout(vids, "test")


def test_restatement_edge_rules():
    """the numpy restatement itself on hand-worked values: what the GPU tests compare against"""
    vids = R.fixture()
    b = R.batch(vids, [("B", 12, 5), ("A", 20, 3), ("C", 8, 1)], 8, "val")
    assert [b[k].dtype for k in R.DTYPES] == list(R.DTYPES.values())
    assert b["se_features"].shape == (3, 512, 8) and b["au_features"].shape == (3, 256, 8) and b["audio"].shape == (3, 8, 200)
    se_b = vids["B"]["se"]
    assert np.array_equal(b["se_features"][0].T, se_b[[12, 13, 14, 14, 14, 14, 14, 14]])       # 15 rows: pads from its own last row
    assert np.array_equal(b["au_features"][0].T, vids["B"]["au"][[12, 13, 14, 15, 16, 16, 16, 16], :256])
    mel = vids["B"]["mel"]                                                      # 40 rows: frame 12 reads 36..40, frame 13 only row 39, 14+ nothing
    assert np.array_equal(b["audio"][0, 0], np.concatenate([mel[36:40].reshape(-1), np.zeros(40, np.float32)]))
    assert np.array_equal(b["audio"][0, 1, :40], mel[39]) and not b["audio"][0, 1, 40:].any() and not b["audio"][0, 2:].any()
    assert not b["audio"][2].any()                                              # 12 fps
    assert not b["expr_valid"][0].any() and not b["class_expr"][0].any()       # no expr labels
    e = vids["A"]["expr"][[20, 21, 22, 22, 22, 22, 22, 22]]
    assert e[2] == -1 and np.array_equal(b["class_expr"][1], np.clip(e, 0, 6)) and np.array_equal(b["expr_valid"][1], e >= 0)
    assert np.array_equal(b["label_valence"][1], vids["A"]["va"][[20, 21, 22, 22, 22, 22, 22, 22], 0])
    assert b["start"].tolist() == [12, 20, 8] and b["length"].tolist() == [5, 3, 1] and b["vid_name"] == ["B", "A", "C"]
    assert R.batch(vids, [("A", 4, 2)], 4, "val")["label_valence"][0, 0] == -5.0            # out-of-range labels pass through
    assert sorted(R.batch(vids, [("A", 4, 2)], 4, "test")) == ["au_features", "audio", "length", "se_features", "start", "vid_name"]


def test_track_store_needs_the_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(M3THipError):
        D.TrackStore(R.fixture(), 8, "val")
    with pytest.raises(ValueError):                                              # host validation comes first
        D.TrackStore({}, 8, "val")
