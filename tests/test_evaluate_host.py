"""m3t.evaluate.plan_tracks -- where every window of an evaluation epoch goes -- against the reference's own
validation_end / test_end outputs (golden: tests/golden/stitch.npz).  Index arithmetic only: CPU, no GPU."""
import numpy as np
import pytest

from conftest import load_golden
from m3t.evaluate import NO_HALVING, plan_tracks

MODES = (("test", True, "valence_pred"), ("val_cat", False, "valence_gt"), ("val_overlap", True, "valence_gt"))


def _windows(g, mode):
    n = int(g["%s.n_items" % mode])
    names = [str(g["%s.in.%d.name" % (mode, i)]) for i in range(n)]
    starts = [int(g["%s.in.%d.start" % (mode, i)]) for i in range(n)]
    lengths = [int(g["%s.in.%d.v_pred" % (mode, i)].shape[0]) for i in range(n)]
    return names, starts, lengths


def _restated(names, starts, lengths, overlap):
    """the plan, said again: per video in first-seen order, (destination, length, row) sorted by start"""
    out = {}
    for v in dict.fromkeys(names):
        rows = sorted((r for r in range(len(names)) if names[r] == v), key=lambda r: starts[r])
        dst, run = [], 0
        for r in rows:
            dst.append(starts[r] if overlap else run)
            run += lengths[r]
        out[v] = [(d, lengths[r], r) for d, r in zip(dst, rows)]
    return out


@pytest.mark.parametrize("mode,overlap,key", MODES)
def test_plan_matches_the_fixture(mode, overlap, key):
    g = load_golden("stitch")
    window = int(g["window"])
    names, starts, lengths = _windows(g, mode)
    plan = plan_tracks(names, starts, lengths, window, overlap)
    assert plan.names == list(dict.fromkeys(names))
    want = {k.split(".")[-1]: int(v.shape[0]) for k, v in g.items() if k.startswith("%s.out.%s." % (mode, key))}
    assert dict(zip(plan.names, plan.nframes.tolist())) == want
    assert sorted(want.values()) == ([16, 25, 37] if overlap else [28, 46, 70])
    assert plan.frame_off.tolist() == [0] + np.cumsum(plan.nframes).tolist()
    assert plan.halve_from == (window // 2 if overlap else NO_HALVING) and NO_HALVING > int(plan.frame_off[-1])
    ref = _restated(names, starts, lengths, overlap)
    assert plan.seg_off.tolist() == [0] + np.cumsum([len(ref[v]) for v in plan.names]).tolist()
    for i, v in enumerate(plan.names):
        a, b = int(plan.seg_off[i]), int(plan.seg_off[i + 1])
        got = list(zip(plan.seg_dst[a:b].tolist(), plan.seg_len[a:b].tolist(), plan.seg_row[a:b].tolist()))
        assert got == ref[v], (mode, v)
    assert sorted(plan.seg_row.tolist()) == list(range(len(names)))          # every window placed exactly once
    for arr in (plan.frame_off, plan.seg_off, plan.seg_dst, plan.seg_len, plan.seg_row):
        assert arr.dtype == np.int64


def test_concatenation_ignores_overlapping_starts():
    """validation_end's torch.cat puts the windows of a video one after the other even where their frames overlap"""
    plan = plan_tracks(["a", "a", "b", "a"], [4, 0, 0, 8], [6, 8, 3, 2], 8, False)
    assert plan.names == ["a", "b"] and plan.nframes.tolist() == [16, 3]
    assert plan.seg_dst.tolist() == [0, 8, 14, 0] and plan.seg_row.tolist() == [1, 0, 3, 2]
    over = plan_tracks(["a", "a", "b", "a"], [4, 0, 0, 8], [6, 8, 3, 2], 8, True)
    assert over.nframes.tolist() == [10, 3] and over.seg_dst.tolist() == [0, 4, 8, 0] and over.halve_from == 4


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("names,starts,lengths,what", [
    (["a", "b", "a"], [4, 4, 4], [8, 8, 8], "start at frame 4"),          # duplicate start within a video (b's 4 is fine)
    (["a", "a"], [0, 4], [8, 0], "length 0"),
    (["a", "a"], [0, 4], [9, 8], "length 9"),
    (["a", "a"], [-4, 4], [8, 8], "negative start"),
])
def test_plan_refuses_bad_windows(overlap, names, starts, lengths, what):
    with pytest.raises(ValueError, match=what):
        plan_tracks(names, starts, lengths, 8, overlap)


def test_same_start_in_two_videos_is_fine():
    plan = plan_tracks(["a", "b"], [0, 0], [1, 8], 8, True)
    assert plan.nframes.tolist() == [1, 8]


def test_window_past_the_end_is_refused():
    """the reference sizes a track by its last window: an earlier window that ends after it cannot be added"""
    with pytest.raises(ValueError, match="runs past the end"):
        plan_tracks(["a", "a"], [0, 4], [8, 2], 8, True)
    assert plan_tracks(["a", "a"], [0, 4], [8, 2], 8, False).nframes.tolist() == [10]      # concatenation has no such case
