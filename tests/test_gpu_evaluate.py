"""The evaluation epoch on the device (m3t.evaluate over csrc/evaluate.hip) against the host route it stands beside:
m3t.stitch (the reference's validation_end / test_end, golden stitch.npz), postproc.smoothed_ccc_report (golden
postproc.npz), Trainer.validate, and float64 numpy for the metrics.  Tracks are compared with tolerance 0: the kernels
do the same fp32 additions in the same order as the host code."""
import argparse
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("v_pred", "a_pred", "v_gt", "a_gt")
METRICS = ("val_ccc_v", "val_ccc_a", "val_mse_v", "val_mse_a", "val_loss")


# ---------------------------------------------------------------------------------------------- the two routes on the same windows
def _feed(windows, T, bs, with_gt, C=2, device_meta=False):
    """windows: dicts {name, start, v_pred, a_pred (, v_gt, a_gt)} of 1-D float32 arrays -> (batches for Evaluator.add as
    (y_hat, batch), outputs for m3t.stitch).  Everything past a window's length is NaN, in predictions and labels alike, and
    so is every channel of y_hat but the last two."""
    batches, outputs = [], []
    for i in range(0, len(windows), bs):
        chunk = windows[i:i + bs]
        N = len(chunk)
        y = np.full((N, T, C), np.nan, np.float32)
        lab = np.full((2, N, T), np.nan, np.float32)
        for n, w in enumerate(chunk):
            L = len(w["v_pred"])
            y[n, :L, C - 2], y[n, :L, C - 1] = w["v_pred"], w["a_pred"]
            if with_gt:
                lab[0, n, :L], lab[1, n, :L] = w["v_gt"], w["a_gt"]
        meta = (lambda a: torch.tensor(a, device=DEV)) if device_meta else torch.tensor
        batch = {"vid_name": [w["name"] for w in chunk], "start": meta([w["start"] for w in chunk]),
                 "length": meta([len(w["v_pred"]) for w in chunk])}
        if with_gt:
            batch["label_valence"], batch["label_arousal"] = torch.from_numpy(lab[0]).to(DEV), torch.from_numpy(lab[1]).to(DEV)
        batches.append((torch.from_numpy(y).to(DEV), batch))
        out = {"vid_names": batch["vid_name"], "start_frames": torch.tensor([w["start"] for w in chunk])}
        for k in KEYS[:4 if with_gt else 2]:
            out[k] = [torch.from_numpy(np.asarray(w[k], np.float32)) for w in chunk]
        outputs.append(out)
    return batches, outputs


def _run(batches, window, overlap, with_gt):
    from m3t.evaluate import Evaluator
    ev = Evaluator(window, overlap, with_gt)
    for y, b in batches:
        ev.add(y, b)
    return ev.finish()


def _host(outputs, window, overlap, with_gt):
    from m3t import stitch
    if not with_gt:
        pv, pa = stitch.stitch_test(outputs, window)
        return {"valence_pred": pv, "arousal_pred": pa}
    gv, ga, pv, pa = stitch.stitch_val(outputs, window, overlap)
    return {"valence_gt": gv, "arousal_gt": ga, "valence_pred": pv, "arousal_pred": pa}


def _same(a, b):
    """bit-for-bit as numbers (NaN in the same places: a NaN label inside a window stays in the label track on both routes)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=4096.0), torch.nan_to_num(b, nan=4096.0))


def _assert_dicts_equal(got, want, what=""):
    assert list(got) == list(want), what
    for k in want:
        assert list(got[k]) == list(want[k]), (what, k)                  # the same videos in the same (first-seen) order
        for vid in want[k]:
            assert not got[k][vid].is_cuda and _same(got[k][vid], want[k][vid]), (what, k, vid)


def _check_against_stitch(windows, T, bs, overlap, with_gt, window=None, **kw):
    window = T if window is None else window
    batches, outputs = _feed(windows, T, bs, with_gt, **kw)
    res = _run(batches, window, overlap, with_gt)
    _assert_dicts_equal(res.to_dicts(), _host(outputs, window, overlap, with_gt))
    return res, outputs


def _slide(name, nframes, T, stride, rs, with_gt=True):
    """a video of nframes frames as sliding windows over one underlying track per quantity (the last ones are short)"""
    full = {k: rs.uniform(-1, 1, nframes).astype(np.float32) for k in KEYS[:4 if with_gt else 2]}
    wins = []
    for s in range(0, nframes, stride):
        w = {"name": name, "start": s}
        w.update({k: v[s:s + T].copy() for k, v in full.items()})
        wins.append(w)
    return wins


def _shuffled(wins, rs):
    return [wins[i] for i in rs.permutation(len(wins))]


# ---------------------------------------------------------------------------------------------- 1. the reference's fixture
def _fixture_windows(g, mode):
    wins = []
    for i in range(int(g["%s.n_items" % mode])):
        w = {"name": str(g["%s.in.%d.name" % (mode, i)]), "start": int(g["%s.in.%d.start" % (mode, i)])}
        w.update({k: g["%s.in.%d.%s" % (mode, i, k)] for k in KEYS if "%s.in.%d.%s" % (mode, i, k) in g})
        wins.append(w)
    return wins


@pytest.mark.parametrize("mode,overlap,with_gt", [("test", True, False), ("val_cat", False, True), ("val_overlap", True, True)])
def test_fixture_parity(mode, overlap, with_gt):
    g = load_golden("stitch")
    window = int(g["window"])
    wins = _fixture_windows(g, mode)
    assert len(wins) % 4 == 1                                             # the last batch holds one window
    res, _ = _check_against_stitch(wins, window, 4, overlap, with_gt)
    got = res.to_dicts()
    for key in got:
        ref = {k.split(".")[-1]: v for k, v in g.items() if k.startswith("%s.out.%s." % (mode, key))}
        assert sorted(got[key]) == sorted(ref)
        for vid in ref:
            np.testing.assert_allclose(got[key][vid].numpy(), ref[vid], rtol=0, atol=1e-7, err_msg="%s %s %s" % (mode, key, vid))
    if with_gt:
        assert tuple(res.metrics) == METRICS and all(isinstance(v, float) for v in res.metrics.values())
        for k in METRICS:
            assert abs(res.metrics[k] - float(g["%s.metric.%s" % (mode, k)])) < 1e-6, (mode, k, res.metrics[k])
    else:
        assert res.metrics is None


# ---------------------------------------------------------------------------------------------- 2. channel pick
def test_channel_pick_is_the_last_two():
    g = load_golden("stitch")
    wins = _fixture_windows(g, "val_overlap")
    a, _ = _check_against_stitch(wins, 8, 4, True, True, C=2)
    b, _ = _check_against_stitch(wins, 8, 4, True, True, C=9)            # y_hat[..., 7:9]; channels 0..6 are NaN
    assert torch.equal(a.tracks, b.tracks) and a.metrics == b.metrics


# ---------------------------------------------------------------------------------------------- 3. more than two covering windows
def test_three_windows_on_one_frame():
    rs = np.random.RandomState(3)
    wins = []
    # window 7: halve_from 3; an 11-frame video at stride 3, so its third window has 5 frames (a longer one would run past
    # the end the last window sets, where the reference's `track[start:start + len] +=` fails); frames 6 and 9 are in three windows
    for start, L in ((0, 7), (3, 7), (6, 5), (9, 2)):
        w = {"name": "odd", "start": start}
        w.update({k: rs.uniform(-1, 1, L).astype(np.float32) for k in KEYS})
        wins.append(w)
    res, _ = _check_against_stitch(wins[::-1], 7, 2, True, True)         # added in reverse, two batches
    assert res.frame_off.tolist() == [0, 11]
    _check_against_stitch(wins[::-1], 7, 2, True, False)


# ---------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("overlap", [True, False])
def test_edges(overlap):
    rs = np.random.RandomState(4)
    one = [{"name": "one", "start": 0, **{k: rs.uniform(-1, 1, 1).astype(np.float32) for k in KEYS}}]
    short = [{"name": "short", "start": 0, **{k: rs.uniform(-1, 1, 3).astype(np.float32) for k in KEYS}}]     # 3 < window // 2
    res, _ = _check_against_stitch(one, 8, 1, overlap, True)
    assert res.frame_off.tolist() == [0, 1]
    res, _ = _check_against_stitch(short, 8, 1, overlap, True)
    assert torch.equal(res.tracks[0].cpu(), torch.from_numpy(short[0]["v_pred"]))                              # nothing halved
    mixed = _shuffled(one + short + _slide("m", 21, 8, 4, rs), rs)
    _check_against_stitch(mixed, 8, 1, overlap, True)                                                            # N = 1 batches


@pytest.mark.parametrize("overlap", [True, False])
def test_long_video_crosses_workgroups(overlap):
    rs = np.random.RandomState(5)
    long = _slide("long", 2400, 8, 4, rs)
    assert len(long) == 600 and len(long[-1]["v_pred"]) == 4
    wins = _shuffled(long + _slide("tail", 13, 8, 4, rs), rs)
    res, _ = _check_against_stitch(wins, 8, 64, overlap, True)
    assert int(res.frame_off[-1]) == (2400 + 13 if overlap else sum(len(w["v_pred"]) for w in wins))


# ---------------------------------------------------------------------------------------------- 5. metrics against float64
def _metric_windows(all_invalid=False):
    rs = np.random.RandomState(55)
    wins = _slide("a", 120, 8, 4, rs) + _slide("b", 100, 8, 4, rs) + _slide("c", 81, 8, 4, rs)       # 301 frames
    for w in wins:                                                                                     # labels per window
        for k in ("v_gt", "a_gt"):
            w[k] = rs.uniform(-1, 1, len(w[k])).astype(np.float32)
            w[k][rs.uniform(size=len(w[k])) < 0.1] = -5.0                                              # ~20 % of the frames lose a label
    wins[7]["v_gt"][:] = -5.0                                                                          # a whole window unannotated
    wins[7]["a_gt"][:] = -5.0
    wins[20]["a_gt"][2] = np.nan
    if all_invalid:
        for w in wins:
            w["v_gt"][:] = -5.0
    return _shuffled(wins, rs)


def _metrics_fp64(wins):
    """two passes, centred, in float64: every window's frames once (a frame in two windows counts twice), the shared mask"""
    cat = lambda k: np.concatenate([w[k] for w in wins]).astype(np.float64)
    vg, ag, vp, ap = cat("v_gt"), cat("a_gt"), cat("v_pred"), cat("a_pred")
    with np.errstate(invalid="ignore"):
        ok = (np.abs(vg) <= 1) & (np.abs(ag) <= 1)

    def ccc(p, g):
        n = p.size
        mp, mg = p.sum() / n, g.sum() / n
        cov = ((p - mp) * (g - mg)).sum() / n
        return 2 * cov / (((p - mp) ** 2).sum() / (n - 1) + ((g - mg) ** 2).sum() / (n - 1) + (mp - mg) ** 2)
    cv, ca = ccc(vp[ok], vg[ok]), ccc(ap[ok], ag[ok])
    return {"val_ccc_v": cv, "val_ccc_a": ca, "val_mse_v": ((vp[ok] - vg[ok]) ** 2).sum() / ok.sum(),
            "val_mse_a": ((ap[ok] - ag[ok]) ** 2).sum() / ok.sum(), "val_loss": 1 - 0.5 * (cv + ca)}, int(ok.sum())


def test_metrics_against_float64():
    wins = _metric_windows()
    want, n_ok = _metrics_fp64(wins)
    assert 300 < n_ok < 0.9 * sum(len(w["v_gt"]) for w in wins)
    for overlap in (True, False):
        res, _ = _check_against_stitch(wins, 8, 16, overlap, True)
        for k in METRICS:
            err = abs(res.metrics[k] - want[k])
            print("%s overlap=%s: %.17g vs %.17g (|diff| %.3e)" % (k, overlap, res.metrics[k], want[k], err))
            # raw moments in fp64: at most n * 2^-53 * max^2 ~ 5e-14 per sum (n = 468 valid frames), over a denominator >= 0.4;
            # measured on an MI355X: 8.7e-18, 1.7e-17, 0, 0, 0
            assert err <= 1e-9, (k, res.metrics[k], want[k])


def test_no_valid_label_gives_nan_metrics():
    wins = _metric_windows(all_invalid=True)
    res, _ = _check_against_stitch(wins, 8, 16, True, True)
    assert tuple(res.metrics) == METRICS and all(np.isnan(v) for v in res.metrics.values()), res.metrics


# ---------------------------------------------------------------------------------------------- 6. start / length on the device
def test_device_side_start_and_length():
    wins = _metric_windows()
    a, _ = _check_against_stitch(wins, 8, 16, True, True)
    b, _ = _check_against_stitch(wins, 8, 16, True, True, device_meta=True)
    assert torch.equal(torch.nan_to_num(a.tracks, nan=4096.0), torch.nan_to_num(b.tracks, nan=4096.0)) and a.metrics == b.metrics


# ---------------------------------------------------------------------------------------------- 7. determinism
def test_two_runs_give_the_same_bits():
    wins = _metric_windows()
    runs = []
    for _ in range(2):
        batches, _ = _feed(wins, 8, 16, True)
        res = _run(batches, 8, True, True)
        printed = []
        rep = res.smoothed_report(window=13, out=printed.append)
        runs.append((res.tracks.cpu().numpy().tobytes(), np.array([res.metrics[k] for k in METRICS]).tobytes(),
                     np.array(list(rep["ccc_v"].values()) + list(rep["ccc_a"].values()) + [rep["ccc_v_all"], rep["ccc_a_all"]]).tobytes(),
                     printed))
    assert runs[0] == runs[1]


# ---------------------------------------------------------------------------------------------- 8. smoothed report
def test_smoothed_report_matches_postproc_and_the_fixture():
    from m3t import postproc
    from m3t.evaluate import EvalResult
    g = load_golden("postproc")
    names = [str(n) for n in g["names"]]
    preds = {"valence_gt": {}, "arousal_gt": {}, "valence_pred": {}, "arousal_pred": {}}
    for v in names:
        for k in ("valence", "arousal"):
            preds[k + "_pred"][v] = torch.from_numpy(g["pred.%s.%s" % (k, v)])
            preds[k + "_gt"][v] = torch.from_numpy(g["gt.%s.%s" % (k, v)])
    res = EvalResult.from_dicts(preds)
    assert res.names == names and res.frame_off.tolist() == [0, 120, 160, 169, 470] and res.tracks.is_cuda
    _assert_dicts_equal(res.to_dicts(), preds)
    printed, printed_ref = [], []
    rep = res.smoothed_report(out=printed.append)
    ref = postproc.smoothed_ccc_report(preds, out=printed_ref.append)
    worst = 0.0
    for v in names:
        assert abs(rep["ccc_v"][v] - float(g["ccc.valence." + v])) < 1e-6, v
        assert abs(rep["ccc_a"][v] - float(g["ccc.arousal." + v])) < 1e-6, v
        worst = max(worst, abs(rep["ccc_v"][v] - ref["ccc_v"][v]), abs(rep["ccc_a"][v] - ref["ccc_a"][v]))
    assert abs(rep["ccc_v_all"] - float(g["ccc_all.valence"])) < 1e-6 and abs(rep["ccc_a_all"] - float(g["ccc_all.arousal"])) < 1e-6
    worst = max(worst, abs(rep["ccc_v_all"] - ref["ccc_v_all"]), abs(rep["ccc_a_all"] - ref["ccc_a_all"]))
    print("largest |device report - postproc report| = %.3e" % worst)
    assert worst <= 1e-12                     # same arithmetic, same reduction tree: bit-equality is the expectation (measured: 0.0)
    assert printed == printed_ref and list(rep["ccc_v"]) == list(ref["ccc_v"])
    for mode in ("median",):
        a, b = [], []
        res.smoothed_report(window=13, mode=mode, top=2, out=a.append)
        postproc.smoothed_ccc_report(preds, window=13, mode=mode, top=2, out=b.append)
        assert a == b


# ---------------------------------------------------------------------------------------------- 9. through the trainer
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _audio_batches():
    rs = np.random.RandomState(9)
    meta = [("x", 0, 8), ("y", 4, 8), ("x", 8, 8), ("z", 0, 5), ("y", 0, 8), ("x", 4, 8), ("y", 8, 5), ("x", 12, 6),
            ("x", 16, 2), ("y", 12, 1)]                                                    # 3 videos, 10 windows: batches of 4, 4, 2
    f = lambda a: torch.from_numpy(a).to(DEV)
    batches = []
    for i in range(0, len(meta), 4):
        chunk = meta[i:i + 4]
        N = len(chunk)
        lab = rs.uniform(-1, 1, (2, N, 8)).astype(np.float32)
        lab[0][rs.uniform(size=(N, 8)) < 0.15] = -5.0
        batches.append({"audio": f(rs.standard_normal((N, 8, 200)).astype(np.float32)), "label_valence": f(lab[0]),
                        "label_arousal": f(lab[1]), "vid_name": [m[0] for m in chunk],
                        "start": torch.tensor([m[1] for m in chunk]), "length": torch.tensor([m[2] for m in chunk])})
    return batches


@pytest.mark.parametrize("test_on_val", [False, True])
def test_trainer_evaluate_equals_validate(tmp_path, monkeypatch, test_on_val):
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(99)
    model = AffWild2VA(_hp(modality="audio", loss="ccc", window=8, test_on_val=test_on_val)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    batches = _audio_batches()
    ref = tr.validate(batches)
    ref_file = torch.load("predictions_val.pt")
    got = tr.evaluate(batches)
    _assert_dicts_equal(torch.load("predictions_val.pt"), ref_file, "predictions_val.pt")
    assert set(got) == set(ref) and set(got["log"]) == set(ref["log"]) == set(METRICS) and set(got["progress_bar"]) == set(ref["progress_bar"])
    assert isinstance(got["val_loss"], float) and abs(got["val_loss"] - float(ref["val_loss"])) < 1e-6
    for k in METRICS:
        assert abs(got["log"][k] - float(ref["log"][k])) < 1e-6, (k, got["log"][k], float(ref["log"][k]))
    for k in ("val_ccc_v", "val_ccc_a"):
        assert got["progress_bar"][k] == got["log"][k]
    # test=True: the module's test_step / test_end (under test_on_val they are the validation hooks, as in the reference)
    name = "predictions_val.pt" if test_on_val else "predictions_test.pt"
    ref_t = model.test_end([model.test_step(b, i) for i, b in enumerate(batches)])
    ref_file = torch.load(name)
    got_t = tr.evaluate(batches, test=True)
    _assert_dicts_equal(torch.load(name), ref_file, name)
    assert set(got_t) == set(ref_t) and (test_on_val or got_t == {})
    tr.evaluate(batches, test=True, out_path="elsewhere.pt")
    _assert_dicts_equal(torch.load("elsewhere.pt"), ref_file, "out_path")


# ---------------------------------------------------------------------------------------------- 10. add() does not synchronise
def test_add_does_not_synchronise():
    from m3t.evaluate import Evaluator
    wins = _metric_windows()
    batches, _ = _feed(wins, 8, 8, True)                                 # 76 windows: ten batches
    dev_batches, _ = _feed(wins, 8, 8, True, device_meta=True)
    todo = batches[:5] + dev_batches[5:]                                 # start / length from the host and on the device
    assert len(todo) == 10
    warm = Evaluator(8, True, True)
    for y, b in todo:                                                    # library load, allocator warm-up
        warm.add(y, b)
    warm.finish()
    torch.cuda.synchronize()
    is_sync = lambda rec: [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.ones(1, device=DEV).item()
        if not is_sync(rec):
            pytest.skip("this torch build raises no warning for a synchronising call under set_sync_debug_mode('warn')")
        ev = Evaluator(8, True, True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for y, b in todo:
                ev.add(y, b)
        assert not is_sync(rec), is_sync(rec)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.finish().metrics is not None
