"""The expression head in the device-side evaluation epoch (m3t.evaluate with expr=True over csrc/evaluate_expr.hip).
The reference never validates the head, so the yardstick is the restatement below: float32 sums in the order the header
states ("zeros, += in start order, * 0.5"), torch.argmax on the CPU for the class rule, exact integer counts, and the
scores in Python floats (float64) from those counts.  Integer outputs must be equal, the logit tracks bit-equal, and the
float64 figures -- a handful of roundings of ratios of exact integers in [0, 1] -- equal to 1e-15 absolute.  The one anchor
the reference gives is training_step's acc_expr (models/model.py:180-181)."""
import argparse
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC = 7
VA_METRICS = ("val_ccc_v", "val_ccc_a", "val_mse_v", "val_mse_a", "val_loss")
EXPR_METRICS = ("val_acc_expr", "val_f1_expr", "val_score_expr")
HEADER = "Neutral,Anger,Disgust,Fear,Happiness,Sadness,Surprise"
TOL = 1e-15


# ---------------------------------------------------------------------------------------------- the restatement
def _argmax(rows):
    """[n, 7] float32 -> classes, by torch.argmax on the CPU: the rule the kernels must follow"""
    return torch.argmax(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).reshape(-1, NC), dim=-1).numpy()


def _window_conf(w):
    """[7, 7] counts of one window: label (clipped to 0..6) x argmax over its valid frames"""
    conf = np.zeros((NC, NC), np.int64)
    pred = _argmax(w["y"][:, :NC])
    for t in range(len(pred)):
        if w["valid"][t]:
            conf[min(max(int(w["cls"][t]), 0), NC - 1), pred[t]] += 1
    return conf


def _scores(conf):
    """the figures from a [7, 7] confusion, class by class in Python floats"""
    conf = np.asarray(conf, dtype=np.int64).reshape(-1, NC, NC).sum(0)
    div = lambda a, b: a / b if b else float("nan")
    total, hit = int(conf.sum()), int(np.trace(conf))
    prec, rec, f1 = [], [], []
    f1sum, present = 0.0, 0
    for c in range(NC):
        tp = int(conf[c, c])
        fp, fn = int(conf[:, c].sum()) - tp, int(conf[c, :].sum()) - tp
        prec.append(div(tp, tp + fp))
        rec.append(div(tp, tp + fn))
        f1.append(div(2 * tp, 2 * tp + fp + fn))
        if tp + fp + fn > 0:
            f1sum += f1[-1]
            present += 1
    acc, f1m = div(hit, total), div(f1sum, present)
    return {"acc": acc, "f1": f1m, "score": 0.67 * f1m + 0.33 * acc, "precision": prec, "recall": rec, "f1_class": f1}


def _stitch(wins, T, overlap, with_gt=True):
    """per video in first-seen order: logits [n, 7] float32, pred [n] and gt [n] (int8), window by window, frame by frame"""
    by_video = {}
    for w in wins:
        by_video.setdefault(w["name"], []).append(w)
    out = {}
    for name, ws in by_video.items():
        ws = sorted(ws, key=lambda w: w["start"])
        dst, pos = [], 0
        for w in ws:
            dst.append(w["start"] if overlap else pos)
            pos += len(w["y"])
        n = dst[-1] + len(ws[-1]["y"])
        track = np.zeros((n, NC), np.float32)
        covered = np.zeros(n, bool)
        gt = np.full(n, -1, np.int8)
        for d, w in zip(dst, ws):
            for t in range(len(w["y"])):
                track[d + t] = track[d + t] + w["y"][t, :NC]
                if not covered[d + t]:
                    covered[d + t] = True
                    if with_gt and w["valid"][t]:
                        gt[d + t] = min(max(int(w["cls"][t]), 0), NC - 1)
        if overlap:
            track[T // 2:] = track[T // 2:] * np.float32(0.5)
        pred = np.where(covered, _argmax(track), -1).astype(np.int8)
        out[name] = (track, pred, gt)
    return out


def _mode_filter(track, window):
    h, n, out = window // 2, len(track), []
    for i in range(n):
        cnt = [0] * NC
        for j in range(max(0, i - h), min(n - 1, i + h) + 1):
            if track[j] >= 0:
                cnt[track[j]] += 1
        best = max(cnt)
        if best == 0:
            out.append(-1)
        elif track[i] >= 0 and cnt[track[i]] == best:
            out.append(int(track[i]))
        else:
            out.append(cnt.index(best))
    return out


def _close(got, want, what=""):
    """float64 figures: NaN in the same places, else within 1e-15"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= TOL), (what, got, want)


def _check_result_metrics(res, conf, what=""):
    want = _scores(conf)
    _close([res.metrics[k] for k in EXPR_METRICS], [want["acc"], want["f1"], want["score"]], what)
    for key, wkey in (("precision", "precision"), ("recall", "recall"), ("f1", "f1_class")):
        _close(list(res.expr_metrics[key].values()), want[wkey], what + key)
    return want


# ---------------------------------------------------------------------------------------------- windows -> batches
def _window(rs, name, start, L, C=9, p_valid=0.8):
    return {"name": name, "start": start, "y": rs.standard_normal((L, C)).astype(np.float32),
            "v_gt": rs.uniform(-1, 1, L).astype(np.float32), "a_gt": rs.uniform(-1, 1, L).astype(np.float32),
            "cls": rs.randint(0, NC, L).astype(np.int64), "valid": rs.uniform(size=L) < p_valid}


def _slide(rs, name, nframes, T, stride, C=9):
    return [_window(rs, name, s, min(T, nframes - s), C) for s in range(0, nframes, stride)]


def _feed(wins, T, bs, with_gt=True, host=False):
    """(y_hat, batch) per batch.  Everything past a window's length is poison: NaN outputs and labels, class 3 marked valid."""
    batches = []
    put = (lambda a: torch.from_numpy(a)) if host else (lambda a: torch.from_numpy(a).to(DEV))
    for i in range(0, len(wins), bs):
        chunk = wins[i:i + bs]
        N, Cn = len(chunk), chunk[0]["y"].shape[1]
        y = np.full((N, T, Cn), np.nan, np.float32)
        lab = np.full((2, N, T), np.nan, np.float32)
        cls, vld = np.full((N, T), 3, np.int64), np.ones((N, T), bool)
        for n, w in enumerate(chunk):
            L = len(w["y"])
            y[n, :L], lab[0, n, :L], lab[1, n, :L], cls[n, :L], vld[n, :L] = w["y"], w["v_gt"], w["a_gt"], w["cls"], w["valid"]
        batch = {"vid_name": [w["name"] for w in chunk], "start": torch.tensor([w["start"] for w in chunk]),
                 "length": torch.tensor([len(w["y"]) for w in chunk])}
        if with_gt:
            batch.update({"label_valence": put(lab[0]), "label_arousal": put(lab[1]), "class_expr": put(cls), "expr_valid": put(vld)})
        batches.append((torch.from_numpy(y).to(DEV), batch))
    return batches


def _run(batches, window, overlap, with_gt=True, expr=True):
    from m3t.evaluate import Evaluator
    ev = Evaluator(window, overlap, with_gt, expr=expr)
    for y, b in batches:
        ev.add(y, b)
    return ev.finish()


def _check_tracks(res, wins, T, overlap, with_gt=True):
    want = _stitch(wins, T, overlap, with_gt)
    assert res.names == list(want)
    assert res.expr.logits.dtype == torch.float32 and res.expr.pred.dtype == torch.int8
    assert tuple(res.expr.logits.shape) == (NC, int(res.frame_off[-1]))
    logits, pred = res.expr.logits.cpu().numpy(), res.expr.pred.cpu().numpy()
    gt = res.expr.gt.cpu().numpy() if with_gt else None
    assert (res.expr.gt is None) == (not with_gt)
    for v, name in enumerate(res.names):
        a, b = int(res.frame_off[v]), int(res.frame_off[v + 1])
        track, p, g = want[name]
        assert b - a == len(p), name
        assert logits[:, a:b].T.tobytes() == track.tobytes(), name               # bit-equal
        assert np.array_equal(pred[a:b], p), name
        if with_gt:
            assert np.array_equal(gt[a:b], g), name
    return want


# ---------------------------------------------------------------------------------------------- the entry points, directly
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib_stream():
    from m3t.ops import lib, _stream
    return lib(), _stream()


def _append(y, lv, la, length, cls=None, vld=None, mtl=True):
    """m3t_eval_append_mtl (or m3t_eval_append) on numpy inputs -> rows, part (, expr_rows, expr_gt, conf) as numpy"""
    from m3t import _lib
    N, T, Cn = y.shape
    dv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV) if a is not None else None
    ty, tlv, tla, tlen = dv(y, torch.float32), dv(lv, torch.float32), dv(la, torch.float32), dv(length, torch.int64)
    tcls, tvld = dv(cls, torch.int64), dv(vld, torch.uint8)
    gt = lv is not None
    rows = torch.full((N, 4 if gt else 2, T), 7.0, dtype=torch.float32, device=DEV)
    part = torch.full((N, 2, 7), 7.0, dtype=torch.float64, device=DEV) if gt else None
    lib, stream = _lib_stream()
    if not mtl:
        _lib.check(lib.m3t_eval_append(_ptr(ty), N, T, Cn, _ptr(tlv), _ptr(tla), _ptr(tlen), _ptr(rows), _ptr(part), stream), "append")
        torch.cuda.synchronize()
        return rows.cpu().numpy(), part.cpu().numpy() if gt else None
    erows = torch.full((N, NC, T), 7.0, dtype=torch.float32, device=DEV)
    egt = torch.full((N, T), 5, dtype=torch.int8, device=DEV) if gt else None
    conf = torch.full((N, NC, NC), 5, dtype=torch.int32, device=DEV) if gt else None
    _lib.check(lib.m3t_eval_append_mtl(_ptr(ty), N, T, Cn, _ptr(tlv), _ptr(tla), _ptr(tcls), _ptr(tvld), _ptr(tlen), _ptr(rows),
                                       _ptr(part), _ptr(erows), _ptr(egt), _ptr(conf), stream), "append_mtl")
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy() if t is not None else None
    return host(rows), host(part), host(erows), host(egt), host(conf)


def _append_case(N, T, Cn, lengths, seed):
    rs = np.random.RandomState(seed)
    y = rs.standard_normal((N, T, Cn)).astype(np.float32)
    lv, la = rs.uniform(-1, 1, (N, T)).astype(np.float32), rs.uniform(-1, 1, (N, T)).astype(np.float32)
    lv[rs.uniform(size=(N, T)) < 0.2] = -5.0
    cls = rs.randint(-2, 10, (N, T)).astype(np.int64)                          # labels outside 0..6: clipped
    vld = rs.uniform(size=(N, T)) < 0.75
    return y, lv, la, cls, vld, np.asarray(lengths, np.int64)


def _check_append(y, lv, la, cls, vld, length):
    N, T, Cn = y.shape
    rows, part, erows, egt, conf = _append(y, lv, la, length, cls, vld)
    for n in range(N):
        L = int(length[n])
        w = {"y": y[n, :L], "cls": cls[n, :L], "valid": vld[n, :L]}
        want_rows = np.zeros((NC, T), np.float32)
        want_rows[:, :L] = y[n, :L, :NC].T
        assert erows[n].tobytes() == want_rows.tobytes(), n
        want_gt = np.full(T, -1, np.int8)
        want_gt[:L] = np.where(vld[n, :L], np.clip(cls[n, :L], 0, NC - 1), -1)
        assert np.array_equal(egt[n], want_gt), n
        assert np.array_equal(conf[n], _window_conf(w)), n
    # frames past the length are never read: poison them and nothing changes
    y2, lv2, la2, cls2, vld2 = y.copy(), lv.copy(), la.copy(), cls.copy(), vld.copy()
    for n in range(N):
        L = int(length[n])
        y2[n, L:], lv2[n, L:], la2[n, L:], cls2[n, L:], vld2[n, L:] = np.nan, np.nan, np.nan, 1 << 40, True
    again = _append(y2, lv2, la2, length, cls2, vld2)
    for a, b in zip((rows, part, erows, egt, conf), again):
        assert a.tobytes() == b.tobytes()
    return rows, part, erows, egt, conf


# ---------------------------------------------------------------------------------------------- 1. valence / arousal unchanged
@pytest.mark.parametrize("with_gt", [True, False])
def test_append_mtl_gives_eval_appends_rows_and_part(with_gt):
    for N, T, lengths in ((3, 5, (5, 2, 1)), (2, 300, (300, 257))):
        y, lv, la, cls, vld, length = _append_case(N, T, 9, lengths, 11)
        lv[0, 1] = np.nan                                                       # a NaN label inside a window
        if not with_gt:
            lv = la = cls = vld = None
        ref = _append(y, lv, la, length, mtl=False)
        got = _append(y, lv, la, length, cls, vld)
        assert got[0].tobytes() == ref[0].tobytes()
        if with_gt:
            assert got[1].tobytes() == ref[1].tobytes()


def _epoch_windows(seed=21, C=9):
    rs = np.random.RandomState(seed)
    wins = _slide(rs, "a", 40, 8, 4, C) + _slide(rs, "b", 29, 8, 4, C) + _slide(rs, "c", 8, 8, 4, C)
    for w in wins:
        w["v_gt"][rs.uniform(size=len(w["v_gt"])) < 0.15] = -5.0
    return [wins[i] for i in rs.permutation(len(wins))]


@pytest.mark.parametrize("overlap", [True, False])
def test_evaluator_va_tracks_and_metrics_unchanged(overlap):
    wins = _epoch_windows()
    a = _run(_feed(wins, 8, 5), 8, overlap, expr=False)
    b = _run(_feed(wins, 8, 5), 8, overlap, expr=True)
    assert a.expr is None and a.expr_metrics is None and tuple(a.metrics) == VA_METRICS
    assert tuple(b.metrics) == VA_METRICS + EXPR_METRICS
    assert a.tracks.cpu().numpy().tobytes() == b.tracks.cpu().numpy().tobytes()
    assert np.array([a.metrics[k] for k in VA_METRICS]).tobytes() == np.array([b.metrics[k] for k in VA_METRICS]).tobytes()
    assert set(a.to_dicts()) == {"valence_gt", "arousal_gt", "valence_pred", "arousal_pred"}


# ---------------------------------------------------------------------------------------------- 2. append
@pytest.mark.parametrize("Cn", [9, 11])
def test_append_small_batch(Cn):
    y, lv, la, cls, vld, length = _append_case(3, 5, Cn, (5, 2, 1), 2)
    vld[1, :] = False                                                           # one clip without a valid label
    vld[0, :] = True
    cls[0, :] = (-3, 9, 7, 6, 0)                                                # clipped to 0, 6, 6, 6, 0
    _, _, _, egt, conf = _check_append(y, lv, la, cls, vld, length)
    assert egt[0].tolist() == [0, 6, 6, 6, 0] and egt[1].tolist() == [-1] * 5 and int(conf[1].sum()) == 0 and int(conf[0].sum()) == 5


def test_append_one_frame():
    _check_append(*_append_case(1, 1, 9, (1,), 3))


def test_append_long_window_strides():
    y, lv, la, cls, vld, length = _append_case(1, 300, 9, (300,), 4)
    conf = _check_append(y, lv, la, cls, vld, length)[4]
    assert int(conf.sum()) == int(vld.sum()) > 200
    _check_append(*_append_case(2, 300, 9, (299, 0), 5))


def test_append_without_labels():
    y, _, _, _, _, length = _append_case(3, 5, 9, (5, 2, 1), 6)
    rows, part, erows, egt, conf = _append(y, None, None, length)
    assert part is None and egt is None and conf is None
    for n, L in enumerate((5, 2, 1)):
        want = np.zeros((NC, 5), np.float32)
        want[:, :L] = y[n, :L, :NC].T
        assert erows[n].tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- 3. the argmax rule
def _argmax_rows():
    nan, inf = np.nan, np.inf
    rows = [[1, 3, 3, 2, 3, 0, -1],            # ties: the first wins
            [0, 1, 2, nan, 9, 1, 1],           # a NaN in the middle beats the 9 after it
            [5, nan, 1, 2, nan, 9, 0],         # two NaNs: the first
            [2, 2, 2, 2, 2, 2, 2],             # all equal
            [-inf] * 7, [0, 0, 0, 0, 0, 0, 1], [nan] * 7, [-0.0, 0.0, -1, -1, -1, -1, -1], [1, 2, 3, 4, 5, 6, inf],
            [inf, 1, inf, nan, 1, 1, 1]]
    return np.asarray(rows, np.float32)


def test_argmax_rule_is_torch_argmax():
    rows = _argmax_rows()
    want = _argmax(rows)
    assert want[:4].tolist() == [1, 3, 1, 0]
    T = len(rows)
    y = np.zeros((1, T, 9), np.float32)
    y[0, :, :NC] = rows
    zeros = np.zeros((1, T), np.float32)
    conf = _append(y, zeros, zeros, np.asarray([T], np.int64), np.zeros((1, T), np.int64), np.ones((1, T), bool))[4]
    assert conf[0, 0].tolist() == np.bincount(want, minlength=NC).tolist() and int(conf[0, 1:].sum()) == 0
    # and through the gather (one window: the stitched logits are the rows)
    w = {"name": "v", "start": 0, "y": y[0], "v_gt": zeros[0], "a_gt": zeros[0], "cls": np.zeros(T, np.int64), "valid": np.ones(T, bool)}
    res = _run(_feed([w], T, 1), T, False)
    assert res.expr.pred.cpu().numpy().tolist() == want.tolist()


# ---------------------------------------------------------------------------------------------- 4. gather
def _gather_windows(C=9):
    rs = np.random.RandomState(7)
    wins = _slide(rs, "seven", 7, 4, 2, C) + _slide(rs, "four", 4, 4, 2, C) + _slide(rs, "one", 1, 4, 2, C)
    wins += [_window(rs, "gap", 0, 4, C), _window(rs, "gap", 6, 2, C)]         # frames 4, 5: no window
    wins += _slide(rs, "long", 301, 4, 2, C)                                    # crosses workgroups; last window: 1 frame
    return [wins[i] for i in rs.permutation(len(wins))]


@pytest.mark.parametrize("overlap", [True, False])
def test_gather(overlap):
    wins = _gather_windows()
    assert [len(w["y"]) for w in wins if w["name"] == "seven" and w["start"] == 6] == [1]       # a last window shorter than T
    res = _run(_feed(wins, 4, 16), 4, overlap)
    want = _check_tracks(res, wins, 4, overlap)
    if overlap:
        assert want["gap"][1][4:6].tolist() == [-1, -1] and want["gap"][2][4:6].tolist() == [-1, -1]
        assert not want["gap"][0][4:6].any() and len(want["seven"][1]) == 7 and len(want["long"][1]) == 301
        # overlapping windows whose labels disagree: the earlier window's label stands
        ws = sorted((w for w in wins if w["name"] == "long"), key=lambda w: w["start"])
        clash = [(a, t) for a, b in zip(ws, ws[1:]) for t in (2, 3) if len(b["y"]) > t - 2 and a["valid"][t] and b["valid"][t - 2]
                 and a["cls"][t] != b["cls"][t - 2]]
        assert len(clash) > 20
        for a, t in clash:                       # (frames start + 2, start + 3 of a window: this window and the next hold them)
            assert want["long"][2][a["start"] + t] == a["cls"][t]
    # the epoch's figures count a frame once per window that holds it, as the VA metrics do
    _check_result_metrics(res, sum(_window_conf(w) for w in wins))


def test_gather_without_labels():
    wins = _gather_windows(C=11)
    res = _run(_feed(wins, 4, 16, with_gt=False), 4, True, with_gt=False)
    assert res.metrics is None and res.expr_metrics is None
    _check_tracks(res, wins, 4, True, with_gt=False)
    d = res.to_dicts()
    assert set(d) == {"valence_pred", "arousal_pred", "expr_logits", "expr_pred"}


def test_labels_from_the_host_give_the_same():
    wins = _epoch_windows()
    a, b = _run(_feed(wins, 8, 5), 8, True), _run(_feed(wins, 8, 5, host=True), 8, True)
    assert torch.equal(a.expr.gt, b.expr.gt) and torch.equal(a.expr.pred, b.expr.pred) and a.metrics == b.metrics


# ---------------------------------------------------------------------------------------------- 5. metrics
def _device_metrics(conf):
    from m3t import _lib
    t = torch.from_numpy(np.ascontiguousarray(conf, dtype=np.int32)).reshape(-1, NC, NC).to(DEV)
    out = torch.full((24,), 7.0, dtype=torch.float64, device=DEV)
    lib, stream = _lib_stream()
    _lib.check(lib.m3t_eval_expr_metrics(_ptr(t), t.size(0), _ptr(out), stream), "m3t_eval_expr_metrics")
    return out.cpu().numpy()


def test_metrics_hand_made_confusion():
    from m3t.evaluate import expr_metrics_from_confusion
    conf = np.zeros((NC, NC), np.int64)
    conf[0, 0], conf[0, 1], conf[1, 1], conf[1, 0], conf[2, 2], conf[2, 5], conf[4, 4], conf[6, 0] = 5, 2, 3, 1, 4, 2, 1, 3
    # class 3: empty (never labelled, never predicted); class 5: predicted only; class 6: labelled, never predicted
    got = _device_metrics(conf)
    f1 = [2 * 5 / (10 + 4 + 2), 2 * 3 / (6 + 2 + 1), 2 * 4 / (8 + 0 + 2), None, 2 * 1 / 2, 0.0, 0.0]
    f1m = (f1[0] + f1[1] + f1[2] + f1[4] + f1[5] + f1[6]) / 6
    acc = 13 / 21
    _close(got[:3], [acc, f1m, 0.67 * f1m + 0.33 * acc])
    _close(got[3:10], [5 / 9, 3 / 5, 1.0, np.nan, 1.0, 0.0, np.nan], "precision")
    _close(got[10:17], [5 / 7, 3 / 4, 4 / 6, np.nan, 1.0, np.nan, 0.0], "recall")
    _close(got[17:24], [np.nan if x is None else x for x in f1], "f1")
    for want in (_scores(conf), expr_metrics_from_confusion(conf)):
        _close(got[:3], [want["acc"], want["f1"], want["score"]])
        _close(got[3:24], np.concatenate([want["precision"], want["recall"], want["f1_class"]]))
    # many windows, more than one per thread: the sum over W
    rs = np.random.RandomState(8)
    many = rs.randint(0, 40, (700, NC, NC))
    want = _scores(many)
    got = _device_metrics(many)
    _close(got[:3], [want["acc"], want["f1"], want["score"]])
    _close(got[3:24], np.concatenate([want["precision"], want["recall"], want["f1_class"]]))


def test_epoch_figures_and_the_training_steps_accuracy():
    """non-overlapping windows: val_acc_expr is training_step's acc_expr (model.py:180-181) over the epoch's frames"""
    from m3t.evaluate import expr_metrics_from_confusion
    rs = np.random.RandomState(31)
    wins = _slide(rs, "a", 48, 8, 8) + _slide(rs, "b", 24, 8, 8)                # full windows only: every frame of y_hat counts
    batches = _feed(wins, 8, 4)
    res = _run(batches, 8, False)
    conf = sum(_window_conf(w) for w in wins)
    _check_result_metrics(res, conf)
    want = expr_metrics_from_confusion(np.stack([_window_conf(w) for w in wins]))
    _close([res.metrics[k] for k in EXPR_METRICS], [want["acc"], want["f1"], want["score"]])
    y_hat = torch.cat([y for y, _ in batches]).cpu()
    expr = torch.cat([b["class_expr"] for _, b in batches]).cpu().view(-1)
    mask = torch.cat([b["expr_valid"] for _, b in batches]).cpu().view(-1)
    valid = int(mask.long().sum())
    max_expr_class = torch.argmax(y_hat[..., :7], dim=-1).view(-1)
    acc_expr = torch.sum(max_expr_class[mask] == expr[mask]).item() / valid
    assert abs(res.metrics["val_acc_expr"] - acc_expr) <= TOL
    # concatenated full windows: the stitched tracks are the frames once, so the report without a filter agrees too
    rep = res.expr_report(out=lambda *_: None)
    assert abs(rep["acc_all"] - acc_expr) <= TOL


def test_no_valid_frame_gives_nan_and_leaves_va_alone():
    wins = _epoch_windows()
    ref = _run(_feed(wins, 8, 5), 8, True)
    for w in wins:
        w["valid"][:] = False
    res = _run(_feed(wins, 8, 5), 8, True)
    assert all(math.isnan(res.metrics[k]) for k in EXPR_METRICS), res.metrics
    assert all(math.isnan(v) for t in res.expr_metrics.values() for v in t.values())
    assert [res.metrics[k] for k in VA_METRICS] == [ref.metrics[k] for k in VA_METRICS] and not math.isnan(res.metrics["val_loss"])
    assert int((res.expr.gt != -1).sum()) == 0


# ---------------------------------------------------------------------------------------------- 6. mode filter
def _mode_device(tracks, window):
    """-> (return code, filtered tracks)"""
    lens = [len(t) for t in tracks]
    flat = torch.tensor([c for t in tracks for c in t], dtype=torch.int8, device=DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    out = torch.full_like(flat, 9)
    lib, stream = _lib_stream()
    rc = lib.m3t_expr_mode_tracks(_ptr(flat), _ptr(offs), len(tracks), window, _ptr(out), stream)
    torch.cuda.synchronize()
    return rc, [t.tolist() for t in torch.split(out.cpu(), lens)]


MODE_TRACKS = [[4], [2, 5], [-1, 3], [1, 1, 2, 2, 3, 0],                       # lengths 1, 2, 6
               [0, 1, 2, 0, 1, 2],                                              # window 3: three-way ties that hold the centre
               [3, -1, 1, -1, 3, 1],                                            # ties without the centre class (the centre is -1)
               [5, 5, -1, -1, -1, -1, -1, 2, 2, 6], [-1, -1, -1, -1], [-1], [6, 0, 0, 6, 6, 0, 3, 3, 3, 0, 0]]


@pytest.mark.parametrize("window", [1, 3, 5])
def test_mode_filter(window):
    rs = np.random.RandomState(window)
    tracks = MODE_TRACKS + [rs.randint(-1, NC, 300).tolist()]                   # and one that strides
    rc, got = _mode_device(tracks, window)
    assert rc == 0
    for t, g in zip(tracks, got):
        assert g == _mode_filter(t, window), (t, g)
    if window == 1:
        assert got == tracks
    if window == 3:
        assert got[5] == [3, 1, 1, 1, 3, 1]     # frame 1: {3, 1} tie, centre -1 -> the smaller class; frame 5: {3, 1} tie, centre 1
        assert got[4] == [0, 1, 2, 0, 1, 2] and got[7] == [-1] * 4 and got[6][3:6] == [-1] * 3


@pytest.mark.parametrize("window", [0, 2, 4, -3])
def test_mode_filter_rejects_even_and_non_positive_windows(window):
    from m3t import _lib
    rc, got = _mode_device([[1, 2, 3]], window)
    assert rc == _lib.M3T_EINVAL and got == [[9, 9, 9]]


# ---------------------------------------------------------------------------------------------- 7. the report
def _report_restated(res_tracks, window):
    """res_tracks: {video: (logits, pred, gt)} -> the overall figures and the per-video accuracy over each frame once"""
    conf_all, acc = np.zeros((NC, NC), np.int64), {}
    for name, (_, pred, gt) in res_tracks.items():
        sm = _mode_filter([int(p) for p in pred], window)
        conf = np.zeros((NC, NC), np.int64)
        for p, g in zip(sm, gt):
            if p >= 0 and g >= 0:
                conf[g, p] += 1
        conf_all += conf
        acc[name] = int(np.trace(conf)) / int(conf.sum()) if conf.sum() else float("nan")
    return _scores(conf_all), acc


@pytest.mark.parametrize("window", [1, 5])
def test_expr_report(window, tmp_path):
    from m3t.evaluate import EvalResult
    wins = _gather_windows()
    for w in wins:
        if w["name"] == "one":
            w["valid"][:] = False                                               # a video without an annotated frame
    res = _run(_feed(wins, 4, 16), 4, True)
    want, want_acc = _report_restated(_stitch(wins, 4, True), window)
    printed = []
    rep = res.expr_report(window=window, top=2, out=printed.append)
    _close([rep["acc_all"], rep["f1_all"], rep["score_all"]], [want["acc"], want["f1"], want["score"]])
    assert list(rep["acc"]) == res.names
    _close([rep["acc"][n] for n in res.names], [want_acc[n] for n in res.names])
    assert math.isnan(rep["acc"]["one"])
    for key, wkey in (("precision", "precision"), ("recall", "recall"), ("f1", "f1_class")):
        _close(list(rep["per_class"][key].values()), want[wkey], key)
    assert printed[:3] == [rep["acc_all"], rep["f1_all"], rep["score_all"]] and printed[3] == "Lowest acc-expr:"
    assert printed[6] == "Highest acc-expr:" and len(printed) == 9
    ranked = sorted((n for n in res.names if n != "one"), key=lambda n: rep["acc"][n])
    assert printed[4].split()[0] == ranked[0] and rep["acc"][printed[7].split()[0]] == rep["acc"][ranked[-1]]
    # save -> torch.load -> from_dicts -> expr_report: the same figures
    path = str(tmp_path / "predictions_val.pt")
    res.save(path)
    d = torch.load(path)
    assert set(d) == {"valence_gt", "arousal_gt", "valence_pred", "arousal_pred", "expr_logits", "expr_pred", "expr_gt"}
    v0 = res.names[0]
    n0 = int(res.frame_off[1])
    assert tuple(d["expr_logits"][v0].shape) == (n0, NC) and d["expr_pred"][v0].dtype == torch.int8 and not d["expr_gt"][v0].is_cuda
    back = EvalResult.from_dicts(d)
    assert torch.equal(back.expr.logits, res.expr.logits) and torch.equal(back.expr.pred, res.expr.pred) and torch.equal(back.expr.gt, res.expr.gt)
    printed2 = []
    rep2 = back.expr_report(window=window, top=2, out=printed2.append)
    assert printed2 == printed and np.array(list(rep2["acc"].values())).tobytes() == np.array(list(rep["acc"].values())).tobytes()
    with pytest.raises(ValueError):
        res.expr_report(window=4)
    with pytest.raises(ValueError):
        _run(_feed(wins, 4, 16), 4, True, expr=False).expr_report()


# ---------------------------------------------------------------------------------------------- 8. through the trainer
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
                        "label_arousal": f(lab[1]), "class_expr": f(rs.randint(0, NC, (N, 8)).astype(np.int64)),
                        "expr_valid": f(rs.uniform(size=(N, 8)) < 0.8), "vid_name": [m[0] for m in chunk],
                        "start": torch.tensor([m[1] for m in chunk]), "length": torch.tensor([m[2] for m in chunk])})
    return batches


def _windows_of(model, batches):
    """the windows of _audio_batches with the model's own outputs, for the restatement"""
    wins = []
    model.eval()
    with torch.no_grad():
        for b in batches:
            y = model.forward(b).cpu().numpy()
            for n, name in enumerate(b["vid_name"]):
                L = int(b["length"][n])
                wins.append({"name": name, "start": int(b["start"][n]), "y": y[n, :L], "cls": b["class_expr"][n, :L].cpu().numpy(),
                             "valid": b["expr_valid"][n, :L].cpu().numpy()})
    return wins


def test_trainer_evaluate_expr(tmp_path, monkeypatch):
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(99)
    model = AffWild2VA(_hp(modality="audio", loss="ccc_mtl", window=8)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    batches = _audio_batches()
    wins = _windows_of(model, batches)
    assert wins[0]["y"].shape[1] == 9
    # expr=False: the parent's keys, in the dict and in the file
    plain = tr.evaluate(batches)
    assert set(plain) == {"val_loss", "progress_bar", "log"} and set(plain["log"]) == set(VA_METRICS)
    assert set(plain["progress_bar"]) == {"val_ccc_v", "val_ccc_a"}
    plain_file = torch.load("predictions_val.pt")
    assert set(plain_file) == {"valence_gt", "arousal_gt", "valence_pred", "arousal_pred"}
    # expr=True, validation: concatenation
    got = tr.evaluate(batches, expr=True)
    assert set(got["log"]) == set(VA_METRICS + EXPR_METRICS) and set(got["progress_bar"]) == {"val_ccc_v", "val_ccc_a", "val_acc_expr"}
    assert got["progress_bar"]["val_acc_expr"] == got["log"]["val_acc_expr"] and isinstance(got["log"]["val_f1_expr"], float)
    for k in VA_METRICS:
        assert got["log"][k] == plain["log"][k]
    want = _scores(sum(_window_conf(w) for w in wins))
    _close([got["log"][k] for k in EXPR_METRICS], [want["acc"], want["f1"], want["score"]])
    _check_tracks(tr.last_eval, wins, 8, False)
    saved = torch.load("predictions_val.pt")
    assert set(saved) == set(plain_file) | {"expr_logits", "expr_pred", "expr_gt"}
    for k in plain_file:
        for v in plain_file[k]:
            assert torch.equal(torch.nan_to_num(saved[k][v], nan=4096.0), torch.nan_to_num(plain_file[k][v], nan=4096.0))
    stitched = _stitch(wins, 8, False)
    for v, (track, pred, gt) in stitched.items():
        assert saved["expr_logits"][v].numpy().tobytes() == track.tobytes() and saved["expr_pred"][v].tolist() == pred.tolist()
        assert saved["expr_gt"][v].tolist() == gt.tolist()
    # test=True: no labels, predictions only, overlap-add
    unlabelled = [{k: v for k, v in b.items() if k not in ("label_valence", "label_arousal", "class_expr", "expr_valid")} for b in batches]
    assert tr.evaluate(unlabelled, test=True, expr=True) == {}
    _check_tracks(tr.last_eval, wins, 8, True, with_gt=False)
    saved = torch.load("predictions_test.pt")
    assert set(saved) == {"valence_pred", "arousal_pred", "expr_logits", "expr_pred"}
    assert tr.evaluate(unlabelled, test=True) == {} and set(torch.load("predictions_test.pt")) == {"valence_pred", "arousal_pred"}


def test_trainer_evaluate_expr_needs_the_expression_head(tmp_path, monkeypatch):
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    model = AffWild2VA(_hp(modality="audio", loss="ccc", window=8)).to(DEV)        # two channels
    tr = Trainer.from_hparams(model, model.hparams)
    with pytest.raises(ValueError, match="mtl"):
        tr.evaluate(_audio_batches(), expr=True)


# ---------------------------------------------------------------------------------------------- 9. ensemble
def test_run_expr_ensemble(tmp_path):
    from m3t import postproc
    rs = np.random.RandomState(12)
    lens = {"u": 9, "v": 4, "w": 1}
    files = []
    for i in range(2):
        d = {"valence_pred": {}, "arousal_pred": {}, "expr_logits": {}, "expr_pred": {}}
        for name, n in lens.items():
            d["expr_logits"][name] = torch.from_numpy(rs.standard_normal((n, NC)).astype(np.float32))
            d["expr_pred"][name] = d["expr_logits"][name].argmax(1).to(torch.int8)
            d["valence_pred"][name] = d["arousal_pred"][name] = torch.zeros(n)
        d["expr_logits"]["u"][5] = 0.0                                           # frame 5 of u: no window in either file
        d["expr_pred"]["u"][5] = -1
        if i == 0:
            d["expr_logits"]["u"][2] = 0.0                                       # frame 2 of u: the second file alone predicts it
            d["expr_pred"]["u"][2] = -1
        files.append(d)
        torch.save(d, str(tmp_path / ("p%d.pt" % i)))
    (tmp_path / "videos.txt").write_text("u\nw\n")                               # v is not listed
    (tmp_path / "scores.txt").write_text("%s\n%s\n" % (tmp_path / "p0.pt", tmp_path / "p1.pt"))
    for window in (1, 3):
        out = postproc.run_expr_ensemble(str(tmp_path / "videos.txt"), str(tmp_path / "scores.txt"),
                                         out_dir=str(tmp_path / ("EXPR-%d" % window)), window=window)
        assert sorted(p.name for p in (tmp_path / ("EXPR-%d" % window)).iterdir()) == ["u.txt", "w.txt"]
        for name in ("u", "w"):
            text = open("%s/%s.txt" % (out, name)).read().splitlines()
            assert text[0] == HEADER and len(text) == 1 + lens[name]
            mean = (files[0]["expr_logits"][name] + files[1]["expr_logits"][name]) / 2
            cls = torch.argmax(mean, dim=1).tolist()
            if name == "u":
                cls[5] = -1
            assert [int(x) for x in text[1:]] == _mode_filter(cls, window), (name, window)
            if name == "u" and window == 1:
                assert text[6] == "-1" and text[3] == str(int(files[1]["expr_logits"]["u"][2].argmax()))
    del files[1]["expr_logits"]
    torch.save(files[1], str(tmp_path / "p1.pt"))
    with pytest.raises(ValueError, match="p1.pt"):
        postproc.run_expr_ensemble(str(tmp_path / "videos.txt"), str(tmp_path / "scores.txt"), out_dir=str(tmp_path / "none"))


# ---------------------------------------------------------------------------------------------- 10. no sync, same bits
def test_add_with_expr_does_not_synchronise():
    from m3t.evaluate import Evaluator
    wins = _epoch_windows()
    todo = _feed(wins, 8, 4)[:3] + _feed(wins, 8, 4, host=True)[3:]             # labels on the device and from the host
    assert len(todo) >= 5
    warm = Evaluator(8, True, True, expr=True)
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
        ev = Evaluator(8, True, True, expr=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for y, b in todo:
                ev.add(y, b)
        assert not is_sync(rec), is_sync(rec)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.finish().metrics["val_acc_expr"] >= 0.0


def test_two_runs_give_the_same_bits():
    wins = _gather_windows()
    runs = []
    for _ in range(2):
        res = _run(_feed(wins, 4, 16), 4, True)
        printed = []
        rep = res.expr_report(window=3, out=printed.append)
        raw = lambda t: t.cpu().numpy().tobytes()
        runs.append((raw(res.tracks), raw(res.expr.logits), raw(res.expr.pred), raw(res.expr.gt),
                     np.array(list(res.metrics.values())).tobytes(), np.array(list(rep["acc"].values())).tobytes(),
                     np.array([v for t in res.expr_metrics.values() for v in t.values()]).tobytes(), [str(p) for p in printed]))
    assert runs[0] == runs[1]
