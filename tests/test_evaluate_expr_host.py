"""The host side of the expression evaluation (m3t.evaluate): expr_metrics_from_confusion against hand-computed cases and a
direct per-class count, and the argument checks of Evaluator(expr=True) / EvalResult that need no device."""
import math

import numpy as np
import pytest
import torch

from m3t.evaluate import EvalResult, Evaluator, expr_metrics_from_confusion, EXPR_CLASSES

NC = 7


def _conf(gt, pred):
    c = np.zeros((NC, NC), np.int64)
    for g, p in zip(gt, pred):
        c[g, p] += 1
    return c


def _direct(gt, pred):
    """accuracy, macro-F1 over the classes in gt or pred, score: counted label by label, Python floats"""
    gt, pred = list(gt), list(pred)
    f1s = []
    for c in range(NC):
        tp = sum(1 for g, p in zip(gt, pred) if g == c and p == c)
        fp = sum(1 for g, p in zip(gt, pred) if g != c and p == c)
        fn = sum(1 for g, p in zip(gt, pred) if g == c and p != c)
        if tp + fp + fn > 0:
            f1s.append(2 * tp / (2 * tp + fp + fn))
    acc = sum(1 for g, p in zip(gt, pred) if g == p) / len(gt)
    f1 = 0.0
    for x in f1s:
        f1 += x
    f1 /= len(f1s)
    return acc, f1, 0.67 * f1 + 0.33 * acc


def test_hand_computed_cases():
    assert EXPR_CLASSES == ("Neutral", "Anger", "Disgust", "Fear", "Happiness", "Sadness", "Surprise")
    # everything right, two classes present
    m = expr_metrics_from_confusion(_conf([0, 0, 4], [0, 0, 4]))
    assert (m["acc"], m["f1"], m["score"]) == (1.0, 1.0, 0.67 * 1.0 + 0.33 * 1.0)
    assert m["precision"][0] == 1.0 and math.isnan(m["precision"][1]) and math.isnan(m["recall"][6]) and math.isnan(m["f1_class"][2])
    # labels 0 0 0 1, predictions 0 0 1 2: class 2 is predicted only (F1 0, counts in the mean), classes 3..6 are absent
    m = expr_metrics_from_confusion(_conf([0, 0, 0, 1], [0, 0, 1, 2]))
    assert m["acc"] == 0.5
    assert m["f1_class"][:3].tolist() == [4 / 5, 0.0, 0.0] and m["f1"] == (4 / 5 + 0.0 + 0.0) / 3
    assert m["score"] == 0.67 * m["f1"] + 0.33 * 0.5
    assert m["precision"][:3].tolist() == [1.0, 0.0, 0.0] and m["recall"][0] == 2 / 3 and m["recall"][1] == 0.0 and math.isnan(m["recall"][2])
    # no frame at all: 0 / 0
    m = expr_metrics_from_confusion(np.zeros((NC, NC), np.int64))
    assert all(math.isnan(m[k]) for k in ("acc", "f1", "score")) and np.isnan(m["f1_class"]).all()
    # leading axes are summed (windows, videos, shards)
    a, b = _conf([1, 2, 3, 3], [1, 2, 3, 1]), _conf([5, 5, 6], [5, 6, 6])
    whole, parts = expr_metrics_from_confusion(a + b), expr_metrics_from_confusion(np.stack([a, b]).astype(np.int32))
    assert (whole["acc"], whole["f1"], whole["score"]) == (parts["acc"], parts["f1"], parts["score"])
    with pytest.raises(ValueError):
        expr_metrics_from_confusion(np.zeros((6, 6)))


def test_random_label_sets_against_a_direct_count():
    try:
        from sklearn.metrics import accuracy_score, f1_score
    except Exception:      # noqa: BLE001  (scikit-learn is optional: the direct count below is the binding check)
        f1_score = accuracy_score = None
    rs = np.random.RandomState(2020)
    seen = set()
    for i in range(200):
        k = 1 + i % NC                                                           # 1 to 7 classes present
        classes = rs.choice(NC, k, replace=False)
        n = int(rs.randint(1, 400))
        gt, pred = classes[rs.randint(0, k, n)], classes[rs.randint(0, k, n)]
        if i % 3 == 0:
            pred = np.where(rs.uniform(size=n) < 0.8, gt, pred)                  # a model that has learnt something
        seen.add(len(set(gt.tolist()) | set(pred.tolist())))
        m = expr_metrics_from_confusion(_conf(gt, pred))
        acc, f1, score = _direct(gt, pred)
        assert m["acc"] == acc and abs(m["f1"] - f1) <= 1e-15 and abs(m["score"] - score) <= 1e-15, (i, m, acc, f1, score)
        if f1_score is not None:
            assert m["f1"] == f1_score(gt, pred, average="macro") and m["acc"] == accuracy_score(gt, pred), i
    assert seen == set(range(1, NC + 1))


def test_argument_checks_without_a_device():
    ev = Evaluator(8, True, with_gt=True, expr=True)
    assert ev.expr and Evaluator(8, True).expr is False
    batch = {"vid_name": ["a"], "start": torch.tensor([0]), "length": torch.tensor([8]),
             "label_valence": torch.zeros(1, 8), "label_arousal": torch.zeros(1, 8)}
    with pytest.raises(ValueError, match="att_dec") as e:
        ev.add(torch.zeros(1, 8, 2), batch)                                      # no expression head
    assert "mtl" in str(e.value)
    with pytest.raises(ValueError, match="class_expr"):
        ev.add(torch.zeros(1, 8, 9), batch)                                      # labels without the expression labels
    with pytest.raises(ValueError, match="expr_valid"):
        ev.add(torch.zeros(1, 8, 9), dict(batch, class_expr=torch.zeros(1, 8, dtype=torch.int64)))
    res = EvalResult(["a"], [0, 3], torch.zeros(4, 3))
    assert res.expr is None and res.expr_metrics is None
    assert set(res.to_dicts()) == {"valence_gt", "arousal_gt", "valence_pred", "arousal_pred"}
    with pytest.raises(ValueError, match="expr=True"):
        res.expr_report()
