"""The oracle of the multi-label evaluation epoch (m3t/cls_evaluate.py, csrc/cls_eval.hip): numpy for the ordering, Python integers and
`fractions` for the arithmetic -- exact, no scikit-learn import.  Per class, with the items ordered by their float32 score (descending;
scores that compare equal -- -0.0 and +0.0 do, two denormals do not -- form one threshold group), TP / FP the counts after a group, dTP /
dFP the group's own:

    AP  = (1 / P) sum_groups dTP TP / (TP + FP)                  (scikit-learn's average_precision_score)
    AUC = sum_groups dFP (2 TP_before + dTP) / (2 P N)           (scikit-learn's roc_auc_score: trapezoids over the ROC points)

tests/test_cls_eval_host.py pins both against scikit-learn where it is installed.
"""
import math
import statistics
from fractions import Fraction

import numpy as np


def groups(scores, labels):
    """one class: [(dTP, dFP)] per threshold group, highest score first.  scores float32 [M] (finite), labels {0, 1} [M]"""
    s = np.asarray(scores, np.float32)
    y = np.asarray(labels).astype(np.int64)
    assert s.ndim == 1 and s.shape == y.shape and np.isin(y, (0, 1)).all() and np.isfinite(s).all()
    order = np.argsort(-s.astype(np.float64), kind="stable")          # (float64 holds every float32, denormals included; -0.0 == 0.0)
    s, y = s[order], y[order]
    out = []
    a = 0
    while a < s.size:
        b = a
        while b < s.size and s[b] == s[a]:
            b += 1
        dtp = int(y[a:b].sum())
        out.append((dtp, (b - a) - dtp))
        a = b
    return out


def class_exact(scores, labels):
    """-> (AP as a Fraction or None, AUC numerator (int), P, N): AP None without a positive; AUC = num / (2 P N), undefined unless P, N >= 1"""
    tp = fp = num = 0
    ap = Fraction(0)
    for dtp, dfp in groups(scores, labels):
        num += dfp * (2 * tp + dtp)
        tp += dtp
        fp += dfp
        if dtp:
            ap += Fraction(dtp * tp, tp + fp)
    return (ap / tp if tp else None), num, tp, fp


def class_metrics(scores, labels):
    """-> (AP, AUC, P, N) as Python floats / ints, NaN where the class is not scored.  AUC is ONE correctly rounded division of two
    exactly representable integers; AP the correctly rounded value of the exact rational."""
    ap, num, P, N = class_exact(scores, labels)
    return (float(ap) if ap is not None else math.nan), (num / (2 * P * N) if P and N else math.nan), P, N


def ap_bar(P):
    """absolute bar on a class's AP: twice the worst-case bound of a float64 sum of at most P correctly rounded terms in any order"""
    return (P + 2) * 2.0 ** -52


def dprime(auc):
    if auc != auc:
        return math.nan
    if auc >= 1.0:
        return math.inf
    if auc <= 0.0:
        return -math.inf
    return math.sqrt(2.0) * statistics.NormalDist().inv_cdf(auc)


def epoch(scores, labels):
    """scores float32 [M, C], labels {0, 1} [M, C] -> dict: per-class 'ap', 'auc' (float64 [C], NaN: not scored), 'ap_exact' (Fractions
    or None), 'num', 'P', 'N'; 'val_map' / 'val_auc' (the exact means over the scored classes, rounded once; NaN: none), 'n_classes_ap',
    'n_classes_auc', 'val_dprime', and the bars 'bar_ap' [C], 'bar_mean'."""
    scores, labels = np.asarray(scores, np.float32), np.asarray(labels)
    M, C = scores.shape
    rows = [class_exact(scores[:, c], labels[:, c]) for c in range(C)]
    ap_x = [r[0] for r in rows]
    num, P, N = [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]
    auc_x = [Fraction(n, 2 * p * q) if p and q else None for n, p, q in zip(num, P, N)]
    ap = np.array([float(a) if a is not None else np.nan for a in ap_x])
    auc = np.array([n / (2 * p * q) if p and q else np.nan for n, p, q in zip(num, P, N)])
    sa, su = [a for a in ap_x if a is not None], [a for a in auc_x if a is not None]
    val_map = float(sum(sa) / len(sa)) if sa else math.nan
    val_auc = float(sum(su) / len(su)) if su else math.nan
    bar_ap = np.array([ap_bar(p) for p in P])
    return {"ap": ap, "auc": auc, "ap_exact": ap_x, "num": num, "P": np.array(P), "N": np.array(N), "val_map": val_map, "val_auc": val_auc,
            "n_classes_ap": len(sa), "n_classes_auc": len(su), "val_dprime": dprime(val_auc), "bar_ap": bar_ap,
            "bar_mean": float(bar_ap.max()) + (C + 1) * 2.0 ** -53}


def scatter(scores, labels, items, M):
    """what m3t_cls_eval_append leaves: (col_scores float32 [C, M], col_labels uint8 [C, M], seen uint8 [M]) from zero-filled matrices"""
    scores, labels, items = np.asarray(scores, np.float32), np.asarray(labels, np.float32), np.asarray(items, np.int64)
    C = scores.shape[1]
    cs, cl, seen = np.zeros((C, M), np.float32), np.zeros((C, M), np.uint8), np.zeros(M, np.uint8)
    cs[:, items] = scores.T
    cl[:, items] = (labels.T == 1.0).astype(np.uint8)
    seen[items] = 1
    return cs, cl, seen
