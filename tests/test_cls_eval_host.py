"""Host side of the multi-label evaluation epoch (m3t/cls_evaluate.py): the oracle (tests/cls_eval_ref.py) against scikit-learn and against
hand-made cases, the result's report / save formats, the drivers' flags, and the device text of the ranking (csrc/cls_eval_core.h) as a
stand-alone host program under the address and undefined-behaviour sanitizers.  No GPU."""
import csv
import json
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import cls_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "m3f.pytorch_amd")


def _column(M, seed, levels=None):
    rs = np.random.RandomState(seed)
    s = rs.standard_normal(M).astype(np.float32)
    if levels:
        s = (np.floor(rs.uniform(size=M) * levels) / levels).astype(np.float32)
    y = (rs.uniform(size=M) < 0.3).astype(np.int64)
    y[0], y[-1] = 1, 0
    return s, y


@pytest.mark.parametrize("M", [37, 257, 1000])
@pytest.mark.parametrize("levels", [None, 4, 8])
def test_oracle_equals_scikit_learn(M, levels):
    skm = pytest.importorskip("sklearn.metrics")
    s, y = _column(M, 100 + M, levels)
    ap, auc, P, N = R.class_metrics(s, y)
    assert P == int(y.sum()) and N == M - P
    assert abs(ap - skm.average_precision_score(y, s)) <= 1e-12
    assert abs(auc - skm.roc_auc_score(y, s)) <= 1e-12


def test_oracle_on_hand_made_cases():
    # untied, perfect ranking
    assert R.class_metrics([4, 3, 2, 1], [1, 1, 0, 0]) == (1.0, 1.0, 2, 2)
    # untied, worst ranking: positives at ranks 3, 4 -> AP = (1/3 + 2/4) / 2
    ap, num, P, N = R.class_exact([4, 3, 2, 1], [0, 0, 1, 1])
    assert (ap, num, P, N) == (Fraction(5, 12), 0, 2, 2)
    # interleaved: + - + - -> AP = (1 + 2/3) / 2, AUC = 3 of 4 pairs
    ap, num, P, N = R.class_exact([4, 3, 2, 1], [1, 0, 1, 0])
    assert ap == Fraction(5, 6) and Fraction(num, 2 * P * N) == Fraction(3, 4)
    # all tied: one group -> AP = P / M, AUC = 1/2
    ap, num, P, N = R.class_exact([1, 1, 1, 1], [1, 0, 0, 0])
    assert ap == Fraction(1, 4) and Fraction(num, 2 * P * N) == Fraction(1, 2)
    # a tie between a positive and a negative at the top: groups {+,-}, {+}, {-}: AP = (1 * 1/2 + 1 * 2/3) / 2, AUC = (0.5 + 1 + 1 + 1) / 4
    ap, num, P, N = R.class_exact([2, 2, 1, 0], [1, 0, 1, 0])
    assert ap == Fraction(7, 12) and Fraction(num, 2 * P * N) == Fraction(5, 8)
    # both zeros tie, two denormals do not
    assert R.groups(np.array([0.0, -0.0], np.float32), [1, 0]) == [(1, 1)]
    assert R.groups(np.array([1e-40, 2e-40], np.float32), [1, 0]) == [(0, 1), (1, 0)]
    # no positive / no negative
    ap, auc, P, N = R.class_metrics([1, 2, 3], [0, 0, 0])
    assert math.isnan(ap) and math.isnan(auc) and (P, N) == (0, 3)
    ap, auc, P, N = R.class_metrics([1, 2, 3], [1, 1, 1])
    assert ap == 1.0 and math.isnan(auc) and (P, N) == (3, 0)
    assert R.dprime(1.0) == math.inf and R.dprime(0.0) == -math.inf and math.isnan(R.dprime(math.nan)) and R.dprime(0.5) == 0.0


def test_epoch_oracle_means_and_exclusions():
    s = np.array([[3, 1, 0], [2, 2, 0], [1, 3, 0], [0, 4, 0]], np.float32)
    y = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 1]])
    y[:, 2] = 0                                               # class 2: no positive
    e = R.epoch(s, y)
    assert e["n_classes_ap"] == 2 and e["n_classes_auc"] == 2 and math.isnan(e["ap"][2]) and math.isnan(e["auc"][2])
    assert e["val_map"] == 1.0 and e["val_auc"] == 1.0 and e["val_dprime"] == math.inf
    assert list(e["P"]) == [2, 2, 0] and list(e["N"]) == [2, 2, 4]


def _result():
    from m3t.cls_evaluate import ClsEvalResult
    metrics = {"val_loss": 0.5, "val_acc": 0.25, "val_map": 0.6, "val_auc": 0.75, "val_dprime": R.dprime(0.75), "n_classes_ap": 3,
               "n_classes_auc": 2, "n_nonfinite": 0, "n_bad_labels": 0}
    per = {"ap": np.array([0.9, math.nan, 0.3, 0.6]), "auc": np.array([0.8, math.nan, math.nan, 0.7]), "P": np.array([2, 0, 5, 1]),
           "N": np.array([3, 5, 0, 4])}
    return ClsEvalResult(metrics, per)


def test_report_format(tmp_path):
    res = _result()
    lines = []
    got = res.report(["Speech", "Music", "Dog, bark", "Rain"], top=2, out=lines.append)
    assert lines == [0.6, 0.75, R.dprime(0.75), "Lowest AP:", "Dog, bark 0.3", "Rain 0.6", "Highest AP:", "Speech 0.9", "Rain 0.6"]
    assert got["ap"] == {"Speech": 0.9, "Dog, bark": 0.3, "Rain": 0.6} and got["map"] == 0.6
    lines = []
    res.report(top=1, out=lines.append)                       # without names: the class indices
    assert lines[3:] == ["Lowest AP:", "2 0.3", "Highest AP:", "0 0.9"]
    names = tmp_path / "class_labels_indices.csv"
    names.write_text('index,mid,display_name\n0,/m/09x0r,"Speech"\n1,/m/04rlf,"Music"\n2,/m/0bt9lr,"Dog, bark"\n3,/m/06mb1,"Rain"\n')
    lines = []
    res.report(str(names), top=1, out=lines.append)
    assert lines[4] == "Dog, bark 0.3"
    with pytest.raises(ValueError, match="3 names for 4 classes"):
        res.report(["a", "b", "c"])


def test_save_writes_json_and_csv(tmp_path):
    res = _result()
    j, c = res.save(str(tmp_path / "audioset_eval.json"), ["Speech", "Music", "Dog, bark", "Rain"])
    assert (os.path.basename(j), os.path.basename(c)) == ("audioset_eval.json", "audioset_eval.csv")
    assert json.load(open(j)) == res.metrics
    rows = list(csv.reader(open(c, newline="")))
    assert rows[0] == ["class", "name", "ap", "auc", "P", "N"] and len(rows) == 5
    assert rows[3] == ["2", "Dog, bark", "0.3", "nan", "5", "0"]
    assert float(rows[1][2]) == 0.9 and float(rows[4][3]) == 0.7


def test_evaluator_refuses_on_the_host():
    """what can be said without a device is said before one is touched: capacity and sizes"""
    from m3t import cls_evaluate as E
    with pytest.raises(ValueError, match="capacity"):
        E.ClsEvaluator(E.MAX_ROWS + 1, 527)
    with pytest.raises(ValueError, match="positive"):
        E.ClsEvaluator(0, 527)
    with pytest.raises(ValueError, match="row 7"):
        E._check_items([0, 7], 7, "add")
    with pytest.raises(ValueError, match="row -1"):
        E._check_items([-1], 7, "add")
    assert E.MAX_ROWS >= 65536 and E._check_items([6, 0], 7, "add").dtype == np.int32


def test_eval_on_device_flag_is_absent_unless_given():
    sys.path.insert(0, PKG)
    import pretrain_audioset as P
    ns = P.make_parser().parse_args([])
    assert not hasattr(ns, "eval_on_device") and not hasattr(ns, "convert_audio")
    assert P.make_parser().parse_args(["--eval_on_device"]).eval_on_device is True


def test_eval_audioset_help():
    r = subprocess.run([sys.executable, os.path.join(PKG, "eval_audioset.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--checkpoint", "--dataset_path", "--out", "--num_hidden"):
        assert flag in r.stdout


def test_ranking_text_on_the_host_under_sanitizers(tmp_path):
    """csrc/cls_eval_core.h -- key, bitonic steps (LDS and chunked schedules), scans and the walk -- as a stand-alone program with its own
    main, built with the address and undefined-behaviour sanitizers: every size x thread count x chunk length x tie pattern agrees with a
    direct restatement, and no index leaves its block."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cls_eval_host_check")
    src = os.path.join(PKG, "csrc", "cls_eval_host_check.cpp")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    b = subprocess.run([cxx] + flags + [src, "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr + b.stdout or b.returncode != 0 and "asan" in (b.stderr + b.stdout).lower():
        b = subprocess.run([cxx, "-O1", "-std=c++17", src, "-o", exe], capture_output=True, text=True)      # no sanitizer runtime installed
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cases agree" in r.stdout
